"""GPU: the element-wise launchers that pick a kernel instantiation from a
runtime dtype (geglu, cfg_affine_step, cfg_dpm_step, group_norm_stats,
gn_merge_stats) in bf16, fp16 and fp32, each at one size the 16-byte vector
path takes and one it cannot, against the same op under DFA_FORCE_EAGER=1 on
the same inputs. A launcher that took the wrong instantiation for a dtype
would read its operands at the wrong width and miss these bounds grossly.

Bounds: bf16 as tests/test_ops_gpu.py has them for the op; fp16 and fp32 twice
the largest error recorded for the (op, dtype) in
profiles/native_dispatch_refactor.md.

Run on an MI355X box: pytest tests/test_dtype_dispatch_gpu.py -m gpu -q -s"""

from types import SimpleNamespace

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

if torch.cuda.is_available():
    from distrifuser_amd import ops
else:  # collected on CPU boxes but never run
    ops = None

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

DEV = "cuda:0"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF16, F16, F32]

# largest |native - eager| allowed, per (op, dtype)
BOUNDS = {
    ("geglu", BF16): 0.02,
    ("geglu", F16): 2 * 0.00390625,
    ("geglu", F32): 2 * 0.0,
    ("cfg_affine_step", BF16): 0.03,
    ("cfg_affine_step", F16): 2 * 0.000244140625,
    ("cfg_affine_step", F32): 2 * 3.4570694e-06,
    ("cfg_dpm_step", BF16): 0.05,
    ("cfg_dpm_step", F16): 2 * 0.0,
    ("cfg_dpm_step", F32): 2 * 7.62939453e-06,
    ("group_norm_stats", BF16): 5e-3,
    ("group_norm_stats", F16): 2 * 0.0,
    ("group_norm_stats", F32): 2 * 1.1920929e-07,
    ("gn_merge_stats", BF16): 2e-2,
    ("gn_merge_stats", F16): 2 * 1.1920929e-07,
    ("gn_merge_stats", F32): 2 * 2.38418579e-07,
}


def _native_and_eager(monkeypatch, fn):
    monkeypatch.delenv("DFA_FORCE_EAGER", raising=False)
    native = fn()
    monkeypatch.setenv("DFA_FORCE_EAGER", "1")
    eager = fn()
    monkeypatch.delenv("DFA_FORCE_EAGER")
    return native, eager


def _check(op, dtype, case, native, eager):
    assert native.dtype == eager.dtype and native.shape == eager.shape
    assert torch.isfinite(native.float()).all()
    err = (native.double() - eager.double()).abs().max().item()
    print(f"dtype_dispatch {op} {dtype} {case}: max err {err:.9g}")
    assert err <= BOUNDS[op, dtype], f"{op} {dtype} {case}: max err {err}"


def _randn(shape, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g).to(dtype)


@requires_gpu
@pytest.mark.parametrize("shape", [(3, 2 * 40), (3, 2 * 7)])  # inner 40: vectors; 7: elements
@pytest.mark.parametrize("dtype", DTYPES)
def test_geglu_dtypes(monkeypatch, dtype, shape):
    h = _randn(shape, dtype, 0)
    native, eager = _native_and_eager(monkeypatch, lambda: ops.geglu(h))
    _check("geglu", dtype, shape, native, eager)


CFG_SHAPES = [(2, 4, 8, 8), (2, 1, 3, 5)]  # 256 elements per sample: vectors; 15: elements


@requires_gpu
@pytest.mark.parametrize("shape", CFG_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cfg_affine_step_dtypes(monkeypatch, dtype, shape):
    from distrifuser_amd.schedulers import DDIMScheduler

    s = DDIMScheduler()
    s.set_timesteps(50)
    noise = _randn(shape, dtype, 1)
    x = _randn((1, *shape[1:]), dtype, 2)
    native, eager = _native_and_eager(
        monkeypatch, lambda: s.guided_step(noise, s.timesteps[7], x, 5.0))
    _check("cfg_affine_step", dtype, shape, native, eager)


@requires_gpu
@pytest.mark.parametrize("shape", CFG_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cfg_dpm_step_dtypes(monkeypatch, dtype, shape):
    """Four steps from the same (x, noise): first order without history, two
    2M steps that read the fp32 x0 of the step before, first order again."""
    from distrifuser_amd.schedulers import DPMSolverMultistepScheduler

    def trajectory():
        s = DPMSolverMultistepScheduler()
        s.set_timesteps(4)
        return torch.stack([
            s.guided_step(_randn(shape, dtype, 10 + i), int(t),
                          _randn((1, *shape[1:]), dtype, 20 + i), 5.0)
            for i, t in enumerate(s.timesteps)
        ])

    native, eager = _native_and_eager(monkeypatch, trajectory)
    _check("cfg_dpm_step", dtype, shape, native, eager)


# (shape, groups): group length 32, vectors in every dtype; 45, elements
@requires_gpu
@pytest.mark.parametrize("shape,groups", [((2, 8, 4, 4), 4), ((2, 6, 3, 5), 2)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_norm_stats_dtypes(monkeypatch, dtype, shape, groups):
    x = _randn(shape, dtype, 3)
    native, eager = _native_and_eager(monkeypatch, lambda: ops.group_norm_stats(x, groups))
    assert native.shape == (2, shape[0], groups, 1, 1, 1)
    _check("group_norm_stats", dtype, shape, native, eager)


class _OneRankComm:
    """The comm manager as PatchGroupNorm sees it, without peers: a flat buffer
    of `n_peers` rows with one registered moment slot at `start`."""

    def __init__(self, buffer, start, shape, own):
        self.buffer, self.starts, self.own = buffer, [start], own
        self.end, self.shape = start + 2 * shape[1] * shape[2], shape

    def get_buffer_list(self, idx):
        return [row[self.starts[idx]:self.end].view(self.shape) for row in self.buffer]

    def wait(self, idx):
        pass

    def enqueue(self, idx, tensor=None):
        if tensor is not None:
            self.buffer[self.own, self.starts[idx]:self.end].copy_(tensor.reshape(-1))


@requires_gpu
@pytest.mark.parametrize("corrected", [True, False])
@pytest.mark.parametrize("n,groups", [(2, 4), (1, 300)])  # 8 moments; 300: a second block
@pytest.mark.parametrize("dtype", DTYPES)
def test_gn_merge_stats_dtypes(monkeypatch, dtype, n, groups, corrected):
    """PatchGroupNorm's steady-state merge: the fused kernel against the torch
    composition the module runs under DFA_FORCE_EAGER=1, on the same stale
    buffer and fresh moments. The moments it hands to group_norm_apply and the
    buffer it leaves behind are what is compared; moments in [0.5, 1.5) make
    the corrected variance negative for many groups, so the guard runs."""
    from distrifuser_amd.parallel.patch_ops import PatchGroupNorm

    peers, own, start = 4, 2, 8
    shape = (2, n, groups, 1, 1, 1)
    g = torch.Generator(device=DEV).manual_seed(5)
    row = start + 2 * n * groups + 24
    buf0 = (torch.rand(peers, row, device=DEV, generator=g) + 0.5).to(dtype)
    fresh = (torch.rand(shape, device=DEV, generator=g) + 0.5).to(dtype)
    x = torch.zeros(n, groups, 2, 2, device=DEV, dtype=dtype)

    monkeypatch.setattr(ops, "group_norm_stats", lambda x, num_groups: fresh)
    monkeypatch.setattr(ops, "group_norm_apply",
                        lambda x, mean, meansq, *a, **k: torch.stack(
                            [mean.float().reshape(-1), meansq.float().reshape(-1)]))

    def merge():
        comm = _OneRankComm(buf0.clone(), start, shape, own)
        cfg = SimpleNamespace(parallelism="patch", n_device_per_batch=peers, split_idx=lambda: own,
                              mode="corrected_async_gn" if corrected else "stale_gn")
        state = SimpleNamespace(config=cfg, comm_manager=comm, in_warmup=False, recording=False)
        gn = PatchGroupNorm(groups, groups, state=state)
        gn._idx = 0
        return gn(x), comm.buffer

    (native, native_buf), (eager, eager_buf) = _native_and_eager(monkeypatch, merge)
    _check("gn_merge_stats", dtype, (n, groups, corrected), native, eager)
    expect = buf0.clone()  # fresh staged into the own slot, nothing else touched
    expect[own, start:start + 2 * n * groups] = fresh.reshape(-1)
    assert torch.equal(native_buf, expect) and torch.equal(eager_buf, expect)
