"""The inpaint kernels of csrc/scheduler.hip (masked affine step, masked
DPM-Solver++ step, 9-channel U-Net input assembly) against their eager fp32
references, and the exactness the pipeline relies on: m == 1 is the unmasked
step bit for bit, m == 0 with (sa, sb) = (1, 0) is init, the DPM x0 state is
the unmasked kernel's.

Tolerance against the reference. Kernel and reference compute the same
expression tree in fp32 and round once to T; only FMA contraction differs. A
contracted product skips one fp32 rounding, so over the tree the fp32 values
differ by at most 4 * eps32 * (sum of the |terms|), which is the bound for
T = fp32. For a 16-bit T that fp32 difference can at most move the final
rounding to the neighbouring value: one unit in the last place of T at the
reference's magnitude.

Run on an MI355X box: pytest tests/test_inpaint_ops_gpu.py -m gpu -q"""

import functools

import pytest
import torch

from distrifuser_amd.ops import eager

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32],
                                 ids=["bf16", "fp16", "fp32"])
SHAPES = pytest.mark.parametrize("shape", [
    (1, 4, 5, 7),  # plane 35: the element-wise path, odd everything
    (1, 4, 8, 8),  # plane 64: the vector path
    (1, 4, 8, 9),  # plane 72: vectors, and the mask index wraps mid-block
    (1, 4, 1, 8),  # one 16-bit vector per plane
], ids=lambda s: "x".join(map(str, s)))
NOISE_BATCH = pytest.mark.parametrize("nb", [2, 1], ids=["cfg-pair", "no-cfg"])
MASKS = pytest.mark.parametrize("soft", [False, True], ids=["binary", "soft"])

G, CA, CB, CC, CX, CE, SA, SB = 5.0, 0.97, -0.13, 0.21, 1.3, -0.7, 0.8, 0.6
EPS32 = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _case(shape, dtype, nb, soft=False):
    """Inputs on the GPU. Cached and shared between the tests: never modified."""
    gen = torch.Generator().manual_seed(sum(shape) * 7 + nb + 3 * soft)
    _, c, h, w = shape
    r = lambda *s: torch.randn(*s, generator=gen)
    mask = torch.rand(h * w, generator=gen)
    if not soft:
        mask = (mask >= 0.5).float()
        mask[0], mask[-1] = 0.0, 1.0  # both values occur
    d = {
        "noise": r(nb, c, h, w).to(dtype), "x": r(*shape).to(dtype),
        "x0_prev": r(*shape) * 3, "init": r(*shape), "init_noise": r(*shape),
        "mask": mask.reshape(1, 1, h, w),
    }
    return {k: v.to(DEV) for k, v in d.items()}


def _ulp(ref):
    """One unit in the last place of ref's dtype at |ref| (fp32 tensor)."""
    mant, emin = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}[ref.dtype]
    _, e = torch.frexp(ref.float().abs())  # |ref| = m * 2^e, m in [0.5, 1)
    return torch.exp2((e - 1).clamp_min(emin).float() - mant)


def _terms(c, nb, dpm, x0_prev):
    """The sum of the |terms| of the expression tree, fp32."""
    n = c["noise"].float().abs()
    eps = n if nb == 1 else n[:1] + G * (n[1:] + n[:1])
    xp = abs(CA) * c["x"].float().abs() + abs(CB) * eps
    if dpm and x0_prev:
        xp = xp + abs(CC) * c["x0_prev"].abs()
    known = SA * c["init"].abs() + SB * c["init_noise"].abs()
    return c["mask"] * xp + (1 - c["mask"]) * known


def _assert_close(got, ref, c, nb, dpm=False, x0_prev=False):
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert torch.isfinite(got.float()).all()
    diff = (got.float() - ref.float()).abs()
    tol = 4 * EPS32 * _terms(c, nb, dpm, x0_prev) if got.dtype == torch.float32 else _ulp(ref)
    bad = diff > tol
    print(f"max diff {diff.max().item():.3e}, differing {int((diff > 0).sum())}/{diff.numel()}")
    assert not bad.any(), (
        f"{int(bad.sum())} of {bad.numel()} beyond tolerance; worst diff "
        f"{diff[bad].max().item():.3e} vs tol {tol[bad].min().item():.3e}")


def _ext():
    from distrifuser_amd.ops.dispatch import hip_ext

    return hip_ext()


def _pair(c, nb):
    """The noise as a CFG pair: a batch-1 noise twice, which makes eps = noise
    exactly (nu + g * (nu - nu))."""
    return c["noise"] if nb == 2 else torch.cat([c["noise"]] * 2)


# ---- against the eager reference -----------------------------------------------------


@requires_gpu
@MASKS
@NOISE_BATCH
@SHAPES
@DTYPES
def test_masked_affine_step_matches_eager(dtype, shape, nb, soft):
    c = _case(shape, dtype, nb, soft)
    args = (c["noise"], c["x"], c["init"], c["init_noise"], c["mask"], G, CA, CB, SA, SB)
    got = _ext().masked_affine_step(*args)
    ref = eager.masked_affine_step(*args)
    torch.cuda.synchronize()
    _assert_close(got, ref, c, nb)


@requires_gpu
@pytest.mark.parametrize("with_prev", [False, True], ids=["first-order", "2M"])
@MASKS
@NOISE_BATCH
@SHAPES
@DTYPES
def test_masked_dpm_step_matches_eager(dtype, shape, nb, soft, with_prev):
    c = _case(shape, dtype, nb, soft)
    prev = c["x0_prev"] if with_prev else None
    args = (c["noise"], c["x"], prev, c["init"], c["init_noise"], c["mask"], G, CA, CB, CC, CX,
            CE, SA, SB)
    got, x0 = _ext().masked_dpm_step(*args)
    ref, x0_ref = eager.masked_dpm_step(*args)
    torch.cuda.synchronize()
    _assert_close(got, ref, c, nb, dpm=True, x0_prev=with_prev)
    assert x0.dtype == torch.float32
    n = c["noise"].float().abs()
    eps = n if nb == 1 else n[:1] + G * (n[1:] + n[:1])
    x0_tol = 4 * EPS32 * (abs(CX) * c["x"].float().abs() + abs(CE) * eps)
    assert ((x0 - x0_ref).abs() <= x0_tol).all()


# ---- exactness -----------------------------------------------------------------------


@requires_gpu
@NOISE_BATCH
@SHAPES
@DTYPES
def test_repainted_pixels_are_the_unmasked_step_bit_for_bit(dtype, shape, nb):
    c = _case(shape, dtype, nb)
    m = c["mask"].expand(shape) == 1
    assert m.any() and not m.all()
    ext = _ext()
    got = ext.masked_affine_step(c["noise"], c["x"], c["init"], c["init_noise"], c["mask"], G, CA,
                                 CB, SA, SB)
    plain = ext.cfg_affine_step(_pair(c, nb), c["x"], G, CA, CB)
    assert torch.equal(got[m], plain[m])
    assert not torch.equal(got[~m], plain[~m])
    for prev in (None, c["x0_prev"]):
        got, x0 = ext.masked_dpm_step(c["noise"], c["x"], prev, c["init"], c["init_noise"],
                                      c["mask"], G, CA, CB, CC, CX, CE, SA, SB)
        plain, x0_plain = ext.cfg_dpm_step(_pair(c, nb), c["x"], prev, G, CA, CB, CC, CX, CE)
        assert torch.equal(got[m], plain[m])
        assert not torch.equal(got[~m], plain[~m])
        assert torch.equal(x0, x0_plain)  # the multistep state is not blended


@requires_gpu
@NOISE_BATCH
@SHAPES
@DTYPES
def test_known_pixels_are_init_bit_for_bit_after_the_last_step(dtype, shape, nb):
    c = _case(shape, dtype, nb)
    m = c["mask"].expand(shape) == 0
    want = c["init"].to(dtype)
    ext = _ext()
    got = ext.masked_affine_step(c["noise"], c["x"], c["init"], c["init_noise"], c["mask"], G, CA,
                                 CB, 1.0, 0.0)
    assert torch.equal(got[m], want[m]) and not torch.equal(got[~m], want[~m])
    got, _ = ext.masked_dpm_step(c["noise"], c["x"], c["x0_prev"], c["init"], c["init_noise"],
                                 c["mask"], G, CA, CB, CC, CX, CE, 1.0, 0.0)
    assert torch.equal(got[m], want[m]) and not torch.equal(got[~m], want[~m])


@requires_gpu
@MASKS
@DTYPES
def test_dpm_state_is_the_unmasked_kernels_for_every_mask(dtype, soft):
    shape = (1, 4, 8, 9)
    c = _case(shape, dtype, 2, soft)
    ext = _ext()
    _, x0_plain = ext.cfg_dpm_step(c["noise"], c["x"], c["x0_prev"], G, CA, CB, CC, CX, CE)
    for mask in (c["mask"], torch.zeros_like(c["mask"]), torch.ones_like(c["mask"])):
        _, x0 = ext.masked_dpm_step(c["noise"], c["x"], c["x0_prev"], c["init"], c["init_noise"],
                                    mask, G, CA, CB, CC, CX, CE, SA, SB)
        assert torch.equal(x0, x0_plain)


# ---- U-Net input assembly ------------------------------------------------------------

EULER_SCALE = (14.6146 ** 2 + 1) ** 0.5  # Euler's first sigma


@requires_gpu
@pytest.mark.parametrize("copies", [1, 2])
@SHAPES
@DTYPES
def test_inpaint_unet_input(dtype, shape, copies):
    c = _case(shape, dtype, 2)
    lat = c["x"]
    mask = c["mask"].to(dtype)
    masked = c["init"].to(dtype)
    ext = _ext()
    got = ext.inpaint_unet_input(lat, mask, masked, 1.0, copies)
    want = torch.cat([torch.cat([lat] * copies), torch.cat([mask] * copies),
                      torch.cat([masked] * copies)], dim=1)
    assert got.shape == (copies, 9, *shape[2:]) and got.dtype == dtype and got.is_contiguous()
    assert torch.equal(got, want)

    got = ext.inpaint_unet_input(lat, mask, masked, EULER_SCALE, copies)
    ref = eager.inpaint_unet_input(lat, mask, masked, EULER_SCALE, copies)
    assert torch.equal(got[:, 4:], want[:, 4:])
    assert torch.equal(got[0], got[-1])
    if dtype == torch.float32:
        tol = 2 * EPS32 * ref[:, :4].abs()
    else:
        tol = _ulp(ref[:, :4])
    assert ((got[:, :4].float() - ref[:, :4].float()).abs() <= tol).all()
    assert not torch.equal(got[:, :4], want[:, :4])


# ---- dispatch ------------------------------------------------------------------------


@requires_gpu
def test_ops_reach_the_extension(monkeypatch):
    """ops.* with DFA_FORCE_EAGER unset calls the extension entry points, and
    with DFA_FORCE_EAGER=1 does not."""
    from distrifuser_amd import ops

    ext = _ext()
    calls = []

    def counted(name):
        real = getattr(ext, name)

        def f(*a, **kw):
            calls.append(name)
            return real(*a, **kw)

        monkeypatch.setattr(ext, name, f)

    for name in ("masked_affine_step", "masked_dpm_step", "inpaint_unet_input"):
        counted(name)
    c = _case((1, 4, 8, 8), torch.bfloat16, 2)
    lat_args = (c["x"], c["mask"].bfloat16(), c["init"].bfloat16(), 2.0, 2)

    def run():
        a = ops.masked_affine_step(c["noise"], c["x"], c["init"], c["init_noise"], c["mask"], G,
                                   CA, CB, SA, SB)
        b, x0 = ops.masked_dpm_step(c["noise"], c["x"], None, c["init"], c["init_noise"],
                                    c["mask"], G, CA, CB, CC, CX, CE, SA, SB)
        u = ops.inpaint_unet_input(*lat_args)
        return a, b, x0, u

    monkeypatch.delenv("DFA_FORCE_EAGER", raising=False)
    native = run()
    assert calls == ["masked_affine_step", "masked_dpm_step", "inpaint_unet_input"]
    monkeypatch.setenv("DFA_FORCE_EAGER", "1")
    forced = run()
    assert len(calls) == 3
    for a, b in zip(native, forced):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert (a.float() - b.float()).abs().max() <= 0.05 * b.float().abs().max()
