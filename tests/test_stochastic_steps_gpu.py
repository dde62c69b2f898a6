"""The stochastic samplers on the GPU: the native Philox normal op against its
eager twin, and the NOISE instantiations of the step kernels of
csrc/scheduler.hip against ops.eager with the same (cn, seed, draw).

Z_TOL (tests/test_philox.py): an fp32 evaluation of the Box-Muller rule is
within about 3e-6 of the float64 rule, so the kernel's normals and the eager
twin's (torch's fp32 log / sqrt / sin / cos on the device) are within 1e-5 of
each other.

Step tolerance: the rule of tests/test_guidance_rescale_gpu.py with the noise
term among the terms. Kernel and reference compute the same tree in fp32 and
differ in FMA contraction alone, 5 * eps32 * (sum of the |terms|, |cn| * |z|
included), and in z itself, |cn| * Z_TOL; a 16-bit result is within one unit in
the last place of T.

Run on an MI355X box: pytest tests/test_stochastic_steps_gpu.py -m gpu -q -s"""

import functools
import math

import pytest
import torch

from distrifuser_amd import ops
from distrifuser_amd.ops import eager
from distrifuser_amd.schedulers import get_scheduler

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32],
                                 ids=["bf16", "fp16", "fp32"])
SHAPE_LIST = [(1, 4, 5, 7), (1, 4, 8, 8), (1, 4, 8, 9), (1, 4, 1, 8)]  # test_inpaint_ops_gpu.py
SHAPES = pytest.mark.parametrize("shape", SHAPE_LIST, ids=lambda s: "x".join(map(str, s)))
MASKED = pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
# the model output: the CFG pair, the pair with a guidance_rescale factor, one branch
BRANCHES = pytest.mark.parametrize("branches", ["pair", "pair-factor", "single"])
EPS32 = 2.0 ** -23
Z_TOL = 1e-5
G, CA, CB, CC, CX, CE, SA, SB = 5.0, 0.97, -0.13, 0.21, 1.3, -0.7, 0.8, 0.6
FACTOR = 0.8125
CN, SEED, DRAW = 0.37, (0xC0FFEE << 32) | 0x1234567, 6
NOISE = (CN, SEED, DRAW)


def _ext():
    from distrifuser_amd.ops.dispatch import hip_ext

    return hip_ext()


# ---- the generator ---------------------------------------------------------------------


@requires_gpu
@pytest.mark.parametrize("n", [1, 141, 65536])
def test_philox_normal_matches_the_eager_twin(n):
    got = ops.philox_normal(n, 233, 3, device=DEV)
    want = eager.philox_normal(n, 233, 3)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (n,)
    diff = (got.cpu() - want).abs().max().item()
    print(f"n={n}: max |native - eager| = {diff:.3e}")
    assert diff <= Z_TOL
    assert torch.equal(got, _ext().philox_normal(n, 233, 3, 0, 0))  # the same bits every run
    if n == 65536:
        mean, std = got.double().mean().item(), got.double().std().item()
        print(f"mean {mean:.5f} std {std:.5f}")
        assert abs(mean) < 4 / math.sqrt(n) and abs(std - 1) < 4 / math.sqrt(2 * n)
        assert got.abs().max().item() <= math.sqrt(48 * math.log(2))
        for other in ((233, 4), (234, 3)):
            assert (ops.philox_normal(n, *other, device=DEV) != got).float().mean() > 0.99


@requires_gpu
def test_philox_normal_offset():
    whole = ops.philox_normal(160, 99, 2, device=DEV)
    for k in (0, 1, 2, 3, 4, 7, 141):
        for n in (1, 5, 16):
            assert torch.equal(ops.philox_normal(n, 99, 2, offset=k, device=DEV), whole[k:k + n])
    off = 1 << 34  # block 2^32: the high counter word
    got = ops.philox_normal(8, 233, 0, offset=off, device=DEV)
    assert (got.cpu() - eager.philox_normal(8, 233, 0, offset=off)).abs().max() <= Z_TOL
    assert not torch.equal(got, ops.philox_normal(8, 233, 0, device=DEV))
    across = ops.philox_normal(8, 233, 0, offset=off - 4, device=DEV)
    assert torch.equal(across[4:], got[:4])
    assert (across.cpu() - eager.philox_normal(8, 233, 0, offset=off - 4)).abs().max() <= Z_TOL
    assert ops.philox_normal(0, 1, 1, device=DEV).shape == (0,)
    with pytest.raises((RuntimeError, TypeError)):
        _ext().philox_normal(4, 1, 1, -1, 0)


# ---- the NOISE step kernels ------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """Inputs on the GPU. Cached and shared: never modified."""
    gen = torch.Generator().manual_seed(sum(shape) * 7)
    _, c, h, w = shape
    r = lambda *s: torch.randn(*s, generator=gen)
    d = {
        "noise": r(2, c, h, w).to(dtype), "x": r(*shape).to(dtype), "x0_prev": r(*shape) * 3,
        "init": r(*shape), "init_noise": r(*shape),
        "mask": torch.rand(h * w, generator=gen).reshape(1, 1, h, w),
    }
    return {k: v.to(DEV) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _z(shape):
    """|z| of NOISE for a sample of this shape, from the eager twin."""
    return eager.philox_normal(math.prod(shape), SEED, DRAW, device=DEV).reshape(shape).abs()


def _ulp(ref):
    mant, emin = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}[ref.dtype]
    _, e = torch.frexp(ref.float().abs())
    return torch.exp2((e - 1).clamp_min(emin).float() - mant)


def _model_output(c, branches):
    return c["noise"][1:] if branches == "single" else c["noise"]


def _factor(branches):
    return torch.full((1,), FACTOR, device=DEV) if branches == "pair-factor" else None


def _eps_terms(c, branches):
    n = c["noise"].float().abs()
    if branches == "single":
        return n[1:]
    return (FACTOR if branches == "pair-factor" else 1.0) * (n[:1] + G * (n[1:] + n[:1]))


def _affine(mod, c, masked, branches, step_noise, mask=None, sa=SA, sb=SB):
    out, f = _model_output(c, branches), _factor(branches)
    if masked:
        return mod.masked_affine_step(out, c["x"], c["init"], c["init_noise"],
                                      c["mask"] if mask is None else mask, G, CA, CB, sa, sb, f,
                                      step_noise)
    return mod.cfg_affine_step(out, c["x"], G, CA, CB, f, step_noise)


def _dpm(mod, c, masked, branches, prev, step_noise, mask=None, sa=SA, sb=SB):
    out, f = _model_output(c, branches), _factor(branches)
    if masked:
        return mod.masked_dpm_step(out, c["x"], prev, c["init"], c["init_noise"],
                                   c["mask"] if mask is None else mask, G, CA, CB, CC, CX, CE,
                                   sa, sb, f, step_noise)
    return mod.cfg_dpm_step(out, c["x"], prev, G, CA, CB, CC, CX, CE, f, step_noise)


def _blend_terms(c, xp_terms, masked):
    if not masked:
        return xp_terms
    known = SA * c["init"].abs() + SB * c["init_noise"].abs()
    return c["mask"] * xp_terms + (1 - c["mask"]) * known


def _assert_close(got, ref, terms, cn_weight):
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert torch.isfinite(got.float()).all()
    diff = (got.float() - ref.float()).abs()
    if got.dtype == torch.float32:
        tol = 5 * EPS32 * terms + abs(CN) * Z_TOL * cn_weight
    else:
        tol = _ulp(ref)
    print(f"max diff {diff.max().item():.3e}, differing {int((diff > 0).sum())}/{diff.numel()}")
    assert (diff <= tol).all()


@requires_gpu
@SHAPES
def test_the_noise_term_alone_is_philox_normal_bit_for_bit(shape):
    """ca = cb = 0, x = 0, model output 0 and cn = 1 leave z itself: every path
    (16-byte and element-wise, plain and masked, pair and one branch, both
    kernels, every dtype) draws the element-indexed stream of the op."""
    n = math.prod(shape)
    want = ops.philox_normal(n, SEED, DRAW, device=DEV).reshape(shape)
    # the stream does not depend on the element count: 256 and 140 elements
    assert torch.equal(ops.philox_normal(256, SEED, DRAW, device=DEV)[:140],
                       ops.philox_normal(140, SEED, DRAW, device=DEV))
    assert torch.equal(want.reshape(-1)[:32], ops.philox_normal(32, SEED, DRAW, device=DEV))
    ones = torch.ones(shape[2] * shape[3], device=DEV)
    zeros = torch.zeros(shape, device=DEV)
    step_noise = (1.0, SEED, DRAW)
    ext = _ext()
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        x = torch.zeros(shape, device=DEV, dtype=dtype)
        for out in (torch.zeros(2, *shape[1:], device=DEV, dtype=dtype), x):
            results = [
                ext.cfg_affine_step(out, x, G, 0.0, 0.0, None, step_noise),
                ext.masked_affine_step(out, x, zeros, zeros, ones, G, 0.0, 0.0, SA, SB, None,
                                       step_noise),
                ext.cfg_dpm_step(out, x, None, G, 0.0, 0.0, CC, CX, CE, None, step_noise)[0],
                ext.masked_dpm_step(out, x, None, zeros, zeros, ones, G, 0.0, 0.0, CC, CX, CE,
                                    SA, SB, None, step_noise)[0],
            ]
            for got in results:
                assert got.dtype == dtype and torch.equal(got, want.to(dtype))


@requires_gpu
@BRANCHES
@MASKED
@SHAPES
@DTYPES
def test_noisy_affine_step_matches_eager(dtype, shape, masked, branches):
    c = _case(shape, dtype)
    got = _affine(_ext(), c, masked, branches, NOISE)
    ref = _affine(eager, c, masked, branches, NOISE)
    xp = (abs(CA) * c["x"].float().abs() + abs(CB) * _eps_terms(c, branches)
          + abs(CN) * _z(shape))
    _assert_close(got, ref, _blend_terms(c, xp, masked), c["mask"] if masked else 1.0)
    if branches != "single" or masked:  # the noise is there, and cn = 0 is the plain call
        plain = _affine(_ext(), c, masked, branches, None)
        assert not torch.equal(got, plain)
        assert torch.equal(_affine(_ext(), c, masked, branches, (0.0, SEED, DRAW)), plain)


@requires_gpu
@pytest.mark.parametrize("with_prev", [False, True], ids=["first-order", "2M"])
@BRANCHES
@MASKED
@SHAPES
@DTYPES
def test_noisy_dpm_step_matches_eager(dtype, shape, masked, branches, with_prev):
    c = _case(shape, dtype)
    prev = c["x0_prev"] if with_prev else None
    got, x0 = _dpm(_ext(), c, masked, branches, prev, NOISE)
    ref, x0_ref = _dpm(eager, c, masked, branches, prev, NOISE)
    eps = _eps_terms(c, branches)
    xp = abs(CA) * c["x"].float().abs() + abs(CB) * eps + abs(CN) * _z(shape)
    if with_prev:
        xp = xp + abs(CC) * c["x0_prev"].abs()
    _assert_close(got, ref, _blend_terms(c, xp, masked), c["mask"] if masked else 1.0)
    assert x0.dtype == torch.float32
    x0_tol = 5 * EPS32 * (abs(CX) * c["x"].float().abs() + abs(CE) * eps)
    assert ((x0 - x0_ref).abs() <= x0_tol).all()
    if branches != "single" or masked:
        plain, x0_plain = _dpm(_ext(), c, masked, branches, prev, None)
        assert torch.equal(x0, x0_plain)  # x0 never sees the noise
        assert not torch.equal(got, plain)
        zero, x0_zero = _dpm(_ext(), c, masked, branches, prev, (0.0, SEED, DRAW))
        assert torch.equal(zero, plain) and torch.equal(x0_zero, x0_plain)


@requires_gpu
@BRANCHES
@SHAPES
@DTYPES
def test_mask_of_one_and_mask_of_zero(dtype, shape, branches):
    c = _case(shape, dtype)
    ext = _ext()
    ones = torch.ones(shape[2] * shape[3], device=DEV)
    zeros = torch.zeros_like(ones)
    known = c["init"].to(dtype)  # sa = 1, sb = 0
    assert torch.equal(_affine(ext, c, True, branches, NOISE, ones),
                       _affine(ext, c, False, branches, NOISE))
    assert torch.equal(_affine(ext, c, True, branches, NOISE, zeros, 1.0, 0.0), known)
    for prev in (None, c["x0_prev"]):
        unmasked, x0 = _dpm(ext, c, False, branches, prev, NOISE)
        got, x0_m = _dpm(ext, c, True, branches, prev, NOISE, ones)
        assert torch.equal(got, unmasked) and torch.equal(x0_m, x0)
        got, x0_m = _dpm(ext, c, True, branches, prev, NOISE, zeros, 1.0, 0.0)
        assert torch.equal(got, known) and torch.equal(x0_m, x0)
    if branches == "single":
        # cn = 0 without a pair and without a blend has no plain instantiation:
        # it adds 0 * z and must still be the masked single-branch plain step
        assert torch.equal(_affine(ext, c, False, branches, (0.0, SEED, DRAW)),
                           _affine(ext, c, True, branches, None, ones))


@requires_gpu
def test_noise_needs_one_sample_and_a_known_output_shape():
    c = _case((1, 4, 8, 8), torch.bfloat16)
    ext = _ext()
    two = torch.cat([c["x"], c["x"]])
    with pytest.raises(RuntimeError):  # the noise is indexed inside one sample
        ext.cfg_affine_step(torch.cat([c["noise"], c["noise"]]), two, G, CA, CB, None, NOISE)
    with pytest.raises(RuntimeError):
        ext.cfg_dpm_step(two, two, None, G, CA, CB, CC, CX, CE, None, NOISE)
    with pytest.raises(RuntimeError):  # one branch without noise: no such plain kernel
        ext.cfg_affine_step(c["noise"][:1], c["x"], G, CA, CB)
    with pytest.raises(RuntimeError):
        ext.cfg_dpm_step(c["noise"][:1], c["x"], None, G, CA, CB, CC, CX, CE)
    with pytest.raises(RuntimeError):  # a factor still needs the pair
        ext.cfg_affine_step(c["noise"][:1], c["x"], G, CA, CB, torch.ones(1, device=DEV), NOISE)
    with pytest.raises(ValueError):
        eager.cfg_affine_step(torch.cat([c["noise"], c["noise"]]), two, G, CA, CB, None, NOISE)


# ---- scheduler level --------------------------------------------------------------------

SAMPLERS = {
    "euler-a": ("euler-a", {}),
    "ddim-eta": ("ddim", {"eta": 0.8}),
    "dpm-sde": ("dpm-solver", {"algorithm_type": "sde-dpmsolver++"}),
}


def _step_terms(sampler, co, x, v, x0_prev):
    """tests/test_guidance_rescale_gpu.py::_step_terms: (folded, unfolded, x0)
    sums of |terms|. Its bounds on the unfolded coefficients hold here too:
    DDIM's direction coefficient only shrinks with eta, Euler's |dt| only
    shrinks with sigma_down <= sigma_next, and DPM's C' = -cb/ce and
    lead = ca + C'*cx are the same algebra with the SDE values."""
    if sampler == "dpm-sde":
        first, (ca, cb, cc, cx, ce) = co
        x0 = abs(cx) * x + abs(ce) * v
        cprime = -cb / ce
        folded = abs(ca) * x + abs(cb) * v
        unfolded = abs(ca + cprime * cx) * x + abs(cprime) * x0
        if not first:
            folded = folded + abs(cc) * x0_prev
            unfolded = unfolded + 2 * abs(cc) * x0_prev + abs(cc) * x0
        return folded, unfolded, x0
    ca, cb = co
    return abs(ca) * x + abs(cb) * v, (2 if sampler == "euler-a" else 1) * x + v, None


@requires_gpu
@pytest.mark.parametrize("mode", ["step", "guided", "masked", "guided-rescale", "masked-rescale"])
@pytest.mark.parametrize("sampler", list(SAMPLERS))
@DTYPES
def test_three_noisy_steps_match_the_eager_composition(dtype, sampler, mode, monkeypatch):
    """Three consecutive steps of each sampler: the native scheduler (one fused
    launch with folded coefficients and in-kernel noise; the factor op in
    front of it with guidance_rescale) against the same scheduler under
    DFA_FORCE_EAGER=1, which composes step(), eager.philox_normal and add_noise
    in fp32. The pattern and the bound of
    test_three_rescaled_v_prediction_steps_match_the_eager_composition, with
    the noise term among the |terms| and |cn| * Z_TOL for z itself."""
    shape = (1, 4, 8, 9)
    g, seed = 6.0, (7 << 40) | 99
    phi = 0.7 if mode.endswith("rescale") else 0.0
    masked, single = mode.startswith("masked"), mode == "step"
    name, extra = SAMPLERS[sampler]
    pred = "v_prediction"  # _step_terms bounds the unfolded v-prediction coefficients
    gen = torch.Generator().manual_seed(17)
    native, ref, coef = (get_scheduler(name, prediction_type=pred, **extra) for _ in range(3))
    for s in (native, ref, coef):
        s.set_noise_seed(seed)
        s.set_timesteps(6)
    x = (torch.randn(shape, generator=gen) * native.init_noise_sigma).to(dtype).to(DEV)
    init = torch.randn(shape, generator=gen).to(DEV)
    init_noise = torch.randn(shape, generator=gen).to(DEV)
    mask = (torch.rand(1, 1, *shape[2:], generator=gen) > 0.5).float().to(DEV)
    calls = []
    ext = _ext()
    for op in ("guidance_rescale_factor", "philox_normal", "cfg_affine_step", "cfg_dpm_step",
               "masked_affine_step", "masked_dpm_step"):
        real = getattr(ext, op)

        def counted(*a, _real=real, _op=op, **kw):
            calls.append(_op)
            return _real(*a, **kw)

        monkeypatch.setattr(ext, op, counted)
    step_op = ("masked_" if masked else "cfg_") + ("dpm" if sampler == "dpm-sde" else "affine")
    want_calls = (["guidance_rescale_factor"] if phi else []) + [step_op + "_step"]

    def step(s, noise, t, sample):
        kw = {"guidance_rescale": phi} if phi else {}
        if masked:
            return s.masked_step(noise, t, sample, g, mask, init, init_noise, **kw)
        if single:
            return s.step(noise, t, sample)
        return s.guided_step(noise, t, sample, g, **kw)

    for i, t in enumerate(native.timesteps[:3]):
        noise = torch.randn(1 if single else 2, *shape[1:], generator=gen).to(dtype).to(DEV)
        x0_prev = native._x0_prev if sampler == "dpm-sde" else None
        co = coef._affine_coeffs(t)  # before any scheduler moves on
        cn = coef._target_sigma()[1] if sampler == "euler-a" else coef._noise_coeff(t)
        assert cn > 0
        monkeypatch.delenv("DFA_FORCE_EAGER", raising=False)
        del calls[:]
        got = step(native, noise, t, x)
        assert calls == want_calls  # the noise costs no launch of its own
        monkeypatch.setenv("DFA_FORCE_EAGER", "1")
        want = step(ref, noise, t, x)
        assert calls == want_calls  # the eager composition reaches no kernel
        assert native._draw == ref._draw == i + 1

        n = noise.float().abs()
        if single:
            v = n
        else:
            f = float(eager.guidance_rescale_factor(noise, g, phi)) if phi else 1.0
            v = abs(f) * (n[:1] + g * (n[1:] + n[:1]))
        z = eager.philox_normal(math.prod(shape), seed, i, device=DEV).reshape(shape).abs()
        folded, unfolded, x0_terms = _step_terms(
            sampler, co, x.float().abs(), v, None if x0_prev is None else x0_prev.abs())
        cb = co[1][1] if sampler == "dpm-sde" else co[1]
        known = init.abs() + native.init_noise_sigma * init_noise.abs() if masked else 0
        tol = 8 * EPS32 * (folded + unfolded + 2 * cn * z + known) + cn * Z_TOL
        if phi:
            tol = tol + 2e-5 * abs(cb) * v
        if dtype != torch.float32:
            tol = tol + _ulp(want)
        diff = (got.float() - want.float()).abs()
        print(f"step {i}: cn {cn:.4f}, max diff {diff.max().item():.3e}, worst diff/tol "
              f"{(diff / tol).max().item():.3f}")
        assert got.dtype == dtype and torch.isfinite(got.float()).all()
        assert (diff <= tol).all()
        if sampler == "dpm-sde":
            ce = co[1][4]
            x0_tol = 8 * EPS32 * 2 * x0_terms + (2e-5 * abs(ce) * v if phi else 0)
            assert ((native._x0_prev - ref._x0_prev).abs() <= x0_tol).all()
            ref._x0_prev = native._x0_prev  # both go on from the native state
            coef._x0_prev, coef._t_prev = native._x0_prev, int(t)
        if hasattr(coef, "_step_index"):
            coef._step_index += 1
        x = got


@requires_gpu
@pytest.mark.parametrize("sampler", list(SAMPLERS))
@pytest.mark.parametrize("do_cfg", [True, False], ids=["cfg", "nocfg"])
def test_tiny_pipeline_on_the_device(do_cfg, sampler, monkeypatch):
    from distrifuser_amd import DistriConfig, DistriSDXLPipeline

    monkeypatch.delenv("DFA_FORCE_EAGER", raising=False)
    name, extra = SAMPLERS[sampler]
    cfg = DistriConfig(height=64, width=64, use_cuda_graph=False, device=DEV,
                       do_classifier_free_guidance=do_cfg)
    torch.manual_seed(0)
    pipe = DistriSDXLPipeline.from_pretrained(cfg, preset="tiny", torch_dtype=torch.bfloat16,
                                              scheduler=name, **extra)
    pipe.scheduler.set_timesteps(4)  # Euler's init_noise_sigma, before the first call
    ext = _ext()
    counts = {}
    for op in ("cfg_affine_step", "cfg_dpm_step"):
        real = getattr(ext, op)

        def counted(*a, _real=real, _op=op, **kw):
            counts[_op] = counts.get(_op, 0) + 1
            return _real(*a, **kw)

        monkeypatch.setattr(ext, op, counted)

    def run(seed):
        counts.clear()
        out = pipe("a prompt", num_inference_steps=4, output_type="latent",
                   generator=torch.Generator().manual_seed(seed),
                   **({} if do_cfg else {"guidance_scale": 1}))
        assert out.dtype == torch.bfloat16 and torch.isfinite(out.float()).all()
        # one fused launch per step, with and without the CFG pair
        assert counts == {"cfg_dpm_step" if sampler == "dpm-sde" else "cfg_affine_step": 4}
        return out

    a = run(3)
    assert torch.equal(a, run(3))
    assert not torch.equal(a, run(4))
