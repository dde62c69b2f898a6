"""guidance_rescale on the GPU: the factor kernels (cfg_moments_kernel,
cfg_rescale_finalize_kernel) against the float64 eager reference, their
determinism, and the RESCALE instantiations of the step kernels of
csrc/scheduler.hip against eager with the same factor tensor.

Factor tolerance. The kernels sum in fp32: a block tree over 8192-element
chunks, then the chunk rows in order, about 100 roundings of 2^-24 on a sum
in the worst case, 1e-5 relative rounded up. The variance is sum x^2 / n -
mean^2, whose condition number is 1 + mu^2 / sigma^2, so the factor (a ratio
of square roots of two such variances) is held to 1e-5 * (1 + mu^2 / sigma^2)
relative, with mu and sigma those of the inputs.

Step tolerance, as in tests/test_inpaint_ops_gpu.py: kernel and reference
compute the same tree in fp32 and differ in FMA contraction alone, at most
4 * eps32 * (sum of the |terms|) there; the product factor * eps adds one
rounding on the eps terms, so 5 * eps32 * (sum of the |terms|) bounds fp32,
and a 16-bit result is within one unit in the last place of T.

Run on an MI355X box: pytest tests/test_guidance_rescale_gpu.py -m gpu -q -s"""

import functools

import pytest
import torch

from distrifuser_amd.ops import eager
from distrifuser_amd.schedulers import get_scheduler

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32],
                                 ids=["bf16", "fp16", "fp32"])
EPS32 = 2.0 ** -23
G_F, PHI = 7.5, 0.7

# (C, h, w) of the [2,C,h,w] pair, and whether it is a view one element into its storage
FACTOR_CASES = pytest.mark.parametrize("chw,offset", [
    ((4, 5, 7), False),  # 140 elements: the element-wise path, under one block
    ((4, 32, 64), False),  # 8192: exactly one chunk
    ((4, 32, 64), True),  # 8192 unaligned: forces the element-wise path
    ((4, 1, 2049), False),  # 8196: one chunk and a 4-element tail block
    ((4, 96, 96), False),  # 36864: 4.5 chunks
], ids=["140", "8192", "8192-unaligned", "8196", "36864"])
DISTS = pytest.mark.parametrize("mean,std", [(0.0, 1.0), (3.0, 0.5)], ids=["n01", "offset"])


def _ext():
    from distrifuser_amd.ops.dispatch import hip_ext

    return hip_ext()


@functools.lru_cache(maxsize=None)
def _noise(chw, offset, dtype, mean=0.0, std=1.0):
    """The CFG pair on the GPU. Cached and shared: never modified."""
    gen = torch.Generator().manual_seed(sum(chw) + 31 * offset)
    n = 2 * chw[0] * chw[1] * chw[2]
    flat = (torch.randn(n + 1, generator=gen) * std + mean).to(dtype).to(DEV)
    pair = flat[1:] if offset else flat[:n]
    pair = pair.view(2, *chw)
    assert pair.is_contiguous() and (pair.data_ptr() % 16 != 0) == offset
    return pair


@requires_gpu
@DISTS
@FACTOR_CASES
@DTYPES
def test_factor_matches_the_float64_reference(dtype, chw, offset, mean, std):
    noise = _noise(chw, offset, dtype, mean, std)
    got = _ext().guidance_rescale_factor(noise, G_F, PHI)
    want = eager.guidance_rescale_factor(noise, G_F, PHI)
    assert got.dtype == torch.float32 and got.shape == (1,) and got.is_cuda
    rel = abs(float(got) - float(want)) / float(want)
    tol = 1e-5 * (1 + mean * mean / (std * std))
    print(f"factor {float(got):.7f} ref {float(want):.7f} rel {rel:.2e} tol {tol:.2e}")
    assert rel <= tol


@requires_gpu
@FACTOR_CASES
@DTYPES
def test_factor_is_deterministic(dtype, chw, offset):
    noise = _noise(chw, offset, dtype, 3.0, 0.5)
    ext = _ext()
    a = ext.guidance_rescale_factor(noise, G_F, PHI)
    b = ext.guidance_rescale_factor(noise, G_F, PHI)
    assert torch.equal(a, b)
    if offset:  # the same chunking and order as the 16-byte path of an aligned copy
        copy = noise.clone()
        assert copy.data_ptr() % 16 == 0
        assert torch.equal(ext.guidance_rescale_factor(copy, G_F, PHI), a)


@requires_gpu
def test_factor_degenerate_values():
    ext = _ext()
    noise = _noise((4, 32, 64), False, torch.float32)
    assert float(ext.guidance_rescale_factor(noise, G_F, 0.0)) == 1.0
    same = torch.cat([noise[:1], noise[:1]])
    assert float(ext.guidance_rescale_factor(same, 1.0, PHI)) == pytest.approx(1.0, abs=2e-7)
    with pytest.raises(RuntimeError):
        ext.guidance_rescale_factor(noise[:1], G_F, PHI)


# ---- the RESCALE step kernels -----------------------------------------------------------

SHAPES = pytest.mark.parametrize("shape", [
    (1, 4, 5, 7), (1, 4, 8, 8), (1, 4, 8, 9), (1, 4, 1, 8),  # tests/test_inpaint_ops_gpu.py
], ids=lambda s: "x".join(map(str, s)))
MASKED = pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
G, CA, CB, CC, CX, CE, SA, SB = 5.0, 0.97, -0.13, 0.21, 1.3, -0.7, 0.8, 0.6
FACTOR = 0.8125


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    gen = torch.Generator().manual_seed(sum(shape) * 7)
    _, c, h, w = shape
    r = lambda *s: torch.randn(*s, generator=gen)
    d = {
        "noise": r(2, c, h, w).to(dtype), "x": r(*shape).to(dtype), "x0_prev": r(*shape) * 3,
        "init": r(*shape), "init_noise": r(*shape),
        "mask": torch.rand(h * w, generator=gen).reshape(1, 1, h, w),
    }
    return {k: v.to(DEV) for k, v in d.items()}


def _ulp(ref):
    mant, emin = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}[ref.dtype]
    _, e = torch.frexp(ref.float().abs())
    return torch.exp2((e - 1).clamp_min(emin).float() - mant)


def _eps_terms(c, f):
    n = c["noise"].float().abs()
    return abs(f) * (n[:1] + G * (n[1:] + n[:1]))


def _assert_close(got, ref, terms):
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert torch.isfinite(got.float()).all()
    diff = (got.float() - ref.float()).abs()
    tol = 5 * EPS32 * terms if got.dtype == torch.float32 else _ulp(ref)
    print(f"max diff {diff.max().item():.3e}, differing {int((diff > 0).sum())}/{diff.numel()}")
    assert (diff <= tol).all()


def _affine(mod, c, masked, factor):
    tail = () if factor is None else (factor,)
    if masked:
        return mod.masked_affine_step(c["noise"], c["x"], c["init"], c["init_noise"], c["mask"],
                                      G, CA, CB, SA, SB, *tail)
    return mod.cfg_affine_step(c["noise"], c["x"], G, CA, CB, *tail)


def _dpm(mod, c, masked, prev, factor):
    tail = () if factor is None else (factor,)
    if masked:
        return mod.masked_dpm_step(c["noise"], c["x"], prev, c["init"], c["init_noise"],
                                   c["mask"], G, CA, CB, CC, CX, CE, SA, SB, *tail)
    return mod.cfg_dpm_step(c["noise"], c["x"], prev, G, CA, CB, CC, CX, CE, *tail)


def _blend_terms(c, xp_terms, masked):
    if not masked:
        return xp_terms
    known = SA * c["init"].abs() + SB * c["init_noise"].abs()
    return c["mask"] * xp_terms + (1 - c["mask"]) * known


@requires_gpu
@MASKED
@SHAPES
@DTYPES
def test_rescaled_affine_step_matches_eager(dtype, shape, masked):
    c = _case(shape, dtype)
    factor = torch.full((1,), FACTOR, device=DEV)
    got = _affine(_ext(), c, masked, factor)
    ref = _affine(eager, c, masked, factor)
    assert not torch.equal(got, _affine(_ext(), c, masked, None))
    xp = abs(CA) * c["x"].float().abs() + abs(CB) * _eps_terms(c, FACTOR)
    _assert_close(got, ref, _blend_terms(c, xp, masked))


@requires_gpu
@pytest.mark.parametrize("with_prev", [False, True], ids=["first-order", "2M"])
@MASKED
@SHAPES
@DTYPES
def test_rescaled_dpm_step_matches_eager(dtype, shape, masked, with_prev):
    c = _case(shape, dtype)
    prev = c["x0_prev"] if with_prev else None
    factor = torch.full((1,), FACTOR, device=DEV)
    got, x0 = _dpm(_ext(), c, masked, prev, factor)
    ref, x0_ref = _dpm(eager, c, masked, prev, factor)
    eps = _eps_terms(c, FACTOR)
    xp = abs(CA) * c["x"].float().abs() + abs(CB) * eps
    if with_prev:
        xp = xp + abs(CC) * c["x0_prev"].abs()
    _assert_close(got, ref, _blend_terms(c, xp, masked))
    assert x0.dtype == torch.float32
    x0_tol = 5 * EPS32 * (abs(CX) * c["x"].float().abs() + abs(CE) * eps)
    assert ((x0 - x0_ref).abs() <= x0_tol).all()


@requires_gpu
@MASKED
@SHAPES
@DTYPES
def test_a_factor_of_one_is_the_plain_step_bit_for_bit(dtype, shape, masked):
    c = _case(shape, dtype)
    ext = _ext()
    one = torch.ones(1, device=DEV)
    assert torch.equal(_affine(ext, c, masked, one), _affine(ext, c, masked, None))
    for prev in (None, c["x0_prev"]):
        got, x0 = _dpm(ext, c, masked, prev, one)
        plain, x0_plain = _dpm(ext, c, masked, prev, None)
        assert torch.equal(got, plain) and torch.equal(x0, x0_plain)


@requires_gpu
def test_a_factor_needs_the_cfg_pair():
    c = _case((1, 4, 8, 8), torch.bfloat16)
    ext = _ext()
    one = torch.ones(1, device=DEV)
    with pytest.raises(RuntimeError):  # batch-1 noise: nothing to rescale towards
        ext.masked_affine_step(c["noise"][:1], c["x"], c["init"], c["init_noise"], c["mask"], G,
                               CA, CB, SA, SB, one)
    with pytest.raises(RuntimeError):
        ext.masked_dpm_step(c["noise"][:1], c["x"], None, c["init"], c["init_noise"], c["mask"],
                            G, CA, CB, CC, CX, CE, SA, SB, one)
    with pytest.raises(RuntimeError):  # the factor lives on the GPU, one fp32
        ext.cfg_affine_step(c["noise"], c["x"], G, CA, CB, torch.ones(1))
    with pytest.raises(RuntimeError):
        ext.cfg_dpm_step(c["noise"], c["x"], None, G, CA, CB, CC, CX, CE,
                         torch.ones(2, device=DEV))


# ---- scheduler level --------------------------------------------------------------------


def _step_terms(name, co, x, v, x0_prev):
    """(folded, unfolded, x0): the sums of the |terms| of the kernel's folded
    form ca*x + cb*v (+ cc*x0_prev), of step()'s own expression, and of the
    DPM-Solver++ state x0 (None elsewhere). The unfolded coefficients are
    bounded from the folded ones: DDIM's Ap*A + Sp*S and Ap*S + Sp*A are at
    most 1, Euler's |dt|*s/(s^2+1) and |dt|/sqrt(s^2+1) are at most 1 next to
    the leading x, and DPM's C' = -cb/ce, s_p/s_t = ca + C'*cx."""
    if name == "dpm-solver":
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
    return abs(ca) * x + abs(cb) * v, (2 if name == "euler" else 1) * x + v, None


@requires_gpu
@MASKED
@pytest.mark.parametrize("name", ["ddim", "euler", "dpm-solver"])
@DTYPES
def test_three_rescaled_v_prediction_steps_match_the_eager_composition(dtype, name, masked,
                                                                       monkeypatch):
    """Three consecutive steps with guidance_rescale=0.7 and v-prediction: the
    native scheduler (factor op, then the RESCALE step with folded
    coefficients) against the same scheduler under DFA_FORCE_EAGER=1, which
    composes the float64 factor, step() and add_noise. Both are fed the native
    trajectory's sample and 2M state, so the per-step bound holds at each of
    the three steps (the state itself is held to its own bound first).

    Per step: the two expression trees differ (folded and not), at most
    8 * eps32 * (sum of the |terms| of both), as in
    tests/test_vpred_schedulers.py; the two factors differ by at most 1e-5
    relative for these N(0,1) inputs (2e-5 taken), which moves the eps term;
    and a 16-bit result may then round to the neighbouring value."""
    shape = (1, 4, 8, 9)
    g, phi = 6.0, 0.7
    gen = torch.Generator().manual_seed(17)
    native, ref, coef = (get_scheduler(name, prediction_type="v_prediction") for _ in range(3))
    for s in (native, ref, coef):
        s.set_timesteps(6)
    x = (torch.randn(shape, generator=gen) * native.init_noise_sigma).to(dtype).to(DEV)
    init = torch.randn(shape, generator=gen).to(DEV)
    init_noise = torch.randn(shape, generator=gen).to(DEV)
    mask = (torch.rand(1, 1, *shape[2:], generator=gen) > 0.5).float().to(DEV)
    calls = []
    ext = _ext()
    for op in ("guidance_rescale_factor", "cfg_affine_step", "cfg_dpm_step",
               "masked_affine_step", "masked_dpm_step"):
        real = getattr(ext, op)

        def counted(*a, _real=real, _op=op, **kw):
            calls.append(_op)
            return _real(*a, **kw)

        monkeypatch.setattr(ext, op, counted)
    step_op = ("masked_" if masked else "cfg_") + ("dpm" if name == "dpm-solver" else "affine")

    def step(s, noise, t, sample):
        if masked:
            return s.masked_step(noise, t, sample, g, mask, init, init_noise,
                                 guidance_rescale=phi)
        return s.guided_step(noise, t, sample, g, guidance_rescale=phi)

    for i, t in enumerate(native.timesteps[:3]):
        noise = torch.randn(2, *shape[1:], generator=gen).to(dtype).to(DEV)
        x0_prev = native._x0_prev if name == "dpm-solver" else None
        co = coef._affine_coeffs(t)  # before any scheduler moves on
        monkeypatch.delenv("DFA_FORCE_EAGER", raising=False)
        del calls[:]
        got = step(native, noise, t, x)
        assert calls == ["guidance_rescale_factor", step_op + "_step"]
        monkeypatch.setenv("DFA_FORCE_EAGER", "1")
        want = step(ref, noise, t, x)
        assert len(calls) == 2  # the eager composition reaches no kernel

        n = noise.float().abs()
        f = float(eager.guidance_rescale_factor(noise, g, phi))
        v = abs(f) * (n[:1] + g * (n[1:] + n[:1]))
        folded, unfolded, x0_terms = _step_terms(
            name, co, x.float().abs(), v, None if x0_prev is None else x0_prev.abs())
        cb = co[1][1] if name == "dpm-solver" else co[1]
        known = init.abs() + native.init_noise_sigma * init_noise.abs() if masked else 0
        tol = 8 * EPS32 * (folded + unfolded + known) + 2e-5 * abs(cb) * v
        if dtype != torch.float32:
            tol = tol + _ulp(want)
        diff = (got.float() - want.float()).abs()
        print(f"step {i}: max diff {diff.max().item():.3e}, worst diff/tol "
              f"{(diff / tol).max().item():.3f}")
        assert got.dtype == dtype and torch.isfinite(got.float()).all()
        assert (diff <= tol).all()
        if name == "dpm-solver":
            ce = co[1][4]
            x0_tol = 8 * EPS32 * 2 * x0_terms + 2e-5 * abs(ce) * v
            assert ((native._x0_prev - ref._x0_prev).abs() <= x0_tol).all()
            ref._x0_prev = native._x0_prev  # both go on from the native state
            coef._x0_prev, coef._t_prev = native._x0_prev, int(t)
        if hasattr(coef, "_step_index"):
            coef._step_index += 1
        x = got
