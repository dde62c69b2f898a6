"""v-prediction, trailing spacing and zero-terminal-SNR betas of the three
schedulers (CPU).

The golden-pinned epsilon schedulers are the oracle: with A = sqrt(acp_t),
S = sqrt(1 - acp_t) a v-prediction scheduler fed v = A*eps - S*x0 must take
the step the epsilon scheduler takes from (x, eps).

Tolerance. Both schedulers evaluate an affine form of the same inputs in
fp32; they differ in the rounding of every product and sum and in the
rounding of v itself (v is formed in float64 and rounded once to fp32). Each
of those is at most eps32 relative to its term, and a form has at most four
roundings stacked on a term, so the two results differ by at most
8 * eps32 * (sum of the |terms| of both forms), the derivation of
tests/test_inpaint_ops_gpu.py with both sides' terms counted."""

import numpy as np
import pytest
import torch

from distrifuser_amd.ops import eager
from distrifuser_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler,
                                        EulerDiscreteScheduler, get_scheduler)
from distrifuser_amd.schedulers.common import SchedulerBase

EPS32 = 2.0 ** -23
NAMES = pytest.mark.parametrize("name", ["ddim", "euler", "dpm-solver"])
SHAPE = (1, 4, 8, 8)
STEPS = 10


def _as(name, t, sched):
    """(A, S) with v = A*eps - S*x0 and (a, s) with x = a*x0 + s*eps at the
    step about to run, float64."""
    if name == "euler":
        sigma = float(sched.sigmas[sched._step_index])
        r = (sigma * sigma + 1.0) ** 0.5
        return 1.0 / r, sigma / r, 1.0, sigma
    acp = float(sched.alphas_cumprod[int(t)])
    return acp ** 0.5, (1 - acp) ** 0.5, acp ** 0.5, (1 - acp) ** 0.5


def _coeff_terms(sched, t, x, out, x0_prev):
    """Sum of the |terms| of sched's folded affine form at the step about to run."""
    c = sched._affine_coeffs(t)
    if isinstance(sched, DPMSolverMultistepScheduler):
        first, (ca, cb, cc, cx, ce) = c
        terms = abs(ca) * x.abs() + abs(cb) * out.abs()
        if not first:
            terms = terms + abs(cc) * x0_prev
        return terms, abs(cx) * x.abs() + abs(ce) * out.abs()
    ca, cb = c
    return abs(ca) * x.abs() + abs(cb) * out.abs(), None


@NAMES
def test_v_prediction_reproduces_the_epsilon_trajectory(name):
    gen = torch.Generator().manual_seed(11)
    eps_s = get_scheduler(name)
    v_s = get_scheduler(name, prediction_type="v_prediction")
    eps_s.set_timesteps(STEPS)
    v_s.set_timesteps(STEPS)
    assert torch.equal(eps_s.timesteps, v_s.timesteps)
    x = torch.randn(SHAPE, generator=gen) * eps_s.init_noise_sigma
    x0_terms = torch.zeros(SHAPE)  # |terms| of the multistep state, both forms
    worst = 0.0
    for t in eps_s.timesteps:
        eps = torch.randn(SHAPE, generator=gen)
        A, S, a, s = _as(name, t, eps_s)
        x0 = (x.double() - s * eps.double()) / a
        v = (A * eps.double() - S * x0).float()
        te, x0e = _coeff_terms(eps_s, t, x, eps, x0_terms)
        tv, x0v = _coeff_terms(v_s, t, x, v, x0_terms)
        want = eps_s.step(eps, t, x)
        got = v_s.step(v, t, x)
        assert got.dtype == torch.float32 and torch.isfinite(got).all()
        tol = 8 * EPS32 * (te + tv)
        diff = (got - want).abs()
        worst = max(worst, float((diff / tol).max()))
        assert (diff <= tol).all(), f"t={int(t)}: {float(diff.max()):.3e} vs {float(tol.min()):.3e}"
        if x0e is not None:
            x0_terms = x0e + x0v
        x = want
    print(f"{name}: worst diff / tol = {worst:.3f}")


def _pair(gen):
    return torch.randn(2, *SHAPE[1:], generator=gen)


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@NAMES
def test_folded_coefficients_equal_step(name, pred):
    """guided_step and masked_step on the GPU run ca*x + cb*out (+ cc*x0_prev)
    with the folded coefficients; here the same composition through the eager
    ops is held against step() (which the CPU guided_step / masked_step call),
    over a whole schedule so that the 2M steps of DPM-Solver++ are covered."""
    gen = torch.Generator().manual_seed(5)
    g = 6.0
    for masked in (False, True):
        ref = get_scheduler(name, prediction_type=pred)
        fold = get_scheduler(name, prediction_type=pred)
        ref.set_timesteps(6)
        fold.set_timesteps(6)
        x = torch.randn(SHAPE, generator=gen) * ref.init_noise_sigma
        init, init_noise = torch.randn(SHAPE, generator=gen), torch.randn(SHAPE, generator=gen)
        mask = (torch.rand(SHAPE[2] * SHAPE[3], generator=gen) > 0.5).float()
        for t in ref.timesteps:
            noise = _pair(gen)
            if masked:
                want = ref.masked_step(noise, t, x, g, mask, init, init_noise)
            else:
                want = ref.guided_step(noise, t, x, g)
            sa, sb = fold._known_coeffs(t)
            if name == "dpm-solver":
                first, co = fold._affine_coeffs(t)
                prev = None if first else fold._x0_prev
                if masked:
                    got, x0 = eager.masked_dpm_step(noise, x, prev, init, init_noise, mask, g,
                                                    *co, sa, sb)
                else:
                    got, x0 = eager.cfg_dpm_step(noise, x, prev, g, *co)
                fold._x0_prev, fold._t_prev = x0, int(t)
                fold._step_index += 1
                assert torch.allclose(x0, ref._x0_prev, rtol=1e-5, atol=1e-5)
            else:
                ca, cb = fold._affine_coeffs(t)
                if masked:
                    got = eager.masked_affine_step(noise, x, init, init_noise, mask, g, ca, cb,
                                                   sa, sb)
                else:
                    got = eager.cfg_affine_step(noise, x, g, ca, cb)
                if name == "euler":
                    fold._step_index += 1
            # fp32 on both sides: a few roundings of terms of the size of x and g*noise
            assert torch.allclose(got, want, rtol=2e-5, atol=2e-5 * float(x.abs().max())), (
                name, pred, masked, int(t), float((got - want).abs().max()))
            x = want


def test_prediction_type_is_validated():
    for bad in ("sample", "v", ""):
        with pytest.raises(ValueError):
            SchedulerBase(prediction_type=bad)
        with pytest.raises(ValueError):
            get_scheduler("ddim", prediction_type=bad)
    with pytest.raises(ValueError):
        SchedulerBase(timestep_spacing="linspace")
    assert get_scheduler("euler", prediction_type="v_prediction").prediction_type == "v_prediction"


# ---- zero terminal SNR ----------------------------------------------------------------


def test_zero_snr_schedule():
    base = SchedulerBase()
    z = SchedulerBase(rescale_betas_zero_snr=True)
    acp = z.alphas_cumprod
    assert acp[-1] == 0
    assert (acp[:-1] > 0).all()
    assert (acp[1:] < acp[:-1]).all()
    # Algorithm 1 keeps the first value; both are float64 results rounded to fp32
    assert abs(float(acp[0]) - float(base.alphas_cumprod[0])) <= 2.0 ** -24


def test_ddim_zero_snr_first_step_is_finite_and_exact():
    s = DDIMScheduler(prediction_type="v_prediction", timestep_spacing="trailing",
                      rescale_betas_zero_snr=True)
    s.set_timesteps(4)
    assert int(s.timesteps[0]) == 999
    gen = torch.Generator().manual_seed(2)
    x, v = torch.randn(SHAPE, generator=gen), torch.randn(SHAPE, generator=gen)
    got = s.step(v, s.timesteps[0], x)
    assert torch.isfinite(got).all()
    acp_prev = s.alphas_cumprod[999 - 250].double()
    want = acp_prev.sqrt() * (-v.double()) + (1 - acp_prev).sqrt() * x.double()
    assert torch.allclose(got.double(), want, rtol=0, atol=4 * EPS32 * float(want.abs().max()))
    ca, cb = s._affine_coeffs(s.timesteps[0])
    assert np.isfinite([ca, cb]).all()
    assert ca == pytest.approx(float((1 - acp_prev).sqrt()), rel=1e-12)
    assert cb == pytest.approx(-float(acp_prev.sqrt()), rel=1e-12)


def test_euler_and_dpm_stay_finite_with_zero_snr():
    e = EulerDiscreteScheduler(rescale_betas_zero_snr=True, timestep_spacing="trailing",
                               prediction_type="v_prediction")
    e.set_timesteps(4)
    assert torch.isfinite(e.sigmas).all() and np.isfinite(e._sigmas_train).all()
    assert float(e.sigmas[0]) == pytest.approx((2.0 ** 24 - 1) ** 0.5, rel=1e-6)
    d = DPMSolverMultistepScheduler(rescale_betas_zero_snr=True, timestep_spacing="trailing",
                                    prediction_type="v_prediction")
    assert torch.isfinite(d.lambda_t).all() and (d.alpha_t > 0).all()
    assert d.alphas_cumprod[-1] == 0  # add_noise keeps the true schedule
    for s in (e, d):
        s.set_timesteps(4)
        gen = torch.Generator().manual_seed(3)
        x = torch.randn(SHAPE, generator=gen) * s.init_noise_sigma
        for t in s.timesteps:
            x = s.step(torch.randn(SHAPE, generator=gen), t, x)
            assert torch.isfinite(x).all()


# ---- trailing spacing -------------------------------------------------------------------


@NAMES
def test_trailing_timesteps(name):
    s = get_scheduler(name, timestep_spacing="trailing")
    s.set_timesteps(4)
    assert s.timesteps.tolist() == [999, 749, 499, 249]
    for n in (1, 4, 50):
        s.set_timesteps(n)
        want = np.round(np.arange(1000, 0, -1000 / n)) - 1
        assert len(s.timesteps) == n
        assert s.timesteps.tolist() == want.tolist()
    s.set_timesteps(1)
    assert s.timesteps.tolist() == [999]


def test_ddim_trailing_previous_timestep_is_t_minus_ratio():
    s = DDIMScheduler(timestep_spacing="trailing")
    s.set_timesteps(4)
    a_t, a_p = s._alphas(499)
    assert a_t == s.alphas_cumprod[499] and a_p == s.alphas_cumprod[249]
    assert s._alphas(249)[1] == s.alphas_cumprod[0]  # 249 - 250 < 0


# ---- defaults ---------------------------------------------------------------------------


@NAMES
def test_defaults_are_todays_schedule(name):
    base = SchedulerBase()
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    assert torch.equal(base.alphas_cumprod, torch.cumprod(1.0 - betas, dim=0).float())
    s = get_scheduler(name)
    assert (s.prediction_type, s.timestep_spacing, s.rescale_betas_zero_snr) == (
        "epsilon", "leading", False)
    assert torch.equal(s.alphas_cumprod, base.alphas_cumprod)
    explicit = get_scheduler(name, prediction_type="epsilon", timestep_spacing="leading",
                             rescale_betas_zero_snr=False)
    for n in (4, 50):
        s.set_timesteps(n)
        explicit.set_timesteps(n)
        assert torch.equal(s.timesteps.long(), base._leading_timesteps(n))
        assert torch.equal(s.timesteps, explicit.timesteps)
