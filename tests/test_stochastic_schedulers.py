"""The stochastic samplers on the CPU: Euler ancestral, DDIM with eta > 0 and
DPM-Solver++ 2M SDE against an independent float64 transcription of their
formulas, with the noise of ops.eager.philox_normal.

Tolerance, built as in tests/test_vpred_schedulers.py. step() evaluates the
sampler's expression in fp32 from the scheduler's fp32 tables (alphas_cumprod,
sigmas, lambda_t); the transcription evaluates it in float64 from the same
tables and the same fp32 noise, so the two differ by step()'s roundings alone.
At most eight of them stack on one term (for DPM-Solver++: three in x0, three
in the coefficient, the product and the sum), each at most eps32 relative to
the term: 8 * eps32 * (sum of the |terms|), the noise term |cn| * |z| among
them."""

import json
import math
import os

import pytest
import torch

from distrifuser_amd import DistriConfig, DistriSDPipeline, DistriSDXLPipeline
from distrifuser_amd.ops import eager
from distrifuser_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler,
                                        EulerAncestralDiscreteScheduler, EulerDiscreteScheduler,
                                        get_scheduler)

EPS32 = 2.0 ** -23
SHAPE = (1, 4, 8, 8)
SEED = 0x5EED0000BEEF
SAMPLERS = {
    "euler-a": ("euler-a", {}),
    "ddim-eta": ("ddim", {"eta": 0.6}),
    "dpm-sde": ("dpm-solver", {"algorithm_type": "sde-dpmsolver++"}),
}
NAMES = pytest.mark.parametrize("sampler", list(SAMPLERS))
PREDS = pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])


def _make(sampler, **kw):
    name, extra = SAMPLERS[sampler]
    return get_scheduler(name, **extra, **kw)


def _z(draw, seed=SEED):
    return eager.philox_normal(math.prod(SHAPE), seed, draw).reshape(SHAPE).double()


def _ref_euler_a(s, i, t, x, out, z, v_pred, state):
    sig, sn = float(s.sigmas[i]), float(s.sigmas[i + 1])
    up = math.sqrt(sn * sn * (sig * sig - sn * sn) / (sig * sig))
    down = math.sqrt(sn * sn - up * up)
    dt = down - sig
    if v_pred:
        kx, kv = sig / (sig * sig + 1), 1 / math.sqrt(sig * sig + 1)
        d, d_terms = x * kx + out * kv, x.abs() * kx + out.abs() * kv
    else:
        d, d_terms = out, out.abs()
    return x + d * dt + up * z, x.abs() + d_terms * abs(dt) + up * z.abs(), up


def _ref_ddim(s, i, t, x, out, z, v_pred, state):
    a_t, a_p = (float(a) for a in s._alphas(t))
    sig = s.eta * math.sqrt((1 - a_p) / (1 - a_t)) * math.sqrt(1 - a_t / a_p)
    A, S = math.sqrt(a_t), math.sqrt(1 - a_t)
    if v_pred:
        x0, x0_terms = A * x - S * out, A * x.abs() + S * out.abs()
        eps, eps_terms = A * out + S * x, A * out.abs() + S * x.abs()
    else:
        x0, x0_terms = (x - S * out) / A, (x.abs() + S * out.abs()) / A
        eps, eps_terms = out, out.abs()
    ap, dirc = math.sqrt(a_p), math.sqrt(1 - a_p - sig * sig)
    return (ap * x0 + dirc * eps + sig * z,
            ap * x0_terms + dirc * eps_terms + sig * z.abs(), sig)


def _ref_dpm_sde(s, i, t, x, out, z, v_pred, state):
    """state: (x0_prev, t_prev) as the scheduler under test holds them."""
    t = int(t)
    tp = int(s.timesteps[i + 1]) if i + 1 < len(s.timesteps) else 0
    tab = lambda table, k: float(table[k])
    a_t, s_t, l_t = tab(s.alpha_t, t), tab(s.sigma_t, t), tab(s.lambda_t, t)
    a_p, s_p, l_p = tab(s.alpha_t, tp), tab(s.sigma_t, tp), tab(s.lambda_t, tp)
    if v_pred:
        x0, x0_terms = a_t * x - s_t * out, a_t * x.abs() + s_t * out.abs()
    else:
        x0, x0_terms = (x - s_t * out) / a_t, (x.abs() + s_t * out.abs()) / a_t
    h = l_p - l_t
    A, B = (s_p / s_t) * math.exp(-h), a_p * (1 - math.exp(-2 * h))
    cn = s_p * math.sqrt(1 - math.exp(-2 * h))
    x0_prev, t_prev = state
    if x0_prev is None or i == len(s.timesteps) - 1:
        return A * x + B * x0 + cn * z, A * x.abs() + B * x0_terms + cn * z.abs(), cn
    r0 = (l_t - tab(s.lambda_t, t_prev)) / h
    prev = A * x + B * (1 + 0.5 / r0) * x0 - (0.5 * B / r0) * x0_prev.double() + cn * z
    terms = (A * x.abs() + B * (1 + 0.5 / r0) * x0_terms + (0.5 * B / r0) * x0_prev.abs()
             + cn * z.abs())
    return prev, terms, cn


REFS = {"euler-a": _ref_euler_a, "ddim-eta": _ref_ddim, "dpm-sde": _ref_dpm_sde}


@PREDS
@NAMES
def test_step_matches_the_float64_transcription(sampler, pred):
    gen = torch.Generator().manual_seed(23)
    s = _make(sampler, prediction_type=pred)
    s.set_noise_seed(SEED)
    s.set_timesteps(5)
    x = torch.randn(SHAPE, generator=gen) * s.init_noise_sigma
    worst, cns = 0.0, []
    for i, t in enumerate(s.timesteps):
        out = torch.randn(SHAPE, generator=gen)
        state = (getattr(s, "_x0_prev", None), getattr(s, "_t_prev", None))
        want, terms, cn = REFS[sampler](s, i, t, x.double(), out.double(), _z(i),
                                        pred == "v_prediction", state)
        got = s.step(out, t, x)
        assert got.dtype == torch.float32 and torch.isfinite(got).all()
        tol = 8 * EPS32 * terms
        diff = (got.double() - want).abs()
        worst = max(worst, float((diff / tol).max()))
        assert (diff <= tol).all(), f"step {i}: {float(diff.max()):.3e} vs {float(tol.min()):.3e}"
        cns.append(cn)
        x = got
    print(f"{sampler}/{pred}: worst diff / tol = {worst:.3f}, cn = {[round(c, 4) for c in cns]}")
    assert all(c > 0 for c in cns[:-1])  # every step but (for Euler a) the last is noisy


def test_the_default_arguments_are_the_deterministic_schedulers():
    gen = torch.Generator().manual_seed(3)
    pairs = [(DDIMScheduler(), DDIMScheduler(eta=0.0)),
             (DPMSolverMultistepScheduler(),
              DPMSolverMultistepScheduler(algorithm_type="dpmsolver++"))]
    mask = (torch.rand(SHAPE[2] * SHAPE[3], generator=gen) > 0.5).float()
    init, init_noise = torch.randn(SHAPE, generator=gen), torch.randn(SHAPE, generator=gen)
    for plain, explicit in pairs:
        assert not plain.stochastic and not explicit.stochastic
        for mode in ("step", "guided", "masked"):
            plain.set_timesteps(4)
            explicit.set_timesteps(4)
            explicit.set_noise_seed(77)  # not read
            x = torch.randn(SHAPE, generator=gen)
            for t in plain.timesteps:
                pair = torch.randn(2, *SHAPE[1:], generator=gen)
                if mode == "step":
                    a, b = plain.step(pair[:1], t, x), explicit.step(pair[:1], t, x)
                elif mode == "guided":
                    a, b = plain.guided_step(pair, t, x, 5.0), explicit.guided_step(pair, t, x, 5.0)
                else:
                    a = plain.masked_step(pair, t, x, 5.0, mask, init, init_noise)
                    b = explicit.masked_step(pair, t, x, 5.0, mask, init, init_noise)
                assert torch.equal(a, b)
                x = a


def test_arguments_are_validated():
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            DDIMScheduler(eta=bad)
    with pytest.raises(ValueError):
        DPMSolverMultistepScheduler(algorithm_type="dpmsolver")
    with pytest.raises(ValueError):
        get_scheduler("euler-b")
    with pytest.raises(ValueError):
        DDIMScheduler().set_noise_seed(-1)
    assert type(get_scheduler("euler-a")) is EulerAncestralDiscreteScheduler
    assert type(get_scheduler("euler_ancestral")) is EulerAncestralDiscreteScheduler
    assert get_scheduler("euler-a").stochastic and DDIMScheduler(eta=1.0).stochastic
    assert not get_scheduler("euler").stochastic


@PREDS
def test_euler_ancestral_shares_eulers_schedule_and_ends_without_noise(pred):
    gen = torch.Generator().manual_seed(9)
    anc = get_scheduler("euler-a", prediction_type=pred)
    eul = get_scheduler("euler", prediction_type=pred)
    anc.set_timesteps(4)
    eul.set_timesteps(4)
    assert torch.equal(anc.sigmas, eul.sigmas) and torch.equal(anc.timesteps, eul.timesteps)
    assert anc.init_noise_sigma == eul.init_noise_sigma
    x, out = torch.randn(SHAPE, generator=gen), torch.randn(SHAPE, generator=gen)
    t = anc.timesteps[-1]
    results = []
    for seed in (0, 12345):
        anc.set_timesteps(4)
        anc.set_noise_seed(seed)
        anc._step_index = 3
        assert anc._sigma_up_down() == (0.0, 0.0)
        results.append(anc.step(out, t, x))
    eul._step_index = 3
    assert torch.equal(results[0], results[1])
    assert torch.equal(results[0], eul.step(out, t, x))  # sigma_down = sigma_next = 0
    # the known region of an inpaint step is Euler's: the image at sigma_next
    anc._step_index = eul._step_index = 1
    assert anc._known_coeffs(anc.timesteps[1]) == eul._known_coeffs(eul.timesteps[1])


def _trajectory(s, seed, steps=4, mode="step", t_start=0):
    gen = torch.Generator().manual_seed(31)
    if seed is not None:
        s.set_noise_seed(seed)
    s.set_timesteps(steps)
    if t_start:
        s.set_begin_index(t_start)
    x = torch.randn(SHAPE, generator=gen) * s.init_noise_sigma
    mask = (torch.rand(SHAPE[2] * SHAPE[3], generator=gen) > 0.5).float()
    init, init_noise = torch.randn(SHAPE, generator=gen), torch.randn(SHAPE, generator=gen)
    xs = []
    for t in s.timesteps:
        pair = torch.randn(2, *SHAPE[1:], generator=gen)
        if mode == "step":
            x = s.step(pair[:1], t, x)
        elif mode == "guided":
            x = s.guided_step(pair, t, x, 4.0)
        else:
            x = s.masked_step(pair, t, x, 4.0, mask, init, init_noise)
        xs.append(x)
    return xs


DETERMINISTIC = {"euler-a": ("euler", {}), "ddim-eta": ("ddim", {}), "dpm-sde": ("dpm-solver", {})}


@NAMES
def test_seeds_and_the_draw_counter(sampler):
    s = _make(sampler)
    a = _trajectory(s, 5)
    assert s._draw == 4
    b = _trajectory(s, 5)  # set_timesteps restarts the draws, the seed stays
    c = _trajectory(s, 6)
    default = _trajectory(_make(sampler), None)
    zero = _trajectory(_make(sampler), 0)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert all(torch.equal(p, q) for p, q in zip(default, zero))  # the default seed is 0
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[0], zero[0])
    # set_begin_index restarts them too: the first executed step takes draw 0
    s.set_noise_seed(5)
    s.set_timesteps(4)
    s._draw = 3
    s.set_begin_index(2)
    assert s._draw == 0
    # a deterministic scheduler counts its steps as well, and adds nothing
    name, extra = DETERMINISTIC[sampler]
    det = get_scheduler(name, **extra)
    plain = _trajectory(det, 5)
    assert det._draw == 4
    assert all(torch.equal(p, q) for p, q in zip(plain, _trajectory(det, 6)))
    # the noise is there at every step that has cn > 0: the first one differs
    # from the deterministic class at once
    assert not torch.equal(a[0], plain[0])


@NAMES
def test_guided_and_masked_steps_add_the_same_noise(sampler):
    """guided_step is step() of the combined eps, masked_step its blend: with
    equal branches the CFG result is the branch itself (nu + g * 0), so
    guided_step must equal step() of it bit for bit, noise included, and the
    repainted region of a masked step (m = 1) must equal the guided step."""
    gen = torch.Generator().manual_seed(2)
    a, b, c = _make(sampler), _make(sampler), _make(sampler)
    for s in (a, b, c):
        s.set_noise_seed(41)
        s.set_timesteps(3)
    x = torch.randn(SHAPE, generator=gen) * a.init_noise_sigma
    init, init_noise = torch.randn(SHAPE, generator=gen), torch.randn(SHAPE, generator=gen)
    mask = torch.zeros(SHAPE[2], SHAPE[3])
    mask[:, :4] = 1.0
    det = get_scheduler(*DETERMINISTIC[sampler][:1])
    det.set_timesteps(3)
    for t in a.timesteps[:2]:
        pair = torch.randn(SHAPE, generator=gen).repeat(2, 1, 1, 1)
        via_step = a.step(pair[1:], t, x)
        guided = b.guided_step(pair, t, x, 4.0)
        masked = c.masked_step(pair, t, x, 4.0, mask, init, init_noise)
        assert torch.equal(guided, via_step)
        assert torch.equal(masked[..., :4], guided[..., :4])
        known = det.add_noise(init, init_noise, det._next_timestep(t))
        assert torch.equal(masked[..., 4:], known[..., 4:])  # m = 0: known exactly
        x = guided
    assert a._draw == b._draw == c._draw == 2
    with pytest.raises(ValueError):  # the noise is indexed inside one sample
        a.step(torch.zeros(2, 4, 8, 8), a.timesteps[2], torch.zeros(2, 4, 8, 8))


@NAMES
def test_guidance_rescale_composes_with_noise(sampler):
    s, r = _make(sampler, prediction_type="v_prediction"), _make(sampler,
                                                                 prediction_type="v_prediction")
    gen = torch.Generator().manual_seed(8)
    for k in (s, r):
        k.set_noise_seed(3)
        k.set_timesteps(3)
    x = torch.randn(SHAPE, generator=gen) * s.init_noise_sigma
    pair = torch.randn(2, *SHAPE[1:], generator=gen)
    t = s.timesteps[0]
    plain = s.guided_step(pair, t, x, 6.0)
    rescaled = r.guided_step(pair, t, x, 6.0, guidance_rescale=0.7)
    assert torch.isfinite(rescaled).all() and not torch.equal(plain, rescaled)
    # the same step of the rescaled eps: the noise term is the same one
    f = eager.guidance_rescale_factor(pair, 6.0, 0.7)
    again = _make(sampler, prediction_type="v_prediction")
    again.set_noise_seed(3)
    again.set_timesteps(3)
    assert torch.equal(again.step(eager._cfg_eps(pair, x, 6.0, f), t, x), rescaled)


# ---- config ---------------------------------------------------------------------------


def test_config_holds_the_class_keys_only():
    assert DDIMScheduler(eta=0.5).config()["eta"] == 0.5
    assert DDIMScheduler().config()["eta"] == 0.0
    assert "algorithm_type" not in DDIMScheduler().config()
    dpm = DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++").config()
    assert dpm["algorithm_type"] == "sde-dpmsolver++" and "eta" not in dpm
    for s in (EulerDiscreteScheduler(), EulerAncestralDiscreteScheduler()):
        assert "eta" not in s.config() and "algorithm_type" not in s.config()
    for s in (DDIMScheduler(eta=0.5), EulerAncestralDiscreteScheduler(),
              DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")):
        assert type(s)(**s.config()).config() == s.config()


def _tiny(cls, scheduler="ddim", pretrained=None, **kw):
    size = 128 if cls is DistriSDXLPipeline else 64
    cfg = DistriConfig(height=size, width=size, use_cuda_graph=False, device="cpu")
    torch.manual_seed(0)
    if pretrained is not None:
        kw["pretrained_model_name_or_path"] = pretrained
    return cls.from_pretrained(cfg, preset="tiny", torch_dtype=torch.float32,
                               scheduler=scheduler, **kw)


@pytest.mark.parametrize("cls", [DistriSDPipeline, DistriSDXLPipeline], ids=["sd", "sdxl"])
def test_scheduler_config_round_trip(cls, tmp_path):
    pipe = _tiny(cls, "ddim", eta=0.75, prediction_type="v_prediction")
    assert pipe.scheduler.eta == 0.75 and pipe.scheduler.stochastic
    out = str(tmp_path / "ddim")
    pipe.save_pretrained(out)
    with open(os.path.join(out, "scheduler", "scheduler_config.json"), encoding="utf-8") as f:
        on_file = json.load(f)
    assert on_file["eta"] == 0.75 and "algorithm_type" not in on_file
    assert _tiny(cls, "ddim", pretrained=out).scheduler.eta == 0.75
    assert _tiny(cls, "ddim", pretrained=out, eta=0.0).scheduler.eta == 0.0  # keyword wins
    for other in ("euler", "euler-a", "dpm-solver"):  # a file with eta loads into them
        s = _tiny(cls, other, pretrained=out).scheduler
        assert s.prediction_type == "v_prediction" and not hasattr(s, "eta")

    sde = _tiny(cls, "dpm-solver", algorithm_type="sde-dpmsolver++")
    assert sde.scheduler.stochastic
    out2 = str(tmp_path / "sde")
    sde.save_pretrained(out2)
    assert _tiny(cls, "dpm-solver", pretrained=out2).scheduler.algorithm_type == "sde-dpmsolver++"
    assert _tiny(cls, "dpm", pretrained=out2,
                 algorithm_type="dpmsolver++").scheduler.algorithm_type == "dpmsolver++"
    assert _tiny(cls, "ddim", pretrained=out2).scheduler.eta == 0.0

    # a keyword the chosen class lacks
    for name, kw in (("euler", {"eta": 0.5}), ("euler-a", {"eta": 0.5}),
                     ("dpm-solver", {"eta": 0.5}), ("ddim", {"algorithm_type": "dpmsolver++"}),
                     ("euler", {"algorithm_type": "sde-dpmsolver++"})):
        with pytest.raises(ValueError):
            _tiny(cls, name, **kw)
    with pytest.raises(ValueError):
        _tiny(cls, "ddim", eta=2.0)
