"""The route from a scheduler's entry points to the fused step ops (CPU).

``use_hip`` is replaced by "always native" and the extension by a stand-in
whose step entries record their arguments and run the eager twins. Every
sampler, prediction type and entry point must then make exactly one step-entry
call per step: the right entry, with the coefficients ``_affine_coeffs``
returns, the noise coefficient, the draw of that step, and x0_prev only on a
multistep step; afterwards the state has moved once. The result is held
against the eager scheduler (run before the stand-in goes in) to the tolerance
of tests/test_vpred_schedulers.py::test_folded_coefficients_equal_step.

``step`` of a deterministic sampler is eager by design: no call at all."""

import pytest
import torch

from distrifuser_amd import ops
from distrifuser_amd.ops import dispatch, eager
from distrifuser_amd.schedulers import DPMSolverMultistepScheduler, get_scheduler

SHAPE = (1, 4, 4, 4)
STEPS = 4  # DPM: a first-order step, two 2M steps, the first-order last step
G = 6.0
PHI = 0.7
SEED = 1234
SAMPLERS = {
    "ddim": ("ddim", {}),
    "ddim-eta": ("ddim", {"eta": 0.5}),
    "euler": ("euler", {}),
    "euler-a": ("euler-a", {}),
    "dpm": ("dpm-solver", {}),
    "dpm-sde": ("dpm-solver", {"algorithm_type": "sde-dpmsolver++"}),
}
ENTRIES = ("step", "guided", "guided_rescale", "masked_pair", "masked_branch")
STEP_ENTRIES = ("cfg_affine_step", "cfg_dpm_step", "masked_affine_step", "masked_dpm_step")


class RecordingExt:
    """The extension's step entries: (name, arguments, result) go to ``calls``."""

    def __init__(self):
        self.calls = []

    def _run(self, name, **kw):
        out = getattr(eager, name)(**kw)
        self.calls.append((name, kw, out))
        return out

    def guidance_rescale_factor(self, noise, g, phi):
        return self._run("guidance_rescale_factor", noise=noise, g=g, phi=phi)

    def cfg_affine_step(self, noise, x, g, ca, cb, factor=None, step_noise=None):
        return self._run("cfg_affine_step", noise=noise, x=x, g=g, ca=ca, cb=cb, factor=factor,
                         step_noise=step_noise)

    def cfg_dpm_step(self, noise, x, x0_prev, g, ca, cb, cc, cx, ce, factor=None,
                     step_noise=None):
        return self._run("cfg_dpm_step", noise=noise, x=x, x0_prev=x0_prev, g=g, ca=ca, cb=cb,
                         cc=cc, cx=cx, ce=ce, factor=factor, step_noise=step_noise)

    def masked_affine_step(self, noise, x, init, init_noise, mask, g, ca, cb, sa, sb,
                           factor=None, step_noise=None):
        return self._run("masked_affine_step", noise=noise, x=x, init=init,
                         init_noise=init_noise, mask=mask, g=g, ca=ca, cb=cb, sa=sa, sb=sb,
                         factor=factor, step_noise=step_noise)

    def masked_dpm_step(self, noise, x, x0_prev, init, init_noise, mask, g, ca, cb, cc, cx, ce,
                        sa, sb, factor=None, step_noise=None):
        return self._run("masked_dpm_step", noise=noise, x=x, x0_prev=x0_prev, init=init,
                         init_noise=init_noise, mask=mask, g=g, ca=ca, cb=cb, cc=cc, cx=cx,
                         ce=ce, sa=sa, sb=sb, factor=factor, step_noise=step_noise)


def _scheduler(sampler, pred):
    name, kw = SAMPLERS[sampler]
    sched = get_scheduler(name, prediction_type=pred, **kw)
    sched.set_noise_seed(SEED)
    sched.set_timesteps(STEPS)
    return sched


def _call(sched, entry, noise, t, x, blend):
    if entry == "step":
        return sched.step(noise, t, x)
    if entry == "guided":
        return sched.guided_step(noise, t, x, G)
    if entry == "guided_rescale":
        return sched.guided_step(noise, t, x, G, guidance_rescale=PHI)
    return sched.masked_step(noise, t, x, G, *blend)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_one_fused_call_per_step(monkeypatch, sampler, pred, entry):
    gen = torch.Generator().manual_seed(7)
    pair = entry in ("guided", "guided_rescale", "masked_pair")
    masked = entry.startswith("masked")
    mask = (torch.rand(SHAPE[2] * SHAPE[3], generator=gen) > 0.5).float()
    init, init_noise = torch.randn(SHAPE, generator=gen), torch.randn(SHAPE, generator=gen)
    blend = (mask, init, init_noise)
    noises = [torch.randn(2 if pair else 1, *SHAPE[1:], generator=gen) for _ in range(STEPS)]

    # the eager trajectory: what every native step below starts from and must give
    ref = _scheduler(sampler, pred)
    xs = [torch.randn(SHAPE, generator=gen) * ref.init_noise_sigma]
    for noise, t in zip(noises, ref.timesteps):
        xs.append(_call(ref, entry, noise, t, xs[-1], blend))

    ext = RecordingExt()
    for module in (ops, dispatch):
        monkeypatch.setattr(module, "use_hip", lambda x: True)
        monkeypatch.setattr(module, "hip_ext", lambda: ext)
    sched = _scheduler(sampler, pred)
    dpm = isinstance(sched, DPMSolverMultistepScheduler)
    fused = entry != "step" or sched.stochastic
    for i, (noise, t) in enumerate(zip(noises, sched.timesteps)):
        x = xs[i]
        coeffs = sched._affine_coeffs(t)
        cn = sched._noise_coeff(t) if sampler in ("ddim", "ddim-eta", "dpm", "dpm-sde") \
            else sched._target_sigma()[1]
        known = sched._known_coeffs(t)
        x0_before = sched._x0_prev if dpm else None
        ext.calls.clear()
        got = _call(sched, entry, noise, t, x, blend)

        names = [c[0] for c in ext.calls]
        step_name = ("masked_" if masked else "cfg_") + ("dpm_step" if dpm else "affine_step")
        front = ["guidance_rescale_factor"] if entry == "guided_rescale" else []
        assert names == front + ([step_name] if fused else []), (i, names)
        if fused:
            _, kw, out = ext.calls[-1]
            assert kw["noise"] is noise and kw["x"] is x
            assert kw["g"] == (1.0 if entry == "step" else G)
            if dpm:
                first, (ca, cb, cc, cx, ce) = coeffs
                assert first == (i in (0, STEPS - 1))
                assert (kw["ca"], kw["cb"], kw["cc"], kw["cx"], kw["ce"]) == (ca, cb, cc, cx, ce)
                assert kw["x0_prev"] is (None if first else x0_before)
                assert got is out[0] and sched._x0_prev is out[1]
            else:
                assert (kw["ca"], kw["cb"]) == coeffs
                assert got is out
            if masked:
                assert (kw["sa"], kw["sb"]) == known
                assert all(torch.equal(kw[k], v) for k, v in
                           zip(("mask", "init", "init_noise"), blend))
            if front:
                assert kw["factor"] is ext.calls[0][2]
                fkw = ext.calls[0][1]
                assert fkw["noise"] is noise and (fkw["g"], fkw["phi"]) == (G, PHI)
            else:
                assert kw["factor"] is None
            want_noise = (float(cn), SEED, i) if sched.stochastic else None
            assert kw["step_noise"] == want_noise

        # the state has moved once
        assert sched._draw == i + 1
        if sampler not in ("ddim", "ddim-eta"):
            assert sched._step_index == i + 1
        if dpm:
            assert sched._t_prev == int(t) and sched._x0_prev is not None
        want = xs[i + 1]
        assert got.dtype == want.dtype
        assert torch.allclose(got, want, rtol=2e-5, atol=2e-5 * float(x.abs().max())), (
            i, float((got - want).abs().max()))
