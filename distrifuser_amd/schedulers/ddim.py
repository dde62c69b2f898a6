"""DDIM (epsilon- or v-prediction) — the benchmark-protocol sampler at its
default eta = 0; eta > 0 adds the DDIM noise term (eta = 1 is DDPM-like)."""

from __future__ import annotations

import torch

from .common import SchedulerBase


class DDIMScheduler(SchedulerBase):
    extra_config_keys = ("eta",)

    def __init__(self, *args, eta: float = 0.0, **kwargs):
        super().__init__(*args, **kwargs)
        if not 0.0 <= eta <= 1.0:
            raise ValueError(f"eta must be in [0, 1], got {eta}")
        self.eta = float(eta)

    @property
    def stochastic(self) -> bool:
        return self.eta > 0

    def config(self) -> dict:
        return {**super().config(), "eta": self.eta}

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        self.num_inference_steps = num_inference_steps
        self.timesteps = self._spaced_timesteps(num_inference_steps)
        if device is not None:
            self.timesteps = self.timesteps.to(device)
        self._draw = 0

    def _alphas(self, timestep):
        """(acp_t, acp_prev) of the step at ``timestep``, fp32 tensors."""
        t = int(timestep)
        prev_t = t - self.num_train_timesteps // self.num_inference_steps
        acp = self.alphas_cumprod
        return acp[t], acp[prev_t] if prev_t >= 0 else acp[0]

    def _noise_coeff(self, timestep) -> float:
        """sig = eta * sqrt((1 - a_prev) / (1 - a_t)) * sqrt(1 - a_t / a_prev),
        the coefficient of the step's noise; 0.0 for eta = 0."""
        if self.eta == 0:
            return 0.0
        alpha_t, alpha_prev = (float(a) for a in self._alphas(timestep))
        var = (1 - alpha_prev) / (1 - alpha_t) * (1 - alpha_t / alpha_prev)
        return self.eta * max(var, 0.0) ** 0.5

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor) -> torch.Tensor:
        from ..ops import cfg_affine_step, use_hip

        if self.stochastic and use_hip(sample):
            # no CFG pair: still the one fused launch, which draws the noise
            ca, cb = self._affine_coeffs(timestep)
            return cfg_affine_step(model_output, sample, 1.0, ca, cb,
                                   step_noise=self._take_draw(self._noise_coeff(timestep)))
        alpha_t, alpha_prev = self._alphas(timestep)
        sig = self._noise_coeff(timestep)

        x = sample.float()
        if self.v_prediction:
            v = model_output.float()
            pred_x0 = alpha_t.sqrt() * x - (1 - alpha_t).sqrt() * v
            eps = alpha_t.sqrt() * v + (1 - alpha_t).sqrt() * x
        else:
            eps = model_output.float()
            pred_x0 = (x - (1 - alpha_t).sqrt() * eps) / alpha_t.sqrt()
        direction = (1 - alpha_prev - sig * sig).clamp_min(0).sqrt() * eps
        prev = alpha_prev.sqrt() * pred_x0 + direction
        return self._add_noise_eager(prev, sig).to(sample.dtype)

    def guided_step(self, noise: torch.Tensor, timestep, sample: torch.Tensor,
                    guidance_scale: float, guidance_rescale: float = 0.0) -> torch.Tensor:
        # CFG combine + DDIM update; noise is the [uncond; cond] pair. On GPU
        # this is ONE fused kernel (csrc/scheduler.hip) - the step math runs
        # outside the captured graphs, so its torch-op launch overhead is
        # otherwise exposed every denoise step. guidance_rescale > 0 adds the
        # two launches of the factor op in front of it; eta > 0 adds none (the
        # kernel draws the noise).
        from ..ops import hip_ext, use_hip
        from ..ops.dispatch import _with_noise

        factor = self._rescale_factor(noise, sample, guidance_scale, guidance_rescale)
        if use_hip(noise):
            ca, cb = self._affine_coeffs(timestep)
            nkw = _with_noise(self._take_draw(self._noise_coeff(timestep)))
            if factor is None:
                return hip_ext().cfg_affine_step(noise, sample, guidance_scale, ca, cb, **nkw)
            return hip_ext().cfg_affine_step(noise, sample, guidance_scale, ca, cb, factor, **nkw)
        if factor is not None:
            return self._guided_step_eager(noise, timestep, sample, guidance_scale, factor)
        nu, nc = noise.float().chunk(2)
        eps = nu + guidance_scale * (nc - nu)
        return self.step(eps, timestep, sample)

    def _affine_coeffs(self, timestep) -> tuple[float, float]:
        # x' = sqrt(a_p) * (x - sqrt(1-a_t) eps)/sqrt(a_t) + sqrt(1-a_p-sig^2) eps
        #    = ca * x + cb * eps
        alpha_t, alpha_prev = (float(a) for a in self._alphas(timestep))
        sig = self._noise_coeff(timestep)
        sp = max(1 - alpha_prev - sig * sig, 0.0) ** 0.5
        if self.v_prediction:
            # x' = Ap*(A x - S v) + Sp*(A v + S x): no division by A
            a, s = alpha_t ** 0.5, (1 - alpha_t) ** 0.5
            ap = alpha_prev ** 0.5
            return ap * a + sp * s, sp * a - ap * s
        ca = (alpha_prev / alpha_t) ** 0.5
        cb = sp - ca * (1 - alpha_t) ** 0.5
        return ca, cb

    def _masked_step_native(self, noise, timestep, sample, guidance_scale, mask, init,
                            init_noise, factor=None) -> torch.Tensor:
        from ..ops import masked_affine_step

        ca, cb = self._affine_coeffs(timestep)
        sa, sb = self._known_coeffs(timestep)
        return masked_affine_step(noise, sample, init, init_noise, mask, guidance_scale, ca, cb,
                                  sa, sb, factor, self._take_draw(self._noise_coeff(timestep)))
