"""Euler discrete (epsilon- or v-prediction)."""

from __future__ import annotations

import numpy as np
import torch

from .common import SchedulerBase


class EulerDiscreteScheduler(SchedulerBase):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        acp = self._finite_alphas_cumprod().double()
        self._sigmas_train = ((1 - acp) / acp).sqrt().numpy()
        self.sigmas: torch.Tensor | None = None
        self._step_index = 0

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        self.num_inference_steps = num_inference_steps
        t = self._spaced_timesteps(num_inference_steps).numpy().astype(np.float64)
        sigmas = np.interp(t, np.arange(self.num_train_timesteps), self._sigmas_train)
        self.sigmas = torch.tensor(np.concatenate([sigmas, [0.0]]), dtype=torch.float32)
        self.timesteps = torch.tensor(t, dtype=torch.float32)
        if device is not None:
            self.timesteps = self.timesteps.to(device)
        self.init_noise_sigma = float((self.sigmas.max() ** 2 + 1) ** 0.5)
        self._step_index = 0
        self._draw = 0

    def set_begin_index(self, t_start: int) -> None:
        super().set_begin_index(t_start)
        self.sigmas = self.sigmas[t_start:]  # sigmas[i] pairs with timesteps[i]
        self._step_index = 0

    def add_noise(self, sample: torch.Tensor, noise: torch.Tensor, timestep) -> torch.Tensor:
        """sample + sigma_t * noise (init_noise_sigma is for pure noise only)."""
        idx = int((self.timesteps == float(timestep)).nonzero()[0])
        sigma = self.sigmas[idx]
        out = sample.float() + sigma * noise.float().to(sample.device)
        return out.to(sample.dtype)

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        sigma = self.sigmas[self._step_index]
        return sample / float((sigma**2 + 1) ** 0.5)

    def _target_sigma(self) -> tuple[torch.Tensor, float]:
        """The sigma the Euler step lands on, and the coefficient of the noise
        it then adds: (sigma_next, 0.0) here."""
        return self.sigmas[self._step_index + 1], 0.0

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor) -> torch.Tensor:
        from ..ops import cfg_affine_step, use_hip

        sigma_next, cn = self._target_sigma()
        if self.stochastic and use_hip(sample):
            # no CFG pair: still the one fused launch, which draws the noise
            ca, cb = self._affine_coeffs()
            self._step_index += 1
            return cfg_affine_step(model_output, sample, 1.0, ca, cb,
                                   step_noise=self._take_draw(cn))
        sigma = self.sigmas[self._step_index].to(sample.device)
        sigma_next = sigma_next.to(sample.device)
        x = sample.float()
        eps = model_output.float()
        if self.v_prediction:
            # v is the output for the scaled input x / sqrt(s^2 + 1): the
            # derivative (x - x0) / s = x * s/(s^2 + 1) + v / sqrt(s^2 + 1)
            eps = x * (sigma / (sigma**2 + 1)) + eps / (sigma**2 + 1) ** 0.5
        # epsilon prediction: derivative d = eps; x_{t+1} = x + d * (s_next - s)
        prev = x + eps * (sigma_next - sigma)
        self._step_index += 1
        return self._add_noise_eager(prev, cn).to(sample.dtype)

    def guided_step(self, noise: torch.Tensor, timestep, sample: torch.Tensor,
                    guidance_scale: float, guidance_rescale: float = 0.0) -> torch.Tensor:
        # CFG combine + Euler update in ONE fused kernel on GPU (the update is
        # affine in (x, eps): ca = 1, cb = sigma_next - sigma); guidance_rescale
        # > 0 adds the two launches of the factor op in front of it
        from ..ops import hip_ext, use_hip
        from ..ops.dispatch import _with_noise

        factor = self._rescale_factor(noise, sample, guidance_scale, guidance_rescale)
        if use_hip(noise):
            ca, cb = self._affine_coeffs()
            nkw = _with_noise(self._take_draw(self._target_sigma()[1]))
            self._step_index += 1
            if factor is None:
                return hip_ext().cfg_affine_step(noise, sample, guidance_scale, ca, cb, **nkw)
            return hip_ext().cfg_affine_step(noise, sample, guidance_scale, ca, cb, factor, **nkw)
        if factor is not None:
            return self._guided_step_eager(noise, timestep, sample, guidance_scale, factor)
        nu, nc = noise.float().chunk(2)
        eps = nu + guidance_scale * (nc - nu)
        return self.step(eps, timestep, sample)

    def _affine_coeffs(self, timestep=None) -> tuple[float, float]:
        """(ca, cb) of x' = ca*x + cb*model_output at the current step index."""
        if not self.v_prediction:
            return 1.0, float(self.sigmas[self._step_index + 1] - self.sigmas[self._step_index])
        sigma = float(self.sigmas[self._step_index])
        dt = float(self.sigmas[self._step_index + 1]) - sigma
        return 1.0 + dt * sigma / (sigma * sigma + 1.0), dt / (sigma * sigma + 1.0) ** 0.5

    # -- inpainting --------------------------------------------------------------

    def model_input_scale(self, timestep=None) -> float:
        sigma = self.sigmas[self._step_index]
        return float((sigma**2 + 1) ** 0.5)

    def _known_coeffs(self, timestep) -> tuple[float, float]:
        # known = init + sigma_next * init_noise; sigma = 0 after the last step
        last = self._step_index + 1 >= len(self.timesteps)
        return 1.0, 0.0 if last else float(self.sigmas[self._step_index + 1])

    def _masked_step_native(self, noise, timestep, sample, guidance_scale, mask, init,
                            init_noise, factor=None) -> torch.Tensor:
        from ..ops import masked_affine_step

        sa, sb = self._known_coeffs(timestep)
        ca, cb = self._affine_coeffs()
        step_noise = self._take_draw(self._target_sigma()[1])
        self._step_index += 1
        return masked_affine_step(noise, sample, init, init_noise, mask, guidance_scale, ca, cb,
                                  sa, sb, factor, step_noise)
