"""Euler ancestral ("Euler a"; epsilon- or v-prediction): the Euler step towards
sigma_down, then fresh noise of scale sigma_up (k-diffusion's
``sample_euler_ancestral``, diffusers' ``EulerAncestralDiscreteScheduler``):

    sigma_up   = sqrt(sn^2 * (s^2 - sn^2) / s^2)
    sigma_down = sqrt(sn^2 - sigma_up^2)
    x' = x + d * (sigma_down - s) + sigma_up * z

with s, sn the current and next sigma of the Euler schedule and d the Euler
derivative. The last step has sn = 0: no noise. Still affine: the fused Euler
step with sigma_down in place of sigma_next, plus the kernel's noise term."""

from __future__ import annotations

import torch

from .euler import EulerDiscreteScheduler


class EulerAncestralDiscreteScheduler(EulerDiscreteScheduler):
    @property
    def stochastic(self) -> bool:
        return True

    def _sigma_up_down(self) -> tuple[float, float]:
        """(sigma_up, sigma_down) at the current step index, float64."""
        s = float(self.sigmas[self._step_index])
        sn = float(self.sigmas[self._step_index + 1])
        up = (sn * sn * (s * s - sn * sn) / (s * s)) ** 0.5
        return up, (sn * sn - up * up) ** 0.5

    def _target_sigma(self) -> tuple[torch.Tensor, float]:
        up, down = self._sigma_up_down()
        return torch.tensor(down, dtype=torch.float32), up

    def _affine_coeffs(self, timestep=None) -> tuple[float, float]:
        """(ca, cb) of the Euler step from sigma to sigma_down."""
        sigma = float(self.sigmas[self._step_index])
        dt = self._sigma_up_down()[1] - sigma
        if not self.v_prediction:
            return 1.0, dt
        return 1.0 + dt * sigma / (sigma * sigma + 1.0), dt / (sigma * sigma + 1.0) ** 0.5

    # _known_coeffs (inpainting) is the Euler rule: the known region is the
    # image noised to sigma_next, the level the whole sample is at after the step
