"""Shared noise-schedule math for the SD-family schedulers.

SD/SDXL training schedule: 1000 steps, scaled_linear betas in
[0.00085, 0.012], epsilon prediction, leading timestep spacing with
steps_offset=1 (the reference inherited these from the diffusers scheduler
configs shipped with the checkpoints).
"""

from __future__ import annotations

import torch


class SchedulerBase:
    order = 1

    def __init__(
        self,
        num_train_timesteps: int = 1000,
        beta_start: float = 0.00085,
        beta_end: float = 0.012,
        steps_offset: int = 1,
    ):
        self.num_train_timesteps = num_train_timesteps
        self.steps_offset = steps_offset
        betas = (
            torch.linspace(beta_start**0.5, beta_end**0.5, num_train_timesteps, dtype=torch.float64)
            ** 2
        )
        alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(alphas, dim=0).float()
        self.timesteps: torch.Tensor | None = None
        self.num_inference_steps: int | None = None
        self.init_noise_sigma = 1.0

    def _leading_timesteps(self, num_inference_steps: int) -> torch.Tensor:
        step_ratio = self.num_train_timesteps // num_inference_steps
        t = (torch.arange(num_inference_steps) * step_ratio).flip(0) + self.steps_offset
        return t.long()

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        raise NotImplementedError

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    # -- img2img: forward noising and a part-way start -----------------------

    def add_noise(self, sample: torch.Tensor, noise: torch.Tensor, timestep) -> torch.Tensor:
        """q(x_t | x_0): sqrt(acp_t) * sample + sqrt(1 - acp_t) * noise, in fp32,
        returned in sample's dtype."""
        acp = self.alphas_cumprod[int(timestep)]
        out = acp.sqrt() * sample.float() + (1 - acp).sqrt() * noise.float().to(sample.device)
        return out.to(sample.dtype)

    # -- inpainting: the step blended with the re-noised known region ---------

    def model_input_scale(self, timestep=None) -> float:
        """The divisor ``scale_model_input`` applies at the current step."""
        return 1.0

    def _next_timestep(self, timestep):
        """The entry after ``timestep`` in the running list, None at its end."""
        idx = int((self.timesteps == float(timestep)).nonzero()[0])
        return self.timesteps[idx + 1] if idx + 1 < len(self.timesteps) else None

    def _known_coeffs(self, timestep) -> tuple[float, float]:
        """(sa, sb) of known = sa*init + sb*init_noise: the init latents noised
        to the next timestep of the running list, and the clean init latents
        (1, 0) after the last step (the diffusers rule)."""
        t_next = self._next_timestep(timestep)
        if t_next is None:
            return 1.0, 0.0
        acp = float(self.alphas_cumprod[int(t_next)])
        return acp ** 0.5, (1 - acp) ** 0.5

    def masked_step(self, noise: torch.Tensor, timestep, sample: torch.Tensor,
                    guidance_scale: float, mask: torch.Tensor, init: torch.Tensor,
                    init_noise: torch.Tensor) -> torch.Tensor:
        """One inpaint step: what ``guided_step`` (noise is the [uncond; cond]
        pair) or ``step`` (noise has sample's batch; guidance_scale is not
        read) computes, then

            out = m * x' + (1 - m) * known

        with known = ``add_noise(init, init_noise, t_next)``, or init itself
        after the last step. mask (1 = repaint) has one value per latent
        pixel; init and init_noise are fp32 [1,C,h,w]. The scheduler state
        advances as in an unmasked step. One fused kernel on GPU; elsewhere
        the composition of ``step`` and ``add_noise`` in fp32."""
        from ..ops import use_hip

        if use_hip(sample):
            return self._masked_step_native(noise, timestep, sample, guidance_scale, mask, init,
                                            init_noise)
        from ..ops.eager import _cfg_eps

        t_next = self._next_timestep(timestep)  # before step() moves on
        eps = _cfg_eps(noise, sample, guidance_scale)
        xp = self.step(eps, timestep, sample.float())
        init = init.float().to(sample.device)
        known = init if t_next is None else self.add_noise(init, init_noise, t_next)
        m = mask.float().to(sample.device).reshape(1, 1, *sample.shape[2:])
        return (m * xp + (1.0 - m) * known).to(sample.dtype)

    def _masked_step_native(self, noise, timestep, sample, guidance_scale, mask, init,
                            init_noise) -> torch.Tensor:
        raise NotImplementedError

    def set_begin_index(self, t_start: int) -> None:
        """Start the schedule at index ``t_start`` of the list that
        ``set_timesteps(n)`` made: ``timesteps`` becomes its last n - t_start
        entries, and every step computes what the full schedule computes at
        that index (the multistep solver takes its first executed step as
        first order: it has no history). Call it once, right after
        ``set_timesteps``."""
        n = len(self.timesteps)
        if not 0 <= t_start < n:
            raise ValueError(f"t_start must be in [0, {n}), got {t_start}")
        self.timesteps = self.timesteps[t_start:]


def img2img_start(num_inference_steps: int, strength: float) -> int:
    """Index of the first executed step for an img2img ``strength`` (the
    diffusers rule): init = min(int(n * strength), n) steps run, so
    t_start = max(n - init, 0). strength must be in (0, 1] and leave at least
    one step."""
    if not 0 < strength <= 1:
        raise ValueError(f"strength must be in (0, 1], got {strength}")
    init = min(int(num_inference_steps * strength), num_inference_steps)
    if init < 1:
        raise ValueError(
            f"strength {strength} leaves no step to run out of {num_inference_steps}")
    return max(num_inference_steps - init, 0)
