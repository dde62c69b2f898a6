"""DPM-Solver++ (2M, multistep; epsilon- or v-prediction), and its SDE variant
(``algorithm_type="sde-dpmsolver++"``, the "DPM++ 2M SDE" sampler): with
A = (s_p / s_t) e^-h and B = a_p (1 - e^-2h),

    first order: prev = A x + B x0 + cn z
    2M:          prev = A x + B (1 + 0.5 / r0) x0 - (0.5 B / r0) x0_prev + cn z
    cn = s_p sqrt(1 - e^-2h),   z ~ N(0, 1)

which is the deterministic update's affine form with other coefficients, plus
the noise term of the fused kernel."""

from __future__ import annotations

import torch

from .common import SchedulerBase


class DPMSolverMultistepScheduler(SchedulerBase):
    extra_config_keys = ("algorithm_type",)
    ALGORITHM_TYPES = ("dpmsolver++", "sde-dpmsolver++")

    def __init__(self, *args, solver_order: int = 2, algorithm_type: str = "dpmsolver++",
                 **kwargs):
        super().__init__(*args, **kwargs)
        if algorithm_type not in self.ALGORITHM_TYPES:
            raise ValueError(
                f"algorithm_type must be one of {self.ALGORITHM_TYPES}, got {algorithm_type!r}")
        self.algorithm_type = algorithm_type
        self.solver_order = solver_order
        acp = self._finite_alphas_cumprod()
        self.alpha_t = acp.sqrt()
        self.sigma_t = (1 - acp).sqrt()
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)
        self._x0_prev: torch.Tensor | None = None
        self._t_prev: int | None = None
        self._step_index = 0

    @property
    def stochastic(self) -> bool:
        return self.algorithm_type == "sde-dpmsolver++"

    def config(self) -> dict:
        return {**super().config(), "algorithm_type": self.algorithm_type}

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        self.num_inference_steps = num_inference_steps
        self.timesteps = self._spaced_timesteps(num_inference_steps)
        if device is not None:
            self.timesteps = self.timesteps.to(device)
        self._x0_prev = None
        self._t_prev = None
        self._step_index = 0
        self._draw = 0

    def set_begin_index(self, t_start: int) -> None:
        super().set_begin_index(t_start)
        # no history: the first executed step is first order, the rest 2M
        self._x0_prev = None
        self._t_prev = None
        self._step_index = 0

    def _prev_timestep(self, t: int) -> int:
        idx = int((self.timesteps == t).nonzero()[0])
        return int(self.timesteps[idx + 1]) if idx + 1 < len(self.timesteps) else 0

    def _noise_coeff(self, timestep) -> float:
        """cn = s_p * sqrt(1 - e^-2h) of the SDE step at ``timestep``, else 0.0."""
        if not self.stochastic:
            return 0.0
        import math

        t = int(timestep)
        t_prev = self._prev_timestep(t)
        h = float(self.lambda_t[t_prev]) - float(self.lambda_t[t])
        return float(self.sigma_t[t_prev]) * math.sqrt(max(1.0 - math.exp(-2.0 * h), 0.0))

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor) -> torch.Tensor:
        from ..ops import cfg_dpm_step, use_hip

        if self.stochastic and use_hip(sample):
            # no CFG pair: still the one fused launch, which draws the noise
            first, coeffs = self._affine_coeffs(timestep)
            prev, x0 = cfg_dpm_step(
                model_output, sample, None if first else self._x0_prev, 1.0, *coeffs,
                step_noise=self._take_draw(self._noise_coeff(timestep)))
            self._x0_prev = x0
            self._t_prev = int(timestep)
            self._step_index += 1
            return prev
        t = int(timestep)
        t_prev = self._prev_timestep(t)
        x = sample.float()
        eps = model_output.float()

        a_t, s_t, l_t = self.alpha_t[t], self.sigma_t[t], self.lambda_t[t]
        a_p, s_p, l_p = self.alpha_t[t_prev], self.sigma_t[t_prev], self.lambda_t[t_prev]
        x0 = a_t * x - s_t * eps if self.v_prediction else (x - s_t * eps) / a_t

        h = l_p - l_t
        first = (self._x0_prev is None or self.solver_order == 1
                 or self._step_index == len(self.timesteps) - 1)
        if self.stochastic:
            lead = (s_p / s_t) * torch.exp(-h)
            b = a_p * (1.0 - torch.exp(-2.0 * h))
            prev = lead * x + b * x0
            if not first:
                r0 = (l_t - self.lambda_t[self._t_prev]) / h
                prev = prev + 0.5 * b * ((x0 - self._x0_prev) / r0)
        elif first:
            # first-order (DPM-Solver++ 1S) update
            prev = (s_p / s_t) * x - a_p * (torch.exp(-h) - 1.0) * x0
        else:
            l_pp = self.lambda_t[self._t_prev]
            h_0 = l_t - l_pp
            r0 = h_0 / h
            d0 = x0
            d1 = (x0 - self._x0_prev) / r0
            prev = (
                (s_p / s_t) * x
                - a_p * (torch.exp(-h) - 1.0) * d0
                - 0.5 * a_p * (torch.exp(-h) - 1.0) * d1
            )

        cn = self._noise_coeff(timestep)
        self._x0_prev = x0
        self._t_prev = t
        self._step_index += 1
        return self._add_noise_eager(prev, cn).to(sample.dtype)

    def guided_step(self, noise: torch.Tensor, timestep, sample: torch.Tensor,
                    guidance_scale: float, guidance_rescale: float = 0.0) -> torch.Tensor:
        """CFG combine + DPM-Solver++(2M) update in ONE fused kernel on GPU.

        The 2M update is affine in (x, eps, x0_prev):
            prev = ca*x + cb*eps + cc*x0_prev,   x0 = cx*x + ce*eps
        with C = a_p*(exp(-h)-1), C' = C*(1 + 0.5/r0) (order 2) or C (order 1):
            ca = s_p/s_t - C'/a_t,  cb = C'*s_t/a_t,  cc = 0.5*C/r0.
        v-prediction changes x0 alone, cx = a_t and ce = -s_t, and with it
            ca = s_p/s_t - C'*cx,  cb = -C'*ce.
        guidance_rescale > 0 adds the two launches of the factor op in front.
        The SDE variant: exp(-2h) for exp(-h) in C, s_p/s_t * exp(-h) for
        s_p/s_t, and the kernel's noise term.
        """
        from ..ops import hip_ext, use_hip
        from ..ops.dispatch import _with_noise

        factor = self._rescale_factor(noise, sample, guidance_scale, guidance_rescale)
        if not use_hip(noise):
            if factor is not None:
                return self._guided_step_eager(noise, timestep, sample, guidance_scale, factor)
            nu, nc = noise.float().chunk(2)
            eps = nu + guidance_scale * (nc - nu)
            return self.step(eps, timestep, sample)

        first, coeffs = self._affine_coeffs(timestep)
        prev, x0 = hip_ext().cfg_dpm_step(
            noise, sample, None if first else self._x0_prev, guidance_scale, *coeffs,
            *(() if factor is None else (factor,)),
            **_with_noise(self._take_draw(self._noise_coeff(timestep))))
        self._x0_prev = x0
        self._t_prev = int(timestep)
        self._step_index += 1
        return prev

    def _affine_coeffs(self, timestep) -> tuple[bool, tuple[float, ...]]:
        """(first, (ca, cb, cc, cx, ce)) of the step at ``timestep``; first:
        a first-order step, which reads no x0_prev."""
        t = int(timestep)
        t_prev = self._prev_timestep(t)
        a_t, s_t, l_t = (float(self.alpha_t[t]), float(self.sigma_t[t]),
                         float(self.lambda_t[t]))
        a_p, s_p, l_p = (float(self.alpha_t[t_prev]), float(self.sigma_t[t_prev]),
                         float(self.lambda_t[t_prev]))
        import math

        h = l_p - l_t
        C = a_p * (math.exp(-h) - 1.0)
        lead = s_p / s_t
        if self.stochastic:
            C = a_p * (math.exp(-2.0 * h) - 1.0)  # -B
            lead = lead * math.exp(-h)  # A
        first = (self._x0_prev is None or self.solver_order == 1
                 or self._step_index == len(self.timesteps) - 1)
        if first:
            cprime, cc = C, 0.0
        else:
            l_pp = float(self.lambda_t[self._t_prev])
            r0 = (l_t - l_pp) / h
            cprime = C * (1.0 + 0.5 / r0)
            cc = 0.5 * C / r0
        if self.v_prediction:
            cx, ce = a_t, -s_t
            return first, (lead - cprime * cx, -cprime * ce, cc, cx, ce)
        ca = lead - cprime / a_t
        cb = cprime * s_t / a_t
        cx = 1.0 / a_t
        ce = -s_t / a_t
        return first, (ca, cb, cc, cx, ce)

    def _masked_step_native(self, noise, timestep, sample, guidance_scale, mask, init,
                            init_noise, factor=None) -> torch.Tensor:
        from ..ops import masked_dpm_step

        first, coeffs = self._affine_coeffs(timestep)
        sa, sb = self._known_coeffs(timestep)
        prev, x0 = masked_dpm_step(noise, sample, None if first else self._x0_prev, init,
                                   init_noise, mask, guidance_scale, *coeffs, sa, sb, factor,
                                   self._take_draw(self._noise_coeff(timestep)))
        self._x0_prev = x0
        self._t_prev = int(timestep)
        self._step_index += 1
        return prev
