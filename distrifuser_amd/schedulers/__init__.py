from .ddim import DDIMScheduler
from .euler import EulerDiscreteScheduler
from .dpm_solver import DPMSolverMultistepScheduler


def get_scheduler(name: str, **config):
    """The scheduler ``name``; ``config`` goes to its constructor
    (prediction_type, timestep_spacing, rescale_betas_zero_snr, the betas)."""
    name = name.lower().replace("_", "-")
    if name == "ddim":
        return DDIMScheduler(**config)
    if name == "euler":
        return EulerDiscreteScheduler(**config)
    if name in ("dpm-solver", "dpmsolver", "dpm"):
        return DPMSolverMultistepScheduler(**config)
    raise ValueError(f"unknown scheduler {name!r} (ddim | euler | dpm-solver)")


__all__ = [
    "DDIMScheduler",
    "EulerDiscreteScheduler",
    "DPMSolverMultistepScheduler",
    "get_scheduler",
]
