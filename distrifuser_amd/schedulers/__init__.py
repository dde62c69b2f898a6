from .ddim import DDIMScheduler
from .euler import EulerDiscreteScheduler
from .euler_ancestral import EulerAncestralDiscreteScheduler
from .dpm_solver import DPMSolverMultistepScheduler

_NAMES = "ddim | euler | euler-a | dpm-solver"


def scheduler_class(name: str):
    """The scheduler class of a ``get_scheduler`` name."""
    name = name.lower().replace("_", "-")
    if name == "ddim":
        return DDIMScheduler
    if name == "euler":
        return EulerDiscreteScheduler
    if name in ("euler-a", "euler-ancestral"):
        return EulerAncestralDiscreteScheduler
    if name in ("dpm-solver", "dpmsolver", "dpm"):
        return DPMSolverMultistepScheduler
    raise ValueError(f"unknown scheduler {name!r} ({_NAMES})")


def get_scheduler(name: str, **config):
    """The scheduler ``name``; ``config`` goes to its constructor
    (prediction_type, timestep_spacing, rescale_betas_zero_snr, the betas, and
    what one class alone takes: ``eta`` for ddim, ``algorithm_type`` for
    dpm-solver, where ``"sde-dpmsolver++"`` is the stochastic variant)."""
    return scheduler_class(name)(**config)


__all__ = [
    "DDIMScheduler",
    "EulerDiscreteScheduler",
    "EulerAncestralDiscreteScheduler",
    "DPMSolverMultistepScheduler",
    "get_scheduler",
    "scheduler_class",
]
