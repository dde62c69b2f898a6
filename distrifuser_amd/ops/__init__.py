"""Device ops: hand-written gfx950 HIP kernels with eager CPU references.

Dispatch rule: on a ROCm GPU the HIP extension is REQUIRED — a missing
extension raises instead of silently falling back to eager PyTorch (so GPU
runs always exercise the native kernels). On CPU the eager reference path
runs, which is what the non-GPU test suite checks numerics against.
Set DFA_FORCE_EAGER=1 to force the eager path on GPU (A/B debugging only).
"""

from .conv import NativeConv2d, conv3x3_halo, pack_conv3x3_weight
from .dispatch import (
    add_layer_norm,
    attention_kv_splits,
    cfg_affine_step,
    cfg_dpm_step,
    flash_attention,
    flash_attention_chunked,
    geglu,
    group_norm_apply,
    group_norm_silu,
    group_norm_stats,
    guidance_rescale_factor,
    hip_ext,
    hip_ext_available,
    inpaint_unet_input,
    layer_norm,
    masked_affine_step,
    masked_dpm_step,
    merge_attention,
    philox_normal,
    tokens_add_nchw,
    use_hip,
    vae_attention,
)
from .norm import PlainGroupNorm

__all__ = [
    "NativeConv2d",
    "PlainGroupNorm",
    "add_layer_norm",
    "attention_kv_splits",
    "cfg_affine_step",
    "cfg_dpm_step",
    "layer_norm",
    "conv3x3_halo",
    "flash_attention",
    "flash_attention_chunked",
    "geglu",
    "group_norm_apply",
    "group_norm_silu",
    "group_norm_stats",
    "guidance_rescale_factor",
    "hip_ext",
    "hip_ext_available",
    "inpaint_unet_input",
    "masked_affine_step",
    "masked_dpm_step",
    "merge_attention",
    "pack_conv3x3_weight",
    "philox_normal",
    "tokens_add_nchw",
    "use_hip",
    "vae_attention",
]
