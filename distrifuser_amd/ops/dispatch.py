"""HIP-extension loading and CPU/GPU dispatch for the hot ops."""

from __future__ import annotations

import os

import torch

from . import eager

_EXT = None
_EXT_ERR: Exception | None = None


def _force_eager() -> bool:
    return os.environ.get("DFA_FORCE_EAGER", "0") == "1"


def hip_ext():
    """Load the in-tree HIP extension (built by setup.py / __graft_entry__.build)."""
    global _EXT, _EXT_ERR
    if _EXT is not None or _EXT_ERR is not None:
        if _EXT is None:
            raise RuntimeError(f"distrifuser_amd HIP extension failed to load: {_EXT_ERR}")
        return _EXT
    try:
        import importlib

        _EXT = importlib.import_module("distrifuser_amd._C")
    except Exception as exc:  # noqa: BLE001
        _EXT_ERR = exc
        raise RuntimeError(
            "distrifuser_amd HIP extension (_C) is not built. Run "
            "`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950). "
            f"Import error: {exc}"
        ) from exc
    return _EXT


def hip_ext_available() -> bool:
    try:
        hip_ext()
        return True
    except RuntimeError:
        return False


def use_hip(x: torch.Tensor) -> bool:
    """The one native-or-eager decision: a GPU tensor, DFA_FORCE_EAGER not 1."""
    return x.is_cuda and not _force_eager()


# -- public ops --------------------------------------------------------------


_FLASH_HEAD_DIMS = (40, 64, 80, 96, 128, 160)  # SD-family head dims
_KERNEL_DTYPES = (torch.bfloat16, torch.float16)  # element types of the MFMA kernels and LN


def _flash_ok(q: torch.Tensor, *kv: torch.Tensor) -> bool:
    if q.dtype not in _KERNEL_DTYPES or q.shape[-1] not in _FLASH_HEAD_DIMS:
        return False
    for t in (q, *kv):
        if t.dtype != q.dtype:
            return False
        if t.stride(-1) != 1:
            return False
        if any(s % 8 != 0 for s in t.stride()[:-1]):
            return False
        if t.dim() == 5 and t.shape[2] > 1 and t.shape[3] % 8 != 0:
            return False  # chunked KV: 8-token windows must not straddle chunks
    return True


def _check_kv_splits(kv_splits: int) -> int:
    if isinstance(kv_splits, bool) or not isinstance(kv_splits, int) or kv_splits < 1:
        raise ValueError(f"kv_splits must be a positive int, got {kv_splits!r}")
    return kv_splits


def flash_attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    *,
    kv_splits: int = 1,
    return_lse: bool = False,
):
    """Attention over (possibly strided) full-sequence KV.

    q: [B, H, Lq, D]; k, v: [B, H, Lkv, D] (arbitrary stride in the Lkv dim).
    kv_splits > 1 splits the KV range over that many blocks per Q block
    (clamped to the number of 128-token tiles) and merges the partials: same
    result up to fp32 rounding, a fuller grid when Lq is short. return_lse
    adds the fp32 softmax log-sum-exp [B, H, Lq]: returns (out, lse). The
    eager path accepts kv_splits and ignores it.
    """
    _check_kv_splits(kv_splits)
    if use_hip(q) and _flash_ok(q, k, v):
        if kv_splits == 1 and not return_lse:
            return hip_ext().flash_attention(q, k, v)
        res = hip_ext().flash_attention_ext(q, k, v, kv_splits, return_lse)
        return (res[0], res[1]) if return_lse else res[0]
    # CPU, or fp32 / odd head-dims on GPU (PyTorch's SDPA, rocm AOTriton path)
    if return_lse:
        return eager.flash_attention_lse(q, k, v)
    return eager.flash_attention(q, k, v)


def flash_attention_chunked(
    q: torch.Tensor, kv_chunks: torch.Tensor, heads: int, dim_head: int, kv_splits: int = 1
) -> torch.Tensor:
    """Displaced-patch attention: q [B, Lq, inner]; kv_chunks is the flat comm
    buffer viewed as [n_peers, B, L_local, 2*inner] (strided — peer rows live
    in the flat buffer). On GPU the gfx950 kernel walks the chunks in place
    (kv_splits as in flash_attention; a split may start mid-chunk); the eager
    path materializes the concatenated KV.
    """
    _check_kv_splits(kv_splits)
    b, lq, inner = q.shape
    n, _, l, _ = kv_chunks.shape
    if use_hip(q):
        q4 = q.view(b, lq, heads, dim_head).permute(0, 2, 1, 3)
        k = kv_chunks[..., :inner].unflatten(-1, (heads, dim_head)).permute(1, 3, 0, 2, 4)
        v = kv_chunks[..., inner:].unflatten(-1, (heads, dim_head)).permute(1, 3, 0, 2, 4)
        if _flash_ok(q4, k, v):
            if kv_splits == 1:
                o = hip_ext().flash_attention(q4, k, v)  # [B,H,Lq,D] (view of B,Lq,H,D)
            else:
                o = hip_ext().flash_attention_ext(q4, k, v, kv_splits, False)[0]
            return o.transpose(1, 2).reshape(b, lq, inner)
    full_kv = kv_chunks.permute(1, 0, 2, 3).reshape(b, n * l, 2 * inner)
    k, v = full_kv.split(inner, dim=-1)
    q4 = q.view(b, lq, heads, dim_head).transpose(1, 2)
    k = k.view(b, n * l, heads, dim_head).transpose(1, 2)
    v = v.view(b, n * l, heads, dim_head).transpose(1, 2)
    out = flash_attention(q4, k.contiguous(), v.contiguous(), kv_splits=kv_splits)
    return out.transpose(1, 2).reshape(b, lq, inner)


def merge_attention(
    o_parts: torch.Tensor,
    lse_parts: torch.Tensor,
    *,
    out_dtype: torch.dtype | None = None,
    return_lse: bool = False,
):
    """Merge attention results over disjoint KV slices by their log-sum-exp.

    o_parts: [S, B, Lq, H, D] (each part normalised over its own slice),
    lse_parts: [S, B, H, Lq]. Returns out [B, Lq, H, D] in out_dtype (default:
    the parts' dtype), with return_lse also the merged fp32 lse [B, H, Lq].
    Parts with lse = -inf weigh 0; all -inf gives zeros and lse = -inf. The
    gfx950 kernel takes contiguous fp32 parts and writes bf16, fp16 or fp32;
    anything else runs the eager reference.
    """
    dt = o_parts.dtype if out_dtype is None else out_dtype
    if (
        use_hip(o_parts)
        and o_parts.dtype == torch.float32
        and lse_parts.dtype == torch.float32
        and dt in (torch.bfloat16, torch.float16, torch.float32)
        and o_parts.dim() == 5
        and o_parts.shape[-1] % 8 == 0
        and o_parts.is_contiguous()
        and lse_parts.is_contiguous()
    ):
        out, lse = hip_ext().merge_attention(o_parts, lse_parts, dt == torch.bfloat16, dt)
    else:
        out, lse = eager.merge_attention(o_parts, lse_parts, dt)
    return (out, lse) if return_lse else out


# Split-KV policy: a three-constant cost model fitted to the sweep in
# profiles/attention_splitkv_notes.md (24 timings, six shapes, head_dim 64).
_KV_TILE = 128  # KV tokens per LDS tile of the kernel; splits are tile-aligned
_Q_BLOCK = 256  # Q rows per block
_TILE_US = 2.4  # one 128-token tile of one block alone on its CU (DPAD 64)
_MERGE_LAUNCH_US = 5.0  # the second launch of a split call
_MERGE_BYTES_PER_US = 4.0e6  # fp32 partials written once and read once
_BLOCKS_PER_CU = 2  # resident 8-wave blocks per CU at DPAD 64 (128 VGPRs)
_MIN_TILES_PER_SPLIT = 2  # one-tile splits measured slower than two-tile ones
_MAX_KV_SPLITS = 8
_MIN_GAIN = 0.05  # predicted gain below this stays unsplit
_DEFAULT_CUS = 256  # MI355X


def attention_kv_splits(
    b: int,
    heads: int,
    lq: int,
    lkv: int,
    dim_head: int,
    device=None,
    *,
    multi_processor_count: int | None = None,
) -> int:
    """How many KV splits the attention kernel should use for this shape.

    Pure shape arithmetic (never synchronises; reads the CU count from the
    device properties unless multi_processor_count is given). Blocks that
    share a CU share its throughput, so with blocks = ceil(lq/256) * b * heads
    and T = ceil(lkv/128) a call costs about
        ceil(T/S) * ceil(blocks * S / CUs) tile times
    plus, for S > 1, a second launch and the fp32 partials' round trip through
    memory. The S in {1, 2, 4, 8}, S <= T // 2, with the least predicted time is returned
    if it gains at least 5 %, else 1. A grid that already takes every resident
    block slot (2 per CU) returns 1 outright, and a short KV range
    (cross-attention, Lkv = 77) has nothing to split. Head dims above 64 return 1: no sweep covers them.
    """
    if dim_head > 64 or min(b, heads, lq, lkv) <= 0:
        return 1
    cus = multi_processor_count
    if cus is None:
        cus = _DEFAULT_CUS
        if torch.cuda.is_available() and (device is None or torch.device(device).type == "cuda"):
            cus = torch.cuda.get_device_properties(device).multi_processor_count
    blocks = -(-lq // _Q_BLOCK) * b * heads
    tiles = -(-lkv // _KV_TILE)
    if blocks >= cus * _BLOCKS_PER_CU:
        return 1  # every resident-block slot is taken: the plain grid fills the GPU
    part_bytes = 2 * 4 * b * heads * lq * dim_head  # one part: written, then read

    def cost(s: int) -> float:
        t = _TILE_US * -(-tiles // s) * -(-blocks * s // cus)
        if s > 1:
            t += _MERGE_LAUNCH_US + s * part_bytes / _MERGE_BYTES_PER_US
        return t

    s_max = max(1, min(_MAX_KV_SPLITS, tiles // _MIN_TILES_PER_SPLIT))
    best = min((s for s in (1, 2, 4, 8) if s <= s_max), key=cost)  # the S values swept
    return best if cost(best) < (1.0 - _MIN_GAIN) * cost(1) else 1


def group_norm_stats(x: torch.Tensor, num_groups: int) -> torch.Tensor:
    if use_hip(x):
        return hip_ext().group_norm_stats(x, num_groups)
    return eager.group_norm_stats(x, num_groups)


def group_norm_apply(x, mean, meansq, weight, bias, eps, silu=False, tokens=False):
    """tokens=True: the same values as [N, H*W, C] contiguous (the kernel
    writes them in that order; no NCHW result exists in between)."""
    if use_hip(x):
        n = x.shape[0]
        g = mean.reshape(n, -1).shape[1]
        return hip_ext().group_norm_apply(
            x,
            mean.reshape(n, g).contiguous(),
            meansq.reshape(n, g).contiguous(),
            weight,
            bias,
            eps,
            silu,
            tokens,
        )
    return eager.group_norm_apply(x, mean, meansq, weight, bias, eps, silu, tokens)


def group_norm_silu(x, num_groups, weight, bias, eps, silu=True, tokens=False):
    if use_hip(x):
        return hip_ext().group_norm_silu(x, num_groups, weight, bias, eps, silu, tokens)
    return eager.group_norm_silu(x, num_groups, weight, bias, eps, silu, tokens)


_BOUNDARY_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def tokens_add_nchw(y: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
    """y [N, H*W, C] + residual [N, C, H, W] -> [N, C, H, W] contiguous.

    The transformer's closing residual add with the token -> NCHW transpose
    inside. residual may be a batch or channel slice of a wider tensor; a
    residual whose (H, W) plane is not contiguous, mixed dtypes and dtypes
    outside bf16 / fp16 / fp32 take the eager composition.
    """
    if (
        use_hip(y)
        and y.dtype in _BOUNDARY_DTYPES
        and residual.dtype == y.dtype
        and residual.is_cuda
        and residual.dim() == 4
        and (residual.shape[3] <= 1 or residual.stride(3) == 1)
        and (residual.shape[2] <= 1 or residual.stride(2) == residual.shape[3])
    ):
        return hip_ext().tokens_add_nchw(y, residual)
    return eager.tokens_add_nchw(y, residual)


def _f32(t: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    return t.to(device=like.device, dtype=torch.float32)


def guidance_rescale_factor(noise: torch.Tensor, g: float, phi: float) -> torch.Tensor:
    """fp32 [1]: phi * std(cond) / std(cfg) + (1 - phi) of the [2,C,h,w] CFG
    pair, cfg = nu + g*(nc - nu), the standard deviations over the one sample
    (diffusers ``rescale_noise_cfg``). Two launches on GPU with fp32 sums in a
    fixed order: the same bits on every run. The step ops take the result as
    their ``factor``."""
    if use_hip(noise) and noise.dtype in _BOUNDARY_DTYPES:
        return hip_ext().guidance_rescale_factor(noise, g, phi)
    return eager.guidance_rescale_factor(noise, g, phi)


def _with_factor(factor) -> tuple:
    """The trailing arguments of a native step: none without a factor, so a
    plain step makes the call it always made."""
    return () if factor is None else (factor,)


def _with_noise(step_noise) -> dict:
    """The keyword of a noisy native step: none without noise, as _with_factor."""
    return {} if step_noise is None else {"step_noise": step_noise}


def philox_normal(numel: int, seed: int, draw: int, offset: int = 0, device=None) -> torch.Tensor:
    """fp32 [numel]: the Philox4x32-10 / Box-Muller standard normals of
    elements offset .. offset + numel - 1 of the stream (seed, draw), the noise
    the stochastic scheduler steps add. A pure function of (seed, draw,
    element index): see ``eager.philox_normal`` for the rule. One launch on a
    GPU device; the eager twin elsewhere."""
    dev = torch.device("cpu" if device is None else device)
    if dev.type == "cuda" and not _force_eager():
        index = torch.cuda.current_device() if dev.index is None else dev.index
        return hip_ext().philox_normal(numel, seed, draw, offset, index)
    return eager.philox_normal(numel, seed, draw, offset, dev)


def cfg_affine_step(noise, x, g, ca, cb, factor=None, step_noise=None):
    """CFG combine + affine scheduler update in one launch on GPU:

        eps = nu + g*(nc - nu),   x' = ca*x + cb*eps (+ cn*z)

    noise is the [2,C,h,w] pair. step_noise = (cn, seed, draw) adds the noise
    term of a stochastic sampler, z = ``philox_normal(x.numel(), seed, draw)``
    drawn inside the kernel; x must then be [1,C,h,w], and noise may also be
    one branch's output in x's shape (eps = noise, g not read). cn == 0 gives
    the bits of the call without step_noise."""
    if use_hip(x) and x.dtype in _BOUNDARY_DTYPES:
        return hip_ext().cfg_affine_step(noise, x, g, ca, cb, *_with_factor(factor),
                                         **_with_noise(step_noise))
    return eager.cfg_affine_step(noise, x, g, ca, cb, factor, step_noise)


def cfg_dpm_step(noise, x, x0_prev, g, ca, cb, cc, cx, ce, factor=None, step_noise=None):
    """CFG combine + DPM-Solver++(2M) update in one launch on GPU ->
    (prev, x0 fp32): prev = ca*x + cb*eps + cc*x0_prev (+ cn*z), x0 = cx*x +
    ce*eps. step_noise as in cfg_affine_step; x0 never sees it."""
    if use_hip(x) and x.dtype in _BOUNDARY_DTYPES:
        prev, x0 = hip_ext().cfg_dpm_step(noise, x, x0_prev, g, ca, cb, cc, cx, ce,
                                          *_with_factor(factor), **_with_noise(step_noise))
        return prev, x0
    return eager.cfg_dpm_step(noise, x, x0_prev, g, ca, cb, cc, cx, ce, factor, step_noise)


def masked_affine_step(noise, x, init, init_noise, mask, g, ca, cb, sa, sb, factor=None,
                       step_noise=None):
    """Inpaint step of DDIM / Euler in one launch on GPU:

        eps = nu + g*(nc - nu)   (noise [2,C,h,w]; eps = noise for [1,C,h,w])
        x'  = ca*x + cb*eps (+ cn*z)
        out = m*x' + (1 - m)*(sa*init + sb*init_noise)

    x [1,C,h,w] in bf16, fp16 or fp32; init, init_noise fp32 [1,C,h,w]; mask
    fp32 with h*w elements, shared by the channels. factor (from
    ``guidance_rescale_factor``, CFG pair only) scales eps first. step_noise
    as in cfg_affine_step."""
    if use_hip(x) and x.dtype in _BOUNDARY_DTYPES:
        return hip_ext().masked_affine_step(noise, x, _f32(init, x), _f32(init_noise, x),
                                            _f32(mask, x), g, ca, cb, sa, sb,
                                            *_with_factor(factor), **_with_noise(step_noise))
    return eager.masked_affine_step(noise, x, init, init_noise, mask, g, ca, cb, sa, sb, factor,
                                    step_noise)


def masked_dpm_step(noise, x, x0_prev, init, init_noise, mask, g, ca, cb, cc, cx, ce, sa, sb,
                    factor=None, step_noise=None):
    """Inpaint step of DPM-Solver++(2M): cfg_dpm_step with the blend of
    masked_affine_step on prev. Returns (prev, x0); x0 (fp32) is not blended.
    factor and step_noise as in masked_affine_step."""
    if use_hip(x) and x.dtype in _BOUNDARY_DTYPES:
        prev, x0 = hip_ext().masked_dpm_step(noise, x, x0_prev, _f32(init, x),
                                             _f32(init_noise, x), _f32(mask, x), g, ca, cb, cc,
                                             cx, ce, sa, sb, *_with_factor(factor),
                                             **_with_noise(step_noise))
        return prev, x0
    return eager.masked_dpm_step(noise, x, x0_prev, init, init_noise, mask, g, ca, cb, cc, cx,
                                 ce, sa, sb, factor, step_noise)


def inpaint_unet_input(latents, mask, masked_latents, scale=1.0, copies=1):
    """The 9-channel inpaint U-Net input [copies, 9, h, w] in one launch on
    GPU: latents [1,4,h,w] / scale, the mask [1,1,h,w] and the masked-image
    latents [1,4,h,w], all in the latents' dtype; copies is 2 with CFG."""
    if use_hip(latents) and latents.dtype in _BOUNDARY_DTYPES:
        return hip_ext().inpaint_unet_input(latents, mask, masked_latents, scale, copies)
    return eager.inpaint_unet_input(latents, mask, masked_latents, scale, copies)


def layer_norm(x, weight, bias, eps):
    if use_hip(x) and x.dtype in _KERNEL_DTYPES and x.shape[-1] % 8 == 0 and x.shape[-1] <= 2048:
        return hip_ext().layer_norm(x, weight, bias, eps)
    return eager.layer_norm(x, weight, bias, eps)


def add_layer_norm(x, res, weight, bias, eps):
    """(x + res, LN(x + res)) in one kernel on GPU."""
    if use_hip(x) and x.dtype in _KERNEL_DTYPES and x.shape[-1] % 8 == 0 and x.shape[-1] <= 2048:
        s, y = hip_ext().add_layer_norm(x, res, weight, bias, eps)
        return s, y
    return eager.add_layer_norm(x, res, weight, bias, eps)


def vae_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """Single-head d=512 attention, q/k/v [B, L, 512] (VAE mid block)."""
    if use_hip(q) and q.dtype in _KERNEL_DTYPES and q.shape[-1] == 512:
        return hip_ext().vae_attention(q, k, v)
    return eager.vae_attention(q, k, v)


def geglu(hidden: torch.Tensor) -> torch.Tensor:
    if use_hip(hidden):
        return hip_ext().geglu(hidden)
    return eager.geglu(hidden)
