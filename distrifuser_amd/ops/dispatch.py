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


def _check_compute_dtype(compute_dtype, kv_splits: int, return_lse: bool) -> bool:
    """True for "fp8"; None is the 16-bit path."""
    if compute_dtype is None:
        return False
    if compute_dtype != "fp8":
        raise ValueError(f"compute_dtype must be None or 'fp8', got {compute_dtype!r}")
    if kv_splits > 1 or return_lse:
        raise ValueError("compute_dtype='fp8' has no split-KV or log-sum-exp mode")
    return True


def split_heads(x: torch.Tensor, heads: int) -> torch.Tensor:
    """[B, L, heads*D] -> [B, heads, L, D], a view: x may be a column slice of
    a fused projection, and the attention kernels read it in place."""
    b, l, inner = x.shape
    return x.view(b, l, heads, inner // heads).transpose(1, 2)


def merge_heads(x: torch.Tensor) -> torch.Tensor:
    """[B, H, L, D] -> [B, L, H*D]: the inverse of split_heads. A view of the
    kernels' output, which is [B, L, H, D] in memory."""
    b, h, l, d = x.shape
    return x.transpose(1, 2).reshape(b, l, h * d)


def _chunk_views(q: torch.Tensor, kv_chunks: torch.Tensor, heads: int):
    """q [B,Lq,inner], kv_chunks [n,B,L,2*inner] -> q [B,H,Lq,D] and k, v
    [B,H,n,L,D], all views: k and v are the two column halves of the buffer."""
    k, v = (t.unflatten(-1, (heads, -1)).permute(1, 3, 0, 2, 4) for t in kv_chunks.chunk(2, dim=-1))
    return split_heads(q, heads), k, v


def _flash_native(q, k, v, kv_splits: int, return_lse: bool, fp8: bool):
    """The result of the extension entry that serves this call (q [B,H,Lq,D],
    k/v [B,H,Lkv,D] or chunked [B,H,NC,LC,D]), or None where none does: CPU,
    DFA_FORCE_EAGER=1, what _flash_ok refuses, fp8 off head_dim 64."""
    if not (use_hip(q) and _flash_ok(q, k, v)) or (fp8 and q.shape[-1] != 64):
        return None
    if fp8:
        return hip_ext().flash_attention_fp8(q, k, v)
    if kv_splits == 1 and not return_lse:
        return hip_ext().flash_attention(q, k, v)
    res = hip_ext().flash_attention_ext(q, k, v, kv_splits, return_lse)
    return (res[0], res[1]) if return_lse else res[0]


def flash_attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    *,
    kv_splits: int = 1,
    return_lse: bool = False,
    compute_dtype: str | None = None,
):
    """Attention over (possibly strided) full-sequence KV.

    q: [B, H, Lq, D]; k, v: [B, H, Lkv, D] (arbitrary stride in the Lkv dim).
    kv_splits > 1 splits the KV range over that many blocks per Q block
    (clamped to the number of 128-token tiles) and merges the partials: same
    result up to fp32 rounding, a fuller grid when Lq is short. return_lse
    adds the fp32 softmax log-sum-exp [B, H, Lq]: returns (out, lse). The
    eager path accepts kv_splits and ignores it.

    compute_dtype="fp8": q, k, v and the probabilities are e4m3 with
    power-of-two block scales, accumulation stays fp32 (the rule is
    ``eager.flash_attention_fp8``). bf16 / fp16 inputs with head_dim 64 run the
    gfx950 fp8 kernels; CPU, DFA_FORCE_EAGER=1, fp32 and other head dims run
    that eager twin, so "fp8" always means the same arithmetic. Not with
    kv_splits > 1 or return_lse.
    """
    _check_kv_splits(kv_splits)
    fp8 = _check_compute_dtype(compute_dtype, kv_splits, return_lse)
    out = _flash_native(q, k, v, kv_splits, return_lse, fp8)
    if out is not None:
        return out
    if fp8:
        if k.dim() == 5:
            k, v = k.flatten(2, 3), v.flatten(2, 3)
        return eager.flash_attention_fp8(q, k, v)
    # CPU, or fp32 / odd head-dims on GPU (PyTorch's SDPA, rocm AOTriton path)
    if return_lse:
        return eager.flash_attention_lse(q, k, v)
    return eager.flash_attention(q, k, v)


def flash_attention_chunked(
    q: torch.Tensor, kv_chunks: torch.Tensor, heads: int, dim_head: int, kv_splits: int = 1,
    compute_dtype: str | None = None,
) -> torch.Tensor:
    """Displaced-patch attention: q [B, Lq, inner]; kv_chunks is the flat comm
    buffer viewed as [n_peers, B, L_local, 2*inner] (strided — peer rows live
    in the flat buffer). On GPU the gfx950 kernel walks the chunks in place
    (kv_splits as in flash_attention; a split may start mid-chunk); the eager
    path materializes the concatenated KV. compute_dtype as in flash_attention
    (the fp8 pre-pass walks the chunks in place).
    """
    _check_kv_splits(kv_splits)
    fp8 = _check_compute_dtype(compute_dtype, kv_splits, False)
    q4, k, v = _chunk_views(q, kv_chunks, heads)
    out = _flash_native(q4, k, v, kv_splits, False, fp8)
    if out is None and fp8:
        out = eager.flash_attention_fp8(q4, k.flatten(2, 3), v.flatten(2, 3))
    elif out is None:
        n, b, l, _ = kv_chunks.shape
        full_kv = kv_chunks.permute(1, 0, 2, 3).reshape(b, n * l, -1)
        k, v = (split_heads(t, heads).contiguous() for t in full_kv.chunk(2, dim=-1))
        out = flash_attention(q4, k, v, kv_splits=kv_splits)  # may still reach the kernel
    return merge_heads(out)


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
        out, lse = hip_ext().merge_attention(o_parts, lse_parts, out_dtype=dt)
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


def _step_ops(x: torch.Tensor, *blend: torch.Tensor) -> tuple:
    """(the module whose fused step ops serve x, *blend as those take it): the
    extension for a GPU x in bf16, fp16 or fp32, with the blend's init,
    init_noise and mask as fp32 on x's device; else the eager twins."""
    if use_hip(x) and x.dtype in _BOUNDARY_DTYPES:
        return hip_ext(), *(_f32(t, x) for t in blend)
    return eager, *blend


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
    (ops,) = _step_ops(x)
    return ops.cfg_affine_step(noise, x, g, ca, cb, factor, step_noise)


def cfg_dpm_step(noise, x, x0_prev, g, ca, cb, cc, cx, ce, factor=None, step_noise=None):
    """CFG combine + DPM-Solver++(2M) update in one launch on GPU ->
    (prev, x0 fp32): prev = ca*x + cb*eps + cc*x0_prev (+ cn*z), x0 = cx*x +
    ce*eps. step_noise as in cfg_affine_step; x0 never sees it."""
    (ops,) = _step_ops(x)
    prev, x0 = ops.cfg_dpm_step(noise, x, x0_prev, g, ca, cb, cc, cx, ce, factor, step_noise)
    return prev, x0


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
    ops, init, init_noise, mask = _step_ops(x, init, init_noise, mask)
    return ops.masked_affine_step(noise, x, init, init_noise, mask, g, ca, cb, sa, sb, factor,
                                  step_noise)


def masked_dpm_step(noise, x, x0_prev, init, init_noise, mask, g, ca, cb, cc, cx, ce, sa, sb,
                    factor=None, step_noise=None):
    """Inpaint step of DPM-Solver++(2M): cfg_dpm_step with the blend of
    masked_affine_step on prev. Returns (prev, x0); x0 (fp32) is not blended.
    factor and step_noise as in masked_affine_step."""
    ops, init, init_noise, mask = _step_ops(x, init, init_noise, mask)
    prev, x0 = ops.masked_dpm_step(noise, x, x0_prev, init, init_noise, mask, g, ca, cb, cc, cx,
                                   ce, sa, sb, factor, step_noise)
    return prev, x0


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


_GL_NT, _GL_KSTEP = 128, 64  # csrc/geglu_linear.hip: outputs per block, k per LDS stage


def pack_geglu_weight(weight: torch.Tensor, dtype: torch.dtype | None = None) -> torch.Tensor:
    """[2*inner, K] (value rows, then gate rows) -> [CT, KP/16, 8, 64, 8] in
    dtype (default: the weight's): the geglu_linear kernel's LDS image.

    Column tile ct (128 outputs), 16-k slice kk, fragment f = vg*4 + sub (vg 0
    value / 1 gate, sub the 32-output sub-tile) holds in lane l the A operand
    of mfma_f32_32x32x16: row vg*inner + ct*128 + sub*32 + (l&31), k = kk*16 +
    (l>>5)*8 + j. A K-step of 64 is four consecutive slices, 32 KiB with value
    and gate interleaved. inner is zero-padded to a multiple of 128, K to 64.
    """
    dtype = weight.dtype if dtype is None else dtype
    if dtype not in _KERNEL_DTYPES:
        raise ValueError(f"pack_geglu_weight: dtype must be bf16 or fp16, got {dtype}")
    two_inner, k = weight.shape
    inner = two_inner // 2
    if two_inner != 2 * inner:
        raise ValueError(f"pack_geglu_weight: weight must be [2*inner, K], got {tuple(weight.shape)}")
    n_p = -(-inner // _GL_NT) * _GL_NT
    k_p = -(-k // _GL_KSTEP) * _GL_KSTEP
    wp = weight.new_zeros(2, n_p, k_p, dtype=dtype)
    wp[:, :inner, :k] = weight.detach().reshape(2, inner, k).to(dtype)
    wp = wp.reshape(2, n_p // _GL_NT, 4, 32, k_p // 16, 2, 8)  # [vg, ct, sub, r, kk, hi, j]
    wp = wp.permute(1, 4, 0, 2, 5, 3, 6)                        # [ct, kk, vg, sub, hi, r, j]
    return wp.reshape(n_p // _GL_NT, k_p // 16, 8, 64, 8).contiguous()


def _geglu_linear_ok(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> bool:
    k = x.shape[-1]
    rows_ok = x.is_contiguous() or (
        x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= k and x.stride(0) % 8 == 0
    )
    return (
        x.dtype in _KERNEL_DTYPES
        and weight.dtype == x.dtype
        and bias.dtype == x.dtype
        and x.numel() > 0
        and k % 8 == 0
        and weight.shape[0] % 16 == 0
        and rows_ok
        and x.stride(-1) == 1
        and x.data_ptr() % 16 == 0
    )


def geglu_linear(x, weight, bias, packed=None):
    """The GEGLU projection in one kernel: x [..., K], weight [2*inner, K]
    (value rows first, gate rows second: ``nn.Linear``'s layout), bias
    [2*inner] -> [..., inner],

        out = round((x.W[:inner] + b[:inner]) * gelu(x.W[inner:] + b[inner:]))

    16-bit products summed in fp32, fp32 bias and erf gelu, one rounding (the
    rule is ``eager.geglu_linear``). On GPU, bf16 or fp16 throughout, K % 8 ==
    0, inner % 8 == 0 and contiguous rows run the gfx950 MFMA kernel on
    ``packed`` (``pack_geglu_weight(weight)``, packed here when not given);
    CPU, DFA_FORCE_EAGER=1, fp32 and every other layout run the eager rule.
    """
    if use_hip(x) and _geglu_linear_ok(x, weight, bias):
        if packed is None:
            packed = pack_geglu_weight(weight)
        return hip_ext().geglu_linear(x, packed, bias, weight.shape[0] // 2)
    return eager.geglu_linear(x, weight, bias)
