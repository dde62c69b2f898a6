"""Eager PyTorch reference implementations of every HIP kernel.

These define the NUMERICS contract: each gfx950 kernel in ops/hip/ is
unit-tested against the fp32 run of the matching function here
(tests/test_ops_gpu.py). They also serve as the CPU execution path for the
no-GPU test suite.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """softmax(q k^T / sqrt(d)) v with rectangular Lq x Lkv.

    q: [B, H, Lq, D]; k, v: [B, H, Lkv, D]. Returns [B, H, Lq, D].
    """
    return F.scaled_dot_product_attention(q, k, v, dropout_p=0.0, is_causal=False)


def flash_attention_lse(
    q: torch.Tensor, k: torch.Tensor, v: torch.Tensor
) -> tuple[torch.Tensor, torch.Tensor]:
    """fp32 reference of attention with its softmax log-sum-exp.

    Returns (out [B, H, Lq, D] in q.dtype, lse [B, H, Lq] fp32) with
    lse = ln sum_k exp(q.k / sqrt(d)). An empty KV range gives out = 0 and
    lse = -inf.
    """
    scores = torch.einsum("bhqd,bhkd->bhqk", q.float(), k.float()) * q.shape[-1] ** -0.5
    lse = torch.logsumexp(scores, dim=-1)
    probs = torch.exp(scores - lse.unsqueeze(-1))
    out = torch.einsum("bhqk,bhkd->bhqd", probs, v.float())
    return out.to(q.dtype), lse


def merge_attention(
    o_parts: torch.Tensor, lse_parts: torch.Tensor, out_dtype: torch.dtype | None = None
) -> tuple[torch.Tensor, torch.Tensor]:
    """Merge attention results computed over disjoint KV slices.

    o_parts: [S, B, Lq, H, D] normalised partial outputs; lse_parts:
    [S, B, H, Lq]. With m = max_s lse_s and w_s = exp(lse_s - m):
    out = sum_s w_s o_s / sum_s w_s and lse = m + ln sum_s w_s, summed in part
    order in fp32. A part with lse = -inf has weight 0 whatever it holds; if
    every part is -inf the output is zeros and lse = -inf (never NaN).
    Returns (out [B, Lq, H, D], lse [B, H, Lq] fp32).
    """
    lse_f = lse_parts.float()
    m = lse_f.max(dim=0).values
    empty = torch.isneginf(m)
    w = torch.exp(lse_f - torch.where(empty, torch.zeros_like(m), m))  # exp(-inf) = 0
    wsum = w.sum(dim=0)
    wq = w.permute(0, 1, 3, 2).unsqueeze(-1)  # [S, B, Lq, H, 1]
    acc = torch.where(wq > 0, wq * o_parts.float(), torch.zeros((), device=w.device)).sum(dim=0)
    denom = torch.where(empty, torch.ones_like(wsum), wsum).permute(0, 2, 1).unsqueeze(-1)
    out = acc / denom
    lse = torch.where(empty, m, m + torch.log(wsum))
    return out.to(o_parts.dtype if out_dtype is None else out_dtype), lse


def group_norm_stats(x: torch.Tensor, num_groups: int) -> torch.Tensor:
    """Per-(sample, group) first/second moments over (group_size, H, W).

    x: [N, C, H, W] -> [2, N, G, 1, 1, 1] stacked (E[x], E[x^2]), computed in
    fp32 and cast back to x.dtype (the stale-stats comm slot dtype).
    """
    n, c, h, w = x.shape
    xg = x.reshape(n, num_groups, -1).float()
    mean = xg.mean(dim=-1)
    meansq = (xg * xg).mean(dim=-1)
    return torch.stack([mean, meansq], dim=0).reshape(2, n, num_groups, 1, 1, 1).to(x.dtype)


def nchw_to_tokens(x: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] -> [N, H*W, C] contiguous (the transformer's token layout)."""
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n, h * w, c).contiguous()


def tokens_add_nchw(y: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
    """y [N, H*W, C] back to NCHW plus residual [N, C, H, W], contiguous."""
    n, c, h, w = residual.shape
    return (y.reshape(n, h, w, c).permute(0, 3, 1, 2) + residual).contiguous()


def group_norm_apply(
    x: torch.Tensor,
    mean: torch.Tensor,
    meansq: torch.Tensor,
    weight: torch.Tensor | None,
    bias: torch.Tensor | None,
    eps: float,
    silu: bool = False,
    tokens: bool = False,
) -> torch.Tensor:
    """Normalize x with externally supplied group stats; optionally fuse SiLU.

    x: [N, C, H, W]; mean/meansq: broadcastable to [N, G] (e.g. the
    [N, G, 1, 1, 1] comm-slot views). var = E[x^2] - E[x]^2 (population
    variance, matching F.group_norm; we deliberately drop the reference's
    n/(n-1) Bessel factor — see reference pp/groupnorm.py:65-66 — so that
    full_sync output is bit-identical to the single-GPU oracle).
    """
    n, c, h, w = x.shape
    g = mean.reshape(n, -1).shape[1]
    mean = mean.reshape(n, g, 1).float()
    meansq = meansq.reshape(n, g, 1).float()
    var = (meansq - mean * mean).clamp_min_(0.0)
    inv_std = torch.rsqrt(var + eps)
    out = (x.reshape(n, g, -1).float() - mean) * inv_std
    out = out.reshape(n, c, h, w)
    if weight is not None:
        out = out * weight.float().view(1, -1, 1, 1)
    if bias is not None:
        out = out + bias.float().view(1, -1, 1, 1)
    if silu:
        out = F.silu(out)
    out = out.to(x.dtype)
    return nchw_to_tokens(out) if tokens else out


def group_norm_silu(
    x: torch.Tensor,
    num_groups: int,
    weight: torch.Tensor | None,
    bias: torch.Tensor | None,
    eps: float,
    silu: bool = True,
    tokens: bool = False,
) -> torch.Tensor:
    """Plain (single-device) GroupNorm with fused SiLU epilogue.

    tokens=True returns the same values as [N, H*W, C] contiguous.
    """
    out = F.group_norm(x.float(), num_groups, None if weight is None else weight.float(),
                       None if bias is None else bias.float(), eps)
    if silu:
        out = F.silu(out)
    out = out.to(x.dtype)
    return nchw_to_tokens(out) if tokens else out


def geglu(hidden: torch.Tensor) -> torch.Tensor:
    """GEGLU gate: split last dim in half, return a * gelu(b) (tanh=false)."""
    a, b = hidden.chunk(2, dim=-1)
    return a * F.gelu(b)


def layer_norm(x, weight, bias, eps):
    import torch.nn.functional as _F

    return _F.layer_norm(x, (x.shape[-1],), weight, bias, eps)


def add_layer_norm(x, res, weight, bias, eps):
    """Fused residual add + LayerNorm: returns (x + res, LN(x + res))."""
    import torch.nn.functional as _F

    s = x + res
    return s, _F.layer_norm(s, (s.shape[-1],), weight, bias, eps)


def vae_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """Single-head attention over [B, L, C] (fp32 softmax)."""
    scale = q.shape[-1] ** -0.5
    scores = torch.einsum("bqc,bkc->bqk", q.float() * scale, k.float())
    probs = scores.softmax(dim=-1)
    return torch.einsum("bqk,bkc->bqc", probs, v.float()).to(q.dtype)


def guidance_rescale_factor(noise: torch.Tensor, g: float, phi: float) -> torch.Tensor:
    """The guidance_rescale factor (diffusers ``rescale_noise_cfg``) of a
    [2,C,h,w] CFG pair [uncond; cond]:

        cfg = nu + g*(nc - nu),   r = phi * std(nc) / std(cfg) + (1 - phi)

    with both standard deviations over (C, h, w) of the one sample. Computed in
    float64 from the inputs as given, returned as fp32 [1]: the reference of
    the kernel pair in csrc/scheduler.hip."""
    if noise.dim() != 4 or noise.shape[0] != 2:
        raise ValueError("guidance_rescale_factor: noise must be the [2,C,h,w] CFG pair")
    nu, nc = noise.double().chunk(2)
    cfg = nu + g * (nc - nu)
    r = phi * (nc.std() / cfg.std()) + (1.0 - phi)
    return r.float().reshape(1)


def _cfg_eps(noise: torch.Tensor, x: torch.Tensor, g: float,
             factor: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 eps of a step: the CFG combine of a [uncond; cond] pair, or the
    noise itself when it has x's batch (no guidance, g not read). factor (one
    fp32 value, CFG pair only) scales the combined result: guidance_rescale."""
    n = noise.float()
    if n.shape[0] == x.shape[0]:
        if factor is not None:
            raise ValueError("a guidance_rescale factor needs the [uncond; cond] noise pair")
        return n
    nu, nc = n.chunk(2)
    eps = nu + g * (nc - nu)
    return eps if factor is None else factor.float().to(eps.device).reshape(()) * eps


def _mask_blend(xp, x, init, init_noise, mask, sa, sb):
    """out = m*x' + (1 - m)*(sa*init + sb*init_noise) in fp32, rounded once to
    x's dtype. In this form m == 1 gives x' and m == 0 gives known exactly."""
    m = mask.float().reshape(1, 1, x.shape[2], x.shape[3])
    known = sa * init.float() + sb * init_noise.float()
    return (m * xp + (1.0 - m) * known).to(x.dtype)


_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57  # Random123 multipliers
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85  # Weyl key increments
_MASK32 = 0xFFFFFFFF


def _mulhilo32(m: int, c: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(hi, lo) words of the 64-bit product m * c; c holds 32-bit values in
    int64. The product is formed from c's 16-bit halves, so nothing passes 2^63."""
    p0 = m * (c & 0xFFFF)
    p1 = m * (c >> 16)
    t = ((p1 & 0xFFFF) << 16) + p0
    return (p1 >> 16) + (t >> 32), t & _MASK32


def philox4x32(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 (Random123 constants) in torch integer ops: counter words
    c0..c3 (int64 tensors of 32-bit values, or ints) and key words k0, k1
    (ints) -> the four output words, int64 tensors."""
    c0, c1, c2, c3 = torch.broadcast_tensors(
        *(torch.as_tensor(c, dtype=torch.int64) for c in (c0, c1, c2, c3)))
    k0, k1 = int(k0) & _MASK32, int(k1) & _MASK32
    for _ in range(10):
        hi0, lo0 = _mulhilo32(_PHILOX_M0, c0)
        hi1, lo1 = _mulhilo32(_PHILOX_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _PHILOX_W0) & _MASK32, (k1 + _PHILOX_W1) & _MASK32
    return c0, c1, c2, c3


def philox_normal(numel: int, seed: int, draw: int, offset: int = 0, device=None) -> torch.Tensor:
    """fp32 [numel]: the standard normals of elements offset .. offset + numel
    - 1 of the stream (seed, draw): the rule of csrc/philox.h. Element i reads
    Philox block q = i >> 2, counter (lo32(q), hi32(q), draw, 0), key
    (lo32(seed), hi32(seed)); the words (r0, r1) and (r2, r3) give two
    Box-Muller pairs in fp32,

        u1 = ((ra >> 8) + 1) * 2^-24,  u2 = (rb >> 8) * 2^-24,
        rad = sqrt(-2 ln u1),  (z_even, z_odd) = rad * (cos, sin)(2 pi u2),

    and element i takes z[i & 3]. Integer ops and elementwise fp32 functions
    only: it runs on any device, and it is the reference of the native op."""
    if numel < 0 or offset < 0:
        raise ValueError("philox_normal: numel and offset must be >= 0")
    seed, draw = int(seed), int(draw)
    if not 0 <= seed < 2 ** 64 or not 0 <= draw < 2 ** 32:
        raise ValueError("philox_normal: seed must fit 64 bits and draw 32 bits, unsigned")
    first = offset >> 2
    nblocks = ((offset + numel - 1) >> 2) - first + 1 if numel else 0
    q = torch.arange(first, first + nblocks, dtype=torch.int64, device=device)
    r = philox4x32(q & _MASK32, q >> 32, torch.full_like(q, draw), torch.zeros_like(q),
                   seed & _MASK32, seed >> 32)
    two_pi = torch.tensor(6.283185307179586, dtype=torch.float32, device=q.device)
    z = []
    for ra, rb in ((r[0], r[1]), (r[2], r[3])):
        u1 = ((ra >> 8) + 1).float() * 2.0 ** -24
        u2 = (rb >> 8).float() * 2.0 ** -24
        rad = torch.sqrt(-2.0 * torch.log(u1))
        ang = two_pi * u2
        z += [rad * torch.cos(ang), rad * torch.sin(ang)]
    lead = offset - (first << 2)
    return torch.stack(z, dim=1).reshape(-1)[lead:lead + numel]


def _add_step_noise(xp: torch.Tensor, x: torch.Tensor, noise) -> torch.Tensor:
    """x' + cn * z for noise = (cn, seed, draw), z indexed by the element's
    offset in the one sample x [1,C,h,w]; x' itself for None or cn == 0."""
    if noise is None:
        return xp
    cn, seed, draw = noise
    if x.dim() != 4 or x.shape[0] != 1:
        raise ValueError("a noisy step needs x [1,C,h,w] (one sample)")
    if cn == 0:
        return xp
    z = philox_normal(x.numel(), seed, draw, device=x.device).reshape(x.shape)
    return xp + cn * z


def cfg_affine_step(noise, x, g, ca, cb, factor=None, step_noise=None):
    """x' = ca*x + cb*eps of a CFG pair, eps scaled by factor when given.
    step_noise = (cn, seed, draw) adds cn * z (``philox_normal``); noise may
    then also be one branch's output in x's shape (eps = noise)."""
    xp = ca * x.float() + cb * _cfg_eps(noise, x, g, factor)
    return _add_step_noise(xp, x, step_noise).to(x.dtype)


def cfg_dpm_step(noise, x, x0_prev, g, ca, cb, cc, cx, ce, factor=None, step_noise=None):
    """DPM-Solver++(2M) step of a CFG pair -> (prev, x0 fp32); eps scaled by
    factor when given. step_noise as in cfg_affine_step: added to prev alone."""
    eps = _cfg_eps(noise, x, g, factor)
    xf = x.float()
    prev = ca * xf + cb * eps
    if x0_prev is not None:
        prev = prev + cc * x0_prev.float()
    return _add_step_noise(prev, x, step_noise).to(x.dtype), cx * xf + ce * eps


def masked_affine_step(noise, x, init, init_noise, mask, g, ca, cb, sa, sb, factor=None,
                       step_noise=None):
    """Inpaint step of the affine schedulers (DDIM, Euler): x' = ca*x + cb*eps
    blended with the known region. noise [2,C,h,w] (CFG pair) or [1,C,h,w];
    x [1,C,h,w]; init, init_noise fp32 [1,C,h,w]; mask h*w elements, shared by
    the channels. factor: the guidance_rescale factor, CFG pair only.
    step_noise = (cn, seed, draw) adds cn * z to x' before the blend."""
    xp = ca * x.float() + cb * _cfg_eps(noise, x, g, factor)
    xp = _add_step_noise(xp, x, step_noise)
    return _mask_blend(xp, x, init, init_noise, mask, sa, sb)


def masked_dpm_step(noise, x, x0_prev, init, init_noise, mask, g, ca, cb, cc, cx, ce, sa, sb,
                    factor=None, step_noise=None):
    """Inpaint step of DPM-Solver++(2M): prev = ca*x + cb*eps (+ cc*x0_prev)
    blended with the known region; x0 = cx*x + ce*eps (fp32) is the unmasked
    step's. Returns (prev, x0). factor: the guidance_rescale factor.
    step_noise as in masked_affine_step."""
    eps = _cfg_eps(noise, x, g, factor)
    xf = x.float()
    prev = ca * xf + cb * eps
    if x0_prev is not None:
        prev = prev + cc * x0_prev.float()
    prev = _add_step_noise(prev, x, step_noise)
    return _mask_blend(prev, x, init, init_noise, mask, sa, sb), cx * xf + ce * eps


def inpaint_unet_input(latents, mask, masked_latents, scale=1.0, copies=1):
    """[copies, 9, h, w]: latents [1,4,h,w] / scale, then the mask [1,1,h,w]
    and the masked-image latents [1,4,h,w] as they are (the latents' dtype)."""
    scaled = (latents.float() / scale).to(latents.dtype)
    one = torch.cat([scaled, mask.reshape(1, 1, *latents.shape[2:]), masked_latents], dim=1)
    return one.repeat(copies, 1, 1, 1)


def conv3x3_halo(
    x: torch.Tensor,
    weight: torch.Tensor,
    bias: torch.Tensor | None,
    stride: int = 1,
    top: torch.Tensor | None = None,
    bot: torch.Tensor | None = None,
    pad_lo: int = 1,
) -> torch.Tensor:
    """3x3 pad-1 conv whose top/bottom halo rows come from separate tensors.

    x: [B, Cin, H, W]; top/bot: [B, Cin, 1, W] neighbour rows (None => zero
    pad at that border). Semantics of the HIP conv3x3 kernel: the reference
    materializes cat([top, x, bot]) per conv
    (/root/reference/distrifuser/modules/pp/conv2d.py:72-88); the kernel —
    and this oracle — treat the halos as extra input rows in place.

    pad_lo=0 (stride 2 only, no top) is the AutoencoderKL downsample: the
    input is padded on the bottom and right alone, F.pad(x, (0, 1, 0, 1)) then
    a padding=0 conv, so output (y, x) reads rows 2y..2y+2 and columns
    2x..2x+2. Row H is bot when given, else zero; column W is zero.
    """
    b, c, h, w = x.shape
    if pad_lo == 0:
        if stride != 2 or top is not None or h < 2 or w < 2:
            raise ValueError("conv3x3_halo: pad_lo=0 needs stride 2, no top halo and H, W >= 2")
        full = x if bot is None else torch.cat([x, bot.reshape(b, c, 1, w)], dim=2)
        full = F.pad(full, [0, 1, 0, 1 if bot is None else 0])
        out = F.conv2d(full, weight, bias, stride=2)
        return out[:, :, : (h - 2) // 2 + 1, :]
    if pad_lo != 1:
        raise ValueError(f"conv3x3_halo: pad_lo must be 0 or 1, got {pad_lo}")
    parts = []
    pad_top = 1 if top is None else 0
    pad_bot = 1 if bot is None else 0
    if top is not None:
        parts.append(top.reshape(b, c, 1, w))
    parts.append(x)
    if bot is not None:
        parts.append(bot.reshape(b, c, 1, w))
    full = torch.cat(parts, dim=2) if len(parts) > 1 else x
    full = F.pad(full, [1, 1, pad_top, pad_bot])
    out = F.conv2d(full, weight, bias, stride=stride)
    # pad-1 stride-s output has ceil(H/s) rows regardless of halo presence
    ho = (h - 1) // stride + 1
    return out[:, :, :ho, :]
