"""Native VAE (AutoencoderKL) decoder and encoder.

The reference delegated VAE decode to diffusers; here it is owned. Every
rank decodes the identical full latent (parity with the reference's
replicated decode — the denoise loop is the parallel part). The mid-block
attention (single 512-dim head over up to 480x480 = 230k tokens at
3840x3840) runs on the split-D gfx950 HIP kernel (csrc/vae_attn.hip) on
GPU; the CPU path uses a query-chunked softmax so no full score matrix is
ever materialized. Convolutions ride the implicit-GEMM conv3x3 kernel
(NativeConv2d).

The encoder (img2img) is built from the same blocks: its three downsample
convs are 3x3 stride-2 convs padded on the bottom and right only, which is
the conv kernel's pad_lo=0 mode (NativeConv2d(asym_pad=True)).
"""

from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn.functional as F
from torch import nn

from ..ops import NativeConv2d, PlainGroupNorm

from .. import ops


@dataclass(frozen=True)
class VAEDecoderConfig:
    latent_channels: int = 4
    out_channels: int = 3
    block_out_channels: tuple = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    scaling_factor: float = 0.13025  # SDXL
    # encoder side (VAEEncoder); the decoder reads neither
    in_channels: int = 3
    double_z: bool = True


SDXL_VAE = VAEDecoderConfig()
SD_VAE = VAEDecoderConfig(scaling_factor=0.18215)
# 4 up blocks = 8x upscale, same ratio as the real VAE
TINY_VAE = VAEDecoderConfig(
    latent_channels=4, block_out_channels=(16, 16, 32, 32), layers_per_block=1,
    norm_num_groups=8, scaling_factor=0.18215,
)


class VAEResnetBlock(nn.Module):
    """ResNet block without time embedding (VAE variant)."""

    def __init__(self, in_ch: int, out_ch: int, groups: int):
        super().__init__()
        self.norm1 = PlainGroupNorm(groups, in_ch, eps=1e-6, fuse_silu=True)
        self.conv1 = NativeConv2d(in_ch, out_ch, 3, padding=1)
        self.norm2 = PlainGroupNorm(groups, out_ch, eps=1e-6, fuse_silu=True)
        self.conv2 = NativeConv2d(out_ch, out_ch, 3, padding=1)
        self.conv_shortcut = NativeConv2d(in_ch, out_ch, 1) if in_ch != out_ch else None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        h = self.conv1(self.norm1(x))
        res = self.conv_shortcut(x) if self.conv_shortcut is not None else x
        return self.conv2(self.norm2(h), residual=res)


def _chunked_single_head_attention(
    q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, chunk: int = 4096
) -> torch.Tensor:
    """[B, L, C] single-head attention with O(chunk*L) memory.

    At 3840^2 the VAE mid block attends over 480*480 = 230k tokens with a
    single 512-dim head; the score slab per chunk is chunk*L fp32
    (4096*230k*4B ~= 3.8 GB) — bounded regardless of resolution.
    """
    scale = q.shape[-1] ** -0.5
    # GPU: bf16 GEMMs (hipBLASLt) with fp32 softmax — at 230k tokens the
    # score GEMM is ~5e16 FLOP and fp32 (vector-ALU only on CDNA4, no fp32
    # MFMA) would take minutes; CPU keeps fp32 for the test oracle.
    # An fp16 input keeps its own type: same GEMM rate, three more mantissa bits.
    if not q.is_cuda:
        mm_dtype = torch.float32
    else:
        mm_dtype = torch.float16 if q.dtype == torch.float16 else torch.bfloat16
    qs = (q.float() * scale).to(mm_dtype)
    ks = k.to(mm_dtype)
    vs = v.to(mm_dtype)
    outs = []
    for s in range(0, q.shape[1], chunk):
        scores = torch.einsum("bqc,bkc->bqk", qs[:, s : s + chunk], ks)
        probs = scores.float().softmax(dim=-1).to(mm_dtype)
        outs.append(torch.einsum("bqk,bkc->bqc", probs, vs))
    return torch.cat(outs, dim=1).to(q.dtype)


class VAEAttention(nn.Module):
    """Single-head spatial self-attention of the VAE mid block."""

    def __init__(self, channels: int, groups: int):
        super().__init__()
        self.group_norm = PlainGroupNorm(groups, channels, eps=1e-6, fuse_silu=False)
        self.to_q = nn.Linear(channels, channels)
        self.to_k = nn.Linear(channels, channels)
        self.to_v = nn.Linear(channels, channels)
        self.to_out = nn.Linear(channels, channels)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        b, c, h, w = x.shape
        residual = x
        x = self.group_norm(x)
        x = x.permute(0, 2, 3, 1).reshape(b, h * w, c)
        q, k, v = self.to_q(x), self.to_k(x), self.to_v(x)
        if x.is_cuda and c == 512 and q.dtype in (torch.bfloat16, torch.float16):
            out = ops.vae_attention(q, k, v)  # split-D HIP kernel
        elif x.is_cuda and c <= 256:
            out = ops.flash_attention(q[:, None], k[:, None], v[:, None])[:, 0]
        else:
            out = _chunked_single_head_attention(q, k, v)
        out = self.to_out(out)
        return out.reshape(b, h, w, c).permute(0, 3, 1, 2) + residual


class UpDecoderBlock2D(nn.Module):
    def __init__(self, in_ch: int, out_ch: int, layers: int, add_upsample: bool, groups: int):
        super().__init__()
        self.resnets = nn.ModuleList(
            [VAEResnetBlock(in_ch if i == 0 else out_ch, out_ch, groups) for i in range(layers)]
        )
        self.upsampler = NativeConv2d(out_ch, out_ch, 3, padding=1) if add_upsample else None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        for r in self.resnets:
            x = r(x)
        if self.upsampler is not None:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = self.upsampler(x)
        return x


@torch.no_grad()
def _tiled_apply(fn, x: torch.Tensor, tile: int, overlap: int, scale_num: int,
                 scale_den: int) -> torch.Tensor:
    """Apply ``fn`` to overlapping ``tile``-sized tiles of ``x`` and linearly
    blend the seams (diffusers AutoencoderKL tiled decode / encode parity).

    ``tile`` and ``overlap`` are in input pixels; ``fn`` scales both spatial
    sides by ``scale_num / scale_den`` (x8 for decode, /8 for encode).
    """
    def out_px(n):
        return n * scale_num // scale_den

    stride = tile - overlap
    b, _, h, w = x.shape
    ys = list(range(0, max(h - overlap, 1), stride))
    xs = list(range(0, max(w - overlap, 1), stride))
    # Full-size tiles run as ONE batched pass (288 GB HBM3E holds all
    # activations comfortably); ragged edge tiles run individually.
    tiles = {}
    full = [(y0, x0) for y0 in ys for x0 in xs
            if y0 + tile <= h and x0 + tile <= w]
    if len(full) > 1 and b == 1:
        batch = torch.cat([x[:, :, y0 : y0 + tile, x0 : x0 + tile]
                           for (y0, x0) in full])
        res = fn(batch)
        for i, key in enumerate(full):
            tiles[key] = res[i : i + 1]
    for y0 in ys:
        for x0 in xs:
            if (y0, x0) not in tiles:
                tiles[(y0, x0)] = fn(x[:, :, y0 : y0 + tile, x0 : x0 + tile])
    rows = [[tiles[(y0, x0)] for x0 in xs] for y0 in ys]

    def blend_v(a, bt, k):
        k = min(k, a.shape[2], bt.shape[2])
        w_ = torch.linspace(0, 1, k, device=a.device, dtype=a.dtype).view(1, 1, k, 1)
        bt[:, :, :k] = a[:, :, a.shape[2] - k :] * (1 - w_) + bt[:, :, :k] * w_
        return bt

    def blend_h(a, bt, k):
        k = min(k, a.shape[3], bt.shape[3])
        w_ = torch.linspace(0, 1, k, device=a.device, dtype=a.dtype).view(1, 1, 1, k)
        bt[:, :, :, :k] = a[:, :, :, a.shape[3] - k :] * (1 - w_) + bt[:, :, :, :k] * w_
        return bt

    ov_out, st_out = out_px(overlap), out_px(stride)
    out_rows = []
    for i, row in enumerate(rows):
        parts = []
        for j, t in enumerate(row):
            if i > 0:
                t = blend_v(rows[i - 1][j], t, ov_out)
            if j > 0:
                t = blend_h(row[j - 1], t, ov_out)
            keep_w = st_out if j < len(row) - 1 else t.shape[3]
            parts.append(t[:, :, :st_out, :keep_w] if i < len(rows) - 1
                         else t[:, :, :, :keep_w])
        out_rows.append(torch.cat(parts, dim=3))
    out = torch.cat(out_rows, dim=2)
    return out[:, :, : out_px(h), : out_px(w)]


class _TilingMixin:
    """Tiling state shared by the decoder and the encoder. The mid-block
    attention is O(L^2) in latent tokens: a full 3840^2 decode attends over
    230k tokens (~109 TFLOP in that one layer). Tiling runs overlapping tiles
    independently and linearly blends the seams — the standard high-resolution
    VAE path. Sizes are in latent pixels on both sides, so an encoder tile is
    tile_latent_size * 8 image pixels."""

    use_tiling: bool = False
    tile_latent_size: int = 96
    tile_overlap: int = 16  # latent pixels blended between neighbouring tiles

    def enable_tiling(self, tile_latent_size: int = 96, tile_overlap: int = 16) -> None:
        self.use_tiling = True
        self.tile_latent_size = tile_latent_size
        self.tile_overlap = tile_overlap

    def disable_tiling(self) -> None:
        self.use_tiling = False


class VAEDecoder(_TilingMixin, nn.Module):
    def __init__(self, config: VAEDecoderConfig):
        super().__init__()
        self.config = config
        ch = config.block_out_channels
        groups = config.norm_num_groups
        top = ch[-1]
        self.post_quant_conv = NativeConv2d(config.latent_channels, config.latent_channels, 1)
        self.conv_in = NativeConv2d(config.latent_channels, top, 3, padding=1)
        self.mid_resnet_1 = VAEResnetBlock(top, top, groups)
        self.mid_attn = VAEAttention(top, groups)
        self.mid_resnet_2 = VAEResnetBlock(top, top, groups)
        rev = list(reversed(ch))
        blocks = []
        prev = top
        for i, out_ch in enumerate(rev):
            blocks.append(
                UpDecoderBlock2D(
                    prev, out_ch, config.layers_per_block + 1,
                    add_upsample=i < len(rev) - 1, groups=groups,
                )
            )
            prev = out_ch
        self.up_blocks = nn.ModuleList(blocks)
        self.conv_norm_out = PlainGroupNorm(groups, ch[0], eps=1e-6, fuse_silu=True)
        self.conv_out = NativeConv2d(ch[0], config.out_channels, 3, padding=1)

    @torch.no_grad()
    def _decode_one(self, z: torch.Tensor) -> torch.Tensor:
        x = self.conv_in(z)
        x = self.mid_resnet_1(x)
        x = self.mid_attn(x)
        x = self.mid_resnet_2(x)
        for block in self.up_blocks:
            x = block(x)
        return self.conv_out(self.conv_norm_out(x))

    def _decode_tiled(self, z: torch.Tensor) -> torch.Tensor:
        return _tiled_apply(self._decode_one, z, self.tile_latent_size, self.tile_overlap, 8, 1)

    @torch.no_grad()
    def decode(self, latents: torch.Tensor) -> torch.Tensor:
        """latents (scaled) -> images in [-1, 1]."""
        z = latents / self.config.scaling_factor
        z = self.post_quant_conv(z)
        if self.use_tiling and (z.shape[2] > self.tile_latent_size
                                or z.shape[3] > self.tile_latent_size):
            return self._decode_tiled(z)
        return self._decode_one(z)

    forward = decode


class DownEncoderBlock2D(nn.Module):
    def __init__(self, in_ch: int, out_ch: int, layers: int, add_downsample: bool, groups: int):
        super().__init__()
        self.resnets = nn.ModuleList(
            [VAEResnetBlock(in_ch if i == 0 else out_ch, out_ch, groups) for i in range(layers)]
        )
        # AutoencoderKL downsample: F.pad(x, (0, 1, 0, 1)) then a padding-0
        # stride-2 conv, i.e. padded on the bottom and right only
        self.downsampler = (NativeConv2d(out_ch, out_ch, 3, stride=2, padding=0, asym_pad=True)
                            if add_downsample else None)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        for r in self.resnets:
            x = r(x)
        if self.downsampler is not None:
            x = self.downsampler(x)
        return x


class VAEEncoder(_TilingMixin, nn.Module):
    """AutoencoderKL encoder: images in [-1, 1] -> posterior moments -> latents.

    Built from the decoder's config values and blocks. ``encode`` returns
    latents already multiplied by ``scaling_factor``, the inverse convention
    of ``VAEDecoder.decode``.
    """

    LOGVAR_MIN, LOGVAR_MAX = -30.0, 20.0
    SPATIAL = 8  # image pixels per latent pixel
    # either latent side at or above this tiles the call automatically: the
    # mid attention is O(L^2) in latent tokens, the wall the decoder hit
    auto_tiling_min_latent = 256

    def __init__(self, config: VAEDecoderConfig):
        super().__init__()
        self.config = config
        ch = config.block_out_channels
        groups = config.norm_num_groups
        assert len(ch) == 4, "the encoder downsamples by 8: four down blocks"
        self.conv_in = NativeConv2d(config.in_channels, ch[0], 3, padding=1)
        blocks = []
        prev = ch[0]
        for i, out_ch in enumerate(ch):
            blocks.append(
                DownEncoderBlock2D(prev, out_ch, config.layers_per_block,
                                   add_downsample=i < len(ch) - 1, groups=groups)
            )
            prev = out_ch
        self.down_blocks = nn.ModuleList(blocks)
        top = ch[-1]
        self.mid_resnet_1 = VAEResnetBlock(top, top, groups)
        self.mid_attn = VAEAttention(top, groups)
        self.mid_resnet_2 = VAEResnetBlock(top, top, groups)
        self.conv_norm_out = PlainGroupNorm(groups, top, eps=1e-6, fuse_silu=True)
        zc = config.latent_channels * (2 if config.double_z else 1)
        self.conv_out = NativeConv2d(top, zc, 3, padding=1)
        self.quant_conv = NativeConv2d(zc, zc, 1)

    @torch.no_grad()
    def _encode_one(self, x: torch.Tensor) -> torch.Tensor:
        """images -> moments [B, 2*latent_channels, H/8, W/8] (after quant_conv)."""
        x = self.conv_in(x)
        for block in self.down_blocks:
            x = block(x)
        x = self.mid_resnet_1(x)
        x = self.mid_attn(x)
        x = self.mid_resnet_2(x)
        return self.quant_conv(self.conv_out(self.conv_norm_out(x)))

    def _encode_tiled(self, x: torch.Tensor) -> torch.Tensor:
        # the MOMENTS are blended, linearly across the overlap, before sampling
        sf = self.SPATIAL
        return _tiled_apply(self._encode_one, x, self.tile_latent_size * sf,
                            self.tile_overlap * sf, 1, sf)

    @torch.no_grad()
    def encode_moments(self, images: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """images [B, in_channels, H, W] in [-1, 1] -> (mean, logvar), each
        [B, latent_channels, H/8, W/8]; logvar is clamped to [-30, 20].

        A call whose latent would have a side >= ``auto_tiling_min_latent``
        runs tiled with the default tile settings for that call only; the
        tiling state it found is restored afterwards.
        """
        sf = self.SPATIAL
        lh, lw = images.shape[2] // sf, images.shape[3] // sf
        saved = (self.use_tiling, self.tile_latent_size, self.tile_overlap)
        auto = not self.use_tiling and max(lh, lw) >= self.auto_tiling_min_latent
        if auto:
            self.enable_tiling()
        try:
            if self.use_tiling and (lh > self.tile_latent_size or lw > self.tile_latent_size):
                moments = self._encode_tiled(images)
            else:
                moments = self._encode_one(images)
        finally:
            self.use_tiling, self.tile_latent_size, self.tile_overlap = saved
        if not self.config.double_z:
            return moments, torch.full_like(moments, self.LOGVAR_MIN)
        mean, logvar = moments.chunk(2, dim=1)
        return mean, logvar.clamp(self.LOGVAR_MIN, self.LOGVAR_MAX)

    @torch.no_grad()
    def encode(self, images: torch.Tensor, generator: torch.Generator | None = None,
               sample: bool = True) -> torch.Tensor:
        """images in [-1, 1] -> latents times ``scaling_factor``.

        ``sample=False`` returns the posterior mode. The sampling noise is
        drawn in fp32 from ``generator`` on the generator's device (the CPU
        by default) and then moved to the model's, the rule the pipelines
        follow for the initial latents: every rank draws identical noise.
        """
        mean, logvar = self.encode_moments(images)
        if not sample:
            return mean * self.config.scaling_factor
        device = generator.device if generator is not None else torch.device("cpu")
        noise = torch.randn(mean.shape, generator=generator, dtype=torch.float32, device=device)
        z = mean.float() + torch.exp(0.5 * logvar.float()) * noise.to(mean.device)
        return (z * self.config.scaling_factor).to(mean.dtype)

    forward = encode
