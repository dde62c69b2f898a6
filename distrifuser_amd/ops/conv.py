"""3x3 conv dispatch: gfx950 implicit-GEMM kernel with in-place halo rows.

The HIP kernel (csrc/conv.hip) computes a pad-1 3x3 conv (stride 1/2) whose
top/bottom halo rows are read from separate tensors — e.g. the displaced-
patch comm buffer — instead of a materialized cat (reference
/root/reference/distrifuser/modules/pp/conv2d.py:72-88 concatenates).
Weights are prepacked once into the kernel's per-lane MFMA A-fragment order.
``pad_lo=0`` selects the kernel's stride-2 mode padded on the bottom and right
only (the AutoencoderKL encoder downsample).
"""

from __future__ import annotations

import torch
from torch import nn

from . import eager
from .dispatch import use_hip, hip_ext


_CONV_DTYPES = (torch.bfloat16, torch.float16)


def pack_conv3x3_weight(weight: torch.Tensor, dtype: torch.dtype | None = None) -> torch.Tensor:
    """[Cout, Cin, 3, 3] -> [9, KS, CT, 64, 8] in A-fragment order, as bf16
    (dtype None, the default) or fp16 (dtype=torch.float16).

    Fragment map (mfma_f32_32x32x16_bf16 / _f16 A operand, the same for both):
    lane l holds cout = ct*32 + (l&31), cin = ks*16 + (l>>5)*8 + j for j in
    0..7. Cin is zero-padded to a multiple of 64 (the kernel's largest staged
    cin tile), Cout to a multiple of 32.
    """
    dtype = torch.bfloat16 if dtype is None else dtype
    if dtype not in _CONV_DTYPES:
        raise ValueError(f"pack_conv3x3_weight: dtype must be bf16 or fp16, got {dtype}")
    cout, cin, kh, kw = weight.shape
    assert kh == 3 and kw == 3, "pack_conv3x3_weight is 3x3 only"
    cin_p = (cin + 63) // 64 * 64
    cout_p = (cout + 31) // 32 * 32
    wp = weight.new_zeros(cout_p, cin_p, 9, dtype=torch.float32)
    wp[:cout, :cin] = weight.reshape(cout, cin, 9).float()
    ks, ct = cin_p // 16, cout_p // 32
    wp = wp.permute(2, 1, 0)              # [9][cin_p][cout_p]
    wp = wp.reshape(9, ks, 2, 8, ct, 32)  # cin = ks*16 + hi*8 + j
    wp = wp.permute(0, 1, 4, 2, 5, 3)     # [9][ks][ct][hi][cout%32][j]
    return wp.reshape(9, ks, ct, 64, 8).contiguous().to(dtype)


def _hip_conv_ok(x: torch.Tensor, stride: int) -> bool:
    return (
        x.dtype in _CONV_DTYPES
        and stride in (1, 2)
        and x.stride(-1) == 1
        and x.stride(-2) == x.shape[-1]
    )


def conv3x3_halo(x, weight, bias, stride=1, top=None, bot=None, packed=None, residual=None,
                 bias2=None, pad_lo=1):
    """Dispatching halo conv. ``packed`` (from :func:`pack_conv3x3_weight`)
    enables the HIP path; eager falls back to the cat-based oracle.
    ``residual`` ([B,Cout,Ho,Wo]) and ``bias2`` ([B,Cout], the time-embedding
    add) are applied in the kernel epilogue. ``pad_lo=0`` (stride 2, no
    ``top``) pads the bottom and right only: the AutoencoderKL downsample."""
    import os
    # In-epilogue residual measured ~0.7% SLOWER end-to-end than a separate
    # add kernel (the epilogue's cout-strided 2 B residual reads are poorly
    # coalesced vs the add kernel's linear pass) — default OFF, opt in with
    # DFA_CONV_RESID=1. bias2 is one scalar per output ROW (like the conv
    # bias) and is free, so it stays on by default.
    if residual is not None and os.environ.get("DFA_CONV_RESID", "0") != "1":
        out = conv3x3_halo(x, weight, bias, stride, top, bot, packed=packed, bias2=bias2,
                           pad_lo=pad_lo)
        return out + residual
    if use_hip(x) and packed is not None and _hip_conv_ok(x, stride):
        cout = weight.shape[0]
        t = top.reshape(top.shape[0], top.shape[1], -1) if top is not None else None
        b = bot.reshape(bot.shape[0], bot.shape[1], -1) if bot is not None else None
        if (t is None or t.stride(-1) == 1) and (b is None or b.stride(-1) == 1):
            return hip_ext().conv3x3(x, packed, bias, cout, stride, t, b, residual, bias2,
                                     pad_lo)
    out = eager.conv3x3_halo(x, weight, bias, stride, top, bot, pad_lo)
    if bias2 is not None:
        out = out + bias2.to(out.dtype)[:, :, None, None]
    return out if residual is None else out + residual


class NativeConv2d(nn.Conv2d):
    """nn.Conv2d that rides the gfx950 implicit-GEMM kernel on GPU.

    State-dict compatible with nn.Conv2d (same parameters); the packed
    fragment-order weight copy is built lazily on first GPU forward and
    cached until the weight storage changes.

    ``asym_pad=True`` (3x3, stride 2, padding 0) is the AutoencoderKL
    downsample: the input is padded on the bottom and right only. On GPU that
    is the kernel's ``pad_lo=0`` mode; elsewhere ``F.pad(x, (0, 1, 0, 1))``
    and the padding-0 conv. The flag adds no parameter or buffer.
    """

    def __init__(self, *args, asym_pad: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        if asym_pad and not (self.kernel_size == (3, 3) and self.stride == (2, 2)
                             and self.padding == (0, 0)):
            raise ValueError("asym_pad needs a 3x3 conv with stride 2 and padding 0")
        self.asym_pad = asym_pad
        self._wp = None
        self._wp_key = None

    def _native_eligible(self, x: torch.Tensor) -> bool:
        return (
            x.is_cuda
            and self.kernel_size == (3, 3)
            and self.padding == ((0, 0) if self.asym_pad else (1, 1))
            and self.stride[0] == self.stride[1]
            and self.stride[0] in (1, 2)
            and self.dilation == (1, 1)
            and self.groups == 1
            and x.dtype in _CONV_DTYPES
        )

    def packed_weight(self) -> torch.Tensor:
        w = self.weight
        key = (w._version, w.data_ptr(), w.dtype, w.device)
        if self._wp is None or self._wp_key != key:
            with torch.no_grad():
                # fp16 weights pack as fp16; anything else as bf16, as ever
                self._wp = pack_conv3x3_weight(
                    w.detach(), torch.float16 if w.dtype == torch.float16 else None)
            self._wp_key = key
        return self._wp

    def forward(self, x: torch.Tensor, top=None, bot=None, residual=None,
                bias2=None) -> torch.Tensor:
        if self._native_eligible(x):
            if not _hip_conv_ok(x, self.stride[0]):
                # e.g. a tiled-decode row-slice view: one contiguous copy is
                # far cheaper than MIOpen's fallback (a naive-conv trial was
                # 595 ms/tile in the tiled-VAE trace)
                x = x.contiguous()
            return conv3x3_halo(
                x, self.weight, self.bias, self.stride[0], top, bot,
                packed=self.packed_weight(), residual=residual, bias2=bias2,
                pad_lo=0 if self.asym_pad else 1,
            )
        if (
            x.is_cuda
            and self.kernel_size == (1, 1)
            and self.stride == (1, 1)
            and self.groups == 1
            and top is None
            and bot is None
        ):
            # 1x1 conv as a hipBLASLt GEMM: MIOpen's find phase was spending
            # ~90 s benchmarking naive kernels for these once the 3x3s moved
            # to the native kernel (rocprof r02 trace).
            b, c, h, w = x.shape
            out = torch.matmul(self.weight.view(self.out_channels, c),
                               x.reshape(b, c, h * w))
            if self.bias is not None:
                out = out + self.bias.view(1, -1, 1)
            return out.view(b, self.out_channels, h, w)
        if self.asym_pad:
            out = eager.conv3x3_halo(x, self.weight, self.bias, 2, top, bot, pad_lo=0)
        elif top is None and bot is None:
            out = super().forward(x)
        else:
            out = eager.conv3x3_halo(x, self.weight, self.bias, self.stride[0], top, bot)
        if bias2 is not None:
            out = out + bias2.to(out.dtype)[:, :, None, None]
        return out if residual is None else out + residual
