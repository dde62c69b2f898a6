"""GroupNorm as a module over the fused HIP kernel (ops.group_norm_silu)."""

from __future__ import annotations

import torch
from torch import nn

from . import dispatch


class PlainGroupNorm(nn.GroupNorm):
    """GroupNorm with optionally fused SiLU, routed through ops (HIP kernel)."""

    def __init__(self, num_groups, num_channels, eps=1e-5, affine=True, fuse_silu=False):
        super().__init__(num_groups, num_channels, eps=eps, affine=affine)
        self.fuse_silu = fuse_silu

    def forward(self, x: torch.Tensor, tokens: bool = False) -> torch.Tensor:
        """tokens=True returns [N, H*W, C] instead of NCHW (same values)."""
        return dispatch.group_norm_silu(
            x, self.num_groups, self.weight, self.bias, self.eps, silu=self.fuse_silu,
            tokens=tokens,
        )
