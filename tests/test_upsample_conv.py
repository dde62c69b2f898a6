"""The fused 2x-upsample + 3x3 conv rule (eager.upsample2x_conv3x3) and its knob."""

import pytest
import torch
import torch.nn.functional as F

from distrifuser_amd import ops
from distrifuser_amd.models.layers import LayerFactory
from distrifuser_amd.models.resnet import Upsample2D
from distrifuser_amd.ops import eager
from distrifuser_amd.parallel.state import ParallelState
from distrifuser_amd.utils.config import DistriConfig


@pytest.mark.parametrize("halo", [False, True], ids=["zero", "halo"])
@pytest.mark.parametrize("w", [1, 2, 3])
@pytest.mark.parametrize("h", [1, 2, 3])
def test_rule_is_interpolate_then_conv_in_float64(h, w, halo):
    """float64 weights are collapsed in float64 and not rounded, so the rule must
    equal interpolate + conv to float64 round-off: the algebra and the borders."""
    gen = torch.Generator().manual_seed(100 * h + 10 * w + halo)
    x = torch.randn(2, 3, h, w, generator=gen, dtype=torch.float64)
    weight = torch.randn(5, 3, 3, 3, generator=gen, dtype=torch.float64)
    bias = torch.randn(5, generator=gen, dtype=torch.float64)
    top, bot = (torch.randn(2, 3, 1, w, generator=gen, dtype=torch.float64) if halo else None
                for _ in range(2))
    got = eager.upsample2x_conv3x3(x, weight, bias, top, bot)
    up = F.interpolate(x, scale_factor=2.0, mode="nearest")
    if halo:  # a neighbour's input row is two equal rows of the upsampled tensor
        up_top, up_bot = (F.interpolate(t, scale_factor=(1.0, 2.0), mode="nearest")
                          for t in (top, bot))
        want = F.conv2d(torch.cat([up_top, up, up_bot], dim=2), weight, bias, padding=(0, 1))
    else:
        want = F.conv2d(up, weight, bias, padding=1)
    assert got.shape == (2, 5, 2 * h, 2 * w)
    assert (got - want).abs().max().item() <= 64 * 2.0 ** -53 * want.abs().max().item()


def test_knob_parsing(monkeypatch):
    monkeypatch.delenv("DFA_UPSAMPLE_FUSED", raising=False)
    assert DistriConfig(device="cpu").upsample_fused is False
    assert DistriConfig(device="cpu", upsample_fused=True).upsample_fused is True
    monkeypatch.setenv("DFA_UPSAMPLE_FUSED", "1")
    assert DistriConfig(device="cpu").upsample_fused is True
    assert DistriConfig(device="cpu", upsample_fused=False).upsample_fused is False
    monkeypatch.setenv("DFA_UPSAMPLE_FUSED", "0")
    assert DistriConfig(device="cpu").upsample_fused is False
    monkeypatch.setenv("DFA_UPSAMPLE_FUSED", "yes")
    with pytest.raises(ValueError, match="upsample_fused"):
        DistriConfig(device="cpu")


@pytest.mark.parametrize("fused", [False, True], ids=["off", "on"])
def test_upsample2d_route(monkeypatch, fused):
    calls = {"fused": 0, "interpolate": 0}

    def count(name, fn):
        def wrapped(*args, **kwargs):
            calls[name] += 1
            return fn(*args, **kwargs)
        return wrapped

    monkeypatch.setattr(ops, "upsample2x_conv3x3", count("fused", ops.upsample2x_conv3x3))
    monkeypatch.setattr(F, "interpolate", count("interpolate", F.interpolate))
    cfg = DistriConfig(height=64, width=64, device="cpu", upsample_fused=fused)
    torch.manual_seed(0)
    up = Upsample2D(8, factory=LayerFactory(ParallelState(cfg))).eval()
    x = torch.randn(2, 8, 3, 5)
    with torch.no_grad():
        out = up(x)
    assert calls == ({"fused": 1, "interpolate": 0} if fused else {"fused": 0, "interpolate": 1})
    conv = up.conv.conv  # PatchConv2d's NativeConv2d
    want = conv(torch.repeat_interleave(torch.repeat_interleave(x, 2, dim=2), 2, dim=3))
    assert out.shape == (2, 8, 6, 10)
    assert (out - want).abs().max().item() <= 1e-5 * want.abs().max().item()
