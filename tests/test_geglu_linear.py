"""The fused GEGLU projection off the GPU: eager.geglu_linear against float64,
FeedForward with ff_fused off (today's composition, bit for bit) and on (the
rule), the unchanged state dict, and how the knob and DFA_FF_FUSED parse."""

import pytest
import torch
import torch.nn.functional as F

from distrifuser_amd import ops
from distrifuser_amd.models.layers import FeedForward
from distrifuser_amd.ops import eager
from distrifuser_amd.utils.config import DistriConfig


def _cfg(**kw):
    return DistriConfig(height=64, width=64, use_cuda_graph=False, device="cpu", **kw)


def test_rule_against_float64():
    """fp32 sums of 40 exact products and a bias: 41 * 2^-24 of the magnitudes for
    a and g (g's through |a| max|gelu'| <= 1.13), 2^-22 for fp32 gelu and the
    product, then one bf16 rounding: half a spacing, at most 2^-8 of the value."""
    torch.manual_seed(0)
    rows, k, inner = 9, 40, 24
    x, w, b = (torch.randn(s).bfloat16() for s in ((rows, k), (2 * inner, k), (2 * inner,)))
    got = eager.geglu_linear(x, w, b)
    xd, wd, bd = x.double(), w.double(), b.double()
    a, g = (xd @ wd.t() + bd).chunk(2, dim=-1)
    ref = a * F.gelu(g)
    mag_a, mag_g = (xd.abs() @ wd.abs().t() + bd.abs()).chunk(2, dim=-1)
    e32 = (k + 1) * 2.0 ** -24 * (mag_a * F.gelu(g).abs() + 1.13 * a.abs() * mag_g)
    e32 = e32 + 2.0 ** -22 * (a.abs() * g.abs() + ref.abs())
    assert ((got.double() - ref).abs() <= 2.0 ** -8 * (ref.abs() + e32) + e32).all()
    h = x.float() @ w.float().t() + b.float()  # one rounding: of the fp32 product
    assert torch.equal(got, (h[:, :inner] * F.gelu(h[:, inner:])).bfloat16())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_feed_forward_knob(dtype):
    torch.manual_seed(1)
    x = torch.randn(2, 5, 16).to(dtype)
    plain = FeedForward(16).to(dtype)
    keys = ["proj_in.weight", "proj_in.bias", "proj_out.weight", "proj_out.bias"]
    today = plain.proj_out(ops.geglu(plain.proj_in(x)))
    for cfg in (None, _cfg(), _cfg(ff_fused=False)):
        off = FeedForward(16, config=cfg).to(dtype)
        off.load_state_dict(plain.state_dict())
        assert torch.equal(off(x), today)
    on = FeedForward(16, config=_cfg(ff_fused=True)).to(dtype)
    assert list(on.state_dict()) == keys == list(plain.state_dict())
    on.load_state_dict(plain.state_dict())
    rule = eager.geglu_linear(x, on.proj_in.weight, on.proj_in.bias)
    assert torch.equal(on(x), on.proj_out(rule))
    assert torch.equal(ops.geglu_linear(x, on.proj_in.weight, on.proj_in.bias), rule)


def test_knob_and_environment(monkeypatch):
    monkeypatch.delenv("DFA_FF_FUSED", raising=False)
    assert _cfg().ff_fused is False and _cfg(ff_fused=True).ff_fused is True
    for text, want in (("1", True), ("0", False), ("", False)):
        monkeypatch.setenv("DFA_FF_FUSED", text)
        assert _cfg().ff_fused is want
        assert _cfg(ff_fused=not want).ff_fused is (not want)  # the argument wins
    for env_junk, arg_junk in (("yes", 1), ("2", "on")):
        monkeypatch.setenv("DFA_FF_FUSED", env_junk)
        with pytest.raises(ValueError, match="ff_fused"):
            _cfg()
        with pytest.raises(ValueError, match="ff_fused"):
            _cfg(ff_fused=arg_junk)
