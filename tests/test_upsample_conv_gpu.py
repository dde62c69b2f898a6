"""The fused upsample conv kernel (csrc/conv_up2x.hip), called through the
extension so that nothing can fall back. Block tile: 8 input rows x 32 input px
x 64 couts, 16-cin slices; 16-byte row loads when W % 8 == 0, 2-byte loads else.
H {1, 2, 7, 8, 9, 16, 17} and W {1, 2, 31, 32, 33, 40, 64} reach each side of the
tile, a second block each way and both load paths; Cin {8, 64, 72} and Cout
{8, 32, 40} the zero-padded tails of the pack.

Bound of the random cases, per element, from the rule alone (u = 2^-24): the
4*Cin products are exact in fp32, so accumulation and bias in any order err by
at most gamma_n (sum |wc||x| + |b|), n = 4*Cin + 1, gamma_n = n u / (1 - n u);
the one rounding adds 2^-8 (bf16) / 2^-11 (fp16) of |ref| + that error, and half
a subnormal spacing, 2^-25, for fp16. Measured error / bound:
profiles/conv_up2x_notes.md."""

import pytest
import torch
import torch.nn.functional as F

from distrifuser_amd import ops
from distrifuser_amd.models.layers import LayerFactory
from distrifuser_amd.models.resnet import Upsample2D
from distrifuser_amd.ops import eager
from distrifuser_amd.parallel.state import ParallelState
from distrifuser_amd.utils.config import DistriConfig

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300),
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")]

DEV = "cuda:0"
U = 2.0 ** -24
B = 2
DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16")]
ROUND = {torch.bfloat16: (2.0 ** -8, 0.0), torch.float16: (2.0 ** -11, 2.0 ** -25)}
# (Cin, Cout, H, W, halo rows, x is a channel slice of a wider tensor)
CASES = [
    (8, 8, 1, 1, False, False),
    (8, 8, 2, 2, True, False),
    (64, 32, 7, 31, False, False),
    (64, 32, 8, 32, True, False),
    (72, 40, 9, 33, True, False),
    (72, 40, 9, 40, True, True),
    (8, 40, 17, 32, False, True),
    (64, 8, 16, 64, True, False),
]


def _native(x, weight, bias, top, bot, view):
    """The extension's entry on packed weights, inputs moved to the GPU."""
    x, top, bot = (None if t is None else t.to(DEV) for t in (x, top, bot))
    if view:  # channels 8.. of a tensor with 8 more: strides of the wider one
        x = torch.cat([torch.full_like(x[:, :8], 3.0), x], dim=1)[:, 8:]
        assert not x.is_contiguous()
    packed = ops.pack_upsample2x_conv3x3_weight(weight.to(DEV), x.dtype)
    out = ops.hip_ext().upsample2x_conv3x3(x, packed, bias.to(DEV), weight.shape[0], top, bot)
    assert out.dtype == x.dtype and out.shape == (B, weight.shape[0], 2 * x.shape[2], 2 * x.shape[3])
    return out.cpu()


def _two_op_float64(x, weight, bias, top, bot):
    """interpolate + conv in float64; a halo row is two equal upsampled rows."""
    up = F.interpolate(x.double(), scale_factor=2.0, mode="nearest")
    rows = [torch.zeros_like(up[:, :, :1]) if t is None
            else F.interpolate(t.double(), scale_factor=(1.0, 2.0), mode="nearest")
            for t in (top, bot)]
    return F.conv2d(torch.cat([rows[0], up, rows[1]], dim=2), weight.double(), bias.double(),
                    padding=(0, 1))


@pytest.mark.parametrize("cin,cout,h,w,halo,view", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_small_integers(dtype, cin, cout, h, w, halo, view):
    """x in {-1, 0, 1}, weight tap (dy, dx) = 2^(3dy+dx) * s(cout, cin), s in
    {-1, 0, 1}: the 16 collapsed taps are 16 different subset sums (a swapped
    parity or tap cannot cancel), each exact in 16 bits, and every sum is an
    integer below 2^24, so the kernel must give the float64 two-op result cast
    once."""
    gen = torch.Generator().manual_seed(cin + 3 * cout + 5 * h + 7 * w)
    x, top, bot = (torch.randint(-1, 2, (B, cin, n, w), generator=gen).to(dtype) for n in (h, 1, 1))
    if not halo:
        top = bot = None
    sign = (torch.arange(cout).view(-1, 1) * 7 + torch.arange(cin) * 5) % 3 - 1
    weight = (sign.view(cout, cin, 1, 1) * torch.exp2(torch.arange(9.0)).view(3, 3)).to(dtype)
    bias = (torch.arange(cout) % 7 - 3).to(dtype)
    want = _two_op_float64(x, weight, bias, top, bot).to(dtype)
    assert torch.equal(_native(x, weight, bias, top, bot, view), want)


@pytest.mark.parametrize("cin,cout,h,w,halo,view", [CASES[4], CASES[5]])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bounded_against_float64_rule(dtype, cin, cout, h, w, halo, view):
    gen = torch.Generator().manual_seed(h * w)
    x, top, bot = (torch.randn(B, cin, n, w, generator=gen).to(dtype) for n in (h, 1, 1))
    weight = (torch.randn(cout, cin, 3, 3, generator=gen) / (9 * cin) ** 0.5).to(dtype)
    bias = torch.randn(cout, generator=gen).to(dtype)
    # the rule in float64 on the ROUNDED collapsed weights, and sum |wc||x| + |b|
    wc = eager.collapse_upsample2x_weight(weight).double()
    xp = F.pad(torch.cat([top, x, bot], dim=2).double(), [1, 1, 0, 0])
    ref = torch.empty(B, cout, 2 * h, 2 * w, dtype=torch.float64)
    mag = torch.empty_like(ref)
    for py in range(2):
        for px in range(2):
            k = wc[py, px].permute(2, 3, 0, 1)
            win = xp[:, :, py : py + h + 1, px : px + w + 1]
            ref[:, :, py::2, px::2] = F.conv2d(win, k, bias.double())
            mag[:, :, py::2, px::2] = F.conv2d(win.abs(), k.abs(), bias.double().abs())
    n = 4 * cin + 1
    e32 = n * U / (1 - n * U) * mag
    rel, floor = ROUND[dtype]
    bound = e32 + rel * (ref.abs() + e32) + floor
    ratio = ((_native(x, weight, bias, top, bot, view).double() - ref).abs() / bound).max().item()
    print(f"upsample2x_conv3x3 {dtype} {cin}x{cout} {h}x{w}: largest error / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_upsample2d_route_and_graph_replay():
    """Knob on: the module gives the bits of the rule (integers: every order of
    summation is exact), eagerly and from a replayed graph."""
    cfg = DistriConfig(height=64, width=64, use_cuda_graph=False, device=DEV, upsample_fused=True)
    up = Upsample2D(40, factory=LayerFactory(ParallelState(cfg))).eval()
    conv = up.conv.conv
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        conv.weight.copy_(torch.randint(-2, 3, conv.weight.shape, generator=gen))
        conv.bias.copy_(torch.randint(-4, 5, conv.bias.shape, generator=gen))
    x = torch.randint(-3, 4, (B, 40, 9, 40), generator=gen).to(torch.bfloat16)
    up = up.to(device=DEV, dtype=torch.bfloat16)
    want = eager.upsample2x_conv3x3(x, conv.weight.cpu(), conv.bias.cpu()).to(DEV)
    x = x.to(DEV)
    with torch.no_grad():
        assert torch.equal(up(x), want)  # packs the weight before the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = up(x)
        for _ in range(3):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)
