"""The fused GEGLU projection kernel (csrc/geglu_linear.hip), called through the
extension so that nothing can fall back. Block tile T = 128 tokens x N = 128
outputs, K-step 64: rows {1, T-1, T, T+1, 2T+1} and inner {8, N, N+8} reach every
tail and a second block each way; K {64, 192, 320} is one, three and five steps,
K = 72 ends in a step with one real 16-byte piece (the zero-filled k tail).

Bound of the random cases, per element, from the rule alone (u = 2^-24):
  accumulation  E = gamma_{K+1} (sum |x||w| + |b|) for a and for g, gamma_n =
                n u / (1 - n u): K exact products and the bias, any order;
  propagation   E_a |gelu(g)| + 1.13 |a| E_g + 1.13 E_a E_g  (|gelu'| <= 1.13);
  geluf         8u |a||g| + 4u |ref| (tests/test_geglu_edges_gpu.py), taken at
                |a| + E_a, |g| + E_g;
  rounding      2^-8 (bf16) / 2^-11 (fp16) of |ref| + the fp32 error, and half
                a subnormal spacing, 2^-25, for fp16.
Measured error / bound: profiles/geglu_linear_notes.md."""

import pytest
import torch
import torch.nn.functional as F

from distrifuser_amd import ops
from distrifuser_amd.models.layers import FeedForward
from distrifuser_amd.ops import eager
from distrifuser_amd.utils.config import DistriConfig

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300),
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")]

DEV = "cuda:0"
U = 2.0 ** -24
T, N = 128, 128
ROWS = (1, T - 1, T, T + 1, 2 * T + 1)
INNERS = (8, N, N + 8)
DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16")]
KS = (64, 72, 192, 320)
ROUND = {torch.bfloat16: (2.0 ** -8, 0.0), torch.float16: (2.0 ** -11, 2.0 ** -25)}


def _native(x, w, b):
    """The extension's entry on packed weights, inputs moved to the GPU."""
    x, w, b = x.to(DEV), w.to(DEV), b.to(DEV)
    out = ops.hip_ext().geglu_linear(x, ops.pack_geglu_weight(w), b, w.shape[0] // 2)
    assert out.dtype == x.dtype and out.shape == (x.shape[0], w.shape[0] // 2)
    return out.cpu()


def _reference(x, w, b):
    """(float64 a * gelu(g), bound) on the rounded inputs."""
    dtype, k = x.dtype, x.shape[1]
    x, w, b = x.double(), w.double(), b.double()
    a, g = (x @ w.t() + b).chunk(2, dim=-1)
    gel = F.gelu(g)
    ref = a * gel
    gamma = (k + 1) * U / (1 - (k + 1) * U)
    e_a, e_g = (gamma * (x.abs() @ w.abs().t() + b.abs())).chunk(2, dim=-1)
    e32 = e_a * gel.abs() + 1.13 * a.abs() * e_g + 1.13 * e_a * e_g
    e32 = e32 + 8 * U * (a.abs() + e_a) * (g.abs() + e_g) + 4 * U * ref.abs()
    rel, floor = ROUND[dtype]
    return ref, e32 + rel * (ref.abs() + e32) + floor


def _random(rows, k, inner, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, k, generator=gen).to(dtype)
    w = (torch.randn(2 * inner, k, generator=gen) / k ** 0.5).to(dtype)
    return x, w, torch.randn(2 * inner, generator=gen).to(dtype)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_gather(dtype, k):
    """Value rows one-hot at column (7i+3) % K, gate rows zero with bias 16:
    out[r, i] = 16 * x[r, (7i+3) % K] exactly (gelu(16) = 16 to the last fp32
    bit, checked first): which half is which, every column, k position and tail."""
    g = torch.tensor([16.0])
    assert (F.gelu(g.double()) - 16.0).abs().item() < 16 * 2.0 ** -60
    assert (0.5 * g * (1.0 + torch.erf(g * 0.70710678118654752440))).item() == 16.0  # geluf()
    for inner in INNERS:
        col = (7 * torch.arange(inner) + 3) % k
        w = torch.zeros(2 * inner, k)
        w[torch.arange(inner), col] = 1.0
        b = torch.cat([torch.zeros(inner), torch.full((inner,), 16.0)])
        for rows in ROWS:
            r = torch.arange(rows).view(-1, 1)
            x = ((r * k + torch.arange(k)) % 17 - 8) * torch.exp2((r % 5 - 2).float())
            got = _native(x.to(dtype), w.to(dtype), b.to(dtype))
            assert torch.equal(got, (16.0 * x[:, col]).to(dtype)), (rows, inner)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bounded_against_float64(dtype, k):
    worst = 0.0
    for inner in INNERS:
        for rows in ROWS:
            x, w, b = _random(rows, k, inner, dtype, seed=rows * 1000 + inner + k)
            ref, bound = _reference(x, w, b)
            ratio = ((_native(x, w, b).double() - ref).abs() / bound).max().item()
            worst = max(worst, ratio)
            assert ratio <= 1.0, (rows, inner, ratio)
    print(f"geglu_linear {dtype} K={k}: largest error / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_rounding_not_two(dtype):
    """No further from float64 than geglu(linear(x)), which rounds the projection
    first. Two roundings can leave the bound (one bf16 element in six does), so
    the comparison runs where that composition, on the CPU first, is inside it."""
    x, w, b = _random(T + 1, 192, N + 8, dtype, seed=7)
    ref, bound = _reference(x, w, b)
    cpu = eager.geglu((x.float() @ w.float().t() + b.float()).to(dtype))
    inside = (cpu.double() - ref).abs() <= bound
    comp = ops.geglu(F.linear(x.to(DEV), w.to(DEV), b.to(DEV))).cpu()
    e_comp, e_fused = ((t.double() - ref).abs()[inside].max().item()
                       for t in (comp, _native(x, w, b)))
    assert e_fused <= e_comp, f"fused {e_fused:.3e}, composition {e_comp:.3e}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_dispatch(dtype):
    x, w, b = (t.to(DEV) for t in _random(T + 1, 72, 24, dtype, seed=3))
    bits = ops.hip_ext().geglu_linear(x, ops.pack_geglu_weight(w), b, 24)
    assert torch.equal(ops.geglu_linear(x, w, b), bits)
    wide = torch.cat([x, x], dim=1)[:, :72]  # rows 144 elements apart: still native
    assert torch.equal(ops.geglu_linear(wide, w, b), bits)
    xt = x.t().contiguous().t()  # not contiguous along K: the eager rule
    assert torch.equal(ops.geglu_linear(xt, w, b), eager.geglu_linear(xt, w, b))
    f32 = (x.float(), w.float(), b.float())
    assert torch.equal(ops.geglu_linear(*f32), eager.geglu_linear(*f32))


def test_feed_forward_graph_replay():
    torch.manual_seed(5)
    cfg = DistriConfig(height=64, width=64, use_cuda_graph=False, device=DEV, ff_fused=True)
    ff = FeedForward(64, config=cfg).to(device=DEV, dtype=torch.bfloat16).eval()
    x = torch.randn(2, T + 3, 64, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        want = ff(x)  # packs the weight before the capture
        rule = ff.proj_out(ops.hip_ext().geglu_linear(x, ff.packed_weight(), ff.proj_in.bias, 256))
        assert torch.equal(want, rule)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ff(x)
        for _ in range(3):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)
