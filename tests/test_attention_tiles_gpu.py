"""Flash-attention tile structure on the GPU: 128-token tiles with a peeled
tail, partial Q blocks, the chunk cursor, padded head dims under transposed
LDS reads, and the defer-max rescale hazard. Every case compares against
ops.eager.flash_attention on fp32 copies with the project's tolerance
(max abs error < 0.03, as tests/test_ops_gpu.py).

Run on an MI355X box: pytest tests/test_attention_tiles_gpu.py -m gpu -q"""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

if torch.cuda.is_available():
    from distrifuser_amd import ops
    from distrifuser_amd.ops import eager
else:  # collected on CPU boxes but never run
    ops = eager = None

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

TOL = 0.03


def _dev():
    return torch.device("cuda:0")


def _check(q, k, v, what):
    out = ops.flash_attention(q, k, v).float()
    ref = eager.flash_attention(q.float(), k.float(), v.float())
    assert out.shape == ref.shape
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    err = (out - ref).abs().max().item()
    print(f"{what}: max err {err:.5f}")
    assert err < TOL, f"{what}: max err {err}"


def _randn(*shape):
    return torch.randn(*shape, device=_dev(), dtype=torch.bfloat16)


@requires_gpu
@pytest.mark.parametrize("lkv", [8, 64, 72, 128, 192, 200, 320])
def test_tile_and_tail_boundaries(lkv):
    """8: less than a tile; 192: 128 + mask-free 64 tail; 200: 128 + masked
    tail; 320: 2 x 128 + 64 tail."""
    torch.manual_seed(lkv)
    _check(_randn(1, 2, 32, 64), _randn(1, 2, lkv, 64), _randn(1, 2, lkv, 64), f"lkv={lkv}")


@requires_gpu
@pytest.mark.parametrize("lq", [1, 33, 256, 257])
def test_partial_q_blocks(lq):
    torch.manual_seed(lq)
    _check(_randn(1, 2, lq, 64), _randn(1, 2, 192, 64), _randn(1, 2, 192, 64), f"lq={lq}")


@requires_gpu
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("nc,lc", [(3, 72), (2, 200), (5, 8)])
def test_chunked_kv_cursor_matches_cat(nc, lc, b):
    """5-D chunked KV with a padded chunk stride: chunk boundaries fall inside
    128-token tiles; the result must agree with attention over the
    concatenated KV."""
    torch.manual_seed(nc * 1000 + lc + b)
    heads, dim_head, lq = 2, 64, 33
    inner = heads * dim_head
    q = _randn(b, lq, inner)
    slot = b * lc * 2 * inner
    buf = _randn(nc, slot + 64)
    kv_chunks = buf[:, :slot].view(nc, b, lc, 2 * inner)
    out = ops.flash_attention_chunked(q, kv_chunks, heads, dim_head).float()

    full = kv_chunks.permute(1, 0, 2, 3).reshape(b, nc * lc, 2 * inner).float()
    kf, vf = full.split(inner, dim=-1)
    qf = q.float().view(b, lq, heads, dim_head).transpose(1, 2)
    kf = kf.view(b, nc * lc, heads, dim_head).transpose(1, 2)
    vf = vf.view(b, nc * lc, heads, dim_head).transpose(1, 2)
    ref = eager.flash_attention(qf, kf, vf).transpose(1, 2).reshape(b, lq, inner)
    err = (out - ref).abs().max().item()
    print(f"nc={nc} lc={lc} b={b}: max err {err:.5f}")
    assert err < TOL, f"nc={nc} lc={lc} b={b}: max err {err}"


@requires_gpu
@pytest.mark.parametrize("d", [40, 80, 160])
def test_padded_head_dims(d):
    torch.manual_seed(d)
    _check(_randn(1, 2, 33, d), _randn(1, 2, 200, d), _randn(1, 2, 200, d), f"d={d}")


@requires_gpu
def test_padded_head_dim_never_reads_past_dh():
    """K and V are strided views whose columns >= Dh hold large garbage in
    memory: the padding lanes of the staged tile must be zeros, not reads."""
    torch.manual_seed(7)
    d, lq, lkv = 40, 33, 200
    q = _randn(1, 2, lq, d)
    kbig = torch.full((1, 2, lkv, d + 24), 3.0e4, device=_dev(), dtype=torch.bfloat16)
    vbig = torch.full((1, 2, lkv, d + 24), -3.0e4, device=_dev(), dtype=torch.bfloat16)
    kbig[..., :d] = _randn(1, 2, lkv, d)
    vbig[..., :d] = _randn(1, 2, lkv, d)
    _check(q, kbig[..., :d], vbig[..., :d], "garbage beyond Dh")


def _stepped_inputs(step_at, even_rows_only=False, lq=64, lkv=320, d=64):
    """Scores that jump by 10 nats (14.4 log2 units, above the 11-unit defer
    threshold) at KV token `step_at`: q and k share the direction u, and k's
    component along u steps from 0 to 10 (q's is 8 = sqrt(d), so the scaled
    score is k's component). |V| <= 4."""
    u = torch.ones(d, device=_dev()) / d ** 0.5
    alpha = torch.full((lq, 1), 8.0, device=_dev())
    if even_rows_only:
        alpha[1::2] = 0.0
    beta = torch.zeros(lkv, 1, device=_dev())
    beta[step_at:] = 10.0
    q = alpha * u + 0.5 * torch.randn(lq, d, device=_dev())
    k = beta * u + 0.5 * torch.randn(lkv, d, device=_dev())
    v = torch.randn(lkv, d, device=_dev()).clamp_(-4.0, 4.0)
    to = lambda t: t.to(torch.bfloat16)[None, None].expand(1, 2, -1, -1).contiguous()
    return to(q), to(k), to(v)


@requires_gpu
@pytest.mark.parametrize(
    "name,step_at,even_only",
    [
        ("tile_boundary", 128, False),      # (a) between the two full tiles
        ("subtile_boundary", 160, False),   # (b) inside a tile, at a 32-token sub-tile
        ("split_row_block", 128, True),     # (c) only even q rows step: rescale + defer mixed
        ("peeled_tail", 288, False),        # (d) inside the 64-token tail
    ],
)
def test_defer_max_rescale_hazard(name, step_at, even_only):
    torch.manual_seed(11)
    q, k, v = _stepped_inputs(step_at, even_only)
    _check(q, k, v, f"defer-max {name}")
