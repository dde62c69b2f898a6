"""Flash-attention KV staging addresses on the GPU: the in-chunk path (uniform
tile cursor + fixed lane offset) against the per-row chunk resolution that
straddling tiles, tiny chunks and the tail take. The chunked cases use the
production fused layout [NC, B, LC, 2*inner] with B = 2 and H = 2, so batch,
head, chunk and token strides all differ, and the padding between chunks in
the backing buffer is NaN: a wrong chunk address shows up in the result.
Reference and bound as tests/test_attention_tiles_gpu.py:
ops.eager.flash_attention on fp32 copies, max abs error < 0.03.

Run on an MI355X box: pytest tests/test_attention_staging_gpu.py -m gpu -q"""

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
B, H = 2, 2
PAD = 64  # elements of NaN between chunks


def _dev():
    return torch.device("cuda:0")


def _randn(*shape):
    return torch.randn(*shape, device=_dev(), dtype=torch.bfloat16)


def _check_chunked(nc, lc, lq=40, dim_head=64):
    torch.manual_seed(nc * 1000 + lc + lq + dim_head)
    inner = H * dim_head
    q = _randn(B, lq, inner)
    slot = B * lc * 2 * inner
    buf = torch.full((nc, slot + PAD), float("nan"), device=_dev(), dtype=torch.bfloat16)
    buf[:, :slot] = _randn(nc, slot)
    kv_chunks = buf[:, :slot].view(nc, B, lc, 2 * inner)
    out = ops.flash_attention_chunked(q, kv_chunks, H, dim_head).float()

    full = kv_chunks.permute(1, 0, 2, 3).reshape(B, nc * lc, 2 * inner).float()
    kf, vf = full.split(inner, dim=-1)
    qf = q.float().view(B, lq, H, dim_head).transpose(1, 2)
    kf = kf.reshape(B, nc * lc, H, dim_head).transpose(1, 2)
    vf = vf.reshape(B, nc * lc, H, dim_head).transpose(1, 2)
    ref = eager.flash_attention(qf, kf, vf).transpose(1, 2).reshape(B, lq, inner)
    what = f"nc={nc} lc={lc} lq={lq} d={dim_head}"
    assert out.shape == ref.shape
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    err = (out - ref).abs().max().item()
    print(f"{what}: max err {err:.5f}")
    assert err < TOL, f"{what}: max err {err}"


@requires_gpu
@pytest.mark.parametrize(
    "nc,lc",
    [
        (2, 128),   # the chunk boundary falls exactly on a tile edge
        (3, 136),   # the second tile straddles by 8 tokens
        (2, 264),   # the straddling tile is the third tile
        (3, 200),   # Lkv = 600: the masked tail itself straddles
        (20, 8),    # a tile spans 16 chunks: per-row resolution throughout
    ],
)
def test_chunk_boundaries_against_tiles(nc, lc):
    _check_chunked(nc, lc)


@requires_gpu
def test_token_stride_wider_than_head_dim():
    """flash_attention proper on strided views: k_sl = v_sl = 96 with head_dim
    64, and NaN in the columns the views leave out."""
    torch.manual_seed(320)
    lq, lkv, d, wide = 40, 320, 64, 96
    q = _randn(B, H, lq, d)
    kbig = torch.full((B, H, lkv, wide), float("nan"), device=_dev(), dtype=torch.bfloat16)
    vbig = torch.full((B, H, lkv, wide), float("nan"), device=_dev(), dtype=torch.bfloat16)
    kbig[..., :d] = _randn(B, H, lkv, d)
    vbig[..., :d] = _randn(B, H, lkv, d)
    k, v = kbig[..., :d], vbig[..., :d]
    assert k.stride(2) == wide
    out = ops.flash_attention(q, k, v).float()
    ref = eager.flash_attention(q.float(), k.float(), v.float())
    assert out.shape == ref.shape
    assert torch.isfinite(out).all(), "strided view: non-finite output"
    err = (out - ref).abs().max().item()
    print(f"strided view: max err {err:.5f}")
    assert err < TOL, f"strided view: max err {err}"


@requires_gpu
def test_padded_head_dim_with_chunks():
    """head_dim 40 in 64-wide tiles: the column predicate together with the
    in-chunk addressing and a straddling tile."""
    _check_chunked(3, 136, dim_head=40)


@requires_gpu
def test_two_q_blocks_with_chunks():
    """Lq = 257: two 256-row blocks per (batch, head), each with its own
    cursor."""
    _check_chunked(3, 136, lq=257)
