"""Flash attention on the GPU: LDS-DMA staging into two KV buffers with one
barrier per tile (head_dim 64), and the register path it alternates with.

A full tile inside one chunk is fetched by LDS-DMA into the buffer the
previous tile is not being read from; a tile that straddles chunks, the tail
and every tile of the other head dims go through registers. The shapes are the
smallest at which each hand-over can go wrong: both buffers reused and then a
tail, DMA and register tiles alternating, a run that ends in DMA tiles only, a
split-KV start on an odd tile or mid-chunk. The chunked cases use the
production fused layout [NC, B, LC, 2*inner] with B = 2 and H = 2 and NaN
between the chunks, so a DMA that reads from the wrong place shows up.
Reference and bound as tests/test_attention_tiles_gpu.py:
ops.eager.flash_attention on fp32 copies, max abs error < 0.03.

Run on an MI355X box: pytest tests/test_attention_dma_gpu.py -m gpu -q"""

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
LSE_TOL = 2e-3  # as tests/test_attention_splitkv_gpu.py
B, H = 2, 2
PAD = 64  # elements of NaN between chunks


def _dev():
    return torch.device("cuda:0")


def _randn(*shape, dtype=torch.bfloat16):
    return torch.randn(*shape, device=_dev(), dtype=dtype)


def _check_plain(lq, lkv, d=64, dtype=torch.bfloat16):
    torch.manual_seed(lq * 7 + lkv + d)
    q, k, v = (_randn(B, H, lq, d, dtype=dtype), _randn(B, H, lkv, d, dtype=dtype),
               _randn(B, H, lkv, d, dtype=dtype))
    out = ops.flash_attention(q, k, v)
    ref = eager.flash_attention(q.float(), k.float(), v.float())
    what = f"lq={lq} lkv={lkv} d={d} {dtype}"
    assert out.shape == ref.shape and out.dtype == dtype
    assert torch.isfinite(out.float()).all(), f"{what}: non-finite output"
    err = (out.float() - ref).abs().max().item()
    print(f"{what}: max err {err:.5f}")
    assert err < TOL, f"{what}: max err {err}"
    return q, k, v, out


def _chunked(nc, lc, lq, dim_head=64, dtype=torch.bfloat16):
    """q, the NaN-separated chunk buffer view and the fp32 reference pieces."""
    torch.manual_seed(nc * 1000 + lc + lq + dim_head)
    inner = H * dim_head
    q = _randn(B, lq, inner, dtype=dtype)
    slot = B * lc * 2 * inner
    buf = torch.full((nc, slot + PAD), float("nan"), device=_dev(), dtype=dtype)
    buf[:, :slot] = _randn(nc, slot, dtype=dtype)
    kv_chunks = buf[:, :slot].view(nc, B, lc, 2 * inner)
    full = kv_chunks.permute(1, 0, 2, 3).reshape(B, nc * lc, 2 * inner).float()
    kf, vf = full.split(inner, dim=-1)
    qf = q.float().view(B, lq, H, dim_head).transpose(1, 2)
    kf = kf.reshape(B, nc * lc, H, dim_head).transpose(1, 2)
    vf = vf.reshape(B, nc * lc, H, dim_head).transpose(1, 2)
    return q, kv_chunks, qf, kf, vf


def _check_chunked(nc, lc, lq=40, dim_head=64, dtype=torch.bfloat16, splits=1):
    q, kv_chunks, qf, kf, vf = _chunked(nc, lc, lq, dim_head, dtype)
    inner = H * dim_head
    kw = {} if splits == 1 else {"kv_splits": splits}
    out = ops.flash_attention_chunked(q, kv_chunks, H, dim_head, **kw).float()
    ref = eager.flash_attention(qf, kf, vf).transpose(1, 2).reshape(B, lq, inner)
    what = f"nc={nc} lc={lc} lq={lq} d={dim_head} S={splits} {dtype}"
    assert out.shape == ref.shape
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    err = (out - ref).abs().max().item()
    print(f"{what}: max err {err:.5f}")
    assert err < TOL, f"{what}: max err {err}"


# ---- 1. both buffers reused, then a tail ------------------------------------------


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("lkv", [3 * 128 + 40, 4 * 128 + 64])
def test_both_buffers_then_tail(lkv, dtype):
    """Lq = 300: a partial second Q block. 3 and 4 DMA tiles, then the masked
    40-token tail / the mask-free 64-token tail through registers."""
    _check_plain(300, lkv, dtype=dtype)


# ---- 2. DMA and register tiles alternating ----------------------------------------


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize(
    "nc,lc",
    [
        (3, 200),   # DMA, straddle, straddle, DMA, masked tail that straddles
        (2, 264),   # DMA, DMA, straddle, DMA, tail
        (3, 136),   # DMA, straddle, straddle, tail
        (2, 256),   # the chunk edge on a tile edge: DMA tiles only, cursor re-seated
        (20, 8),    # no DMA tile at all
    ],
)
def test_dma_and_register_tiles_alternate(nc, lc, dtype):
    _check_chunked(nc, lc, dtype=dtype)


@requires_gpu
def test_alternating_tiles_two_q_blocks():
    _check_chunked(3, 200, lq=300)


# ---- 3. a run that ends in DMA tiles only -----------------------------------------


@requires_gpu
@pytest.mark.parametrize("lkv", [128, 384])
def test_dma_tiles_only(lkv):
    """No tail: nothing behind the last DMA tile that could hide its being late."""
    _check_plain(300, lkv)


# ---- 4. split-KV --------------------------------------------------------------------


@requires_gpu
@pytest.mark.parametrize("splits", [2, 3])
def test_split_plain(splits):
    """Lkv = 5*128 + 40, 6 tiles: S = 2 starts split 1 on tile 3 (odd), S = 3 on
    tiles 2 and 4; merged output and LSE against the reference."""
    torch.manual_seed(splits)
    lq, lkv = 300, 5 * 128 + 40
    q, k, v = _randn(B, H, lq, 64), _randn(B, H, lkv, 64), _randn(B, H, lkv, 64)
    out, lse = ops.flash_attention(q, k, v, kv_splits=splits, return_lse=True)
    ref, ref_lse = eager.flash_attention_lse(q.float(), k.float(), v.float())
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    err = (out.float() - ref).abs().max().item()
    lse_err = (lse - ref_lse).abs().max().item()
    print(f"S={splits}: max err {err:.5f}, lse err {lse_err:.2e}")
    assert err < TOL, f"S={splits}: max err {err}"
    assert lse_err < LSE_TOL, f"S={splits}: lse err {lse_err}"
    assert torch.equal(ops.flash_attention(q, k, v, kv_splits=splits), out)


@requires_gpu
@pytest.mark.parametrize("splits", [2, 3])
def test_split_chunked(splits):
    """NC = 4, LC = 200, 7 tiles: the splits start mid-chunk (S = 2: token 384
    = chunk 1, token 184, a straddling tile; S = 3: tokens 256 and 512)."""
    _check_chunked(4, 200, splits=splits)
    q, kv_chunks, qf, kf, vf = _chunked(4, 200, 40)
    inner = H * 64
    k5 = kv_chunks[..., :inner].unflatten(-1, (H, 64)).permute(1, 3, 0, 2, 4)
    v5 = kv_chunks[..., inner:].unflatten(-1, (H, 64)).permute(1, 3, 0, 2, 4)
    q4 = q.view(B, 40, H, 64).permute(0, 2, 1, 3)
    _, lse = ops.flash_attention(q4, k5, v5, kv_splits=splits, return_lse=True)
    _, ref_lse = eager.flash_attention_lse(qf, kf, vf)
    lse_err = (lse - ref_lse).abs().max().item()
    print(f"chunked S={splits}: lse err {lse_err:.2e}")
    assert lse_err < LSE_TOL


# ---- 5. the other head dims -----------------------------------------------------------


@requires_gpu
@pytest.mark.parametrize("d", [40, 80, 128, 160])
def test_register_path_head_dims(d):
    """40 (padded to 64), 80, 128 and 160 keep register staging and one buffer."""
    _check_plain(300, 3 * 128 + 40, d=d)
    _check_chunked(3, 200, dim_head=d)


# ---- 6. token stride wider than the head dim -----------------------------------------


@requires_gpu
def test_token_stride_wider_than_head_dim():
    """k_sl = v_sl = 96 with head_dim 64, NaN in the columns the views leave
    out: the swizzled source column of a DMA lane stays inside the head."""
    torch.manual_seed(452)
    lq, lkv, d, wide = 300, 3 * 128 + 40, 64, 96
    q = _randn(B, H, lq, d)
    kbig = torch.full((B, H, lkv, wide), float("nan"), device=_dev(), dtype=torch.bfloat16)
    vbig = torch.full((B, H, lkv, wide), float("nan"), device=_dev(), dtype=torch.bfloat16)
    kbig[..., :d] = _randn(B, H, lkv, d)
    vbig[..., :d] = _randn(B, H, lkv, d)
    k, v = kbig[..., :d], vbig[..., :d]
    assert k.stride(2) == wide
    out = ops.flash_attention(q, k, v).float()
    ref = eager.flash_attention(q.float(), k.float(), v.float())
    assert torch.isfinite(out).all(), "strided view: non-finite output"
    err = (out - ref).abs().max().item()
    print(f"strided view: max err {err:.5f}")
    assert err < TOL, f"strided view: max err {err}"


# ---- 7. determinism ---------------------------------------------------------------------


@requires_gpu
def test_same_call_twice_same_bits():
    """A DMA / barrier race would most likely show as a run-to-run difference.
    Enough Q blocks (2 * 2 * 24) that blocks share CUs."""
    q, k, v, out = _check_plain(6000, 9 * 128 + 40)
    assert torch.equal(ops.flash_attention(q, k, v), out)
    qc, kv_chunks, *_ = _chunked(3, 200, 300)
    o1 = ops.flash_attention_chunked(qc, kv_chunks, H, 64)
    o2 = ops.flash_attention_chunked(qc, kv_chunks, H, 64)
    assert torch.equal(o1, o2)
