"""fp16 instantiations of the flash-attention and merge kernels on the GPU.

Every case builds its inputs as bf16 and casts them to fp16 (values that do not
survive the cast are zeroed), so the bf16 kernel and the fp16 kernel see the
same numbers. The reference is ops.eager on fp32 copies. For each case
(a) the fp16 error is under the project's bound (0.03 max abs; LSE 2e-3) and
(b) it is no larger than the bf16 kernel's error on the same case: fp16 carries
three more mantissa bits and every accumulation is fp32 in both.

The kernels are called through ops.hip_ext() directly: a dispatch-level call
would fall back to eager without saying so.

Run on an MI355X box: pytest tests/test_fp16_attention_gpu.py -m gpu -q -s"""

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
LSE_TOL = 2e-3
B, H = 2, 2
PAD = 64  # elements of NaN between chunk slots


def _dev():
    return torch.device("cuda:0")


def _both(*shape, scale=1.0):
    """(bf16, fp16) tensors holding the same values."""
    xb = (torch.randn(*shape, device=_dev()) * scale).to(torch.bfloat16)
    x16 = xb.to(torch.float16)
    bad = x16.float() != xb.float()  # below fp16's subnormal grid: rare
    xb[bad] = 0
    x16[bad] = 0
    assert torch.equal(x16.float(), xb.float())
    return xb, x16


def _errs(what, out16, outb, ref):
    assert out16.dtype == torch.float16 and outb.dtype == torch.bfloat16
    assert out16.shape == ref.shape
    assert torch.isfinite(out16.float()).all(), f"{what}: non-finite fp16 output"
    e16 = (out16.float() - ref).abs().max().item()
    eb = (outb.float() - ref).abs().max().item()
    print(f"{what}: fp16 err {e16:.6f}  bf16 err {eb:.6f}")
    assert e16 < TOL, f"{what}: fp16 max err {e16}"
    assert e16 <= eb, f"{what}: fp16 err {e16} above the bf16 kernel's {eb}"


def _plain_case(lq, lkv, d, qscale=1.0, what=None):
    torch.manual_seed(lq * 7 + lkv + d)
    qb, q16 = _both(1, 2, lq, d, scale=qscale)
    kb, k16 = _both(1, 2, lkv, d)
    vb, v16 = _both(1, 2, lkv, d)
    ext = ops.hip_ext()
    out16 = ext.flash_attention(q16, k16, v16)
    outb = ext.flash_attention(qb, kb, vb)
    ref = eager.flash_attention(qb.float(), kb.float(), vb.float())
    _errs(what or f"lq={lq} lkv={lkv} d={d}", out16, outb, ref)


@requires_gpu
@pytest.mark.parametrize("d", [40, 64, 80, 96, 120, 128, 152, 160])
@pytest.mark.parametrize("lkv", [8, 200, 320])
def test_fp16_attention_shapes(lkv, d):
    """Sub-tile, tile + masked tail, two tiles + mask-free tail; every DPAD,
    full and padded."""
    _plain_case(33, lkv, d)


@requires_gpu
def test_fp16_attention_two_q_blocks():
    """Lq = 300: two 256-row blocks, invalid rows in the last."""
    _plain_case(300, 320, 64)


@requires_gpu
def test_fp16_attention_wide_scores():
    """q scaled by 4: the scores spread over tens of units, so most P values
    of a row lie below 2^-14, subnormal in fp16 where bf16 holds them as
    normal numbers."""
    _plain_case(33, 320, 64, qscale=4.0, what="wide scores (q x4) lkv=320 d=64")


def _chunked(nc, lc, d, lq=33):
    torch.manual_seed(nc * 1000 + lc + d)
    inner = H * d
    qb, q16 = _both(B, lq, inner)
    slot = B * lc * 2 * inner
    valb, val16 = _both(nc, slot)
    views = []
    for val, dt in ((valb, torch.bfloat16), (val16, torch.float16)):
        buf = torch.full((nc, slot + PAD), float("nan"), device=_dev(), dtype=dt)
        buf[:, :slot] = val
        kv = buf[:, :slot].view(nc, B, lc, 2 * inner)
        k5 = kv[..., :inner].unflatten(-1, (H, d)).permute(1, 3, 0, 2, 4)
        v5 = kv[..., inner:].unflatten(-1, (H, d)).permute(1, 3, 0, 2, 4)
        views.append((kv, k5, v5))
    q4b = qb.view(B, lq, H, d).permute(0, 2, 1, 3)
    q416 = q16.view(B, lq, H, d).permute(0, 2, 1, 3)
    kvb = views[0][0]
    full = kvb.permute(1, 0, 2, 3).reshape(B, nc * lc, 2 * inner).float()
    kf, vf = full.split(inner, dim=-1)
    kf = kf.reshape(B, nc * lc, H, d).transpose(1, 2)
    vf = vf.reshape(B, nc * lc, H, d).transpose(1, 2)
    return (q4b, views[0][1], views[0][2]), (q416, views[1][1], views[1][2]), (q4b.float(), kf, vf)


@requires_gpu
@pytest.mark.parametrize("d", [64, 40])
@pytest.mark.parametrize("lc", [40, 72])
def test_fp16_attention_chunked(lc, d):
    """NC = 4 slots of a strided flat buffer with NaN between them; tiles start
    mid-chunk."""
    argb, arg16, argf = _chunked(4, lc, d)
    ext = ops.hip_ext()
    _errs(f"chunked nc=4 lc={lc} d={d}", ext.flash_attention(*arg16), ext.flash_attention(*argb),
          eager.flash_attention(*argf))


# ---- LSE and split-KV -----------------------------------------------------------


@requires_gpu
@pytest.mark.parametrize("d", [40, 160])
def test_fp16_lse_at_one_split_leaves_output_bits(d):
    torch.manual_seed(d)
    _, q16 = _both(1, 2, 33, d)
    _, k16 = _both(1, 2, 320, d)
    _, v16 = _both(1, 2, 320, d)
    ext = ops.hip_ext()
    out, lse = ext.flash_attention_ext(q16, k16, v16, 1, True)
    assert out.dtype == torch.float16 and lse.dtype == torch.float32
    assert torch.equal(out, ext.flash_attention(q16, k16, v16))
    _, ref_lse = eager.flash_attention_lse(q16.float(), k16.float(), v16.float())
    err = (lse - ref_lse).abs().max().item()
    print(f"lse S=1 d={d}: err {err:.3e}")
    assert err < LSE_TOL


@requires_gpu
@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("d", [40, 160])
@pytest.mark.parametrize("splits", [2, 3])
def test_fp16_split_kv(splits, d, chunked):
    """Lkv = 320 (chunked: 4 chunks of 80) over S splits, merged into fp16."""
    if chunked:
        argb, arg16, argf = _chunked(4, 80, d)
    else:
        torch.manual_seed(splits * 100 + d)
        qb, q16 = _both(1, 2, 33, d)
        kb, k16 = _both(1, 2, 320, d)
        vb, v16 = _both(1, 2, 320, d)
        argb, arg16, argf = (qb, kb, vb), (q16, k16, v16), (qb.float(), kb.float(), vb.float())
    ext = ops.hip_ext()
    out16, lse16 = ext.flash_attention_ext(*arg16, splits, True)
    outb, _ = ext.flash_attention_ext(*argb, splits, True)
    ref, ref_lse = eager.flash_attention_lse(*argf)
    what = f"S={splits} d={d} chunked={chunked}"
    _errs(what, out16, outb, ref)
    lse_err = (lse16 - torch.logsumexp(
        torch.einsum("bhqd,bhkd->bhqk", argf[0], argf[1]) * d ** -0.5, dim=-1)).abs().max().item()
    print(f"{what}: lse err {lse_err:.3e}")
    assert lse_err < LSE_TOL and (lse16 - ref_lse).abs().max().item() < LSE_TOL
    again, lse_again = ext.flash_attention_ext(*arg16, splits, True)
    assert torch.equal(again, out16) and torch.equal(lse_again, lse16), "split call not reproducible"
    assert torch.equal(ext.flash_attention_ext(*arg16, splits, False)[0], out16)


@requires_gpu
@pytest.mark.parametrize("d", [64, 40])
def test_merge_to_fp16_is_the_rounded_fp32_result(d):
    torch.manual_seed(d)
    s, b, h, lq = 3, 2, 2, 33
    o_parts = torch.randn(s, b, lq, h, d, device=_dev())
    lse_parts = torch.randn(s, b, h, lq, device=_dev()) * 3
    lse_parts[1, 0] = float("-inf")
    ext = ops.hip_ext()
    out32, lse32 = ext.merge_attention(o_parts, lse_parts, False)
    out16, lse16 = ext.merge_attention(o_parts, lse_parts, False, torch.float16)
    assert out32.dtype == torch.float32 and out16.dtype == torch.float16
    assert torch.equal(out16, out32.half()) and torch.equal(lse16, lse32)
    ref, _ = eager.merge_attention(o_parts.cpu(), lse_parts.cpu())
    assert (out32.cpu() - ref).abs().max().item() < 1e-5
    # the dispatcher reaches the same kernel; the bool entry still means bf16
    assert torch.equal(ops.merge_attention(o_parts, lse_parts, out_dtype=torch.float16), out16)
    assert ext.merge_attention(o_parts, lse_parts, True)[0].dtype == torch.bfloat16


@requires_gpu
def test_dispatch_takes_the_kernel_for_fp16(monkeypatch):
    """ops.flash_attention / flash_attention_chunked hand fp16 to the native
    entries (counted), kv_splits included."""
    ext = ops.hip_ext()
    calls = {"flash_attention": 0, "flash_attention_ext": 0}
    for name in calls:
        real = getattr(ext, name)

        def counted(*a, _real=real, _name=name):
            calls[_name] += 1
            return _real(*a)

        monkeypatch.setattr(ext, name, counted)
    _, arg16, _ = _chunked(4, 80, 64)
    q4, k5, v5 = arg16
    ops.flash_attention(q4, k5[:, :, 0], v5[:, :, 0])
    ops.flash_attention(q4, k5[:, :, 0], v5[:, :, 0], kv_splits=2)
    assert calls == {"flash_attention": 1, "flash_attention_ext": 1}


@requires_gpu
def test_attention_rejects_mixed_dtypes():
    qb, q16 = _both(1, 2, 33, 64)
    kb, k16 = _both(1, 2, 64, 64)
    ext = ops.hip_ext()
    with pytest.raises(RuntimeError, match="k must have q's dtype"):
        ext.flash_attention(q16, kb, k16)
    with pytest.raises(RuntimeError, match="v must have q's dtype"):
        ext.flash_attention(q16, k16, kb)
    with pytest.raises(RuntimeError, match="k must have q's dtype"):
        ext.flash_attention_ext(qb, k16, kb, 1, False)
    with pytest.raises(RuntimeError, match="bf16 or fp16 only"):
        ext.flash_attention(q16.float(), k16.float(), k16.float())
