"""fp16 instantiations of LayerNorm, add-LayerNorm and the VAE mid-block
attention on the GPU, called through ops.hip_ext() directly.

Inputs are built as bf16 and cast to fp16, so both kernels see the same
numbers; the reference is ops.eager on fp32 copies; bounds are the project's
(LayerNorm 0.05, VAE attention 0.03 max abs) and the fp16 error may not exceed
the bf16 kernel's.

Run on an MI355X box: pytest tests/test_fp16_norm_vae_gpu.py -m gpu -q -s"""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

if torch.cuda.is_available():
    from distrifuser_amd import ops
    from distrifuser_amd.ops import eager
else:  # collected on CPU boxes but never run
    ops = eager = None

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

DEV = "cuda:0"
LN_TOL = 0.05
VAE_TOL = 0.03


def _both(*shape, scale=1.0):
    xb = (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16)
    x16 = xb.to(torch.float16)
    bad = x16.float() != xb.float()
    xb[bad] = 0
    x16[bad] = 0
    assert torch.equal(x16.float(), xb.float())
    return xb, x16


def _errs(what, got16, gotb, ref, tol):
    assert got16.dtype == torch.float16 and got16.shape == ref.shape
    assert torch.isfinite(got16.float()).all()
    e16 = (got16.float() - ref).abs().max().item()
    eb = (gotb.float() - ref).abs().max().item()
    print(f"{what}: fp16 err {e16:.6f}  bf16 err {eb:.6f}")
    assert e16 < tol, f"{what}: fp16 max err {e16}"
    assert e16 <= eb, f"{what}: fp16 err {e16} above the bf16 kernel's {eb}"


@requires_gpu
@pytest.mark.parametrize("rows,c", [(33, 1280), (17, 2048)])
def test_fp16_layer_norm(rows, c):
    torch.manual_seed(rows)
    xb, x16 = _both(rows, c, scale=2.0)
    wb, w16 = _both(c)
    bb, b16 = _both(c)
    ext = ops.hip_ext()
    ref = eager.layer_norm(xb.float(), wb.float(), bb.float(), 1e-5)
    _errs(f"layer_norm {rows}x{c}", ext.layer_norm(x16, w16, b16, 1e-5),
          ext.layer_norm(xb, wb, bb, 1e-5), ref, LN_TOL)
    # fp32 master parameters are cast to x's dtype, as the bf16 entry always did
    assert torch.equal(ext.layer_norm(x16, w16.float(), b16.float(), 1e-5),
                       ext.layer_norm(x16, w16, b16, 1e-5))


@requires_gpu
@pytest.mark.parametrize("rows,c", [(33, 1280), (17, 2048)])
def test_fp16_add_layer_norm(rows, c):
    torch.manual_seed(rows + 1)
    xb, x16 = _both(rows, c, scale=2.0)
    rb, r16 = _both(rows, c)
    wb, w16 = _both(c)
    bb, b16 = _both(c)
    ext = ops.hip_ext()
    ref_sum, ref = eager.add_layer_norm(xb.float(), rb.float(), wb.float(), bb.float(), 1e-5)
    s16, y16 = ext.add_layer_norm(x16, r16, w16, b16, 1e-5)
    sb, yb = ext.add_layer_norm(xb, rb, wb, bb, 1e-5)
    _errs(f"add_layer_norm sum {rows}x{c}", s16, sb, ref_sum, LN_TOL)
    # y normalises the fp32 sum in both kernels, not the rounded one
    _errs(f"add_layer_norm y {rows}x{c}", y16, yb, ref, LN_TOL)


@requires_gpu
@pytest.mark.parametrize("b,l", [(1, 256), (2, 1000)])
def test_fp16_vae_attention(b, l):
    torch.manual_seed(l)
    qb, q16 = _both(b, l, 512)
    kb, k16 = _both(b, l, 512)
    vb, v16 = _both(b, l, 512)
    ext = ops.hip_ext()
    ref = eager.vae_attention(qb.float(), kb.float(), vb.float())
    _errs(f"vae_attention B={b} L={l}", ext.vae_attention(q16, k16, v16),
          ext.vae_attention(qb, kb, vb), ref, VAE_TOL)


@requires_gpu
def test_vae_attention_module_takes_the_kernel_in_fp16(monkeypatch):
    from distrifuser_amd.models.vae import VAEAttention

    ext = ops.hip_ext()
    calls = []
    real = ext.vae_attention
    monkeypatch.setattr(ext, "vae_attention", lambda *a: (calls.append(a[0].dtype), real(*a))[1])
    torch.manual_seed(7)
    attn = VAEAttention(512, 32).to(device=DEV, dtype=torch.float16).eval()
    x = torch.randn(1, 512, 8, 12, device=DEV, dtype=torch.float16)
    with torch.no_grad():
        out = attn(x)
    assert calls == [torch.float16]
    assert out.dtype == torch.float16 and torch.isfinite(out.float()).all()


@requires_gpu
def test_norm_and_vae_entries_reject_mixed_dtypes():
    xb, x16 = _both(8, 64)
    wb, w16 = _both(64)
    ext = ops.hip_ext()
    with pytest.raises(RuntimeError, match="weight must have x's dtype"):
        ext.layer_norm(x16, wb, w16, 1e-5)
    with pytest.raises(RuntimeError, match="bias must have x's dtype"):
        ext.layer_norm(xb, wb, w16, 1e-5)
    with pytest.raises(RuntimeError, match="res must have x's dtype"):
        ext.add_layer_norm(x16, xb, w16, w16, 1e-5)
    with pytest.raises(RuntimeError, match="weight must have x's dtype"):
        ext.add_layer_norm(x16, x16, wb, w16, 1e-5)
    qb, q16 = _both(1, 40, 512)
    with pytest.raises(RuntimeError, match="k must have q's dtype"):
        ext.vae_attention(q16, qb, q16)
    with pytest.raises(RuntimeError, match="v must have q's dtype"):
        ext.vae_attention(qb, qb, q16)
