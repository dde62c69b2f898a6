"""fp16 instantiation of the implicit-GEMM 3x3 conv on the GPU.

Inputs are built as bf16 and cast to fp16, so both kernels see the same
numbers; the reference is ops.eager on fp32 copies; the bound is the project's
0.02 * max(scale, 1), and the fp16 error may not exceed the bf16 kernel's.
The kernel is called through ops.hip_ext().conv3x3 directly.

Run on an MI355X box: pytest tests/test_fp16_conv_gpu.py -m gpu -q -s"""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

if torch.cuda.is_available():
    from distrifuser_amd import ops
    from distrifuser_amd.ops import conv as conv_ops
    from distrifuser_amd.ops import eager
else:  # collected on CPU boxes but never run
    ops = conv_ops = eager = None

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

DEV = "cuda:0"


def _both(t):
    """(bf16, fp16) copies of t holding the same values."""
    xb = t.to(torch.bfloat16)
    x16 = xb.to(torch.float16)
    bad = x16.float() != xb.float()
    xb[bad] = 0
    x16[bad] = 0
    assert torch.equal(x16.float(), xb.float())
    return xb, x16


def _f(t):
    return None if t is None else t.float()


def _row3(t):
    return None if t is None else t.reshape(t.shape[0], t.shape[1], -1)


def _kernel(x, weight, bias, stride, top=None, bot=None, residual=None, bias2=None):
    packed = conv_ops.pack_conv3x3_weight(
        weight, torch.float16 if x.dtype == torch.float16 else None)
    assert packed.dtype == x.dtype
    return ops.hip_ext().conv3x3(x, packed, bias, weight.shape[0], stride, _row3(top), _row3(bot),
                                 residual, bias2)


def _check(what, args16, argsb, ref):
    """args: (x, weight, bias, stride, top, bot, residual, bias2)"""
    got16 = _kernel(*args16)
    gotb = _kernel(*argsb)
    assert got16.dtype == torch.float16 and got16.shape == ref.shape
    assert torch.isfinite(got16.float()).all()
    e16 = (got16.float() - ref).abs().max().item()
    eb = (gotb.float() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"{what}: fp16 err {e16:.6f}  bf16 err {eb:.6f}  scale {scale:.3f}")
    assert e16 <= 0.02 * max(scale, 1.0), f"{what}: fp16 max err {e16} vs scale {scale}"
    assert e16 <= eb, f"{what}: fp16 err {e16} above the bf16 kernel's {eb}"
    return got16


@requires_gpu
@pytest.mark.parametrize(
    "cin,cout,h,w,stride,halos",
    [
        (320, 320, 30, 120, 1, True),
        (320, 640, 16, 60, 1, False),
        (64, 64, 129, 130, 1, True),
        (4, 320, 32, 96, 1, False),
        (48, 40, 20, 50, 1, True),
        (320, 4, 12, 40, 1, False),
        (320, 640, 32, 120, 2, True),
        (128, 128, 64, 250, 2, False),
    ],
)
def test_fp16_conv3x3_vs_fp32(cin, cout, h, w, stride, halos):
    """The eight shapes of tests/test_ops_gpu.py::test_conv3x3_vs_fp32."""
    torch.manual_seed(0)
    xb, x16 = _both(torch.randn(2, cin, h, w, device=DEV) * 0.5)
    wb, w16 = _both(torch.randn(cout, cin, 3, 3, device=DEV) * (cin * 9) ** -0.5)
    bb, b16 = _both(torch.randn(cout, device=DEV))
    tb = t16 = botb = bot16 = None
    if halos:
        tb, t16 = _both(torch.randn(2, cin, 1, w, device=DEV) * 0.5)
        if stride == 1:
            botb, bot16 = _both(torch.randn(2, cin, 1, w, device=DEV) * 0.5)
    ref = eager.conv3x3_halo(xb.float(), wb.float(), bb.float(), stride, _f(tb), _f(botb))
    _check(f"{cin}->{cout} {h}x{w} s{stride}", (x16, w16, b16, stride, t16, bot16, None, None),
           (xb, wb, bb, stride, tb, botb, None, None), ref)


@requires_gpu
@pytest.mark.parametrize(
    "cin,cout,h,w,stride",
    [
        (48, 40, 20, 50, 1),   # halos on both sides
        (56, 64, 17, 70, 2),   # stride 2, top halo, odd sizes, two x blocks
    ],
)
def test_fp16_conv3x3_small_integers_are_exact(cin, cout, h, w, stride):
    """|x| <= 4, weights in {-1, 0, 1}, bias in [-4, 4]: every result is an
    integer of magnitude <= 4 * 9 * cin + 4 < 2048, exact in fp32 and in fp16."""
    torch.manual_seed(cin)
    assert 4 * 9 * cin + 4 < 2048
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, device=DEV).float()  # noqa: E731
    xb, x16 = _both(ri(-4, 4, 2, cin, h, w))
    wb, w16 = _both(ri(-1, 1, cout, cin, 3, 3))
    bb, b16 = _both(ri(-4, 4, cout))
    tb, t16 = _both(ri(-4, 4, 2, cin, 1, w))
    botb = bot16 = None
    if stride == 1:
        botb, bot16 = _both(ri(-4, 4, 2, cin, 1, w))
    ref = eager.conv3x3_halo(xb.float(), wb.float(), bb.float(), stride, _f(tb), _f(botb))
    assert torch.equal(ref, ref.round()) and ref.abs().max().item() < 2048
    got16 = _kernel(x16, w16, b16, stride, t16, bot16)
    assert torch.equal(got16.float(), ref), "fp16 conv of small integers is not exact"
    gotb = _kernel(xb, wb, bb, stride, tb, botb)
    small = ref.abs() <= 256  # integers bf16 holds exactly too
    assert small.any()
    assert torch.equal(got16.float()[small], gotb.float()[small])


@requires_gpu
def test_fp16_conv3x3_channel_slice_view():
    torch.manual_seed(1)
    fullb, full16 = _both(torch.randn(2, 128, 24, 48, device=DEV))
    wb, w16 = _both(torch.randn(96, 64, 3, 3, device=DEV) * 0.04)
    xb, x16 = fullb[:, 32:96], full16[:, 32:96]
    assert not x16.is_contiguous() and x16.stride(2) == x16.shape[3]
    ref = eager.conv3x3_halo(xb.float(), wb.float(), None, 1)
    _check("channel slice", (x16, w16, None, 1, None, None, None, None),
           (xb, wb, None, 1, None, None, None, None), ref)


@requires_gpu
def test_fp16_conv3x3_row_band_with_halo_pointers():
    """x is a row band of a larger tensor and the halos are its neighbour
    rows, read in place; the band ends the allocation's last channel early."""
    torch.manual_seed(2)
    fullb, full16 = _both(torch.randn(2, 64, 24, 56, device=DEV) * 0.5)
    wb, w16 = _both(torch.randn(64, 64, 3, 3, device=DEV) * 0.04)
    bb, b16 = _both(torch.randn(64, device=DEV))

    def band(t):
        return t[:, :, 8:16], t[:, :, 7:8], t[:, :, 16:17]

    (xb, tb, botb), (x16, t16, bot16) = band(fullb), band(full16)
    ref = eager.conv3x3_halo(xb.float(), wb.float(), bb.float(), 1, tb.float(), botb.float())
    whole = eager.conv3x3_halo(fullb.float(), wb.float(), bb.float(), 1)[:, :, 8:16]
    assert torch.allclose(ref, whole, atol=1e-5)  # the band really is the middle of the image
    _check("row band", (x16, w16, b16, 1, t16, bot16, None, None),
           (xb, wb, bb, 1, tb, botb, None, None), ref)


@requires_gpu
@pytest.mark.parametrize("stride", [1, 2])
def test_fp16_conv3x3_bias2_and_residual(stride, monkeypatch):
    torch.manual_seed(3 + stride)
    cin, cout, h, w = 64, 96, 18, 40
    xb, x16 = _both(torch.randn(2, cin, h, w, device=DEV) * 0.5)
    wb, w16 = _both(torch.randn(cout, cin, 3, 3, device=DEV) * 0.04)
    bb, b16 = _both(torch.randn(cout, device=DEV))
    b2b, b216 = _both(torch.randn(2, cout, device=DEV))
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    rb, r16 = _both(torch.randn(2, cout, ho, wo, device=DEV))
    ref = eager.conv3x3_halo(xb.float(), wb.float(), bb.float(), stride)
    ref = ref + b2b.float()[:, :, None, None] + rb.float()
    got16 = _check(f"bias2+residual s{stride}", (x16, w16, b16, stride, None, None, r16, b216),
                   (xb, wb, bb, stride, None, None, rb, b2b), ref)
    # the module-level route with the in-epilogue residual switched on
    monkeypatch.setenv("DFA_CONV_RESID", "1")
    packed = conv_ops.pack_conv3x3_weight(w16, torch.float16)
    via = conv_ops.conv3x3_halo(x16, w16, b16, stride, packed=packed, residual=r16, bias2=b216)
    assert torch.equal(via, got16)


@requires_gpu
def test_fp16_conv3x3_overflow_is_inf_not_saturated():
    """A result beyond 65504 becomes inf, as torch's fp16 cast does."""
    x = torch.full((1, 16, 8, 32), 64.0, device=DEV, dtype=torch.float16)
    weight = torch.full((32, 16, 3, 3), 8.0, device=DEV, dtype=torch.float16)
    got = _kernel(x, weight, None, 1)
    ref = eager.conv3x3_halo(x.float(), weight.float(), None, 1)
    assert ref.max().item() == 64.0 * 8.0 * 9 * 16 > 65504
    assert torch.equal(got, ref.half())
    assert torch.isinf(got).any() and torch.isfinite(got).any()


@requires_gpu
def test_native_conv2d_runs_the_kernel_in_fp16(monkeypatch):
    ext = ops.hip_ext()
    calls = []
    real = ext.conv3x3
    monkeypatch.setattr(ext, "conv3x3", lambda *a: (calls.append(a[0].dtype), real(*a))[1])
    torch.manual_seed(5)
    conv = conv_ops.NativeConv2d(32, 32, 3, padding=1).to(device=DEV, dtype=torch.float16)
    x = torch.randn(1, 32, 16, 40, device=DEV, dtype=torch.float16)
    out = conv(x)
    assert calls == [torch.float16] and out.dtype == torch.float16
    ref = eager.conv3x3_halo(x.float(), conv.weight.float(), conv.bias.float(), 1)
    assert (out.float() - ref).abs().max().item() <= 0.02 * max(ref.abs().max().item(), 1.0)


@requires_gpu
def test_conv3x3_rejects_mixed_dtypes():
    xb, x16 = _both(torch.randn(1, 16, 8, 32, device=DEV))
    wb, w16 = _both(torch.randn(32, 16, 3, 3, device=DEV))
    bb, b16 = _both(torch.randn(32, device=DEV))
    tb, t16 = _both(torch.randn(1, 16, 32, device=DEV))
    rb, r16 = _both(torch.randn(1, 32, 8, 32, device=DEV))
    b2b, b216 = _both(torch.randn(1, 32, device=DEV))
    ext = ops.hip_ext()
    p16 = conv_ops.pack_conv3x3_weight(w16, torch.float16)
    pb = conv_ops.pack_conv3x3_weight(wb)
    for args, name in (
        ((x16, pb, b16, 32, 1, None, None, None, None), "wp"),
        ((xb, p16, bb, 32, 1, None, None, None, None), "wp"),
        ((x16, p16, bb, 32, 1, None, None, None, None), "bias"),
        ((x16, p16, b16, 32, 1, tb, None, None, None), "halo"),
        ((x16, p16, b16, 32, 1, None, tb, None, None), "halo"),
        ((x16, p16, b16, 32, 1, None, None, rb, None), "residual"),
        ((x16, p16, b16, 32, 1, None, None, None, b2b), "bias2"),
    ):
        with pytest.raises(RuntimeError, match=f"{name} must have x's dtype"):
            ext.conv3x3(*args)
    ext.conv3x3(x16, p16, b16, 32, 1, t16, t16, r16, b216)  # all fp16: fine
