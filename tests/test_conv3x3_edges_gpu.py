"""conv3x3 kernel (csrc/conv.hip) at its tile edges, checked for EXACT
equality. With integer-valued bf16 data every product and every fp32 partial
sum of the conv is an exact integer, so the kernel's output must be
bit-identical to a float64 reference whatever the accumulation order; an
impulse input makes every output a single weight (or zero) and pins the tap,
channel and position maps independently. The shapes walk the three launch
configurations of launch_conv3x3 (wide 64-px tiles, small 32-px tiles,
stride 2) through vectorised and scalar staging, partial x/y/cin/cout tiles,
missing halos and strided views.

The GPU tests call the extension entry point directly: ops.conv.conv3x3_halo
falls back to eager when a layout check fails, which would compare eager
with eager. The unmarked tests check, on the CPU and from the reference
alone, that the data is what the exactness argument needs.

Run on an MI355X box: pytest tests/test_conv3x3_edges_gpu.py -m gpu -q"""

import functools

import pytest
import torch

from distrifuser_amd.ops import eager
from distrifuser_amd.ops.conv import pack_conv3x3_weight

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")


def gpu_test(fn):
    return pytest.mark.gpu(pytest.mark.timeout(300)(requires_gpu(fn)))


BF16 = torch.bfloat16

# (B, Cin, Cout, H, W, stride, halos)
SHAPES = [
    # ---- stride 1, wide config (YB=8, NCT=4, PW=2, 64-px tiles), vectorised staging
    # three x-blocks, the last 8 px wide; two y-blocks, the last with 1 row; a
    # cin tail inside a 16-cin tile; CT=2 < NCT=4 takes the zero-fill branch
    # of stage_weights; npix=12 takes the early exit of the grid decode
    pytest.param(2, 24, 40, 9, 136, 1, "both", id="s1-wide-vec-tails"),
    # Cin crosses the 64-channel pack boundary, so the staged cin tiles are
    # all zero beyond channel 80; CT=5 gives ncb=2 with a partial last
    # cout-block; W is an exact multiple of 64
    pytest.param(1, 80, 160, 8, 192, 1, "none", id="s1-wide-vec-2coutblocks"),
    # H < YB, with a missing bot at a border
    pytest.param(1, 16, 32, 3, 200, 1, "top", id="s1-wide-vec-shortH"),
    # wide config, scalar path, odd row alignment
    pytest.param(1, 8, 32, 5, 131, 1, "both", id="s1-wide-scalar-oddW"),
    # ---- stride 1, small config (YB=8, NCT=2, PW=1, 32-px tiles)
    # H=1, so every output row reads top, interior and bot; one 8-px window
    pytest.param(2, 16, 32, 1, 8, 1, "both", id="s1-small-H1-W8"),
    # either side of the Wo <= 128 switch
    pytest.param(1, 8, 32, 2, 128, 1, "both", id="s1-small-W128"),
    pytest.param(1, 8, 32, 2, 136, 1, "both", id="s1-wide-W136"),
    # odd CT=3 with NCT=2
    pytest.param(1, 40, 96, 17, 40, 1, "bot", id="s1-small-oddCT"),
    # W < 8
    pytest.param(1, 8, 32, 4, 5, 1, "none", id="s1-small-W5"),
    # ---- stride 2 (YB=4, XW=2, NCT=2, PW=1)
    # odd H, so the last output row reads bot; Wo=68 gives two x-blocks on
    # the vectorised path, with xb0 * S != 0; Ho=5 gives two y-blocks
    pytest.param(2, 32, 64, 9, 136, 2, "both", id="s2-vec-oddH-2xblocks"),
    # Wo=132, three x-blocks, both x-waves, even H
    pytest.param(1, 24, 40, 8, 264, 2, "top", id="s2-vec-3xblocks"),
    # odd H and W, scalar path
    pytest.param(1, 16, 32, 7, 13, 2, "both", id="s2-scalar-odd"),
    # H=1
    pytest.param(1, 16, 32, 1, 8, 2, "both", id="s2-H1-W8"),
]

EPILOGUE_SHAPES = [
    pytest.param(2, 24, 40, 9, 136, 1, "both", id="s1-wide"),
    pytest.param(2, 32, 64, 9, 136, 2, "both", id="s2"),
]
EPILOGUES = ["bias", "bias+bias2", "bias+bias2+residual"]


def _randint(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(BF16)


def _sparse_weight(gen, cout, cin):
    """Exactly 3 non-zero input channels per (cout, tap), each +-1."""
    chans = torch.rand(cout, 9, cin, generator=gen).argsort(dim=-1)[..., :3]
    signs = torch.randint(0, 2, (cout, 9, 3), generator=gen) * 2 - 1
    w = torch.zeros(cout, 9, cin)
    w.scatter_(2, chans, signs.float())
    return w.permute(0, 2, 1).reshape(cout, cin, 3, 3).contiguous().to(BF16)


def _reference(c):
    """eager.conv3x3_halo on float64 copies (+ bias2 + residual), uncast."""
    f64 = lambda t: None if t is None else t.double()
    ref = eager.conv3x3_halo(f64(c["x"]), f64(c["weight"]), f64(c["bias"]), c["stride"],
                             f64(c["top"]), f64(c["bot"]))
    if c["bias2"] is not None:
        ref = ref + c["bias2"].double()[:, :, None, None]
    if c["residual"] is not None:
        ref = ref + c["residual"].double()
    return ref


@functools.lru_cache(maxsize=None)
def _exact_case(b, cin, cout, h, w, stride, halos, epilogue="none"):
    """Integer-valued bf16 inputs and their exact reference, on the CPU.
    Cached and shared between the CPU and GPU tests: never modified."""
    gen = torch.Generator().manual_seed(
        sum(p * v for p, v in zip((1, 3, 5, 7, 11, 13), (b, cin, cout, h, w, stride)))
        + len(halos) + 17 * len(epilogue))
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    c = {"stride": stride, "cout": cout}
    c["x"] = _randint(gen, -2, 2, b, cin, h, w)
    c["top"] = _randint(gen, -2, 2, b, cin, 1, w) if halos in ("both", "top") else None
    c["bot"] = _randint(gen, -2, 2, b, cin, 1, w) if halos in ("both", "bot") else None
    c["weight"] = _sparse_weight(gen, cout, cin)
    c["bias"] = _randint(gen, -8, 8, cout) if "bias" in epilogue else None
    c["bias2"] = _randint(gen, -8, 8, b, cout) if "bias2" in epilogue else None
    c["residual"] = _randint(gen, -16, 16, b, cout, ho, wo) if "residual" in epilogue else None

    ref = _reference(c)
    # preconditions of the exactness argument, from the reference alone
    for name in ("x", "top", "bot", "weight", "bias", "bias2", "residual"):
        t = c[name]
        assert t is None or torch.equal(t.double(), t.double().round()), f"{name} not integral"
    nz = (c["weight"] != 0).sum(dim=1)
    assert torch.equal(nz, torch.full_like(nz, 3)), "weights: 3 non-zero cins per (cout, tap)"
    assert c["weight"].abs().max() == 1
    assert ref.shape == (b, cout, ho, wo)
    assert torch.equal(ref, ref.round()), "reference not integral"
    assert ref.abs().max() <= 256, "reference leaves bf16's exact-integer range"
    assert (ref != 0).double().mean() >= 0.5, "reference mostly zero: vacuous"
    c["ref"] = ref.to(BF16)
    assert torch.equal(c["ref"].double(), ref)
    return c


def _ext_conv(x, weight, bias, stride, top=None, bot=None, residual=None, bias2=None):
    """The extension entry point, with the halos flattened to [B, Cin, W] as
    ops.conv.conv3x3_halo does."""
    from distrifuser_amd.ops.dispatch import hip_ext

    dev = torch.device("cuda:0")
    packed = pack_conv3x3_weight(weight).to(dev)
    flat = lambda t: None if t is None else t.reshape(t.shape[0], t.shape[1], -1)
    assert top is None or flat(top).data_ptr() == top.data_ptr()  # stayed a view
    assert bot is None or flat(bot).data_ptr() == bot.data_ptr()
    out = hip_ext().conv3x3(x, packed, bias, weight.shape[0], stride, flat(top), flat(bot),
                            residual, bias2)
    torch.cuda.synchronize()
    return out.cpu()


def _gpu(t):
    return None if t is None else t.to("cuda:0")


def _run_case(c):
    return _ext_conv(_gpu(c["x"]), c["weight"], _gpu(c["bias"]), c["stride"], _gpu(c["top"]),
                     _gpu(c["bot"]), _gpu(c["residual"]), _gpu(c["bias2"]))


def _assert_equal(got, ref, what):
    assert got.shape == ref.shape, what
    bad = (got != ref).nonzero()
    assert bad.numel() == 0, (
        f"{what}: {bad.shape[0]} of {ref.numel()} outputs differ; first (b, cout, y, x) = "
        f"{bad[0].tolist()}: got {got[tuple(bad[0])].item()}, want {ref[tuple(bad[0])].item()}; "
        f"wrong couts {bad[:, 1].unique().tolist()[:8]}, rows {bad[:, 2].unique().tolist()[:8]}, "
        f"cols {bad[:, 3].unique().tolist()[:8]}")
    assert torch.equal(got, ref), what


# ---- CPU: the data is what the exactness argument needs -------------------------


@pytest.mark.parametrize("b,cin,cout,h,w,stride,halos", SHAPES)
def test_exact_data_preconditions(b, cin, cout, h, w, stride, halos):
    c = _exact_case(b, cin, cout, h, w, stride, halos)
    assert c["ref"].dtype == BF16 and c["ref"].abs().max() <= 54


@pytest.mark.parametrize("epilogue", EPILOGUES)
@pytest.mark.parametrize("b,cin,cout,h,w,stride,halos", EPILOGUE_SHAPES)
def test_exact_epilogue_data_preconditions(b, cin, cout, h, w, stride, halos, epilogue):
    c = _exact_case(b, cin, cout, h, w, stride, halos, epilogue)
    assert c["ref"].abs().max() <= 54 + 8 + 8 + 16


def test_view_data_preconditions():
    _exact_case(2, 24, 40, 6, 136, 1, "both")
    for stride in (1, 2):
        _exact_case(*_HALO_VIEW_SHAPES[stride])
    _row_band_case()


# ---- GPU: exact equality ---------------------------------------------------------


@gpu_test
@pytest.mark.parametrize("b,cin,cout,h,w,stride,halos", SHAPES)
def test_conv3x3_exact(b, cin, cout, h, w, stride, halos):
    c = _exact_case(b, cin, cout, h, w, stride, halos)
    _assert_equal(_run_case(c), c["ref"], f"{(b, cin, cout, h, w, stride, halos)}")


@gpu_test
@pytest.mark.parametrize("epilogue", EPILOGUES)
@pytest.mark.parametrize("b,cin,cout,h,w,stride,halos", EPILOGUE_SHAPES)
def test_conv3x3_exact_epilogue(b, cin, cout, h, w, stride, halos, epilogue):
    c = _exact_case(b, cin, cout, h, w, stride, halos, epilogue)
    _assert_equal(_run_case(c), c["ref"], f"stride {stride} {epilogue}")


# ---- views -------------------------------------------------------------------------

POISON = 64.0  # any read of it moves an output by >= 64: off the reference


@gpu_test
def test_conv3x3_exact_batch_and_channel_slice():
    """x = full[:, 8:32] of a [2, 40, 6, 136] tensor: x_sb != Cin * x_sc."""
    c = _exact_case(2, 24, 40, 6, 136, 1, "both")
    full = torch.full((2, 40, 6, 136), POISON, dtype=BF16, device="cuda:0")
    full[:, 8:32] = _gpu(c["x"])
    x = full[:, 8:32]
    assert x.stride(0) != x.shape[1] * x.stride(1) and not x.is_contiguous()
    got = _ext_conv(x, c["weight"], None, 1, _gpu(c["top"]), _gpu(c["bot"]))
    _assert_equal(got, c["ref"], "channel-slice view")


_HALO_VIEW_SHAPES = {1: (2, 24, 40, 9, 136, 1, "both"), 2: (2, 32, 64, 9, 136, 2, "both")}


@gpu_test
@pytest.mark.parametrize("stride", [1, 2])
def test_conv3x3_exact_halo_buffer_views(stride):
    """Halos are views into padded buffers, like comm-buffer slots: their
    batch and channel strides differ from x's and from each other, and the
    rest of the buffers holds POISON, so a read beyond W, in the wrong slot or
    in the wrong channel row breaks equality."""
    c = _exact_case(*_HALO_VIEW_SHAPES[stride])
    b, cin, _, w = c["top"].shape
    buf_t = torch.full((b, 3, cin + 2, w + 24), POISON, dtype=BF16, device="cuda:0")
    buf_b = torch.full((b, 2, cin, w + 40), POISON, dtype=BF16, device="cuda:0")
    top = buf_t[:, 1, 1 : cin + 1, 8 : 8 + w]
    bot = buf_b[:, 1, :, 16 : 16 + w]
    top.copy_(c["top"][:, :, 0])
    bot.copy_(c["bot"][:, :, 0])
    x = _gpu(c["x"])
    strides = {(t.stride(0), t.stride(1)) for t in (x, top, bot)}
    assert len(strides) == 3 and top.stride(-1) == 1 and bot.stride(-1) == 1
    got = _ext_conv(x, c["weight"], None, stride, top, bot)
    _assert_equal(got, c["ref"], f"halo views, stride {stride}")


_BANDS = ((0, 7), (7, 16), (16, 24))


@functools.lru_cache(maxsize=None)
def _row_band_case():
    """A [1, 8, 24, 136] image, with no halos: the image's own rows are the
    bands' halos."""
    return _exact_case(1, 8, 32, 24, 136, 1, "none")


@gpu_test
def test_conv3x3_exact_row_band_views():
    """Interior and both halos are adjacent-row views of one tensor (the
    sliced conv_in path) in the wide config; each band must equal the matching
    rows of the full conv."""
    c = _row_band_case()
    full = _gpu(c["x"])
    for h0, h1 in _BANDS:
        band = full[:, :, h0:h1]
        top = full[:, :, h0 - 1 : h0] if h0 > 0 else None
        bot = full[:, :, h1 : h1 + 1] if h1 < full.shape[2] else None
        got = _ext_conv(band, c["weight"], None, 1, top, bot)
        _assert_equal(got, c["ref"][:, :, h0:h1], f"rows {h0}:{h1}")


# ---- impulses --------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _impulse_case(stride):
    """Single 1.0 entries at (y, x) in {0, 7, 8, H-1} x {0, 31, 32, 63, 64, W-1}
    and in each halo row at x in {0, W-1}, every one in a channel of its own.
    Neighbouring positions (7/8, 31/32, 63/64) go to different batch images, so
    that no output sees two impulses: each output is one weight or zero."""
    b, cin, cout, h, w = 4, 28, 40, 12, 136
    ys, xs = (0, 7, 8, h - 1), (0, 31, 32, 63, 64, w - 1)
    x = torch.zeros(b, cin, h, w)
    top = torch.zeros(b, cin, 1, w)
    bot = torch.zeros(b, cin, 1, w)
    ch = 0
    for y in ys:
        for xx in xs:
            x[2 * (y == 8) + (xx in (32, 64)), ch, y, xx] = 1.0
            ch += 1
    for xx in (0, w - 1):
        top[1, ch, 0, xx] = 1.0      # image 1 has its y=0 impulses at x = 32, 64
        bot[3, ch + 1, 0, xx] = 1.0  # image 3 has only y=8 impulses
        ch += 2
    assert ch == cin
    gen = torch.Generator().manual_seed(29)
    weight = torch.randn(cout, cin, 3, 3, generator=gen).to(BF16)

    ones = torch.ones(1, cin, 3, 3, dtype=torch.float64)
    hits = eager.conv3x3_halo(x.double(), ones, None, stride, top.double(), bot.double())
    assert hits.max() == 1, "two impulses meet in one output"
    ref = eager.conv3x3_halo(x.double(), weight.double(), None, stride, top.double(),
                             bot.double())
    assert (ref != 0).sum() == (hits != 0).sum() * cout
    # every output is a weight: the cast to bf16 is exact
    assert torch.equal(ref.to(BF16).double(), ref)
    return {"x": x.to(BF16), "top": top.to(BF16), "bot": bot.to(BF16), "weight": weight,
            "stride": stride, "ref": ref.to(BF16), "bias": None, "bias2": None,
            "residual": None}


@pytest.mark.parametrize("stride", [1, 2])
def test_impulse_data_preconditions(stride):
    c = _impulse_case(stride)
    # stride 1: the 24 interior impulses reach >= 4 outputs each (a corner's
    # 2x2), the 4 halo ones 2 each
    if stride == 1:
        assert (c["ref"] != 0).any(dim=1).sum() >= 24 * 4 + 4 * 2


@gpu_test
@pytest.mark.parametrize("stride", [1, 2])
def test_conv3x3_impulse_response(stride):
    c = _impulse_case(stride)
    _assert_equal(_run_case(c), c["ref"], f"impulses, stride {stride}")


# ---- dispatch --------------------------------------------------------------------


@gpu_test
def test_native_conv2d_rides_the_kernel_wide_config():
    """The public path at a wide-config shape returns exactly what the direct
    extension call returns (an eager fallback would round differently)."""
    from distrifuser_amd.ops import NativeConv2d

    torch.manual_seed(3)
    dev = "cuda:0"
    m = NativeConv2d(24, 40, 3, padding=1).to(dev, BF16)
    x = torch.randn(2, 24, 9, 136, device=dev, dtype=BF16)
    top = torch.randn(2, 24, 1, 136, device=dev, dtype=BF16)
    bot = torch.randn(2, 24, 1, 136, device=dev, dtype=BF16)
    with torch.no_grad():
        got = m(x, top=top, bot=bot).cpu()
        direct = _ext_conv(x, m.weight.detach().cpu(), m.bias.detach(), 1, top, bot)
        f32 = lambda t: t.detach().float().cpu()
        ref = eager.conv3x3_halo(f32(x), f32(m.weight), f32(m.bias), 1, f32(top), f32(bot))
    assert torch.equal(got, direct)
    err = (got.float() - ref).abs().max().item()
    assert err <= 0.02 * max(ref.abs().max().item(), 1.0)
