"""conv3x3 kernel (csrc/conv.hip) in its bottom/right-only padding mode
(pad_lo=0, stride 2: the AutoencoderKL downsample), checked for EXACT equality
by the method of test_conv3x3_edges_gpu.py. With integer-valued 16-bit data
every product and every fp32 partial sum is an exact integer, so the kernel
must return the float64 reference

    F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)

bit for bit, whatever its accumulation order. The shapes cover both x-waves
and several x- and y-blocks, the right edge at exact multiples of the 128-px
input tile (where the last tap's column x = W is, in memory, the next row's
first element), cin/cout tails, odd sizes on the scalar staging path, the
smallest legal input, a bot halo row, strided views and the epilogue.

The GPU tests call the extension entry point directly, so a silent eager
fallback cannot pass. The unmarked tests prove on the CPU, from the reference
alone, that the data is what the exactness argument needs.

Run on an MI355X box: pytest tests/test_conv3x3_asym_gpu.py -m gpu -q"""

import functools

import pytest
import torch
import torch.nn.functional as F

from distrifuser_amd.ops.conv import pack_conv3x3_weight

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")


def gpu_test(fn):
    return pytest.mark.gpu(pytest.mark.timeout(300)(requires_gpu(fn)))


BF16, FP16 = torch.bfloat16, torch.float16
FIRST = (2, 32, 64, 10, 136)

# (B, Cin, Cout, H, W, bot)
SHAPES = [
    # Wo=68: two x-blocks on the vectorised path; Ho=5: two y-blocks; the last
    # output row reads the zero row H
    pytest.param(*FIRST, False, id="2xblocks-2yblocks"),
    # Wo an exact multiple of 64: the last tap of the last column reads x = W
    pytest.param(1, 16, 32, 4, 128, False, id="W128-right-edge"),
    pytest.param(1, 16, 32, 4, 256, False, id="W256-right-edge"),
    # three x-blocks, cin and cout tails
    pytest.param(1, 24, 40, 8, 264, False, id="3xblocks-tails"),
    # odd H and W, scalar staging, Ho=4, Wo=6: neither pad is ever read
    pytest.param(1, 16, 32, 9, 13, False, id="odd-scalar"),
    # one output row that reads the zero row; the smallest legal input
    pytest.param(1, 16, 32, 2, 8, False, id="H2-W8"),
    pytest.param(1, 8, 32, 2, 2, False, id="H2-W2"),
    # row H read in place from a separate tensor
    pytest.param(*FIRST, True, id="bot-halo"),
]
FP16_SHAPES = [
    pytest.param(*FIRST, False, id="2xblocks-2yblocks"),
    pytest.param(1, 16, 32, 4, 128, False, id="W128-right-edge"),
    pytest.param(*FIRST, True, id="bot-halo"),
]


def _randint_nonzero(gen, *shape):
    """Integers in {-2, -1, 1, 2}: no element is zero, so data wrapped in from
    the next row, channel or batch image always moves an output."""
    mag = torch.randint(1, 3, shape, generator=gen)
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (mag * sign).float()


def _sparse_weight(gen, cout, cin):
    """Exactly 3 non-zero input channels per (cout, tap), each +-1."""
    chans = torch.rand(cout, 9, cin, generator=gen).argsort(dim=-1)[..., :3]
    signs = torch.randint(0, 2, (cout, 9, 3), generator=gen) * 2 - 1
    w = torch.zeros(cout, 9, cin)
    w.scatter_(2, chans, signs.float())
    return w.permute(0, 2, 1).reshape(cout, cin, 3, 3).contiguous()


def _out_size(h, w):
    return (h - 2) // 2 + 1, (w - 2) // 2 + 1


def _reference(x, weight, bot=None, bias=None, bias2=None, residual=None):
    """float64 F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2); a bot row takes
    the place of the zero row H. Uncast."""
    ho, _ = _out_size(x.shape[2], x.shape[3])
    full = x.double()
    if bot is None:
        full = F.pad(full, (0, 1, 0, 1))
    else:
        full = F.pad(torch.cat([full, bot.double()], dim=2), (0, 1, 0, 0))
    ref = F.conv2d(full, weight.double(), None if bias is None else bias.double(), stride=2)
    ref = ref[:, :, :ho]
    if bias2 is not None:
        ref = ref + bias2.double()[:, :, None, None]
    if residual is not None:
        ref = ref + residual.double()
    return ref


@functools.lru_cache(maxsize=None)
def _exact_case(b, cin, cout, h, w, bot, epilogue=False):
    """Integer-valued fp32 inputs (exact in bf16 and fp16 alike) and their
    exact reference, on the CPU. Cached and shared between the CPU and GPU
    tests: never modified."""
    gen = torch.Generator().manual_seed(
        sum(p * v for p, v in zip((1, 3, 5, 7, 11), (b, cin, cout, h, w))) + 2 * bot + epilogue)
    ho, wo = _out_size(h, w)
    c = {"cout": cout}
    c["x"] = _randint_nonzero(gen, b, cin, h, w)
    c["bot"] = _randint_nonzero(gen, b, cin, 1, w) if bot else None
    c["weight"] = _sparse_weight(gen, cout, cin)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()
    c["bias"] = ri(-8, 8, cout) if epilogue else None
    c["bias2"] = ri(-8, 8, b, cout) if epilogue else None
    c["residual"] = ri(-16, 16, b, cout, ho, wo) if epilogue else None

    ref = _reference(c["x"], c["weight"], c["bot"], c["bias"], c["bias2"], c["residual"])
    # preconditions of the exactness argument, from the reference alone
    for name in ("x", "bot", "weight", "bias", "bias2", "residual"):
        t = c[name]
        assert t is None or torch.equal(t, t.round()), f"{name} not integral"
    assert (c["x"] != 0).all() and c["x"].abs().max() == 2
    nz = (c["weight"] != 0).sum(dim=1)
    assert torch.equal(nz, torch.full_like(nz, 3)), "weights: 3 non-zero cins per (cout, tap)"
    assert c["weight"].abs().max() == 1
    # every partial sum is an integer of magnitude <= 9 taps * 3 cins * 2
    # (+ 8 + 8 + 16 with the epilogue): exact in fp32, and in bf16 up to 256
    bound = 54 + (32 if epilogue else 0)
    assert ref.shape == (b, cout, ho, wo)
    assert torch.equal(ref, ref.round()), "reference not integral"
    assert ref.abs().max() <= bound <= 256
    assert (ref != 0).double().mean() >= 0.5, "reference mostly zero: vacuous"
    for dt in (BF16, FP16):
        assert torch.equal(ref.to(dt).double(), ref), f"reference not representable in {dt}"
    c["ref"] = ref
    return c


def _ext_conv(x, weight, bias=None, stride=2, top=None, bot=None, residual=None, bias2=None,
              pad_lo=0):
    """The extension entry point, with the halos flattened to [B, Cin, W] as
    ops.conv.conv3x3_halo does. weight is a CPU tensor; the rest live on the GPU."""
    from distrifuser_amd.ops.dispatch import hip_ext

    packed = pack_conv3x3_weight(weight, x.dtype).to(x.device)
    flat = lambda t: None if t is None else t.reshape(t.shape[0], t.shape[1], -1)
    assert bot is None or flat(bot).data_ptr() == bot.data_ptr()  # stayed a view
    out = hip_ext().conv3x3(x, packed, bias, weight.shape[0], stride, flat(top), flat(bot),
                            residual, bias2, pad_lo)
    torch.cuda.synchronize()
    return out.cpu()


def _gpu(t, dtype):
    return None if t is None else t.to("cuda:0", dtype)


def _run_case(c, dtype, x=None):
    return _ext_conv(_gpu(c["x"], dtype) if x is None else x, c["weight"],
                     _gpu(c["bias"], dtype), 2, None, _gpu(c["bot"], dtype),
                     _gpu(c["residual"], dtype), _gpu(c["bias2"], dtype))


def _assert_equal(got, ref, what):
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    got = got.double()
    bad = (got != ref).nonzero()
    assert bad.numel() == 0, (
        f"{what}: {bad.shape[0]} of {ref.numel()} outputs differ; first (b, cout, y, x) = "
        f"{bad[0].tolist()}: got {got[tuple(bad[0])].item()}, want {ref[tuple(bad[0])].item()}; "
        f"wrong couts {bad[:, 1].unique().tolist()[:8]}, rows {bad[:, 2].unique().tolist()[:8]}, "
        f"cols {bad[:, 3].unique().tolist()[:8]}")


# ---- CPU: the data is what the exactness argument needs -------------------------


@pytest.mark.parametrize("b,cin,cout,h,w,bot", SHAPES)
def test_exact_data_preconditions(b, cin, cout, h, w, bot):
    c = _exact_case(b, cin, cout, h, w, bot)
    assert c["ref"].shape[2:] == _out_size(h, w)


def test_size_formula_and_pads_read():
    """Odd H and W: Ho = 4, Wo = 6, and no output reads row H or column W
    (2*3+2 = 8 < 9, 2*5+2 = 12 < 13). Even sizes read both."""
    assert _out_size(9, 13) == (4, 6)
    assert _out_size(10, 136) == (5, 68) and 2 * 4 + 2 == 10 and 2 * 67 + 2 == 136
    assert _out_size(2, 2) == (1, 1)


def test_right_edge_data_would_show_a_wrap():
    """At W = 128 and 256 the element after a row's end is the next row's
    first: the reference with that element read as data differs from the true
    one in the last output column, so a kernel that wrapped could not pass."""
    for w in (128, 256):
        c = _exact_case(1, 16, 32, 4, w, False)
        x = c["x"]
        flat = torch.cat([x.reshape(-1), torch.ones(1)])
        wrapped = F.pad(x, (0, 1, 0, 1))
        # column W of row y holds memory element (y * W + W) of each channel
        for ch in range(x.shape[1]):
            for y in range(x.shape[2]):
                wrapped[0, ch, y, w] = flat[(ch * x.shape[2] + y) * w + w]
        bad = F.conv2d(wrapped.double(), c["weight"].double(), stride=2)
        assert (bad[..., -1] != c["ref"][..., -1]).any()
        assert torch.equal(bad[..., :-1], c["ref"][..., :-1])


def test_epilogue_and_view_data_preconditions():
    _exact_case(*FIRST, False, True)
    assert POISON > 54  # one POISON read moves an output off the reference


# ---- GPU: exact equality ---------------------------------------------------------


@gpu_test
@pytest.mark.parametrize("b,cin,cout,h,w,bot", SHAPES)
def test_conv3x3_asym_exact_bf16(b, cin, cout, h, w, bot):
    c = _exact_case(b, cin, cout, h, w, bot)
    _assert_equal(_run_case(c, BF16), c["ref"], f"bf16 {(b, cin, cout, h, w, bot)}")


@gpu_test
@pytest.mark.parametrize("b,cin,cout,h,w,bot", FP16_SHAPES)
def test_conv3x3_asym_exact_fp16(b, cin, cout, h, w, bot):
    c = _exact_case(b, cin, cout, h, w, bot)
    _assert_equal(_run_case(c, FP16), c["ref"], f"fp16 {(b, cin, cout, h, w, bot)}")


@gpu_test
@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
def test_conv3x3_asym_exact_epilogue(dtype):
    c = _exact_case(*FIRST, False, True)
    _assert_equal(_run_case(c, dtype), c["ref"], "bias + bias2 + residual")


# ---- views -------------------------------------------------------------------------

POISON = 64.0  # any read of it moves an output by >= 64: off the reference


@gpu_test
def test_conv3x3_asym_exact_channel_slice():
    """x = full[:, 8:40] of a [2, 48, 10, 136] tensor: x_sb != Cin * x_sc."""
    c = _exact_case(*FIRST, False)
    full = torch.full((2, 48, 10, 136), POISON, dtype=BF16, device="cuda:0")
    full[:, 8:40] = _gpu(c["x"], BF16)
    x = full[:, 8:40]
    assert x.stride(0) != x.shape[1] * x.stride(1) and not x.is_contiguous()
    _assert_equal(_run_case(c, BF16, x), c["ref"], "channel-slice view")


@gpu_test
def test_conv3x3_asym_exact_row_band_ending_allocation():
    """x = the last 10 rows of a [2, 32, 14, 136] tensor. Row H of a channel
    is, in memory, the next channel's first POISON row, and for the last
    channel of the last image it lies past the allocation: the zero row must
    never be loaded."""
    c = _exact_case(*FIRST, False)
    full = torch.full((2, 32, 14, 136), POISON, dtype=BF16, device="cuda:0")
    full[:, :, 4:] = _gpu(c["x"], BF16)
    x = full[:, :, 4:]
    assert x.stride(1) == 14 * 136 and x.stride(2) == 136
    assert x.storage_offset() + (2 * 32 - 1) * 14 * 136 + 10 * 136 == full.numel()
    _assert_equal(_run_case(c, BF16, x), c["ref"], "row-band view")


# ---- impulses --------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _impulse_case():
    """A one-hot at (c=3, 0, 0) and another at (c=5, 2, 3). By the definition
    (output (y, x) reads rows 2y + dy and columns 2x + dx) the first reaches
    output (0, 0) alone, through tap (0, 0); the second reaches (0, 1) through
    tap (2, 1) and (1, 1) through tap (0, 1). The expected output is written
    from that definition, not from a conv."""
    cin, cout, h, w = 8, 32, 6, 8
    x = torch.zeros(1, cin, h, w)
    x[0, 3, 0, 0] = 1.0
    x[0, 5, 2, 3] = 1.0
    gen = torch.Generator().manual_seed(31)
    weight = torch.randn(cout, cin, 3, 3, generator=gen).to(BF16).float()
    ho, wo = _out_size(h, w)
    want = torch.zeros(1, cout, ho, wo, dtype=torch.float64)
    want[0, :, 0, 0] = weight[:, 3, 0, 0]
    want[0, :, 0, 1] = weight[:, 5, 2, 1]
    want[0, :, 1, 1] = weight[:, 5, 0, 1]
    return x, weight, want


def test_impulse_definition_separates_the_modes():
    x, weight, want = _impulse_case()
    assert torch.equal(_reference(x, weight), want)
    # pad-1 stride 2: the same impulse at (0, 0) reaches output (0, 0) through
    # tap (1, 1), so the two modes cannot be mistaken for each other
    pad1 = F.conv2d(x.double(), weight.double(), stride=2, padding=1)
    assert torch.equal(pad1[0, :, 0, 0], weight[:, 3, 1, 1].double())
    assert not torch.equal(pad1[0, :, 0, 0], want[0, :, 0, 0])
    # every output is one bf16 weight or zero: the cast back is exact
    assert torch.equal(want.to(BF16).double(), want)


@gpu_test
def test_conv3x3_asym_impulse_response():
    x, weight, want = _impulse_case()
    got = _ext_conv(x.to("cuda:0", BF16), weight)
    _assert_equal(got, want, "impulses")


# ---- rejections ------------------------------------------------------------------


@gpu_test
def test_conv3x3_asym_rejections():
    c = _exact_case(1, 16, 32, 2, 8, False)
    x = _gpu(c["x"], BF16)
    top = torch.zeros(1, 16, 1, 8, dtype=BF16, device="cuda:0")
    with pytest.raises(RuntimeError, match="stride 2"):
        _ext_conv(x, c["weight"], stride=1)
    with pytest.raises(RuntimeError, match="top"):
        _ext_conv(x, c["weight"], top=top)
    with pytest.raises(RuntimeError, match="H, W >= 2"):
        _ext_conv(x[:, :, :1], c["weight"])
    with pytest.raises(RuntimeError, match="H, W >= 2"):
        _ext_conv(x[:, :, :, :1].contiguous(), c["weight"])
    with pytest.raises(RuntimeError, match="pad_lo"):
        _ext_conv(x, c["weight"], pad_lo=2)
