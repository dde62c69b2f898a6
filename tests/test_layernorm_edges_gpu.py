"""LayerNorm / add_layer_norm (csrc/layernorm.hip, ln_kernel) against float64,
in bf16 and fp16: rows whose result is known to the bit, a NaN arena around
the inputs, and a conditioning ladder that climbs mean/std.

Exact rows. Row r holds m_r +- s_r, C/2 of each sign at positions permuted per
row, m_r = r - 4 a small integer and s_r = 2^(r-4), eps = 0. Every value and
every partial sum of the values, of their squares and of (x - mean)^2 is a
dyadic number of fewer than 24 bits, so in fp32, in any summation order, sum =
C*m_r, mean = m_r, var = s_r^2 (by either variance formula) and, __frsqrt_rn
being correctly rounded, inv = 1/s_r: all exact. (x - mean) * inv = +-1, and
w_c, b_c are dyadic with +-w_c + b_c exact in fp32 (24 bits between 2^8 and
2^-15), so y = +-w_c + b_c meets exactly one rounding, the output's, and must
torch.equal the float64 result cast to the dtype. The (w_c, b_c) are distinct
per channel and (m_r, s_r) per row, so a row or column mix-up changes bits.
add_layer_norm gets x = m_r and res = +-s_r: x + res is the same row, its
written sum is exact, y as before. The fp32 twin below (the kernel's lane
layout, per-lane order and butterfly in torch fp32) reproduces all of this on
the CPU. Allowance before the output rounding: 0, and the twin uses 0 of it.

Widths walk the VPT dispatch (C <= 512 / 1024 / 1536 / 2048): each boundary,
the first width past it (520 / 1032 / 1544: one lane alone holds the last
vector, 63 lanes of that trip are padding), 504 (lane 63 idle), and C = 8, 16.
Row counts walk WPB = 4: a lone row, partial last blocks, full blocks.

One rounding of the sum. The kernel adds x and res in fp32 and rounds to 16
bits. The fp32 add of two 16-bit values is inexact only when their exponents
are more than 24 - p bits apart (p = 8 or 11); the smaller is then below a
quarter ulp_16 of the larger, and both the twice- and the once-rounded sum are
the larger value. So the written sum must be bit-equal to the float64 sum
rounded once, on randn data.

Conditioning ladder. x = offset + randn rounded to the dtype, random w and b,
eps = 1e-5; the reference is float64 LayerNorm of the rounded inputs. No
allowance is derived here: the bound is the error of a sound fp32 LayerNorm on
the same inputs, measured in the same test, e_native <= 2 * e_eager with
e_eager = max|F.layer_norm(x.float(), ...).to(dtype) - ref64| on the same
device. The factor 2 covers a different but equally sound summation order. A
one-pass variance ss/C - mean^2 loses log2((mean/std)^2) bits to cancellation:
its twin is at 48x (C = 320) and 55x (C = 1280) of e_eager at fp16, mean/std =
512, and at 2.1x already at fp16, 64, C = 320 (a CPU test below keeps the top
rung as the proof that the ladder has teeth); the two-pass twin measures 1.00
of e_eager on every rung (profiles/elementwise_edges_notes.md).

Run on an MI355X box: pytest tests/test_layernorm_edges_gpu.py -m gpu -q -s"""

import functools

import pytest
import torch
import torch.nn.functional as F

# the gpu mark is per test: the tests without it check the cases and the bound on the CPU
pytestmark = [pytest.mark.timeout(300)]

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

DEV = "cuda:0"
WAVE, WPB = 64, 4
DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16")]
WIDTHS = [8, 16, 504, 512, 520, 1024, 1032, 1536, 1544, 2048]
ROWS = [1, 3, 4, 5, 9]
# C -> (VPT the launcher picks, live lanes of the last trip)
PATHS = {8: (1, 1), 16: (1, 2), 504: (1, 63), 512: (1, 64), 520: (2, 1), 1024: (2, 64),
         1032: (3, 1), 1536: (3, 64), 1544: (4, 1), 2048: (4, 64)}
LADDER_SHAPES = [(16, 320), (16, 1280)]
LADDER = [(dt, rung) for dt, rungs in ((torch.bfloat16, (0, 8, 64)),
                                       (torch.float16, (0, 8, 64, 512))) for rung in rungs]
LADDER_IDS = [f"{'bf16' if dt == torch.bfloat16 else 'fp16'}-mean{rung}" for dt, rung in LADDER]


def _vpt(c):
    return 1 if c <= 512 else 2 if c <= 1024 else 3 if c <= 1536 else 4


# ---- the fp32 twin: ln_kernel's arithmetic in torch fp32 ops ----------------


def _wave_sum(v):
    """wave_all_reduce_sum: [rows, 64] per-lane values -> [rows]."""
    lanes = torch.arange(WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ off]
    return v[:, 0]


def _twin(v32, w, b, eps, two_pass=True):
    """v32: the fp32 row values (x, or x + res) [rows, C]. Element d of a row
    sits in lane (d / 8) % 64, trip d / 512, slot d % 8; a lane adds its slots
    in (trip, slot) order, then the butterfly. Returns (mean, var, y fp32)."""
    rows, c = v32.shape
    vpt = _vpt(c)
    pad = torch.zeros(rows, vpt * WAVE * 8)
    pad[:, :c] = v32
    t = pad.view(rows, vpt, WAVE, 8)
    live = (torch.arange(vpt * WAVE * 8) < c).view(1, vpt, WAVE, 8)
    s = torch.zeros(rows, WAVE)
    ss = torch.zeros(rows, WAVE)
    for k in range(vpt):
        for j in range(8):
            s = s + t[:, k, :, j]
            ss = ss + t[:, k, :, j] * t[:, k, :, j]
    mean = _wave_sum(s) / c
    if two_pass:
        d = torch.where(live, t - mean.view(rows, 1, 1, 1), torch.zeros(()))
        sq = torch.zeros(rows, WAVE)
        for k in range(vpt):
            for j in range(8):
                sq = sq + d[:, k, :, j] * d[:, k, :, j]
        var = (_wave_sum(sq) / c).clamp_min(0.0)
    else:  # the one-pass form the kernel had before: kept to show what the ladder catches
        var = (_wave_sum(ss) / c - mean * mean).clamp_min(0.0)
    inv = (var + torch.tensor(eps, dtype=torch.float32)).double().rsqrt().float()  # __frsqrt_rn
    y = (v32 - mean[:, None]) * inv[:, None] * w.float() + b.float()
    assert y.dtype == torch.float32
    return mean, var, y


# ---- exact rows -------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _affine(c, dtype):
    """Distinct dyadic (w_c, b_c): 8-bit mantissas, exponents in [-8, 8)."""
    i = torch.arange(c)
    w = (1 + (i % 128).double() / 128) * 2.0 ** ((i // 128) - 8).double()
    b = (1 + ((37 * i + 11) % 128).double() / 128) * 2.0 ** (((i // 128) * 5 + 3) % 16 - 8).double()
    b = b * (1 - 2 * (i % 2)).double()
    return w.to(dtype), b.to(dtype)


@functools.lru_cache(maxsize=None)
def _exact_rows(rows, c, dtype):
    """(x, base, res, w, b, sum64, y64). x = base + res = m_r +- s_r. Shared:
    never modified."""
    gen = torch.Generator().manual_seed(1000 * rows + c)
    r = torch.arange(rows).double()
    m, s = (r - 4).view(rows, 1), (2.0 ** (r - 4)).view(rows, 1)
    sign = torch.stack([(torch.randperm(c, generator=gen) < c // 2).double() * 2 - 1
                        for _ in range(rows)])
    w, b = _affine(c, dtype)
    base = m.expand(rows, c).contiguous()
    res = sign * s
    y64 = sign * w.double() + b.double()
    return ((base + res).to(dtype), base.to(dtype), res.to(dtype), w, b, base + res, y64)


@pytest.mark.parametrize("c", WIDTHS)
def test_widths_take_the_paths_they_name(c):
    vpt, last_live = PATHS[c]
    assert _vpt(c) == vpt and c % 8 == 0
    assert (c - (vpt - 1) * WAVE * 8) // 8 == last_live
    # WPB = 4: a lone row, partial last blocks (1, 3, 5, 9) and a full one (4)
    assert sorted(n % WPB for n in ROWS) == [0, 1, 1, 1, 3]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", WIDTHS)
def test_exact_rows_are_exact_in_fp32(c, dtype):
    """The construction is representable, and the twin finds mean = m_r, var =
    s_r^2 (by both variance formulas) and y = +-w + b with nothing rounded
    before the output: 0 of an allowance of 0."""
    for rows in ROWS:
        x, base, res, w, b, sum64, y64 = _exact_rows(rows, c, dtype)
        assert torch.equal(x.double(), sum64)
        assert torch.equal(base.double() + res.double(), sum64)
        assert torch.equal(y64.float().double(), y64)  # +-w + b is exact in fp32
        r = torch.arange(rows).double()
        for v32 in (x.float(), base.float() + res.float()):
            for two_pass in (True, False):
                mean, var, y = _twin(v32, w, b, 0.0, two_pass)
                assert torch.equal(mean.double(), r - 4)
                assert torch.equal(var.double(), 4.0 ** (r - 4))
                assert torch.equal(y.double(), y64)
    w, b = _affine(c, dtype)
    assert len(set(zip(w.tolist(), b.tolist()))) == c and w.unique().numel() == c


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", WIDTHS)
def test_exact_rows_bit_equal_float64(c, dtype):
    from distrifuser_amd.ops.dispatch import hip_ext

    for rows in ROWS:
        x, base, res, w, b, sum64, y64 = _exact_rows(rows, c, dtype)
        want = y64.to(dtype)
        wd, bd = w.to(DEV), b.to(DEV)
        y = hip_ext().layer_norm(x.to(DEV), wd, bd, 0.0)
        assert torch.equal(y.cpu(), want), f"layer_norm rows={rows}"
        s, y = hip_ext().add_layer_norm(base.to(DEV), res.to(DEV), wd, bd, 0.0)
        assert torch.equal(s.cpu(), sum64.to(dtype)), f"add_layer_norm sum rows={rows}"
        assert torch.equal(y.cpu(), want), f"add_layer_norm y rows={rows}"


@functools.lru_cache(maxsize=None)
def _randn_pair(rows, c, dtype):
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(rows, c, generator=gen).to(dtype)
    # a wide range of magnitudes in res, so the two exponents differ by 0..20 bits
    res = (torch.randn(rows, c, generator=gen)
           * torch.exp2(torch.randint(-16, 5, (rows, c), generator=gen).float())).to(dtype)
    return x, res


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp32_sum_rounded_to_16_bits_is_the_once_rounded_sum(dtype):
    """The docstring's argument, checked on the data the GPU test uses."""
    x, res = _randn_pair(9, 1544, dtype)
    assert torch.equal((x.float() + res.float()).to(dtype), (x.double() + res.double()).to(dtype))


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_layer_norm_sum_is_rounded_once(dtype):
    from distrifuser_amd.ops.dispatch import hip_ext

    x, res = _randn_pair(9, 1544, dtype)
    w, b = _affine(1544, dtype)
    s, _ = hip_ext().add_layer_norm(x.to(DEV), res.to(DEV), w.to(DEV), b.to(DEV), 1e-5)
    assert torch.equal(s.cpu(), (x.double() + res.double()).to(dtype))


# ---- arena ------------------------------------------------------------------


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [520, 8])
def test_inputs_from_nan_arena(c, dtype):
    """x and res sit inside a NaN-filled allocation at 16-byte-aligned offsets.
    A lane with d0 >= C that read (the last row's would read the arena) puts a
    NaN into the row's sums."""
    from distrifuser_amd.ops.dispatch import hip_ext

    rows = 5
    numel = rows * c
    gen = torch.Generator().manual_seed(3)
    arena = torch.full((2 * numel + 3 * 2048,), float("nan"), device=DEV, dtype=dtype)

    def carve(i):
        off = 2048 + i * (numel + 2048)  # a multiple of 8 elements: 16-byte aligned
        t = arena[off: off + numel].view(rows, c)
        t.copy_(torch.randn(rows, c, generator=gen))
        assert t.data_ptr() % 16 == 0
        return t

    x, res = carve(0), carve(1)
    w = torch.randn(c, generator=gen).to(DEV, dtype)
    b = torch.randn(c, generator=gen).to(DEV, dtype)
    y = hip_ext().layer_norm(x, w, b, 1e-5)
    assert torch.isfinite(y.float()).all()
    assert torch.equal(y, hip_ext().layer_norm(x.clone(), w, b, 1e-5))
    s, y = hip_ext().add_layer_norm(x, res, w, b, 1e-5)
    s2, y2 = hip_ext().add_layer_norm(x.clone(), res.clone(), w, b, 1e-5)
    assert torch.isfinite(s.float()).all() and torch.isfinite(y.float()).all()
    assert torch.equal(s, s2) and torch.equal(y, y2)
    assert torch.isnan(arena[:2048]).all() and torch.isnan(arena[-2048:]).all()


# ---- conditioning ladder ----------------------------------------------------


@functools.lru_cache(maxsize=None)
def _ladder_case(rows, c, dtype, offset):
    """(x, w, b, ref64): ref64 is float64 LayerNorm of the rounded inputs.
    Shared: never modified."""
    gen = torch.Generator().manual_seed(rows + c + offset)
    x = (offset + torch.randn(rows, c, generator=gen)).to(dtype)
    w = torch.randn(c, generator=gen).to(dtype)
    b = torch.randn(c, generator=gen).to(dtype)
    ref = F.layer_norm(x.double(), (c,), w.double(), b.double(), 1e-5)
    return x, w, b, ref


def _err(y, ref):
    return (y.double().cpu() - ref).abs().max().item()


def _cpu_errors(rows, c, dtype, offset, two_pass):
    x, w, b, ref = _ladder_case(rows, c, dtype, offset)
    e_twin = _err(_twin(x.float(), w, b, 1e-5, two_pass)[2].to(dtype), ref)
    e_eager = _err(F.layer_norm(x.float(), (c,), w.float(), b.float(), 1e-5).to(dtype), ref)
    return e_twin, e_eager


@pytest.mark.parametrize("dtype,offset", LADDER, ids=LADDER_IDS)
@pytest.mark.parametrize("rows,c", LADDER_SHAPES)
def test_twin_stays_on_the_ladder(rows, c, dtype, offset):
    e_twin, e_eager = _cpu_errors(rows, c, dtype, offset, two_pass=True)
    print(f"\nC={c} {dtype} mean/std={offset}: two-pass twin {e_twin:.3e} "
          f"eager fp32 {e_eager:.3e} ratio {e_twin / e_eager:.2f}")
    assert e_twin <= 2 * e_eager


@pytest.mark.parametrize("rows,c", LADDER_SHAPES)
def test_one_pass_variance_falls_off_the_top_rung(rows, c):
    """The ladder has teeth: ss/C - mean^2 in the kernel's own order is an
    order of magnitude over the bound at fp16, mean/std = 512."""
    e_twin, e_eager = _cpu_errors(rows, c, torch.float16, 512, two_pass=False)
    assert e_twin > 10 * e_eager


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("dtype,offset", LADDER, ids=LADDER_IDS)
@pytest.mark.parametrize("rows,c", LADDER_SHAPES)
def test_conditioning_ladder(rows, c, dtype, offset):
    from distrifuser_amd.ops.dispatch import hip_ext

    x, w, b, ref = _ladder_case(rows, c, dtype, offset)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    e_native = _err(hip_ext().layer_norm(xd, wd, bd, 1e-5), ref)
    e_eager = _err(F.layer_norm(xd.float(), (c,), wd.float(), bd.float(), 1e-5).to(dtype), ref)
    print(f"\nC={c} {dtype} mean/std={offset}: native {e_native:.3e} eager fp32 {e_eager:.3e} "
          f"ratio {e_native / e_eager:.2f}")
    assert e_native <= 2 * e_eager
