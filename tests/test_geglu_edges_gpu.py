"""GEGLU (csrc/geglu.hip, geglu_kernel: out = a * gelu(gate), the two halves of
the last dimension) against float64: every finite 16-bit gate, the vector and
the element path in every dtype, NaN containment inside a vector, which half
is which, and the smallest tensors that send the grid-stride loop round a
second time.

Bound. The reference is, in float64 on the rounded inputs,

    ref = a * g * Phi(g),   Phi(g) = (1 + erf(g / sqrt 2)) / 2 = erfc(-g / sqrt 2) / 2

(the erfc form keeps the left tail, where 1 + erf cancels in any precision).
The kernel computes a * (0.5 * g * (1 + erff(g * 0.70710678f))) in fp32. With
u = 2^-24: the argument of erff carries 2u relative (the constant, the
product), which moves erf by at most |z erf'(z)| 2u <= 0.86 u; erff itself is
good to a few ulp of its value, <= 4u absolutely; the add rounds once. So
1 + erff is within 6u of 2 Phi(g) ABSOLUTELY. That is no relative bound where
Phi is small, and it is multiplied by |a g| / 2: 3u |a| |g|. The three products
add 3u |ref|. With the slack that takes the place of second-order terms,

    |y - ref| <= eps_a := 8u |a| |g| + 4u |ref|,

and the output is accepted when |got - ref| <= ulp_out(ref) / 2 + eps_a, ulp_out
the spacing of the output dtype at ref (subnormal range included). Where
|ref| + eps_a reaches the rounding threshold to infinity (fp16: a * g up to
3 * 65504), the infinity of ref's sign is accepted too. No constant comes from
kernel output. The fp32 twin is the kernel's expression in torch fp32 ops on
the CPU: over every gate below it uses at most 0.19 of eps_a where half is
allowed (torch's own F.gelu, a different erf, uses 0.47 on the same gates).

Run on an MI355X box: pytest tests/test_geglu_edges_gpu.py -m gpu -q"""

import functools
import math

import pytest
import torch

# the gpu mark is per test: the tests without it check the cases and the bound on the CPU
pytestmark = [pytest.mark.timeout(300)]

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

DEV = "cuda:0"
U = 2.0 ** -24
GRID_CAP = 4096 * 256  # work items of one trip: grid_for() in csrc/dispatch.h
# significand bits, least normal exponent, largest finite value
FORMATS = {torch.bfloat16: (8, -126, torch.finfo(torch.bfloat16).max),
           torch.float16: (11, -14, 65504.0),
           torch.float32: (24, -126, torch.finfo(torch.float32).max)}
DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16"),
          pytest.param(torch.float32, id="fp32")]
A_VALUES = (1.0, -3.0, 0.3330078125)
SWEEP_INNER = 8192
# (rows, inner, dtype, path, work items)
BIG = [
    pytest.param(1030, 8192, torch.bfloat16, "vector", 1054720, id="bf16-vector"),
    pytest.param(1018, 1031, torch.float32, "element", 1049558, id="fp32-element"),
]


def _path(rows, inner, dtype):
    """(path, work items) of launch_geglu: vectors iff inner % V == 0."""
    v = 16 // torch.empty((), dtype=dtype).element_size()
    vec = inner % v == 0
    return ("vector" if vec else "element"), rows * inner // (v if vec else 1)


def _half_ulp(ref, dtype):
    """Half the spacing of dtype at ref (float64), subnormal range included."""
    p, emin, _ = FORMATS[dtype]
    e = torch.frexp(ref.abs())[1] - 1  # floor(log2 |ref|)
    e = torch.where(ref == 0, torch.full_like(e, emin), e).clamp_min(emin)
    return torch.ldexp(torch.full_like(ref, 0.5), e - (p - 1))


def _reference(h):
    """(ref, allowance) in float64 from the rounded input [..., 2 * inner]."""
    a, g = h.double().chunk(2, dim=-1)
    ref = a * g * 0.5 * torch.special.erfc(-g / math.sqrt(2.0))
    return ref, 8 * U * a.abs() * g.abs() + 4 * U * ref.abs()


def _check(got, h, what):
    """NaN exactly where the reference has one; elsewhere inside the bound, or
    the right infinity where the reference can round to it."""
    dtype = h.dtype
    assert got.dtype == dtype and got.shape == h.shape[:-1] + (h.shape[-1] // 2,)
    ref, allow = _reference(h)
    half = _half_ulp(ref, dtype)
    fmax = FORMATS[dtype][2]
    got = got.double().cpu()
    err = (got - ref).abs()
    to_inf = (ref.abs() + allow >= fmax + _half_ulp(torch.full_like(ref, fmax), dtype)) \
        & (got == torch.sign(ref) * math.inf)
    ok = torch.where(ref.isnan(), got.isnan(), (err <= half + allow) | to_inf)
    assert ok.all(), (f"{what}: {(~ok).sum().item()} of {ok.numel()} outside the bound, first at "
                      f"{(~ok).nonzero()[0].tolist()}")


def _twin_ratio(h):
    a, g = h.float().chunk(2, dim=-1)
    twin = a * (0.5 * g * (1.0 + torch.erf(g * 0.70710678118654752440)))  # geluf() in common.h
    assert twin.dtype == torch.float32
    ref, allow = _reference(h)
    return ((twin.double() - ref).abs() / allow.clamp_min(1e-300)).max().item()


# ---- exhaustive gate sweep ------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _sweep(dtype):
    """[8, 2 * 8192]: 2^16 gates, a from A_VALUES varying along the row (period
    3: every vector mixes them). Shared: never modified."""
    if dtype == torch.float32:
        mag = torch.exp2(torch.linspace(-20.0, math.log2(40.0), 32767, dtype=torch.float64))
        g = torch.cat([mag, -mag, torch.tensor([0.0, -0.0], dtype=torch.float64)]).float()
    else:  # every 16-bit pattern; the non-finite ones and |g| > 65504 give way to 0
        g = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)
        g = torch.where(g.float().abs() <= 65504.0, g, torch.zeros((), dtype=dtype))
    g = g.view(-1, SWEEP_INNER)
    rows = g.shape[0]
    pick = (torch.arange(SWEEP_INNER).view(1, -1) + torch.arange(rows).view(-1, 1)) % 3
    a = torch.tensor(A_VALUES)[pick].to(dtype)
    return torch.cat([a, g], dim=-1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_holds_every_gate_and_the_twin_uses_at_most_half(dtype):
    h = _sweep(dtype)
    assert h.shape == (8, 2 * SWEEP_INNER) and _path(8, SWEEP_INNER, dtype)[0] == "vector"
    g = h[:, SWEEP_INNER:]
    assert torch.isfinite(g.float()).all()
    if dtype != torch.float32:  # every finite pattern up to 65504, each once (0 fills the rest)
        want = 2 * (0x7BFF + 1) if dtype == torch.float16 else 2 * (0x477F + 1)
        assert g.view(torch.int16).unique().numel() == want
        assert g.float().abs().max() == (65504.0 if dtype == torch.float16 else 65280.0)
    else:
        assert g.unique().numel() == 65535 and g.abs().max() == 40.0
        assert g[g != 0].abs().min() == 2.0 ** -20 and (g == 0).sum() == 2
    ratio = _twin_ratio(h)
    print(f"\n{dtype}: twin uses {ratio:.3f} of the allowance")
    assert ratio <= 0.5


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_gate(dtype):
    from distrifuser_amd import ops

    h = _sweep(dtype)
    _check(ops.geglu(h.to(DEV)), h, "gate sweep")


@functools.lru_cache(maxsize=None)
def _nan_case(dtype):
    """Row 0: a NaN gate at slot 3 of its vector; row 1: a NaN a at slot 5."""
    gen = torch.Generator().manual_seed(5)
    h = (torch.randn(2, 16, generator=gen) * 2).to(dtype)
    h[0, 8 + 3] = float("nan")
    h[1, 5] = float("nan")
    return h


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_stays_in_its_slot(dtype):
    from distrifuser_amd import ops

    h = _nan_case(dtype)
    got = ops.geglu(h.to(DEV))
    want = torch.zeros(2, 8, dtype=torch.bool)
    want[0, 3] = want[1, 5] = True
    assert torch.equal(got.isnan().cpu(), want)
    _check(got, h, "NaN containment")  # the seven neighbours are inside the bound


# ---- shapes and halves --------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _halves_case(rows, inner, dtype, ramp_is_gate):
    """3-D [2, rows, 2 * inner]: one half is 1, the other a ramp over [-4, 4]
    that differs at every position. Shared: never modified."""
    ramp = torch.linspace(-4.0, 4.0, 2 * rows * inner).view(2, rows, inner)
    ones = torch.ones_like(ramp)
    return torch.cat([ones, ramp] if ramp_is_gate else [ramp, ones], dim=-1).to(dtype)


SHAPES = [(rows, inner) for inner in (8, 40, 7, 1) for rows in (1, 3)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes_take_the_paths_they_name_and_swapped_halves_show(dtype):
    for rows, inner in SHAPES:
        assert _path(2 * rows, inner, dtype)[0] == ("vector" if inner in (8, 40) else "element")
        for ramp_is_gate in (True, False):
            h = _halves_case(rows, inner, dtype, ramp_is_gate)
            assert _twin_ratio(h) <= 0.5
            # what a kernel that read the halves the other way round would write
            a, g = h.chunk(2, dim=-1)
            swapped = _reference(torch.cat([g, a], dim=-1))[0].to(dtype)
            with pytest.raises(AssertionError, match="outside the bound"):
                _check(swapped, h, "swapped halves")


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,inner", SHAPES)
def test_shapes_and_halves(rows, inner, dtype):
    from distrifuser_amd import ops

    for ramp_is_gate in (True, False):
        h = _halves_case(rows, inner, dtype, ramp_is_gate)
        _check(ops.geglu(h.to(DEV)), h, f"ramp_is_gate={ramp_is_gate}")


# ---- second trip ----------------------------------------------------------------


@pytest.mark.parametrize("rows,inner,dtype,path,items", BIG)
def test_big_cases_take_a_second_trip_on_the_path_they_name(rows, inner, dtype, path, items):
    assert _path(rows, inner, dtype) == (path, items)
    assert GRID_CAP < items <= 2 * GRID_CAP
    assert max(_path(2 * r, i, dt)[1] for r, i in SHAPES for dt in FORMATS) <= GRID_CAP
    assert _path(8, SWEEP_INNER, torch.float32)[1] <= GRID_CAP


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("rows,inner,dtype,path,items", BIG)
def test_second_trip(rows, inner, dtype, path, items):
    from distrifuser_amd import ops

    gen = torch.Generator().manual_seed(items)
    h = (torch.randn(rows, 2 * inner, generator=gen) * 2).to(dtype)
    _check(ops.geglu(h.to(DEV)), h, "second trip")
