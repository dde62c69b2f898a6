"""GroupNorm apply (csrc/groupnorm.hip, gn_apply_kernel) against float64, with
caller-supplied fp32 moments: every dtype, with and without SiLU and affine,
on the vector and the element path, at group sizes 1, 2, 3 and 10, and at the
smallest tensors that send the grid-stride loop round a second time.

Bound. With u = 2^-24 and the supplied fp32 moments (m, q) taken as exact
inputs, the reference is, in float64,

    var = max(q - m^2, 0),  sc64 = w / sqrt(var + eps),  ref = (x - m) * sc64 + b

(eps is the fp32 value the kernel receives). The kernel (gn_scale_shift /
gn_norm) forms var with one fma (one rounding, u; it clamps where float64
clamps, or within u of it), var + eps (u), rsqrtf (<= 1 ulp = 2u), sc = w * inv
(u): sc is within (u/2 + u/2 + 2u + u) = 4u of sc64, relatively. Then sh = b -
m * sc in one fma or two roundings (<= u * (|b| + 2 |m sc|)) and y = x * sc + sh
likewise (<= u * (|b| + 2 |x sc| + |m sc|)). Together

    |y - ref| <= 4u (|x| + |m|) |sc| + u (2 |b| + 3 |m sc| + 2 |x sc|)
              <= eps_a := 8u (|x| + |m|) |sc64| + 2u |b|,

and the output is accepted when |got - ref| <= ulp_out(ref) / 2 + eps_a, ulp_out
the spacing of the output dtype at ref. With SiLU, ref = silu(ref) and
eps_a' = 1.1 eps_a + 2^-20 |ref|: |silu'| <= 1.1, and __expf plus the divide
are allowed 2^-20 relative. No constant comes from kernel output. The fp32
twin is ops/eager.py's group_norm_apply run in fp32 on the CPU: it uses at most
0.44 of eps_a on the cases below (0.38 end to end) where half is allowed.

The supplied moments differ per (sample, group): means are multiples of 1/8
in +-8, variances 2^-6 .. 2^6, and one group has q < m^2 (the var < 0 -> 0
clamp). They are dyadic, so m^2 and q - m^2 are exact in fp32 and the twin,
which squares and subtracts in two roundings, computes the same variance as the
kernel's fma. w and b differ per channel. A reference with the group index
shifted by one, or the channel index, violates the bound in every group (CPU
tests below), so a wrong index cannot hide inside it.

End to end, group_norm_silu runs on integer data m_g +- s_g: every partial sum
is an integer below 2^24, so the kernel's moments are known to the bit in any
summation order: fl(fl(sum) * fl(1 / n)), the launcher's arithmetic, exact
(m_g, m_g^2 + s_g^2) when n is a power of two. The same bound applies with
those moments.

Second trip: grid_for() caps a launch at 4096 blocks of 256 threads; the three
large cases hold a few thousand work items more than that, so some threads run
`vid += stride` once, on the vector path (bf16, fp32) and the element path.

Run on an MI355X box: pytest tests/test_groupnorm_apply_edges_gpu.py -m gpu -q"""

import functools

import pytest
import torch

from distrifuser_amd.ops import eager

# the gpu mark is per test: the tests without it check the cases and the bound on the CPU
pytestmark = [pytest.mark.timeout(300)]

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

DEV = "cuda:0"
U = 2.0 ** -24
EPS = 1e-5
GRID_CAP = 4096 * 256  # work items of one trip: grid_for() in csrc/dispatch.h
FORMATS = {torch.bfloat16: (8, -126), torch.float16: (11, -14), torch.float32: (24, -126)}
DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16"),
          pytest.param(torch.float32, id="fp32")]

# (shape, groups, path of the 16-bit types, path of fp32)
SMALL = [
    pytest.param((2, 8, 4, 4), 4, "vector", "vector", id="2x8x4x4-g4"),
    pytest.param((2, 6, 3, 5), 2, "element", "element", id="2x6x3x5-g2"),
    pytest.param((1, 32, 2, 6), 32, "element", "vector", id="1x32x2x6-g32"),
    pytest.param((2, 96, 5, 7), 32, "element", "element", id="2x96x5x7-g32"),
    pytest.param((1, 30, 8, 8), 3, "vector", "vector", id="1x30x8x8-g3"),
]
# (shape, groups, dtype, silu, path, work items)
BIG = [
    pytest.param((1, 8, 1024, 1032), 4, torch.bfloat16, False, "vector", 1056768, id="bf16-vector"),
    pytest.param((1, 4, 1024, 1028), 2, torch.float32, False, "vector", 1052672, id="fp32-vector"),
    pytest.param((1, 4, 513, 513), 2, torch.float16, True, "element", 1052676, id="fp16-element"),
]
E2E = [pytest.param((2, 8, 4, 4), 4, id="2x8x4x4-g4"), pytest.param((2, 6, 3, 5), 2, id="2x6x3x5-g2")]


def _path(shape, dtype):
    """(path, work items) of launch_gn_apply: vectors iff HW % V == 0."""
    n, c, h, w = shape
    v = 16 // torch.empty((), dtype=dtype).element_size()
    vec = (h * w) % v == 0
    return ("vector" if vec else "element"), n * c * h * w // (v if vec else 1)


def _half_ulp(ref, dtype):
    """Half the spacing of dtype at ref (float64), subnormal range included."""
    p, emin = FORMATS[dtype]
    e = torch.frexp(ref.abs())[1] - 1  # floor(log2 |ref|)
    e = torch.where(ref == 0, torch.full_like(e, emin), e).clamp_min(emin)
    return torch.ldexp(torch.full_like(ref, 0.5), e - (p - 1))


def _moments(n, g):
    """fp32 (mean, meansq) [n, g]: distinct dyadic means in +-8, variances
    2^-6 .. 2^6, and meansq < mean^2 in the last group."""
    i = torch.arange(n * g)
    mean = (((5 * i + 3) % 129) - 64).double() / 8
    var = 2.0 ** ((3 * i) % 13 - 6).double()
    var[-1] = -(2.0 ** -4)
    msq = mean * mean + var
    return mean.float().view(n, g), msq.float().view(n, g), var.view(n, g)


def _reference(x, mean, msq, w, b, groups, silu, dtype):
    """float64 result and bound from the rounded inputs and fp32 moments."""
    n, c, h, wd = x.shape
    per_ch = lambda t: t.double().repeat_interleave(c // groups, dim=1).view(n, c, 1, 1)
    m, q = per_ch(mean), per_ch(msq)
    w64 = torch.ones(c, dtype=torch.float64) if w is None else w.double()
    b64 = torch.zeros(c, dtype=torch.float64) if b is None else b.double()
    w64, b64 = w64.view(1, c, 1, 1), b64.view(1, c, 1, 1)
    eps32 = torch.tensor(EPS, dtype=torch.float32).double()
    sc = w64 / torch.sqrt((q - m * m).clamp_min(0.0) + eps32)
    x64 = x.double()
    ref = (x64 - m) * sc + b64
    allow = 8 * U * (x64.abs() + m.abs()) * sc.abs() + 2 * U * b64.abs()
    if silu:
        ref = ref * torch.sigmoid(ref)
        allow = 1.1 * allow + 2.0 ** -20 * ref.abs()
    return ref, allow, _half_ulp(ref, dtype) + allow


def _affine(c, gen, dtype):
    w = torch.linspace(0.5, 1.5, c)[torch.randperm(c, generator=gen)].to(dtype)
    b = torch.linspace(-1.0, 1.0, c)[torch.randperm(c, generator=gen)].to(dtype)
    return w, b


def _inputs(shape, groups, dtype, seed):
    n, c, h, wd = shape
    gen = torch.Generator().manual_seed(seed)
    mean, msq, var = _moments(n, groups)
    std = var.clamp_min(2.0 ** -6).sqrt()  # the clamped group: data 1/8 around its mean
    z = torch.randn(n, groups, c // groups * h * wd, generator=gen).double()
    x = (mean.double().unsqueeze(-1) + std.unsqueeze(-1) * z).view(shape).to(dtype)
    w, b = _affine(c, gen, dtype)
    return x, mean, msq, w, b


@functools.lru_cache(maxsize=None)
def _small_case(shape, groups, dtype, silu, affine):
    """Shared: never modified."""
    x, mean, msq, w, b = _inputs(shape, groups, dtype, seed=sum(shape) + groups)
    if not affine:
        w = b = None
    return (x, mean, msq, w, b) + _reference(x, mean, msq, w, b, groups, silu, dtype)


def _twin(x, mean, msq, w, b, silu):
    """ops/eager.py's apply in fp32: the value before the output rounding."""
    out = eager.group_norm_apply(x.float(), mean, msq, None if w is None else w.float(),
                                 None if b is None else b.float(), EPS, silu=silu)
    assert out.dtype == torch.float32
    return out.double()


# ---- CPU-run: paths, construction, twin, teeth --------------------------------


@pytest.mark.parametrize("shape,groups,path16,path32", SMALL)
def test_small_cases_take_the_paths_they_name(shape, groups, path16, path32):
    assert _path(shape, torch.bfloat16)[0] == _path(shape, torch.float16)[0] == path16
    assert _path(shape, torch.float32)[0] == path32
    assert max(_path(shape, dt)[1] for dt in FORMATS) <= GRID_CAP  # one trip


@pytest.mark.parametrize("shape,groups,dtype,silu,path,items", BIG)
def test_big_cases_take_a_second_trip_on_the_path_they_name(shape, groups, dtype, silu, path,
                                                            items):
    assert _path(shape, dtype) == (path, items)
    assert GRID_CAP < items <= 2 * GRID_CAP
    n, c, h, w = shape
    assert n * c * h * w * torch.empty((), dtype=dtype).element_size() < 40e6


def test_moments_are_exact_and_distinct():
    for n, g in [(2, 4), (2, 2), (1, 32), (2, 32), (1, 3), (1, 4), (1, 2)]:
        mean, msq, var = _moments(n, g)
        assert torch.equal(msq.double() - mean.double() ** 2, var)  # q - m^2 exact
        assert torch.equal((mean * mean).double(), mean.double() ** 2)  # m^2 exact in fp32
        assert mean.unique().numel() == n * g and mean.abs().max() <= 8
        assert (var < 0).sum() == 1 and var.max() <= 2.0 ** 6


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,groups,path16,path32", SMALL)
def test_twin_uses_at_most_half_the_allowance(shape, groups, path16, path32, dtype):
    worst = 0.0
    for silu in (False, True):
        for affine in (True, False):
            x, mean, msq, w, b, ref, allow, _ = _small_case(shape, groups, dtype, silu, affine)
            worst = max(worst, ((_twin(x, mean, msq, w, b, silu) - ref).abs() / allow).max().item())
    print(f"\n{shape} g={groups} {dtype}: twin uses {worst:.3f} of the allowance")
    assert worst <= 0.5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,groups,path16,path32", SMALL)
def test_a_shifted_group_or_channel_index_violates_the_bound(shape, groups, path16, path32,
                                                             dtype):
    """What a kernel with the right arithmetic and the group (channel) index
    off by one would write is outside the bound in every (sample, group)."""
    n, c = shape[:2]
    for silu in (False, True):
        x, mean, msq, w, b, ref, _, bound = _small_case(shape, groups, dtype, silu, True)
        wrong_group = _reference(x, mean.roll(1, 1), msq.roll(1, 1), w, b, groups, silu, dtype)[0]
        wrong_chan = _reference(x, mean, msq, w.roll(1), b.roll(1), groups, silu, dtype)[0]
        for wrong in (wrong_group, wrong_chan):
            out = wrong.to(dtype).double()  # that kernel's output, rounded as well as can be
            bad = ((out - ref).abs() > bound).view(n, groups, -1)
            assert bad.any(-1).all()
            assert bad.double().mean() > 0.5


# ---- GPU: supplied moments ------------------------------------------------------


def _check(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    ok = err <= bound  # a NaN or inf in got fails
    assert ok.all(), (f"{what}: {(~ok).sum().item()} of {ok.numel()} outside the bound, worst "
                      f"err/bound {(err / bound).max().item():.3g}")


def _dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("silu", [False, True], ids=["gn", "gn-silu"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,groups,path16,path32", SMALL)
def test_apply_with_supplied_moments(shape, groups, path16, path32, dtype, silu, affine):
    from distrifuser_amd import ops

    x, mean, msq, w, b, ref, _, bound = _small_case(shape, groups, dtype, silu, affine)
    got = ops.group_norm_apply(x.to(DEV), mean.to(DEV), msq.to(DEV), _dev(w), _dev(b), EPS,
                               silu=silu)
    assert got.dtype == dtype and got.shape == x.shape
    _check(got, ref, bound, "group_norm_apply")


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("shape,groups,dtype,silu,path,items", BIG)
def test_apply_second_trip(shape, groups, dtype, silu, path, items):
    from distrifuser_amd import ops

    x, mean, msq, w, b = _inputs(shape, groups, dtype, seed=items)
    ref, _, bound = _reference(x, mean, msq, w, b, groups, silu, dtype)
    got = ops.group_norm_apply(x.to(DEV), mean.to(DEV), msq.to(DEV), w.to(DEV), b.to(DEV), EPS,
                               silu=silu)
    _check(got, ref, bound, "group_norm_apply")


# ---- end to end on integer data -----------------------------------------------


@functools.lru_cache(maxsize=None)
def _e2e_case(shape, groups, dtype, silu, affine):
    """x = m_g +- s_g (integers); the moments group_norm_silu computes from
    it, known to the bit: fl(fl(sum) * fl(1 / n)). Shared: never modified."""
    n, c, h, wd = shape
    glen = c // groups * h * wd
    gen = torch.Generator().manual_seed(glen)
    i = torch.arange(n * groups).view(n, groups, 1)
    m, s = (i % 5 - 2).double(), 2.0 ** (i % 3).double()
    sign = torch.stack([(torch.randperm(glen, generator=gen) < glen // 2).double() * 2 - 1
                        for _ in range(n * groups)]).view(n, groups, glen)
    xg = m + sign * s
    inv_n = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(glen), dtype=torch.float32)
    mean = xg.sum(-1).float() * inv_n
    msq = (xg * xg).sum(-1).float() * inv_n
    assert (xg * xg).sum(-1).max() < 2 ** 24
    x = xg.view(shape).to(dtype)
    assert torch.equal(x.double(), xg.view(shape))
    w, b = _affine(c, gen, dtype) if affine else (None, None)
    return (x, mean, msq, w, b) + _reference(x, mean, msq, w, b, groups, silu, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,groups", E2E)
def test_end_to_end_moments_and_twin(shape, groups, dtype):
    worst = 0.0
    for silu in (False, True):
        for affine in (True, False):
            x, mean, msq, w, b, ref, allow, _ = _e2e_case(shape, groups, dtype, silu, affine)
            worst = max(worst, ((_twin(x, mean, msq, w, b, silu) - ref).abs() / allow).max().item())
    n, c, h, wd = shape
    glen = c // groups * h * wd
    if glen & (glen - 1) == 0:  # a power of two: the exact (m_g, m_g^2 + s_g^2)
        i = torch.arange(n * groups).view(n, groups)
        assert torch.equal(mean.double(), (i % 5 - 2).double())
        assert torch.equal(msq.double(), (i % 5 - 2).double() ** 2 + 4.0 ** (i % 3).double())
    print(f"\n{shape} g={groups} {dtype}: twin uses {worst:.3f} of the allowance")
    assert worst <= 0.5


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("silu", [False, True], ids=["gn", "gn-silu"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,groups", E2E)
def test_group_norm_silu_end_to_end(shape, groups, dtype, silu, affine):
    from distrifuser_amd import ops

    x, mean, msq, w, b, ref, _, bound = _e2e_case(shape, groups, dtype, silu, affine)
    got = ops.group_norm_silu(x.to(DEV), groups, _dev(w), _dev(b), EPS, silu=silu)
    _check(got, ref, bound, "group_norm_silu")
