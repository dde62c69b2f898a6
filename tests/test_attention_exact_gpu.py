"""The 16-bit flash-attention kernel (csrc/attention.hip) against exact and
float64-bounded expectations, B = H = 2 with different data per (b, h).

1. Exact gather. K rows are sign codes, q = 32 k[sel]: the selected score
   leads by >= 40 nats, the output is V[sel] bit for bit. Mutants that live
   here: a wrong token, chunk, split, batch or head stride, two V rows or P
   rows exchanged, a dropped boundary token. Shapes: every Lkv around the
   128-token tile and the 32-token sub-tile for head dims 64 (DMA) and 40
   (descriptor loads, padded columns), the other head dims at one masked tail
   and one multi-tile length, all chunk layouts, Lq edges, lse, split+merge.
2. Exact uniform mean. Q = 0, V = m[d] + s[t, d] with s summing to zero: the
   output is m bit for bit. Mutants: a token dropped or doubled, a pad row
   counted, a row of another head or batch. Same Lkv sweep and chunk layouts.
3. Float64-bounded. Peaked and stepped scores against float64 attention on
   the same operands under a bound derived from the kernel's arithmetic
   (profiles/attention_exact_notes.md); split+merge of family 2 is held to
   the same bound. Mutants: a rescale applied to the wrong rows, a P or exp
   error that the one-hot weights of family 1 cannot show.
4. Unmarked CPU tests: eager float64 attention with each defect built in
   leaves the expected bits (families 1, 2) or the bound by 4 x (family 3).

The kernel is called through ops.hip_ext(), so nothing can fall back to eager.
The 16-bit output of the plain entry is allocated by the binding; the canary
cases go through flash_attention_partial, the entry that writes into caller
memory.

Run on an MI355X box: pytest tests/test_attention_exact_gpu.py -m gpu -q -s"""

import functools
import math

import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")


def gpu_test(fn):
    return pytest.mark.gpu(pytest.mark.timeout(300)(requires_gpu(fn)))


B, H = 2, 2
BF16, F16 = torch.bfloat16, torch.float16
TILE, SUB = 128, 32
LKVS = (1, 31, 32, 33, 64, 127, 128, 129, 192, 200, 424, 576)
CHUNKS = ((3, 72), (2, 200), (5, 8), (3, 128), (2, 320))
# unit roundoff of round-to-nearest into 8 (bf16) and 11 (fp16) significant bits:
# the P pack and the output store
U_P = U_OUT = {BF16: 2.0 ** -8, F16: 2.0 ** -11}
U32 = 2.0 ** -24


def _dt(i):
    return (BF16, F16)[i % 2]


def _name(dtype):
    return "bf16" if dtype == BF16 else "fp16"


def _splits_used(lkv, splits):
    return max(1, min(splits, -(-lkv // TILE)))


# ---- float64 reference and the defects ------------------------------------------


def attention64(q, k, v):
    """float64 attention on [B,H,L,D] -> (o, lse, sum p|v| / sum p, scaled scores)."""
    q, k, v = q.double(), k.double(), v.double()
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * q.shape[-1] ** -0.5
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    return p @ v, lse, p @ v.abs(), s


def _split_ranges(lkv, splits):
    tiles, s_used = -(-lkv // TILE), _splits_used(lkv, splits)
    return [(s * tiles // s_used * TILE, min((s + 1) * tiles // s_used * TILE, lkv))
            for s in range(s_used)]


def mutants(q, k, v, chunks=None, splits=1):
    """name -> float64 output of attention with that defect, where it applies."""
    lkv, out = k.shape[2], {}
    o64 = lambda kk, vv, qq=q: attention64(qq, kk, vv)[0]
    drop = lambda t: (torch.cat([k[:, :, :t], k[:, :, t + 1:]], 2),
                      torch.cat([v[:, :, :t], v[:, :, t + 1:]], 2))
    if lkv > 1:
        out["last token dropped"] = o64(*drop(lkv - 1))
        a = lkv - 2 if (lkv - 1) % SUB else 0  # a pair inside one sub-tile
        vs = v.clone()
        vs[:, :, [a, a + 1]] = v[:, :, [a + 1, a]]
        out["two V rows swapped"] = o64(k, vs)
    for t in (127, 128):
        if lkv > t + 1:
            out[f"token {t} dropped"] = o64(*drop(t))
    if lkv % TILE not in (0, 64):
        zero = torch.zeros_like(k[:, :, :1])
        out["zero pad row admitted"] = o64(torch.cat([k, zero], 2), torch.cat([v, zero], 2))
    if chunks:
        nc, lc = chunks
        km = k.clone()
        km[:, :, (nc - 1) * lc:] = k[:, :, (nc - 2) * lc:(nc - 1) * lc]
        out["K of the last chunk read at the chunk before"] = o64(km, v)
    ranges = _split_ranges(lkv, splits)
    if len(ranges) > 1:
        parts = [attention64(q, k[:, :, a:b], v[:, :, a:b]) for a, b in ranges]
        lse = torch.stack([p[1] for p in parts])
        w = torch.exp(lse - lse.amax(0))
        for j in range(len(ranges)):
            wj = w.clone()
            wj[j] = 1.0
            out[f"split {j} merged with weight 1"] = (
                sum(wj[i][..., None] * parts[i][0] for i in range(len(parts)))
                / wj.sum(0)[..., None])
    ob = o64(k, v)
    ob[1] = o64(k[:1], v[:1], q[1:])[0]
    out["batch 1 served from batch 0"] = ob
    return out


# ---- family 1: exact gather ------------------------------------------------------


def sign_codes(lkv, d, salt):
    """[lkv, d] in {-1, 1}: column c carries bit (c + salt) % 10 of t ^ salt. Ten
    bits, not nine: Lkv reaches 640. Two tokens differ in >= d // 10 columns."""
    t = torch.arange(lkv) ^ salt
    return (((t[:, None] >> ((torch.arange(d) + salt) % 10)) & 1) * 2 - 1).float()


def _edge_tokens(lkv, chunks, splits):
    """Last and first token of the whole range, of every tile, the tail, every
    chunk and split, then of the sub-tiles, in that order of priority."""
    edges = [lkv, 0] + list(range(TILE, lkv, TILE)) + [a for a, _ in _split_ranges(lkv, splits)]
    if chunks:
        edges += [c * chunks[1] for c in range(1, chunks[0])]
    edges += list(range(SUB, lkv, SUB))
    seen = []
    for e in edges:
        for t in (e - 1, e):
            if 0 <= t < lkv and t not in seen:
                seen.append(t)
    return seen


@functools.lru_cache(maxsize=None)
def gather_case(d, lkv, lq, dtype, chunks=None, splits=1):
    gen = torch.Generator().manual_seed(d * 100003 + lkv * 101 + lq)
    k = torch.stack([sign_codes(lkv, d, 37 * bh + 5) for bh in range(B * H)]).view(B, H, lkv, d)
    edge = _edge_tokens(lkv, chunks, splits)
    sel = []
    for bh in range(B * H):  # the edges, rotated per (b, h), then every other token
        r = bh * -(-len(edge) // (B * H)) % len(edge)
        rest = [t for t in torch.randperm(lkv, generator=gen).tolist() if t not in edge]
        seq = edge[r:] + edge[:r] + rest
        sel.append((seq * -(-lq // lkv))[:lq])
    sel = torch.tensor(sel).view(B, H, lq)
    q = 32.0 * torch.gather(k, 2, sel[..., None].expand(-1, -1, -1, d))
    shape = (B, H, lkv, d)
    v = (torch.randint(0, 2, shape, generator=gen) * 2 - 1) * torch.ldexp(
        1 + torch.randint(0, 128, shape, generator=gen) / 128.0,
        torch.randint(-6, 2, shape, generator=gen))
    want = torch.gather(v, 2, sel[..., None].expand(-1, -1, -1, d)).to(dtype)
    return q.to(dtype), k.to(dtype), v.to(dtype), want


def _case(d, lkv=None, lq=33, dtype=BF16, chunks=None, padded=False, splits=1, lse=False):
    lkv = chunks[0] * chunks[1] if chunks else lkv
    kv = f"{chunks[0]}x{chunks[1]}" if chunks else f"L{lkv}"
    ident = f"d{d}-{kv}-q{lq}-{_name(dtype)}" + ("-pad" if padded else "") + (
        f"-S{splits}" if splits > 1 else "") + ("-lse" if lse else "")
    return pytest.param(d, lkv, lq, dtype, chunks, padded, splits, lse, id=ident)


GATHER = (
    # every tile / sub-tile edge: DMA (64) and descriptor loads with padded columns (40)
    [_case(d, l, dtype=_dt(i + j)) for j, d in enumerate((64, 40)) for i, l in enumerate(LKVS)]
    # per-row staging (80), DFULL row passes (128), DPAD 160: masked tail, many tiles
    + [_case(d, l, dtype=dt) for d in (80, 128, 160) for l in (129, 424) for dt in (BF16, F16)]
    # chunks: straddling, exactly filled and in-chunk tiles in turn, poison around the slots
    + [_case(d, chunks=c, dtype=_dt(i + d // 8), padded=True)
       for d in (64, 40, 128) for i, c in enumerate(CHUNKS)]
    + [_case(80, chunks=c, dtype=_dt(i), padded=True) for i, c in enumerate(CHUNKS[:2])]
    + [_case(64, chunks=c, dtype=_dt(i)) for i, c in enumerate(CHUNKS)]
    # Lq: one row, a full block, a second block with one live row
    + [_case(64, 200, lq=lq, dtype=_dt(lq)) for lq in (1, 256, 257)] + [_case(160, 200, lq=257)]
    # lse at one split; splits 2 and 3, clamped where Lkv has fewer tiles
    + [_case(d, l, dtype=_dt(l), lse=True) for d in (64, 40, 128) for l in (129, 576)]
    + [_case(d, l, dtype=_dt(i), splits=s, lse=True)
       for d in (64, 40) for i, l in enumerate((31, 129, 424, 576)) for s in (2, 3)]
    + [_case(64, chunks=c, splits=s, dtype=_dt(s), lse=True)
       for c, s in (((5, 8), 2), ((3, 128), 3), ((2, 200), 2), ((2, 200), 3), ((2, 320), 3))]
    # strided K/V inside a poisoned parent: NaN / 3e4 past Lkv and past Dh
    + [_case(d, l, dtype=_dt(i), padded=True)
       for i, d in enumerate((40, 64, 80, 128, 160)) for l in (33, 200)]
)


def test_case_count():
    total = len(GATHER) + len(UNIFORM) + len(BOUNDED) + len(CANARY) + len(NAN_HEAD) + 1
    assert total <= 200, total


def _gather_args(p):
    d, lkv, lq, dtype, chunks, _, splits, _ = p.values
    return d, lkv, lq, dtype, chunks, splits


def _unique(params, key):
    seen = {}
    for p in params:
        seen.setdefault(key(p), pytest.param(*key(p), id=p.id))
    return list(seen.values())


@pytest.mark.parametrize("d,lkv,lq,dtype,chunks,splits", _unique(GATHER, _gather_args))
def test_gather_inputs(d, lkv, lq, dtype, chunks, splits):
    """The selected score leads by >= 40 nats, float64 attention rounds to
    V[sel], and every defect but the zero pad row (score 0 against a selected
    score of 32 sqrt(d): family 2 owns it) changes bits."""
    q, k, v, want = gather_case(d, lkv, lq, dtype, chunks, splits)
    assert (v.float().abs() >= 2.0 ** -6).all() and (v.float().abs() <= 4).all()
    o, _, _, s = attention64(q, k, v)
    if lkv > 1:
        top = s.topk(2, dim=-1).values
        assert (top[..., 0] - top[..., 1] >= 40).all()
    assert torch.equal(o.to(dtype), want)
    for name, om in mutants(q, k, v, chunks, splits).items():
        if name != "zero pad row admitted" and lq >= 33:  # fewer rows cannot select every edge
            assert not torch.equal(om.to(dtype), want), name


# ---- family 2: exact uniform mean ------------------------------------------------


@functools.lru_cache(maxsize=None)
def uniform_case(d, lkv, dtype):
    """V = m + n / 8, n[t] = 2 (r[t] - r[t+1]) cyclically with r[0] = 0 and
    r[t] in 1..4, neighbours different: the sum over any run of tokens
    telescopes, the whole is 0, a suffix from t0 is 2 r[t0] / 8 != 0, a single
    token is never 0. m is a multiple of 2^-6 in [2^-4, 2], so |V| <= 3 lies
    on the 2^-6 grid (exact in 16 bits) and sums of 640 of them in fp32."""
    gen = torch.Generator().manual_seed(d * 1009 + lkv)
    m = torch.randint(4, 129, (B, H, 1, d), generator=gen) / 64.0
    m[..., 0], m[..., 1], m[..., 2] = 2.0 ** -4, 127 / 64.0, 1.0
    m = m * (torch.randint(0, 2, m.shape, generator=gen) * 2 - 1)
    r = torch.randint(1, 5, (B, H, lkv, d), generator=gen)
    r[:, :, 0] = 0
    for t in range(1, lkv):
        r[:, :, t] = torch.where(r[:, :, t] == r[:, :, t - 1], r[:, :, t] % 4 + 1, r[:, :, t])
    v = m + 2 * (r - r.roll(-1, dims=2)) / 8.0
    k = torch.randn(B, H, lkv, d, generator=gen)
    assert torch.equal(v.to(dtype).float(), v) and torch.equal(m.to(dtype).float(), m)
    return k.to(dtype), v.to(dtype), m.to(dtype)


UNIFORM = (
    [_case(d, l, dtype=_dt(i + j), lse=True)
     for j, d in enumerate((40, 64)) for i, l in enumerate(LKVS)]
    + [_case(d, chunks=c, dtype=_dt(i), padded=True) for d in (64, 128) for i, c in enumerate(CHUNKS)]
    + [_case(d, l, dtype=_dt(l)) for d in (80, 160) for l in (129, 200)]
)


@pytest.mark.parametrize("d,lkv,dtype", _unique(UNIFORM, lambda p: (p.values[0], p.values[1],
                                                                    p.values[3])))
def test_uniform_inputs(d, lkv, dtype):
    k, v, m = uniform_case(d, lkv, dtype)
    s = v.double() - m.double()
    assert (s.sum(2) == 0).all() and (s * 8 == (s * 8).round()).all()
    if lkv > 1:
        assert (s != 0).all(), "a single token sums to zero"
        suffix = s.flip(2).cumsum(2)[:, :, :min(32, lkv - 1)]
        assert (suffix != 0).all(), "a suffix of 1..32 tokens sums to zero"
    q = torch.zeros(B, H, 33, d, dtype=dtype)
    want = m.expand(B, H, 33, d)
    o, lse, _, _ = attention64(q, k, v)
    assert torch.equal(o.to(dtype), want) and (lse - math.log(lkv)).abs().max() < 1e-12
    for name, om in mutants(q, k, v).items():
        if name != "two V rows swapped":  # a mean cannot see a permutation: family 1
            assert not torch.equal(om.to(dtype), want), name


# ---- family 3: float64 bound -----------------------------------------------------


def bounds(q, k, v, dtype, splits=1):
    """(o64, per-element bound, lse64, per-row lse bound); the derivation is in
    profiles/attention_exact_notes.md, section 1."""
    o64, lse64, a, s = attention64(q, k, v)
    d, lkv = q.shape[-1], k.shape[2]
    gamma = lambda n: n * U32 / (1 - n * U32)
    qk = torch.einsum("bhqd,bhkd->bhqk", q.double().abs(), k.double().abs()).amax(-1) * d ** -0.5
    smax = s.abs().amax(-1)
    eps_s = gamma(d) * qk + 4 * U32 * smax + 2.0 ** -23       # nats, per row
    delta_s = torch.expm1(2 * eps_s)[..., None]
    acc = gamma(lkv + 2 * -(-lkv // SUB) + 2)                  # l, PV, rescales, 1/l
    e_lse = eps_s + acc + 2.0 ** -19 + 4 * U32 * (smax + lse64.abs())
    rel = U_P[dtype] + delta_s + acc
    s_used = _splits_used(lkv, splits)
    if s_used > 1:
        eta = torch.expm1(2 * (e_lse + 2.0 ** -22))
        rel = rel + (2 * eta + gamma(s_used + 2))[..., None]
        e_lse = e_lse + eta + 2.0 ** -22 * (1 + lse64.abs())
    e_pre = rel * a
    return o64, e_pre + U_OUT[dtype] * (o64.abs() + e_pre), lse64, e_lse


def rule64(q, k, v, dtype):
    """The kernel's rule with float64 sums: p against the row maximum, packed
    to 16 bits for PV, l from the unpacked p, the quotient rounded once."""
    s = attention64(q, k, v)[3]
    p = torch.exp(s - s.amax(-1, keepdim=True))
    return ((p.float().to(dtype).double() @ v.double()) / p.sum(-1, keepdim=True)).float().to(dtype)


STRUCTURES = ("peaked", "tile_boundary", "subtile_boundary", "split_row_block", "peeled_tail",
              "creep")
CREEP = 4.85 / math.log2(math.e)  # nats per sub-tile: two steps stay under 11 log2 units


@functools.lru_cache(maxsize=None)
def structured_case(name, d, lkv, dtype):
    """score(i, t) = gain_i level_t + noise + 40 [t = target_i]: q and k share
    the direction u (components alpha and beta), the random parts are
    orthogonal to it. Levels are <= -24 nats, so an admitted zero pad row
    (score 0) takes the row. Rows 0..3 of every (b, h) carry a target each
    (last token, 127, 128, the one before the last), 40 nats up."""
    gen = torch.Generator().manual_seed(STRUCTURES.index(name) * 7919 + d * 31 + lkv)
    lq = 33 if name == "peaked" else 64
    u = torch.ones(d) / d ** 0.5
    perp = lambda x: x - (x @ u)[..., None] * u
    amp_q, amp_k = (6.0, 1.0) if name == "peaked" else (0.5, 0.5)
    level = torch.full((lkv,), -24.0)
    gain = torch.ones(lq)
    if name == "creep":
        level = -24.0 - CREEP * (torch.arange(lkv).flip(0) // SUB)
    elif name != "peaked":
        step_at = {"tile_boundary": 128, "subtile_boundary": 160, "split_row_block": 128,
                   "peeled_tail": 288}[name]
        level[:step_at] = -34.0
        if name == "split_row_block":
            gain[1::2] = 0.0
    kp = amp_k * perp(torch.randn(B, H, lkv, d, generator=gen))
    qp = amp_q * perp(torch.randn(B, H, lq, d, generator=gen))
    targets = [t for t in (lkv - 1, 127, 128, lkv - 2) if 0 <= t < lkv]
    for i, t in enumerate(targets):
        kt = kp[:, :, t]
        qp[:, :, i] = 0.5 * qp[:, :, i] + 40.0 * d ** 0.5 * kt / (kt * kt).sum(-1, keepdim=True)
    alpha = d ** 0.25 * 24.0 ** 0.5  # alpha beta / sqrt(d) = 24 at level -24
    q = qp + (gain * alpha)[:, None] * u
    k = kp + (level / 24.0 * alpha)[:, None] * u
    v = torch.randn(B, H, lkv, d, generator=gen).clamp_(-4.0, 4.0)
    return q.to(dtype), k.to(dtype), v.to(dtype)


def _bcase(name, d, lkv, dtype, chunks=None):
    kv = f"{chunks[0]}x{chunks[1]}" if chunks else f"L{lkv}"
    return pytest.param(name, d, lkv, dtype, chunks, id=f"{name}-d{d}-{kv}-{_name(dtype)}")


BOUNDED = (
    [_bcase("peaked", d, l, dt) for d in (64, 40, 80, 128, 160) for l in (200, 424)
     for dt in (BF16, F16)]
    + [_bcase("peaked", d, nc * lc, _dt(d // 8 + nc), (nc, lc)) for d in (64, 40)
       for nc, lc in ((3, 72), (2, 200))]
    + [_bcase(n, 64, 320, dt) for n in STRUCTURES[1:] for dt in (BF16, F16)]
    + [_bcase("creep", 40, 320, dt) for dt in (BF16, F16)]
    + [_bcase("uniform", d, l, _dt(l)) for d, l in ((64, 200), (64, 576), (40, 424), (128, 129))]
)


def _bounded_inputs(name, d, lkv, dtype):
    if name == "uniform":
        k, v, _ = uniform_case(d, lkv, dtype)
        return torch.zeros(B, H, 33, d, dtype=dtype), k, v
    return structured_case(name, d, lkv, dtype)


@pytest.mark.parametrize("name,d,lkv,dtype,chunks", BOUNDED)
def test_bounded_inputs(name, d, lkv, dtype, chunks):
    """The structure each case is named after holds on the scores the kernel
    sees, and every defect leaves the bound by 4 x somewhere. The uniform
    inputs are held to their bits by family 2 and enter here only through
    split+merge: no check of theirs."""
    if name == "uniform":
        return
    q, k, v = structured_case(name, d, lkv, dtype)
    o64, bound, _, _ = bounds(q, k, v, dtype, splits=3)  # the widest of the bounds used
    s = attention64(q, k, v)[3]
    assert ((rule64(q, k, v, dtype).double() - o64).abs() <= bounds(q, k, v, dtype)[1]).all()
    if name not in ("peaked", "split_row_block"):
        assert s[:, :, 4:].max() < -10.0
    sub = torch.stack([s[..., a:a + SUB].amax(-1) for a in range(0, lkv, SUB)], -1)[:, :, 32:]
    rise = (sub[..., 1:] - sub[..., :-1].cummax(-1).values) * math.log2(math.e)
    if name == "creep":  # no rescale over two sub-tiles, one at the third
        two, three = sub[..., 2:] - sub[..., :-2], sub[..., 3:] - sub[..., :-3]
        assert (two * math.log2(math.e) < 11).all() and (three * math.log2(math.e) > 11).all()
        assert (two * math.log2(math.e) > 8.5).all()
    elif name != "peaked":
        at = {"tile_boundary": 4, "subtile_boundary": 5, "split_row_block": 4, "peeled_tail": 9}[name]
        rows = slice(0, None, 2) if name == "split_row_block" else slice(None)
        assert (rise[:, :, rows, at - 1] > 11).all()
        assert (rise[:, :, rows, :at - 1] < 11).all() and (rise[:, :, rows, at:] < 11).all()
        if name == "split_row_block":
            assert (rise[:, :, 1::2] < 11).all()
    for split_count in (1, 2, 3):
        for mname, om in mutants(q, k, v, chunks, split_count).items():
            if split_count > 1 and "split" not in mname:
                continue
            worst = ((om - o64).abs() / bound).max().item()
            assert worst >= 4, f"{mname}: only {worst:.2f} x the bound"


# ---- the kernel ------------------------------------------------------------------


def _dpad(d):
    return next(p for p in (64, 96, 128, 160) if d <= p)


def device_kv(k, v, chunks, padded):
    """[B,H,Lkv,D] on the CPU -> K and V on the GPU as views of one flat buffer
    [NC, slot + 64] -> [NC, B, rows, 2, H, Dp], the fused to_kv layout with a
    padded slot stride. padded: rows = LC + 8 and Dp = DPAD + 8, so the token
    stride is wider than the head dim, and every element that is not K or V,
    the gap behind each slot included, is poison: NaN, 3e4 where K would be."""
    (b, h, lkv, d), dev = k.shape, "cuda:0"
    nc, lc = chunks or (1, lkv)
    rows, dp = (lc + 8, _dpad(d) + 8) if padded else (lc, d)
    slot = b * rows * 2 * h * dp
    buf = torch.full((nc, slot + 64), float("nan"), dtype=k.dtype, device=dev)
    six = buf[:, :slot].view(nc, b, rows, 2, h, dp)
    six[:, :, :, 0] = 3.0e4
    views = []
    for i, t in enumerate((k, v)):
        six[:, :, :lc, i, :, :d] = t.to(dev).view(b, h, nc, lc, d).permute(2, 0, 3, 1, 4)
        view = six[:, :, :lc, i, :, :d].permute(1, 3, 0, 2, 4)
        views.append(view if chunks else view[:, :, 0])
    return views


def run(q, k, v, chunks=None, padded=False, splits=1, lse=False):
    """-> (out [B,H,Lq,D], lse [B,H,Lq] or None) on the CPU."""
    from distrifuser_amd import ops

    kg, vg = device_kv(k, v, chunks, padded)
    qg = torch.cat([q, q], dim=-1).to("cuda:0")[..., :q.shape[-1]]  # a slice of a fused projection
    if splits == 1 and not lse:
        res = [ops.hip_ext().flash_attention(qg, kg, vg)]
    else:
        res = ops.hip_ext().flash_attention_ext(qg, kg, vg, splits, lse)
    torch.cuda.synchronize()
    return res[0].cpu(), (res[1].cpu() if lse else None)


def assert_same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = (got != want).any(dim=-1).nonzero()
    assert bad.numel() == 0, (
        f"{what}: {bad.shape[0]} of {want[..., 0].numel()} rows differ, first (b, h, row) = "
        f"{bad[0].tolist()}, wrong columns there "
        f"{(got != want)[tuple(bad[0])].nonzero().flatten().tolist()[:8]}")
    assert torch.equal(got, want)


def assert_within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    ratio = (err / bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, err/bound {ratio:.3f}")
    assert torch.isfinite(got).all() and ratio <= 1, f"{what}: {ratio:.3f} x the bound"
    return ratio


@gpu_test
@pytest.mark.parametrize("d,lkv,lq,dtype,chunks,padded,splits,lse", GATHER)
def test_exact_gather(d, lkv, lq, dtype, chunks, padded, splits, lse):
    q, k, v, want = gather_case(d, lkv, lq, dtype, chunks, splits)
    got, got_lse = run(q, k, v, chunks, padded, splits, lse)
    assert_same_bits(got, want, "gather")
    if lse:
        _, _, lse64, e_lse = bounds(q, k, v, dtype, splits)
        assert_within(got_lse, lse64, e_lse, "gather lse")


NAN_HEAD = [_case(64, 200), _case(40, 200, dtype=F16), _case(64, chunks=(3, 72), dtype=F16),
            _case(40, chunks=(3, 72))]


@gpu_test
@pytest.mark.parametrize("d,lkv,lq,dtype,chunks,padded,splits,lse", NAN_HEAD)
def test_nan_head_stays_in_its_head(d, lkv, lq, dtype, chunks, padded, splits, lse):
    """All K and V of (b, h) = (1, 0) are NaN: every other head's rows are
    finite and the gathered bits."""
    q, k, v, want = gather_case(d, lkv, lq, dtype, chunks, splits)
    k, v = k.clone(), v.clone()
    k[1, 0] = v[1, 0] = float("nan")
    got, _ = run(q, k, v, chunks, padded=True)
    keep = torch.ones(B, H, dtype=torch.bool)
    keep[1, 0] = False
    assert torch.isfinite(got[keep]).all()
    assert_same_bits(got[keep], want[keep], "beside a NaN head")


CANARY = [pytest.param(lq, s, _dt(lq + s), id=f"q{lq}-S{s}-{_name(_dt(lq + s))}")
          for lq in (1, 33, 256, 257) for s in (1, 2)]


@gpu_test
@pytest.mark.parametrize("lq,splits,dtype", CANARY)
def test_partial_rows_stay_inside_lq(lq, splits, dtype):
    """Partial waves, a full 256-row block and a second block with one live
    row, through the entry that writes into caller memory: the partial O and
    lse lie inside canary-filled buffers, every element of theirs is written,
    no canary moves, and the merge gives the gathered bits."""
    from distrifuser_amd import ops

    d, lkv, canary, guard = 64, 200, 12345.0, 1 << 16
    q, k, v, want = gather_case(d, lkv, lq, dtype, None, splits)
    kg, vg = device_kv(k, v, None, False)
    n_o, n_l = splits * B * lq * H * d, splits * B * H * lq
    o_buf = torch.full((guard + n_o + guard,), canary, device="cuda:0")
    l_buf = torch.full((guard + n_l + guard,), canary, device="cuda:0")
    o_part = o_buf[guard:guard + n_o].view(splits, B, lq, H, d)
    lse_part = l_buf[guard:guard + n_l].view(splits, B, H, lq)
    assert ops.hip_ext().flash_attention_partial(q.to("cuda:0"), kg, vg, splits, o_part,
                                                 lse_part) == splits
    for buf, n in ((o_buf, n_o), (l_buf, n_l)):
        assert (buf[:guard] == canary).all() and (buf[guard + n:] == canary).all(), "canary moved"
        assert not (buf[guard:guard + n] == canary).any(), "rows left unwritten"
    out = ops.hip_ext().merge_attention(o_part, lse_part, out_dtype=dtype)[0]
    assert_same_bits(out.permute(0, 2, 1, 3).cpu(), want, "merged partials")


@gpu_test
def test_gather_through_64_bit_offsets():
    """Token stride 2^23 elements: 128 rows span 2^31 bytes, fits_off32 is
    false and the full tile takes the per-row 64-bit staging. The 2 GiB parent
    is never filled: only the 128 + 5 rows in use are written."""
    d, lkv, stride = 64, 133, 1 << 23
    q, k, v, want = gather_case(d, lkv, 33, BF16)
    try:
        buf = torch.empty(lkv * stride, dtype=BF16, device="cuda:0")
    except RuntimeError as exc:  # out of memory
        pytest.skip(f"no room for the 2 GiB K/V parent: {exc}")
    views = []
    for i, t in enumerate((k, v)):  # [B,H,Lkv,D] at element (i*B*H + b*H + h)*d of every row
        view = buf.as_strided((B, H, lkv, d), (H * d, d, stride, 1), i * B * H * d)
        view.copy_(t.to("cuda:0"))
        views.append(view)
    from distrifuser_amd import ops

    got = ops.hip_ext().flash_attention(q.to("cuda:0"), *views)
    torch.cuda.synchronize()
    assert_same_bits(got.cpu(), want, "64-bit staging")


@gpu_test
@pytest.mark.parametrize("d,lkv,lq,dtype,chunks,padded,splits,lse", UNIFORM)
def test_exact_uniform_mean(d, lkv, lq, dtype, chunks, padded, splits, lse):
    k, v, m = uniform_case(d, lkv, dtype)
    q = torch.zeros(B, H, lq, d, dtype=dtype)
    got, _ = run(q, k, v, chunks, padded)
    assert_same_bits(got, m.expand(B, H, lq, d), "uniform mean")
    if lse:
        got, got_lse = run(q, k, v, chunks, padded, lse=True)
        assert_same_bits(got, m.expand(B, H, lq, d), "uniform mean with lse")
        _, _, lse64, e_lse = bounds(q, k, v, dtype)
        assert_within(got_lse, lse64, e_lse, "uniform lse")
        assert (lse64 - math.log(lkv)).abs().max() < 1e-12


@gpu_test
@pytest.mark.parametrize("name,d,lkv,dtype,chunks", BOUNDED)
def test_bounded_against_float64(name, d, lkv, dtype, chunks):
    q, k, v = _bounded_inputs(name, d, lkv, dtype)
    for splits in (1, 2, 3):
        if name == "uniform" and splits == 1:
            continue  # family 2 holds it to its bits
        o64, bound, lse64, e_lse = bounds(q, k, v, dtype, splits)
        what = f"{name} d={d} lkv={lkv} {_name(dtype)} S={splits}"
        got, got_lse = run(q, k, v, chunks, padded=bool(chunks), splits=splits, lse=True)
        assert_within(got, o64, bound, what)
        assert_within(got_lse, lse64, e_lse, what + " lse")
        if splits == 1:
            assert torch.equal(run(q, k, v, chunks, padded=bool(chunks))[0], got), "plain != lse mode"
