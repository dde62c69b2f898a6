"""VAE mid-attention kernel (csrc/vae_attn.hip: one head, d=512 split over
four 128-wide d-slices, 32-token KV tiles) at its tile edges.

* One-hot keys turn the attention into a row gather of V, which must be
  bit-identical: a wrong token, d-slice, batch offset or tail mask moves
  whole rows.
* Peaked random scores and stepped scores (the running maximum rising at
  every tile boundary, never, for half the rows, or inside the 8-token tail)
  compare against ops.eager.vae_attention on fp32 copies with the project's
  tolerance, max abs error < 0.03.
* The unmarked tests check on the CPU, with eager only, that the inputs keep
  mutants apart: attention without the tail tokens, or with one d-slice of q
  dropped, differs from the truth by ten times the tolerance. i.i.d. randn
  q/k would not: their softmax is nearly uniform.

The GPU tests call the extension entry point directly.

Run on an MI355X box: pytest tests/test_vae_attention_edges_gpu.py -m gpu -q"""

import functools

import pytest
import torch

from distrifuser_amd.ops import eager

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")


def gpu_test(fn):
    return pytest.mark.gpu(pytest.mark.timeout(300)(requires_gpu(fn)))


BF16 = torch.bfloat16
C = 512     # channels = head dim
TILE = 32   # KV tokens per tile
TOL = 0.03
SEPARATION = 10 * TOL


def _ext_attention(q, k, v):
    from distrifuser_amd.ops.dispatch import hip_ext

    dev = torch.device("cuda:0")
    out = hip_ext().vae_attention(q.to(dev), k.to(dev), v.to(dev))
    torch.cuda.synchronize()
    return out.cpu()


# ---- exact gather ----------------------------------------------------------------

GATHER_L = [1, 8, 31, 32, 33, 104, 512]


@functools.lru_cache(maxsize=None)
def _gather_case(b, l):
    """k[b, t] = 32 e_t, q[b, i] = 32 e_perm_b(i): the matching score leads
    every other by 1024 / sqrt(512) ~ 45 nats, the rest of the softmax mass is
    below 512 e^-45 ~ 1.5e-17, so the output is v[b, perm_b] bit for bit."""
    gen = torch.Generator().manual_seed(1000 * b + l)
    k = (32.0 * torch.eye(l, C)).expand(b, l, C).contiguous().to(BF16)
    perm = torch.stack([torch.randperm(l, generator=gen) for _ in range(b)])
    q = torch.stack([k[i][perm[i]] for i in range(b)])
    v = torch.randn(b, l, C, generator=gen).to(BF16)
    want = torch.stack([v[i][perm[i]] for i in range(b)])
    if b > 1 and l > 8:
        assert not torch.equal(perm[0], perm[1])
    return q, k, v, want


@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("l", GATHER_L)
def test_gather_reference_is_exact(l, b):
    q, k, v, want = _gather_case(b, l)
    ref = eager.vae_attention(q.double(), k.double(), v.double())
    assert ref.dtype == torch.float64
    assert torch.equal(ref.to(BF16), want)


@gpu_test
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("l", GATHER_L)
def test_vae_attention_exact_gather(l, b):
    q, k, v, want = _gather_case(b, l)
    got = _ext_attention(q, k, v)
    assert got.shape == want.shape
    bad = (got != want).any(dim=-1).nonzero()
    assert bad.numel() == 0, (
        f"L={l} B={b}: {bad.shape[0]} of {b * l} rows differ, first (b, i) = {bad[0].tolist()}, "
        f"wrong channels there {(got != want)[tuple(bad[0])].nonzero().flatten().tolist()[:8]}")
    assert torch.equal(got, want)


# ---- peaked and stepped scores ---------------------------------------------------

PEAKED_L = [40, 104, 200]
STEPPED = ["every_tile", "tile0_highest", "even_rows_only", "inside_tail"]
STEPPED_L = 104  # three full tiles and an 8-token tail


@functools.lru_cache(maxsize=None)
def _peaked_inputs(l):
    """q = 6 randn: scores have a standard deviation of 6 nats, so a few
    tokens carry each row. |v| <= 2."""
    gen = torch.Generator().manual_seed(l)
    q = (6.0 * torch.randn(2, l, C, generator=gen)).to(BF16)
    k = torch.randn(2, l, C, generator=gen).to(BF16)
    v = torch.randn(2, l, C, generator=gen).clamp_(-2.0, 2.0).to(BF16)
    return q, k, v


# zero-sum sign rows over the four d-slices, in negated pairs (2i, 2i+1): an
# even-length run of tokens from an even token has as many +1 as -1 per slice
_SLICE_SIGNS = [(1., 1., -1., -1.), (-1., -1., 1., 1.), (1., -1., 1., -1.),
                (-1., 1., -1., 1.), (1., -1., -1., 1.), (-1., 1., 1., -1.)]


@functools.lru_cache(maxsize=None)
def _stepped_inputs(name):
    """q and k share a direction (as _stepped_inputs of the flash-attention
    tile suite): q ~ ones, and k[t] carries level[t] + 8 c[t, j] on d-slice j,
    scaled so that the scaled score of token t is level[t] + 2 sum_j c[t, j].
    The sign rows c[t] sum to zero, so the score is the level, and tokens of
    one level share the softmax evenly; without d-slice j the tokens with
    c[t, j] = +1 fall 4 nats behind those with -1 and lose it. Levels are all
    far below zero, so that a zero-filled K row left unmasked in the tail tile
    would take the whole softmax. |v| <= 2."""
    l = STEPPED_L
    gen = torch.Generator().manual_seed({n: 3 + i for i, n in enumerate(STEPPED)}[name])
    tile = torch.arange(l) // TILE
    gain = torch.ones(l, 1)
    if name == "every_tile":          # (a) up 16 at every tile boundary: corr < 1 every tile
        level = -64.0 + 16.0 * tile
    elif name == "tile0_highest":     # (b) the maximum never moves after tile 0: corr == 1,
        level = torch.full((l,), -40.0)   # yet the tail still carries weight
        level[:4] = -16.0
        level[96:] = -17.0
    elif name == "even_rows_only":    # (c) odd query rows see flat scores
        level = -64.0 + 16.0 * tile
        gain[1::2] = 0.0
    elif name == "inside_tail":       # (d) up 24 at token 100 of 104
        level = torch.full((l,), -40.0)
        level[100:] = -16.0
    c = torch.tensor(_SLICE_SIGNS)[torch.arange(l) % len(_SLICE_SIGNS)]
    per_slice = (level[:, None] + 8.0 * c) * (C ** 0.5 / C)          # [l, 4]
    k = per_slice.repeat_interleave(C // 4, dim=1) + 0.05 * torch.randn(l, C, generator=gen)
    q = gain * torch.ones(l, C) + 0.25 * torch.randn(l, C, generator=gen)
    v = torch.randn(l, C, generator=gen).clamp_(-2.0, 2.0)
    q, k, v = (t.to(BF16)[None] for t in (q, k, v))

    # the property the case is named after, on the scores the kernel will see
    s = torch.einsum("qc,kc->qk", q[0].double(), k[0].double()) / C ** 0.5
    tmax = torch.stack([s[:, t0 : t0 + TILE].amax(dim=1) for t0 in range(0, l, TILE)], dim=1)
    rise = tmax[:, 1:] - tmax[:, :-1].cummax(dim=1).values  # over the running maximum
    assert s[gain[:, 0] > 0].max() < -10.0
    if name == "every_tile":
        assert (rise >= 10.0).all()
    elif name == "tile0_highest":
        assert (rise < 0.0).all()
    elif name == "even_rows_only":
        assert (rise[0::2] >= 10.0).all() and (rise[1::2] < 10.0).all()
    elif name == "inside_tail":
        assert (rise[:, 2] >= 10.0).all() and (rise[:, :2].abs() < 10.0).all()
        assert (s[:, 96:100].amax(dim=1) + 10.0 <= s[:, 100:].amax(dim=1)).all()
    return q, k, v


def _numeric_cases():
    return [pytest.param(_peaked_inputs, l, id=f"peaked-L{l}") for l in PEAKED_L] + [
        pytest.param(_stepped_inputs, n, id=f"stepped-{n}") for n in STEPPED]


def _ref(q, k, v):
    return eager.vae_attention(q.float(), k.float(), v.float())


@pytest.mark.parametrize("make,arg", _numeric_cases())
def test_inputs_separate_mutants(make, arg):
    """A kernel that loses the tail tokens, or one d-slice of the split-K sum,
    is at least 10 x the tolerance away from the reference on these inputs."""
    q, k, v = make(arg)
    l = q.shape[1]
    ref = _ref(q, k, v)
    assert ref.abs().max() <= 2.0
    drop = l % TILE or 8
    no_tail = _ref(q, k[:, : l - drop], v[:, : l - drop])
    sep = (no_tail - ref).abs().max().item()
    print(f"last {drop} tokens dropped: {sep:.3f} away")
    assert sep >= SEPARATION, f"tail of {drop} tokens carries too little: {sep}"
    for sl in range(4):
        qz = q.clone()
        qz[..., sl * 128 : (sl + 1) * 128] = 0
        sep = (_ref(qz, k, v) - ref).abs().max().item()
        print(f"d-slice {sl} of q zeroed: {sep:.3f} away")
        assert sep >= SEPARATION, f"d-slice {sl} carries too little: {sep}"


@gpu_test
@pytest.mark.parametrize("make,arg", _numeric_cases())
def test_vae_attention_peaked_and_stepped(make, arg):
    """Tolerance: |v| <= 2, so the bf16 rounding of the output is <= 2^-8 * 2
    ~ 0.008 and the bf16 rounding of P adds <= 2^-9 * sum(p |v|) ~ 0.004."""
    q, k, v = make(arg)
    got = _ext_attention(q, k, v).float()
    ref = _ref(q, k, v)
    assert got.shape == ref.shape
    assert torch.isfinite(got).all(), f"{arg}: non-finite output"
    err = (got - ref).abs().max().item()
    print(f"{make.__name__.strip('_')} {arg}: max err {err:.5f}")
    assert err < TOL, f"{arg}: max err {err}"
