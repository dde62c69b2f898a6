"""GPU: the token-layout GroupNorm apply and tokens_add_nchw are bit-identical
(torch.equal) to the NCHW kernel / torch add followed or preceded by the
permute they absorb, on every tile edge of the two kernels, and the tiny
SDXL-style transformer computes the same with and without DFA_NO_BOUNDARY_FUSE.

Run on an MI355X box: pytest tests/test_transformer_boundary_gpu.py -m gpu -q"""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

if torch.cuda.is_available():
    from distrifuser_amd import ops
else:  # collected on CPU boxes but never run
    ops = None

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

DEV = "cuda:0"
N = 2
# (C, G, H, W): which edge of the 64 x 64 (vector) / 32 x 32 (scalar) tile it hits
SHAPES = [
    (32, 32, 8, 8),      # group size 1; one tile, half empty in the channel direction
    (96, 32, 5, 7),      # HW = 35: scalar path, partial tiles both ways
    (64, 32, 24, 40),    # HW = 960 = 15 * 64: many pixel tiles; 960 % 128 != 0
    (640, 32, 16, 24),   # the workload's channel count: 10 channel tiles, 6 pixel tiles
    (1288, 8, 8, 8),     # C = 20 * 64 + 8: partial channel tile of one 16-byte chunk
    (72, 8, 9, 8),       # HW = 72: vector path with a partial pixel tile (one 8-pixel vector)
    (20, 4, 8, 8),       # C % 8 != 0: element-wise tile here, vectorised NCHW kernel there
]
DTYPES = [torch.bfloat16, torch.float16]


def _to_tokens(x):
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n, h * w, c).contiguous()


def _gn_inputs(c, h, w, dtype, seed=0, exact_stats=False):
    """exact_stats: x holds integers in [-8, 8]. group_norm_silu sums a large
    group's moments with one float atomicAdd per block, in arrival order, so
    two calls on random data can differ in the last bit of a moment whatever
    the output layout. With these integers every partial sum is exact in fp32
    (at most 10304 * 64 < 2^24), the moments are the same in any order, and
    torch.equal between two calls is meaningful. The normalised values are
    still arbitrary floats (random weight and bias)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if exact_stats:
        x = torch.randint(-8, 9, (N, c, h, w), device=DEV, generator=g).to(dtype)
    else:
        x = (torch.randn(N, c, h, w, device=DEV, generator=g) * 1.5 + 0.3).to(dtype)
    wt = torch.randn(c, device=DEV, generator=g).to(dtype)
    b = torch.randn(c, device=DEV, generator=g).to(dtype)
    return x, wt, b


@requires_gpu
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_group_norm_tokens_equals_nchw_permuted(shape, dtype, silu):
    c, g, h, w = shape
    x, wt, b = _gn_inputs(c, h, w, dtype, exact_stats=True)
    ref = ops.group_norm_silu(x, g, wt, b, 1e-6, silu=silu)
    got = ops.group_norm_silu(x, g, wt, b, 1e-6, silu=silu, tokens=True)
    assert got.shape == (N, h * w, c) and got.is_contiguous()
    assert torch.equal(got, _to_tokens(ref))
    # given moments: nothing but the apply kernel runs, on random data
    x, wt, b = _gn_inputs(c, h, w, dtype)
    stats = ops.group_norm_stats(x, g)
    ref = ops.group_norm_apply(x, stats[0], stats[1], wt, b, 1e-6, silu=silu)
    got = ops.group_norm_apply(x, stats[0], stats[1], wt, b, 1e-6, silu=silu, tokens=True)
    assert got.shape == (N, h * w, c) and got.is_contiguous()
    assert torch.equal(got, _to_tokens(ref))


@requires_gpu
@pytest.mark.parametrize("shape", [(96, 32, 5, 7), (64, 32, 24, 40)])
def test_group_norm_tokens_fp32(shape):
    c, g, h, w = shape
    x, wt, b = _gn_inputs(c, h, w, torch.float32)
    stats = ops.group_norm_stats(x, g)
    for silu in (False, True):
        ref = ops.group_norm_apply(x, stats[0], stats[1], wt, b, 1e-6, silu=silu)
        got = ops.group_norm_apply(x, stats[0], stats[1], wt, b, 1e-6, silu=silu, tokens=True)
        assert torch.equal(got, _to_tokens(ref))
    x, wt, b = _gn_inputs(c, h, w, torch.float32, exact_stats=True)
    ref = ops.group_norm_silu(x, g, wt, b, 1e-6, silu=True)
    got = ops.group_norm_silu(x, g, wt, b, 1e-6, silu=True, tokens=True)
    assert torch.equal(got, _to_tokens(ref))


@requires_gpu
def test_group_norm_tokens_no_affine():
    x, _, _ = _gn_inputs(64, 8, 8, torch.bfloat16)
    ref = ops.group_norm_silu(x, 32, None, None, 1e-6, silu=False)
    got = ops.group_norm_silu(x, 32, None, None, 1e-6, silu=False, tokens=True)
    assert torch.equal(got, _to_tokens(ref))


@requires_gpu
@pytest.mark.parametrize("shape", [(1288, 8, 8, 8), (96, 32, 5, 7)])
def test_inputs_from_nan_arena(shape):
    """The ops expose no out= argument, so the guard is on the input side:
    x, the residual and y sit inside NaN-filled arenas. A read outside them
    would put a NaN into the result."""
    c, g, h, w = shape
    dtype = torch.bfloat16
    numel = N * c * h * w
    g_ = torch.Generator(device=DEV).manual_seed(2)
    arena = torch.full((3 * numel + 3 * 4096,), float("nan"), device=DEV, dtype=dtype)

    def carve(i, shp):
        off = 2048 + i * (numel + 4096)  # 16-byte aligned, NaN on both sides
        t = arena[off : off + numel].view(shp)
        # integers: exact group moments in any summation order (see _gn_inputs)
        t.copy_(torch.randint(-8, 9, shp, device=DEV, generator=g_))
        return t

    x = carve(0, (N, c, h, w))
    res = carve(1, (N, c, h, w))
    y = carve(2, (N, h * w, c))
    wt = torch.randn(c, device=DEV, generator=g_).to(dtype)
    b = torch.randn(c, device=DEV, generator=g_).to(dtype)
    tok = ops.group_norm_silu(x, g, wt, b, 1e-6, silu=False, tokens=True)
    assert not torch.isnan(tok).any()
    assert torch.equal(tok, _to_tokens(ops.group_norm_silu(x, g, wt, b, 1e-6, silu=False)))
    out = ops.tokens_add_nchw(y, res)
    assert not torch.isnan(out).any()
    assert torch.equal(out, y.reshape(N, h, w, c).permute(0, 3, 1, 2) + res)


def _add_inputs(c, h, w, dtype, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    y = torch.randn(N, h * w, c, device=DEV, generator=g).to(dtype)
    res = (torch.randn(N, c, h, w, device=DEV, generator=g) * 2.0).to(dtype)
    return y, res


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES + [torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_tokens_add_nchw_equals_torch(shape, dtype):
    c, _, h, w = shape
    y, res = _add_inputs(c, h, w, dtype)
    ref = y.reshape(N, h, w, c).permute(0, 3, 1, 2) + res
    got = ops.tokens_add_nchw(y, res)
    assert got.shape == (N, c, h, w) and got.is_contiguous()
    assert torch.equal(got, ref)


@requires_gpu
@pytest.mark.parametrize("shape", [(640, 32, 16, 24), (96, 32, 5, 7)])
def test_tokens_add_nchw_channel_slice_residual(shape):
    """residual = a channel slice of a wider tensor (a skip-concat view): batch
    and channel strides differ from the dense ones, the kernel takes them."""
    c, _, h, w = shape
    y, _ = _add_inputs(c, h, w, torch.bfloat16)
    wide = torch.randn(N, c + 40, h, w, device=DEV).to(torch.bfloat16)
    res = wide[:, 24 : 24 + c]
    assert not res.is_contiguous()
    ref = y.reshape(N, h, w, c).permute(0, 3, 1, 2) + res
    assert torch.equal(ops.tokens_add_nchw(y, res), ref)


@requires_gpu
def test_tokens_add_nchw_strided_plane_falls_back():
    """A residual whose (H, W) plane is not contiguous takes the eager path."""
    c, h, w = 64, 8, 8
    y, _ = _add_inputs(c, h, w, torch.bfloat16)
    wide = torch.randn(N, c, h, w + 8, device=DEV).to(torch.bfloat16)
    res = wide[..., :w]
    ref = y.reshape(N, h, w, c).permute(0, 3, 1, 2) + res
    got = ops.tokens_add_nchw(y, res)
    assert got.is_contiguous() and torch.equal(got, ref)
    nhwc = torch.randn(N, h, w, c, device=DEV).to(torch.bfloat16).permute(0, 3, 1, 2)
    ref = y.reshape(N, h, w, c).permute(0, 3, 1, 2) + nhwc
    assert torch.equal(ops.tokens_add_nchw(y, nhwc), ref)
    with pytest.raises(RuntimeError):
        ops.hip_ext().tokens_add_nchw(y, res)  # the binding itself refuses it


def _tiny_transformer(monkeypatch, no_fuse):
    from distrifuser_amd.models.layers import LayerFactory
    from distrifuser_amd.models.transformer import Transformer2DModel
    from distrifuser_amd.parallel.state import ParallelState
    from distrifuser_amd.utils.config import DistriConfig

    if no_fuse:
        monkeypatch.setenv("DFA_NO_BOUNDARY_FUSE", "1")
    else:
        monkeypatch.delenv("DFA_NO_BOUNDARY_FUSE", raising=False)
    cfg = DistriConfig(height=64, width=96, use_cuda_graph=False, device=DEV)
    torch.manual_seed(0)
    model = Transformer2DModel(64, 2, 32, 1, 32, factory=LayerFactory(ParallelState(cfg)))
    assert model.boundary_fuse == (not no_fuse)
    return model.to(device=DEV, dtype=torch.bfloat16).eval()


@requires_gpu
def test_tiny_transformer_switch(monkeypatch, capsys):
    old = _tiny_transformer(monkeypatch, True)
    new = _tiny_transformer(monkeypatch, False)
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(2, 64, 8, 12, device=DEV, generator=g).to(torch.bfloat16)
    ehs = torch.randn(2, 7, 32, device=DEV, generator=g).to(torch.bfloat16)
    with torch.no_grad():
        a1, a2, b = old(x, ehs), old(x, ehs), new(x, ehs)
    assert b.shape == x.shape and b.is_contiguous()
    if torch.equal(a1, a2):
        branch = "old-vs-old identical: new-vs-old must be torch.equal"
        ok = torch.equal(a1, b)
    else:
        noise = (a1.float() - a2.float()).abs().max().item()
        err = (a1.float() - b.float()).abs().max().item()
        branch = f"old-vs-old max abs {noise}: new-vs-old max abs {err} must not exceed it"
        ok = err <= noise
    with capsys.disabled():
        print(f"\n[tiny transformer] {branch}")
    assert ok, branch
