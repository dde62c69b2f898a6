"""Flash attention on the GPU: log-sum-exp output, split-KV partials and the
merge kernel. bf16 inputs; the reference is ops.eager on fp32 copies; outputs
are held to the project's tolerance (max abs error < 0.03, as
tests/test_attention_tiles_gpu.py).

Split s of S owns the 128-token tiles [floor(s*T/S), floor((s+1)*T/S)) of the
T = ceil(Lkv/128) tiles, and S is clamped to T.

Run on an MI355X box: pytest tests/test_attention_splitkv_gpu.py -m gpu -q"""

import math

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

if torch.cuda.is_available():
    from distrifuser_amd import ops
    from distrifuser_amd.ops import eager
else:  # collected on CPU boxes but never run
    ops = eager = None

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

TOL = 0.03
# bf16 products are exact in fp32; an fp32 sum of <= 160 randn-sized terms stays
# below 1e-3; exp2/log2 add a few ulps of an O(10) value
LSE_TOL = 2e-3
MERGE_LSE_TOL = 1e-5


def _dev():
    return torch.device("cuda:0")


def _randn(*shape):
    return torch.randn(*shape, device=_dev(), dtype=torch.bfloat16)


def _ref(q, k, v):
    return eager.flash_attention_lse(q.float(), k.float(), v.float())


def _check_split(q, k, v, splits, what):
    out, lse = ops.flash_attention(q, k, v, kv_splits=splits, return_lse=True)
    ref, ref_lse = _ref(q, k, v)
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    assert lse.shape == ref_lse.shape and lse.dtype == torch.float32
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all(), f"{what}: non-finite"
    err = (out.float() - ref).abs().max().item()
    lse_err = (lse - ref_lse).abs().max().item()
    print(f"{what}: max err {err:.5f}, lse err {lse_err:.2e}")
    assert err < TOL, f"{what}: max err {err}"
    assert lse_err < LSE_TOL, f"{what}: lse err {lse_err}"
    # without the lse output the same kernels run: same bits
    assert torch.equal(ops.flash_attention(q, k, v, kv_splits=splits), out)


# ---- 1. LSE of the unsplit kernel ---------------------------------------------


@requires_gpu
@pytest.mark.parametrize("d", [64, 40])
@pytest.mark.parametrize("lkv", [8, 200, 320])
def test_lse_unsplit(lkv, d):
    """Measured on MI355X: at most 9.5e-7 over these six cases
    (profiles/attention_splitkv_notes.md)."""
    torch.manual_seed(lkv + d)
    q, k, v = _randn(1, 2, 33, d), _randn(1, 2, lkv, d), _randn(1, 2, lkv, d)
    out, lse = ops.flash_attention(q, k, v, return_lse=True)
    ref, ref_lse = _ref(q, k, v)
    assert lse.shape == (1, 2, 33) and lse.dtype == torch.float32
    lse_err = (lse - ref_lse).abs().max().item()
    err = (out.float() - ref).abs().max().item()
    print(f"lse unsplit lkv={lkv} d={d}: lse err {lse_err:.3e}, out err {err:.5f}")
    assert lse_err < LSE_TOL, f"lse err {lse_err}"
    assert err < TOL
    assert torch.equal(out, ops.flash_attention(q, k, v)), "S=1 with lse changed the output bits"


# ---- 2. split boundaries, plain KV --------------------------------------------


@requires_gpu
@pytest.mark.parametrize(
    "lkv,splits",
    [
        (256, 2),  # one full tile each
        (320, 2),
        (320, 3),  # the last split is the 64-token mask-free tail alone
        (328, 3),  # the last split is a masked 72-token tail alone
        (640, 2),  # 5 tiles, uneven partition
        (640, 4),
        (200, 4),  # S clamps to the 2 tiles
    ],
)
def test_split_boundaries(lkv, splits):
    torch.manual_seed(lkv * 10 + splits)
    _check_split(_randn(1, 2, 33, 64), _randn(1, 2, lkv, 64), _randn(1, 2, lkv, 64), splits,
                 f"lkv={lkv} S={splits}")


# ---- 3. the split weights are really applied ------------------------------------


@requires_gpu
@pytest.mark.parametrize("hot", [0, 1, 2])
def test_split_weights_are_applied(hot):
    """Lkv = 384, S = 3: the K rows of tile `hot` are scaled x4, so that tile
    carries nearly all of the softmax weight, and the V rows of tile s all
    equal s + 1, so part s is exactly s + 1 and a merge that ignored the
    weights would return their uniform average, 2. For hot = 0 and 2 the true
    output (about 1 and 3) is far from 2, which the test asserts on the CPU
    reference before it looks at the kernel. With the middle tile hot the true
    output is itself about 2 = the uniform average (the part values 1, 2, 3 are
    symmetric about it), so that input cannot tell right from wrong and is
    held to the output tolerance only."""
    torch.manual_seed(3)
    lq, lkv, d = 33, 384, 64
    q = _randn(1, 2, lq, d)
    k = _randn(1, 2, lkv, d)
    k[:, :, hot * 128:(hot + 1) * 128] *= 4
    v = torch.empty(1, 2, lkv, d, device=_dev(), dtype=torch.bfloat16)
    for s in range(3):
        v[:, :, s * 128:(s + 1) * 128] = s + 1
    ref, _ = _ref(q.cpu(), k.cpu(), v.cpu())
    parts = [
        eager.flash_attention(q.cpu().float(), k.cpu().float()[:, :, s * 128:(s + 1) * 128],
                              v.cpu().float()[:, :, s * 128:(s + 1) * 128])
        for s in range(3)
    ]
    uniform = torch.stack(parts).mean(dim=0)
    gap = (uniform - ref).abs().max().item()
    print(f"hot={hot}: uniform average is off by {gap:.3f}")
    if hot != 1:
        assert gap > 10 * TOL, f"the input cannot tell weighted from uniform: gap {gap}"
    out = ops.flash_attention(q, k, v, kv_splits=3).float().cpu()
    err = (out - ref).abs().max().item()
    print(f"hot={hot}: max err {err:.5f}")
    assert err < TOL, f"max err {err}"


# ---- 4. chunked KV with a padded chunk stride ----------------------------------


@requires_gpu
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize(
    "nc,lc,splits",
    [
        (3, 72, 2),   # 2 tiles: split 1 starts at token 128 = chunk 1, token 56
        (5, 200, 3),  # 8 tiles: splits start at tokens 256 and 640, both mid-chunk, each
                      # followed by in-chunk and chunk-straddling tiles and, last, the tail
        (2, 512, 4),  # every split is full in-chunk tiles: descriptor path, non-zero cursor
    ],
)
def test_split_chunked_kv(nc, lc, splits, b):
    torch.manual_seed(nc * 1000 + lc + b)
    heads, dim_head, lq = 2, 64, 33
    inner = heads * dim_head
    q = _randn(b, lq, inner)
    slot = b * lc * 2 * inner
    buf = _randn(nc, slot + 64)
    kv_chunks = buf[:, :slot].view(nc, b, lc, 2 * inner)
    out = ops.flash_attention_chunked(q, kv_chunks, heads, dim_head, kv_splits=splits).float()

    full = kv_chunks.permute(1, 0, 2, 3).reshape(b, nc * lc, 2 * inner).float()
    kf, vf = full.split(inner, dim=-1)
    qf = q.float().view(b, lq, heads, dim_head).transpose(1, 2)
    kf = kf.view(b, nc * lc, heads, dim_head).transpose(1, 2)
    vf = vf.view(b, nc * lc, heads, dim_head).transpose(1, 2)
    ref = eager.flash_attention(qf, kf, vf).transpose(1, 2).reshape(b, lq, inner)
    err = (out - ref).abs().max().item()
    print(f"nc={nc} lc={lc} S={splits} b={b}: max err {err:.5f}")
    assert err < TOL, f"nc={nc} lc={lc} S={splits} b={b}: max err {err}"
    # the 5-D views the chunked op builds, with the lse
    k5 = kv_chunks[..., :inner].unflatten(-1, (heads, dim_head)).permute(1, 3, 0, 2, 4)
    v5 = kv_chunks[..., inner:].unflatten(-1, (heads, dim_head)).permute(1, 3, 0, 2, 4)
    q4 = q.view(b, lq, heads, dim_head).permute(0, 2, 1, 3)
    _, lse = ops.flash_attention(q4, k5, v5, kv_splits=splits, return_lse=True)
    _, ref_lse = eager.flash_attention_lse(qf, kf, vf)
    assert (lse - ref_lse).abs().max().item() < LSE_TOL


# ---- 5. partial Q blocks ---------------------------------------------------------


@requires_gpu
@pytest.mark.parametrize("lq", [1, 257])
def test_split_partial_q_blocks_store_nothing_past_lq(lq):
    """The raw partial entry writes into caller buffers: they are carved out of
    sentinel-filled allocations, so a store for a row >= Lq of the last
    (split, batch, head) lands in the guard zone behind them."""
    torch.manual_seed(lq)
    h, d, lkv, splits, guard = 2, 64, 320, 2, 4096
    q, k, v = _randn(1, h, lq, d), _randn(1, h, lkv, d), _randn(1, h, lkv, d)
    sentinel = 12345.0
    n_o, n_l = splits * lq * h * d, splits * h * lq
    o_buf = torch.full((n_o + guard,), sentinel, device=_dev())
    l_buf = torch.full((n_l + guard,), sentinel, device=_dev())
    o_part = o_buf[:n_o].view(splits, 1, lq, h, d)
    lse_part = l_buf[:n_l].view(splits, 1, h, lq)
    used = ops.hip_ext().flash_attention_partial(q, k, v, splits, o_part, lse_part)
    assert used == splits
    assert (o_buf[n_o:] == sentinel).all(), "partial O written past the last valid row"
    assert (l_buf[n_l:] == sentinel).all(), "lse written past the last valid row"
    assert not (o_part == sentinel).any() and not (lse_part == sentinel).any(), "rows left unwritten"
    assert torch.isfinite(lse_part).all() and lse_part.numel() == splits * h * lq

    out, lse = ops.merge_attention(o_part, lse_part, out_dtype=torch.bfloat16, return_lse=True)
    ref, ref_lse = _ref(q, k, v)
    err = (out.float().transpose(1, 2) - ref).abs().max().item()
    print(f"lq={lq}: max err {err:.5f}")
    assert err < TOL
    assert (lse - ref_lse).abs().max().item() < LSE_TOL
    _check_split(q, k, v, splits, f"lq={lq} S={splits}")


# ---- 6. padded head dims ---------------------------------------------------------


@requires_gpu
@pytest.mark.parametrize("d", [40, 80, 160])
def test_split_padded_head_dims(d):
    torch.manual_seed(d)
    _check_split(_randn(1, 2, 33, d), _randn(1, 2, 200, d), _randn(1, 2, 200, d), 2, f"d={d} S=2")


# ---- 7. the merge kernel against eager -------------------------------------------


@requires_gpu
@pytest.mark.parametrize("d", [64, 40])
def test_merge_attention_matches_eager(d):
    torch.manual_seed(d)
    s, b, h, lq = 3, 2, 2, 33
    o_parts = torch.randn(s, b, lq, h, d, device=_dev())
    lse_parts = torch.randn(s, b, h, lq, device=_dev()) * 3
    o_parts[1] = float("nan")  # an empty part may hold anything
    lse_parts[1] = -math.inf
    lse_parts[:, 0, 0, 0] = -math.inf  # one row with no KV at all
    ref, ref_lse = eager.merge_attention(o_parts.cpu(), lse_parts.cpu())

    out32, lse = ops.merge_attention(o_parts, lse_parts, return_lse=True)
    assert out32.dtype == torch.float32 and out32.shape == (b, lq, h, d)
    assert not torch.isnan(out32).any() and not torch.isnan(lse).any()
    assert (out32[0, 0, 0] == 0).all() and lse[0, 0, 0] == -math.inf
    err32 = (out32.cpu() - ref).abs().max().item()
    finite = torch.isfinite(ref_lse)
    assert torch.equal(torch.isfinite(lse).cpu(), finite)
    lse_err = (lse.cpu()[finite] - ref_lse[finite]).abs().max().item()
    print(f"merge d={d}: fp32 out err {err32:.2e}, lse err {lse_err:.2e}")
    assert err32 < MERGE_LSE_TOL and lse_err < MERGE_LSE_TOL

    out16 = ops.merge_attention(o_parts, lse_parts, out_dtype=torch.bfloat16)
    assert out16.dtype == torch.bfloat16
    assert (out16.float().cpu() - ref).abs().max().item() < TOL
    assert torch.equal(out16, out32.to(torch.bfloat16)), "bf16 store is the rounded fp32 result"


# ---- 8. determinism ----------------------------------------------------------------


@requires_gpu
def test_split_is_deterministic_and_lse_leaves_the_output_alone():
    torch.manual_seed(8)
    q, k, v = _randn(2, 2, 300, 64), _randn(2, 2, 1000, 64), _randn(2, 2, 1000, 64)
    o1, l1 = ops.flash_attention(q, k, v, kv_splits=3, return_lse=True)
    o2, l2 = ops.flash_attention(q, k, v, kv_splits=3, return_lse=True)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    plain = ops.flash_attention(q, k, v)
    o_lse, _ = ops.flash_attention(q, k, v, kv_splits=1, return_lse=True)
    assert torch.equal(o_lse, plain)


# ---- 9. graph capture ----------------------------------------------------------------


def _graph_nodes_and_edges(graph_handle):
    """(node count, [(from, to)]) of a captured graph, read with the HIP
    runtime torch itself has loaded (hipGraphGetNodes / hipGraphGetEdges)."""
    import ctypes

    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, f"expected one loaded HIP runtime, found {paths}"
    hip = ctypes.CDLL(paths.pop())
    vp, szp = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, vp, szp]
    hip.hipGraphGetNodes.restype = ctypes.c_int
    hip.hipGraphGetEdges.argtypes = [ctypes.c_void_p, vp, vp, szp]
    hip.hipGraphGetEdges.restype = ctypes.c_int
    graph = ctypes.c_void_p(graph_handle)
    n_nodes, n_edges = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n_nodes)) == 0
    assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(n_edges)) == 0
    src = (ctypes.c_void_p * max(n_edges.value, 1))()
    dst = (ctypes.c_void_p * max(n_edges.value, 1))()
    assert hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(n_edges)) == 0
    return n_nodes.value, [(src[i], dst[i]) for i in range(n_edges.value)]


@requires_gpu
def test_split_call_under_graph_capture():
    torch.manual_seed(9)
    q, k, v = _randn(1, 2, 300, 64), _randn(1, 2, 640, 64), _randn(1, 2, 640, 64)
    eager_out, eager_lse = ops.flash_attention(q, k, v, kv_splits=2, return_lse=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)  # keeps the captured graph for inspection
    with torch.cuda.graph(g):
        out, lse = ops.flash_attention(q, k, v, kv_splits=2, return_lse=True)
    n_nodes, edges = _graph_nodes_and_edges(g.raw_cuda_graph())
    g.instantiate()
    out.zero_()
    lse.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_out) and torch.equal(lse, eager_lse)

    # one linear chain: N nodes, N - 1 edges, no node with two successors or
    # two predecessors
    print(f"captured graph: {n_nodes} nodes, {len(edges)} edges")
    assert n_nodes >= 2, "the partial and the merge kernel are two nodes"
    assert len(edges) == n_nodes - 1, "not a single chain"
    assert len({a for a, _ in edges}) == len(edges), "a node with two successors: parallel branches"
    assert len({b for _, b in edges}) == len(edges), "a node with two predecessors: a join"


# ---- 10. module level -------------------------------------------------------------------


def _unet_out(model_cfg, height, splits, ehs_dim, added):
    from distrifuser_amd import DistriConfig
    from distrifuser_amd.models import DistriUNet

    kw = {} if splits is None else {"attn_kv_splits": splits}
    cfg = DistriConfig(height=height, width=height, do_classifier_free_guidance=False,
                       use_cuda_graph=False, device="cuda:0", **kw)
    torch.manual_seed(0)
    unet = DistriUNet(model_cfg, cfg).to(device="cuda:0", dtype=torch.bfloat16).eval()
    gen = torch.Generator("cuda:0").manual_seed(1)
    n = height // 8
    x = torch.randn(1, 4, n, n, device="cuda:0", dtype=torch.bfloat16, generator=gen)
    ehs = torch.randn(1, 7, ehs_dim, device="cuda:0", dtype=torch.bfloat16, generator=gen)
    with torch.no_grad():
        unet.set_counter(0)
        return unet(x, 500.0, ehs, added).float()


@requires_gpu
def test_unet_with_kv_splits_matches_default(monkeypatch):
    """attn_kv_splits=4 against the default through DistriUNet, at the
    tolerance of the graph-versus-eager parity test (tests/test_gpu_pipeline.py):
    the tiny preset (its head_dim-16 attention rides the eager path, where the
    knob is a no-op) and a two-block U-Net with 64-wide heads at 32 x 32
    latents, whose 1024- and 256-token self-attentions do split."""
    from distrifuser_amd.models.unet import TINY_UNET, UNetConfig

    monkeypatch.delenv("DFA_ATTN_KV_SPLITS", raising=False)
    gen = torch.Generator("cuda:0").manual_seed(2)
    added = {
        "text_embeds": torch.randn(1, 16, device="cuda:0", dtype=torch.bfloat16, generator=gen),
        "time_ids": torch.tensor([[128, 128, 0, 0, 128, 128]], device="cuda:0",
                                 dtype=torch.bfloat16),
    }
    d64 = UNetConfig(
        block_out_channels=(64, 128),
        down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
        layers_per_block=1,
        transformer_layers_per_block=(1, 1),
        num_attention_heads=(1, 2),
        cross_attention_dim=64,
        norm_num_groups=8,
        use_linear_projection=True,
        addition_embed_type=None,
        sample_size=32,
    )
    seen = []
    real = ops.flash_attention

    def recording(q, k, v, **kw):
        seen.append((q.shape[-1], k.shape[-2], kw.get("kv_splits", 1)))
        return real(q, k, v, **kw)

    monkeypatch.setattr(ops, "flash_attention", recording)
    for name, model_cfg, height, ehs_dim, kwargs in (
        ("tiny", TINY_UNET, 128, 32, added),
        ("d64", d64, 256, 64, None),
    ):
        base = _unet_out(model_cfg, height, None, ehs_dim, kwargs)
        assert all(s == 1 for _, _, s in seen), "the default must not split"
        split = _unet_out(model_cfg, height, 4, ehs_dim, kwargs)
        if name == "d64":  # self-attention got the knob, cross-attention (Lkv 7) did not
            assert (64, 1024, 4) in seen and (64, 256, 4) in seen
            assert all(s == 1 for _, lkv, s in seen if lkv == 7)
        seen.clear()
        assert torch.isfinite(base).all() and torch.isfinite(split).all()
        err = (split - base).abs().max().item()
        print(f"{name}: kv_splits=4 vs default max diff {err:.5f}")
        assert err < 0.05, f"{name}: attn_kv_splits=4 drifted from the default: {err}"
