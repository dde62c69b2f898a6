"""The attention route on the GPU: a module's output equals the binding called
by hand on the same [B, H, L, D] views of its projections, bit for bit, under
each knob; ops.flash_attention_chunked equals the bindings on hand-built
[B, H, NC, LC, D] views into a strided buffer. L = 256 is two 128-token tiles,
so kv_splits = 2 really splits.

Run on an MI355X box: pytest tests/test_attention_route_gpu.py -m gpu -q"""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

if torch.cuda.is_available():
    from distrifuser_amd import ops
    from distrifuser_amd.models.layers import PlainSelfAttention
    from distrifuser_amd.parallel.patch_ops import PatchSelfAttention
    from distrifuser_amd.parallel.state import ParallelState
    from distrifuser_amd.utils.config import DistriConfig
else:  # collected on CPU boxes but never run
    ops = None

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

B, HEADS, D, L, DIM = 2, 2, 64, 256, 64
INNER = HEADS * D
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
KNOBS = {
    "default": {},
    "splits-2": {"attn_kv_splits": 2},
    "fp8": {"attn_dtype": "fp8"},
}


def _by_hand(knob, q, k, v):
    ext = ops.hip_ext()
    if knob == "fp8":
        return ext.flash_attention_fp8(q, k, v)
    if knob == "splits-2":
        return ext.flash_attention_ext(q, k, v, 2, False)[0]
    return ext.flash_attention(q, k, v)


def _heads(t):
    return t.view(t.shape[0], t.shape[1], HEADS, D).transpose(1, 2)


@requires_gpu
@DTYPES
@pytest.mark.parametrize("knob", list(KNOBS))
@pytest.mark.parametrize("module", ["plain", "patch"])
def test_module_equals_binding_by_hand(module, knob, dtype):
    dev = torch.device("cuda:0")
    cfg = DistriConfig(height=64, width=64, use_cuda_graph=False, device=dev, **KNOBS[knob])
    torch.manual_seed(11)
    if module == "plain":
        m = PlainSelfAttention(DIM, HEADS, D, config=cfg)
    else:
        m = PatchSelfAttention(DIM, HEADS, D, state=ParallelState(cfg))
    m = m.to(device=dev, dtype=dtype).eval()
    x = torch.randn(B, L, DIM, device=dev).to(dtype)
    with torch.no_grad():
        got = m(x)
        if module == "plain":
            q, kv = m.to_q(x), m.to_kv(x)
        else:  # the fused GEMM's column slices, read in place
            q, kv = m._qkv(x)
        o = _by_hand(knob, _heads(q), _heads(kv[..., :INNER]), _heads(kv[..., INNER:]))
        want = m.to_out(o.transpose(1, 2).reshape(B, L, INNER))
    assert got.dtype == dtype and torch.isfinite(got.float()).all()
    assert torch.equal(got, want)


@requires_gpu
@DTYPES
@pytest.mark.parametrize("knob", list(KNOBS))
def test_chunked_equals_binding_on_hand_built_views(knob, dtype):
    dev = torch.device("cuda:0")
    torch.manual_seed(12)
    n, lc = 2, 128
    width = B * lc * 2 * INNER
    flat = torch.randn(n, 64 + width + 32, device=dev).to(dtype)
    kv = flat[:, 64:64 + width].view(n, B, lc, 2 * INNER)  # strided: rows of the flat buffer
    q = torch.randn(B, L, INNER, device=dev).to(dtype)
    kw = {"default": {}, "splits-2": {"kv_splits": 2}, "fp8": {"compute_dtype": "fp8"}}[knob]
    got = ops.flash_attention_chunked(q, kv, HEADS, D, **kw)
    k5 = kv[..., :INNER].unflatten(-1, (HEADS, D)).permute(1, 3, 0, 2, 4)
    v5 = kv[..., INNER:].unflatten(-1, (HEADS, D)).permute(1, 3, 0, 2, 4)
    assert k5.data_ptr() == kv.data_ptr() and k5.shape == (B, HEADS, n, lc, D)
    want = _by_hand(knob, _heads(q), k5, v5).transpose(1, 2).reshape(B, L, INNER)
    assert got.dtype == dtype and torch.isfinite(got.float()).all()
    assert torch.equal(got, want)
