"""fp16 through the public ops without a GPU: the fp16 weight pack, the fp16
merge output and the eager paths' dtype handling."""

import pytest
import torch

from distrifuser_amd import ops
from distrifuser_amd.ops import conv as conv_ops
from distrifuser_amd.ops import eager


def _exact_weight(cout, cin, seed=0):
    """Values k/8, |k| <= 16: exact in bf16 and in fp16."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-16, 17, (cout, cin, 3, 3), generator=g).float() / 8


def test_pack_fp16_fragment_order():
    cout, cin = 40, 20  # both padded: Cout -> 64, Cin -> 64
    w = _exact_weight(cout, cin)
    wp = conv_ops.pack_conv3x3_weight(w, dtype=torch.float16)
    assert wp.dtype == torch.float16
    assert wp.shape == (9, 4, 2, 64, 8) and wp.is_contiguous()
    # lane l, element j of fragment (tap, ks, ct): cout = ct*32 + (l&31),
    # cin = ks*16 + (l>>5)*8 + j; zero beyond the real channels
    want = torch.zeros(9, 4, 2, 64, 8)
    for ks in range(4):
        for ct in range(2):
            for lane in range(64):
                co = ct * 32 + (lane & 31)
                for j in range(8):
                    ci = ks * 16 + (lane >> 5) * 8 + j
                    if co < cout and ci < cin:
                        want[:, ks, ct, lane, j] = w[co, ci].reshape(9)
    assert torch.equal(wp.float(), want)


def test_pack_fp16_values_equal_default_pack():
    w = _exact_weight(96, 64, seed=1)
    default = conv_ops.pack_conv3x3_weight(w)
    assert default.dtype == torch.bfloat16
    assert torch.equal(conv_ops.pack_conv3x3_weight(w, dtype=None), default)
    assert torch.equal(conv_ops.pack_conv3x3_weight(w, dtype=torch.bfloat16), default)
    half = conv_ops.pack_conv3x3_weight(w, dtype=torch.float16)
    assert half.shape == default.shape
    assert torch.equal(half.float(), default.float())


def test_pack_rejects_other_dtypes():
    with pytest.raises(ValueError, match="bf16 or fp16"):
        conv_ops.pack_conv3x3_weight(_exact_weight(32, 16), dtype=torch.float32)


def test_native_conv_packs_in_fp16_weight_dtype():
    conv = conv_ops.NativeConv2d(16, 32, 3, padding=1)
    assert conv.packed_weight().dtype == torch.bfloat16  # fp32 weights: as before
    conv = conv.to(torch.float16)
    assert conv.packed_weight().dtype == torch.float16
    conv = conv.to(torch.bfloat16)
    assert conv.packed_weight().dtype == torch.bfloat16


def test_merge_attention_fp16_is_fp32_result_rounded():
    torch.manual_seed(2)
    s, b, lq, h, d = 3, 2, 5, 2, 16
    o_parts = torch.randn(s, b, lq, h, d)
    lse_parts = torch.randn(s, b, h, lq)
    lse_parts[1, 0, 0, 0] = float("-inf")
    out32, lse32 = ops.merge_attention(o_parts, lse_parts, return_lse=True)
    out16, lse16 = ops.merge_attention(o_parts, lse_parts, out_dtype=torch.float16,
                                       return_lse=True)
    assert out16.dtype == torch.float16 and lse16.dtype == torch.float32
    assert torch.equal(out16, out32.half())
    assert torch.equal(lse16, lse32)


def test_eager_attention_accepts_fp16():
    torch.manual_seed(3)
    q = torch.randn(1, 2, 9, 40).half()
    k = torch.randn(1, 2, 24, 40).half()
    v = torch.randn(1, 2, 24, 40).half()
    out = ops.flash_attention(q, k, v)
    assert out.dtype == torch.float16 and out.shape == q.shape
    ref = eager.flash_attention(q.float(), k.float(), v.float())
    assert (out.float() - ref).abs().max().item() < 0.03
    out, lse = ops.flash_attention(q, k, v, return_lse=True)
    assert out.dtype == torch.float16 and lse.dtype == torch.float32


def test_eager_chunked_attention_accepts_fp16():
    torch.manual_seed(4)
    b, lq, heads, dh, nc, lc = 1, 9, 2, 40, 3, 8
    inner = heads * dh
    q = torch.randn(b, lq, inner).half()
    kv = torch.randn(nc, b, lc, 2 * inner).half()
    out = ops.flash_attention_chunked(q, kv, heads, dh)
    assert out.dtype == torch.float16 and out.shape == q.shape
    full = kv.permute(1, 0, 2, 3).reshape(b, nc * lc, 2 * inner).float()
    kf, vf = full.split(inner, dim=-1)
    ref = eager.flash_attention(
        q.float().view(b, lq, heads, dh).transpose(1, 2),
        kf.reshape(b, nc * lc, heads, dh).transpose(1, 2),
        vf.reshape(b, nc * lc, heads, dh).transpose(1, 2),
    ).transpose(1, 2).reshape(b, lq, inner)
    assert (out.float() - ref).abs().max().item() < 0.03


def test_eager_layer_norm_and_vae_attention_accept_fp16():
    torch.manual_seed(5)
    x = torch.randn(5, 64).half()
    w, bias = torch.randn(64).half(), torch.randn(64).half()
    y = ops.layer_norm(x, w, bias, 1e-5)
    assert y.dtype == torch.float16 and y.shape == x.shape
    s, y2 = ops.add_layer_norm(x, x, w, bias, 1e-5)
    assert s.dtype == torch.float16 and y2.dtype == torch.float16
    q = torch.randn(1, 12, 512).half()
    out = ops.vae_attention(q, q, q)
    assert out.dtype == torch.float16 and out.shape == q.shape
    ref = eager.vae_attention(q.float(), q.float(), q.float())
    assert (out.float() - ref).abs().max().item() < 0.03


def test_vae_chunked_attention_keeps_cpu_fp32_math():
    """The CPU oracle of the chunked VAE attention stays fp32 whatever comes
    in; only the GPU GEMM dtype follows an fp16 input."""
    from distrifuser_amd.models.vae import _chunked_single_head_attention

    torch.manual_seed(6)
    q = torch.randn(1, 10, 32).half()
    out = _chunked_single_head_attention(q, q, q, chunk=4)
    assert out.dtype == torch.float16
    ref = eager.vae_attention(q.float(), q.float(), q.float())
    # fp32 math on both sides (GEMM blocking may differ by an fp32 ulp), then
    # one rounding to fp16: at most one fp16 ulp apart, 2^-9 for |x| < 4
    assert ref.abs().max().item() < 4.0
    assert (out.float() - ref).abs().max().item() <= 2.0 ** -9
