"""compute_dtype="fp8" off the GPU: the eager twin's rule, argument checks, the
config knob, and a tiny U-Net that takes the fp8 path."""

import dataclasses

import pytest
import torch

from distrifuser_amd import DistriConfig, ops
from distrifuser_amd.models import DistriUNet
from distrifuser_amd.models.unet import TINY_UNET
from distrifuser_amd.ops import eager


def attention64(qd, kd, vd):
    """float64 softmax(q k^T / sqrt(d)) v -> (o, sum p|v| / sum p)."""
    q, k, v = qd.double(), kd.double(), vd.double()
    p = torch.softmax(torch.einsum("bhqd,bhkd->bhqk", q, k) * q.shape[-1] ** -0.5, dim=-1)
    return p @ v, p @ v.abs()


@pytest.mark.parametrize("lq,lkv", [(1, 1), (33, 31), (40, 129), (64, 512)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_twin_against_float64_on_its_operands(lq, lkv, dtype):
    """The twin differs from exact attention on its own dequantised operands
    by the e4m3 rounding of p (relative 2^-4), the fp32 score / exp error
    (2^-10 covers it), p below the e4m3 subnormal half step (2^-18 each) and
    the output rounding (2^-8 relative for bf16):
    |o - o64| <= (2^-4 + 2^-10) sum p|v| / sum p + Lkv 2^-18 max|v| + 2^-8 |o64|."""
    torch.manual_seed(lq * 1000 + lkv)
    q, k, v = (torch.randn(2, 2, n, 64).to(dtype) for n in (lq, lkv, lkv))
    qd, kd, vd = eager.fp8_attention_operands(q, k, v)
    for x, xd in ((q, qd), (k, kd), (v, vd)):  # e4m3 keeps 3 fraction bits
        assert ((xd - x.float()).abs() <= 2.0 ** -4 * x.float().abs().amax() + 1e-30).all()
    o64, pav = attention64(qd, kd, vd)
    bound = (2.0 ** -4 + 2.0 ** -10) * pav + lkv * 2.0 ** -18 * vd.abs().max() + 2.0 ** -8 * o64.abs()
    err = (ops.flash_attention(q, k, v, compute_dtype="fp8").double() - o64).abs()
    print("max err", err.max().item(), "mean bound", bound.mean().item())
    assert (err <= bound).all()


def test_block_exponent_is_ceil_log2():
    amax = torch.tensor([0.0, 448.0, 448.5, 224.0, 225.0, 1.0, 1.75, 1.76, 3e-5, 6e4])
    want = torch.ceil(torch.log2(amax.double() / 448)).to(torch.int32)
    want[0] = 0
    assert torch.equal(eager.fp8_block_exponent(amax), want)


@pytest.mark.parametrize("kwargs", [{"kv_splits": 2}, {"return_lse": True}])
def test_fp8_rejects_splits_and_lse(kwargs):
    q = torch.randn(1, 1, 8, 64)
    with pytest.raises(ValueError):
        ops.flash_attention(q, q, q, compute_dtype="fp8", **kwargs)
    with pytest.raises(ValueError):
        ops.flash_attention(q, q, q, compute_dtype="int8")
    with pytest.raises(ValueError):
        ops.flash_attention_chunked(q[0], q.new_zeros(2, 1, 8, 128), 1, 64, kv_splits=2,
                                    compute_dtype="fp8")


def test_chunked_fp8_is_the_twin_on_the_concatenated_kv():
    torch.manual_seed(0)
    q = torch.randn(2, 16, 128)
    kv = torch.randn(3, 2, 8, 256)
    k, v = (t.reshape(2, 24, 2, 64).transpose(1, 2)
            for t in kv.permute(1, 0, 2, 3).reshape(2, 24, 256).split(128, dim=-1))
    want = eager.flash_attention_fp8(q.view(2, 16, 2, 64).transpose(1, 2), k, v)
    got = ops.flash_attention_chunked(q, kv, 2, 64, compute_dtype="fp8")
    assert torch.equal(got, want.transpose(1, 2).reshape(2, 16, 128))


def test_config_knob_and_environment(monkeypatch):
    kw = dict(use_cuda_graph=False, device="cpu")
    monkeypatch.delenv("DFA_ATTN_DTYPE", raising=False)
    assert DistriConfig(**kw).attn_dtype is None
    assert DistriConfig(attn_dtype="fp8", **kw).attn_compute_dtype(64) == "fp8"
    assert DistriConfig(attn_dtype="fp8", **kw).attn_compute_dtype(40) is None
    monkeypatch.setenv("DFA_ATTN_DTYPE", "FP8")
    assert DistriConfig(**kw).attn_dtype == "fp8"
    monkeypatch.setenv("DFA_ATTN_DTYPE", "")
    assert DistriConfig(**kw).attn_dtype is None
    monkeypatch.setenv("DFA_ATTN_DTYPE", "fp4")
    with pytest.raises(ValueError):
        DistriConfig(**kw)
    with pytest.raises(ValueError):
        DistriConfig(attn_dtype="bf16", **kw)


@torch.no_grad()
def test_tiny_unet_takes_the_fp8_path():
    def run(attn_dtype):
        cfg = DistriConfig(height=128, width=128, do_classifier_free_guidance=False,
                           use_cuda_graph=False, device="cpu", attn_dtype=attn_dtype)
        torch.manual_seed(0)
        # 64 channels over one head: the head dim the knob covers
        unet = DistriUNet(dataclasses.replace(TINY_UNET, num_attention_heads=(2, 1)), cfg).eval()
        sample = torch.randn(1, 4, 16, 16)
        added = {"text_embeds": torch.randn(1, 16),
                 "time_ids": torch.tensor([[128.0, 128, 0, 0, 128, 128]])}
        unet.set_counter(0)
        return unet(sample, 3.0, torch.randn(1, 7, 32), added)

    base, fp8 = run(None), run("fp8")
    assert torch.isfinite(fp8).all() and fp8.shape == base.shape
    rel = ((fp8 - base).norm() / base.norm()).item()
    assert 0 < rel < 0.1, rel
