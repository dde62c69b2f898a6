"""Attention log-sum-exp and the merge of partial attention results on the
CPU reference path, the split-KV policy, and the DistriConfig knob.

The merge tolerance (1e-5) is fp32 arithmetic on O(1) values: randn inputs,
softmax-weighted averages of them, a handful of exp/log/divide roundings."""

import inspect
import math

import pytest
import torch

from distrifuser_amd import DistriConfig, ops
from distrifuser_amd.ops import eager

MERGE_TOL = 1e-5


def _qkv(lq=17, lkv=96, b=2, h=3, d=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (
        torch.randn(b, h, lq, d, generator=g),
        torch.randn(b, h, lkv, d, generator=g),
        torch.randn(b, h, lkv, d, generator=g),
    )


def _parts(q, k, v, bounds):
    """Eager attention over KV slices [bounds[i], bounds[i+1]) stacked as
    merge_attention takes them: o [S, B, Lq, H, D], lse [S, B, H, Lq]."""
    os_, ls_ = [], []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        o, lse = eager.flash_attention_lse(q, k[:, :, lo:hi], v[:, :, lo:hi])
        os_.append(o.transpose(1, 2))
        ls_.append(lse)
    return torch.stack(os_), torch.stack(ls_)


def test_eager_lse_is_logsumexp_of_scaled_scores():
    q, k, v = _qkv()
    out, lse = eager.flash_attention_lse(q, k, v)
    scores = (q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    assert lse.dtype == torch.float32 and lse.shape == q.shape[:3]
    assert torch.allclose(lse, torch.logsumexp(scores, dim=-1), atol=1e-6, rtol=0)
    assert torch.allclose(out, eager.flash_attention(q, k, v), atol=MERGE_TOL, rtol=0)


def test_ops_flash_attention_returns_lse_and_ignores_kv_splits_on_eager():
    q, k, v = _qkv()
    ref_out, ref_lse = eager.flash_attention_lse(q, k, v)
    out, lse = ops.flash_attention(q, k, v, kv_splits=3, return_lse=True)
    assert torch.equal(out, ref_out) and torch.equal(lse, ref_lse)
    assert torch.equal(ops.flash_attention(q, k, v, kv_splits=4), ops.flash_attention(q, k, v))
    with pytest.raises(ValueError):
        ops.flash_attention(q, k, v, kv_splits=0)


@pytest.mark.parametrize("bounds", [(0, 48, 96), (0, 32, 64, 96), (0, 5, 90, 96)])
def test_merged_slices_equal_full_attention(bounds):
    q, k, v = _qkv()
    full, full_lse = eager.flash_attention_lse(q, k, v)
    o_parts, lse_parts = _parts(q, k, v, bounds)
    out, lse = eager.merge_attention(o_parts, lse_parts)
    assert out.shape == (q.shape[0], q.shape[2], q.shape[1], q.shape[3])
    assert (out.transpose(1, 2) - full).abs().max().item() < MERGE_TOL
    assert (lse - full_lse).abs().max().item() < MERGE_TOL
    out2, lse2 = ops.merge_attention(o_parts, lse_parts, return_lse=True)
    assert torch.equal(out2, out) and torch.equal(lse2, lse)
    assert ops.merge_attention(o_parts, lse_parts, out_dtype=torch.bfloat16).dtype == torch.bfloat16


def test_merge_gives_neg_inf_parts_weight_zero():
    q, k, v = _qkv()
    o_parts, lse_parts = _parts(q, k, v, (0, 48, 96))
    ref_out, ref_lse = eager.merge_attention(o_parts, lse_parts)
    # an empty slice in the middle, holding garbage (NaN included) as its output
    junk = torch.full_like(o_parts[0], float("nan"))
    o3 = torch.stack([o_parts[0], junk, o_parts[1]])
    l3 = torch.stack([lse_parts[0], torch.full_like(lse_parts[0], -math.inf), lse_parts[1]])
    out, lse = eager.merge_attention(o3, l3)
    assert torch.equal(out, ref_out) and torch.equal(lse, ref_lse)
    # the eager attention over an empty KV range is such a part
    o_e, lse_e = eager.flash_attention_lse(q, k[:, :, :0], v[:, :, :0])
    assert torch.isneginf(lse_e).all() and (o_e == 0).all()


def test_merge_of_all_neg_inf_parts_is_zeros_not_nan():
    o_parts = torch.randn(3, 2, 5, 2, 8)
    lse_parts = torch.full((3, 2, 2, 5), -math.inf)
    out, lse = eager.merge_attention(o_parts, lse_parts)
    assert (out == 0).all() and torch.isneginf(lse).all()


# ---- the policy ---------------------------------------------------------------


def test_policy_fixed_points():
    f = lambda *a: ops.attention_kv_splits(*a, multi_processor_count=256)
    assert f(1, 10, 57600, 57600, 64) == 1   # the grid already fills the GPU
    assert f(1, 10, 4096, 77, 64) == 1       # cross-attention
    assert f(2, 20, 1024, 77, 64) == 1
    assert f(1, 20, 256, 1024, 64) > 1       # 20 blocks on 512 slots


def test_policy_reads_the_cu_count_from_the_device(monkeypatch):
    class Props:
        multi_processor_count = 256

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda device=None: Props())
    assert ops.attention_kv_splits(1, 20, 256, 1024, 64, "cuda:0") == ops.attention_kv_splits(
        1, 20, 256, 1024, 64, multi_processor_count=256
    )
    Props.multi_processor_count = 8  # a small device is full at once
    assert ops.attention_kv_splits(1, 20, 256, 1024, 64, "cuda:0") == 1


def test_policy_never_exceeds_the_tile_count():
    for d in (40, 64, 80, 128, 160):
        for lkv in (1, 77, 128, 129, 200, 256, 1000, 1024, 4096, 57600):
            for b, h, lq in ((1, 1, 1), (1, 20, 256), (2, 10, 1024), (1, 10, 7200)):
                s = ops.attention_kv_splits(b, h, lq, lkv, d, multi_processor_count=256)
                assert isinstance(s, int) and 1 <= s <= -(-lkv // 128), (b, h, lq, lkv, d, s)


# ---- the knob -----------------------------------------------------------------


def _cfg(**kw):
    return DistriConfig(height=128, width=128, device="cpu", **kw)


def test_knob_default_is_one(monkeypatch):
    monkeypatch.delenv("DFA_ATTN_KV_SPLITS", raising=False)
    assert _cfg().attn_kv_splits == 1
    assert inspect.signature(DistriConfig.__init__).parameters["attn_kv_splits"].default == 1
    assert _cfg().attn_splits(1, 20, 256, 1024, 64) == 1


def test_knob_accepts_ints_and_auto(monkeypatch):
    monkeypatch.delenv("DFA_ATTN_KV_SPLITS", raising=False)
    assert _cfg(attn_kv_splits=4).attn_kv_splits == 4
    assert _cfg(attn_kv_splits=4).attn_splits(1, 20, 256, 1024, 64) == 4
    auto = _cfg(attn_kv_splits="auto")
    assert auto.attn_kv_splits == "auto"
    assert auto.attn_splits(1, 20, 256, 1024, 64) == ops.attention_kv_splits(
        1, 20, 256, 1024, 64, "cpu"
    )
    assert auto.attn_splits(1, 10, 4096, 77, 64) == 1


@pytest.mark.parametrize("bad", [0, -1, "x"])
def test_knob_rejects(bad, monkeypatch):
    monkeypatch.delenv("DFA_ATTN_KV_SPLITS", raising=False)
    with pytest.raises(ValueError):
        _cfg(attn_kv_splits=bad)


def test_knob_environment_applies_only_to_the_default(monkeypatch):
    monkeypatch.setenv("DFA_ATTN_KV_SPLITS", "4")
    assert _cfg().attn_kv_splits == 4
    assert _cfg(attn_kv_splits=2).attn_kv_splits == 2
    assert _cfg(attn_kv_splits=1).attn_kv_splits == 1  # an explicit 1 is not "left at default"
    monkeypatch.setenv("DFA_ATTN_KV_SPLITS", "auto")
    assert _cfg().attn_kv_splits == "auto"
    assert _cfg(attn_kv_splits=3).attn_kv_splits == 3
    monkeypatch.setenv("DFA_ATTN_KV_SPLITS", "x")
    with pytest.raises(ValueError):
        _cfg()
