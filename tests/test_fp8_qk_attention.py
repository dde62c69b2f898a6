"""The fp8-QK^T / 16-bit-PV rule with K mean-centring (ops.eager.flash_attention_fp8_qk)
against float64 attention, next to the e4m3 twin. The rule has no kernel: the
figures printed here are the ones profiles/attention_fp8_qk_notes.md decided on.

pytest tests/test_fp8_qk_attention.py -q -s"""

import pytest
import torch

from distrifuser_amd.ops import eager

B, H, L, D = 2, 2, 512, 64
DTYPES = [torch.bfloat16, torch.float16]


def rel_l2(o, q, k, v):
    """rel-L2 of o to float64 softmax(q k^T / sqrt(d)) v on the same inputs"""
    q, k, v = q.double(), k.double(), v.double()
    o64 = torch.softmax(torch.einsum("bhqd,bhkd->bhqk", q, k) * D ** -0.5, dim=-1) @ v
    return ((o.double() - o64).norm() / o64.norm()).item()


@pytest.mark.parametrize("dtype", DTYPES)
def test_closer_to_float64_than_the_fp8_twin_and_blind_to_a_channel_offset(dtype):
    """randn: the rule is strictly closer than the e4m3 twin (1.35 x measured,
    not the tenfold a kernel would have needed). A per-channel offset of about
    50 shared by all K tokens: k + c is rounded to the input dtype and the
    reference sees the same rounded k, so the rule meets another draw of the
    same quantisation noise and nothing else; it is held to 1.25 x its
    no-offset distance, the margin the fp8 suite uses between two evaluations
    of one rule. The e4m3 twin, which spends its range on c, gets worse."""
    torch.manual_seed(512)
    q, k, v = (torch.randn(B, H, L, D).to(dtype) for _ in range(3))
    kc = (k.float() + 50 * torch.randn(D)).to(dtype)
    qk, qk_c = (rel_l2(eager.flash_attention_fp8_qk(q, x, v), q, x, v) for x in (k, kc))
    f8, f8_c = (rel_l2(eager.flash_attention_fp8(q, x, v), q, x, v) for x in (k, kc))
    print(f"{dtype}: fp8_qk {qk:.5f} (offset {qk_c:.5f}), fp8 {f8:.5f} (offset {f8_c:.5f})")
    assert qk < f8
    assert qk_c <= 1.25 * qk
    assert f8_c > f8 and qk_c < f8_c


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lkv", [128, 129])
def test_identical_k_rows_give_the_exact_mean_of_v(lkv, dtype):
    """Every K row the same small-integer vector: the tile sums and their
    total are exact, the true division returns the vector, k' = 0, every p is
    1, and with small-integer V the output is the correctly rounded mean."""
    torch.manual_seed(lkv)
    k = torch.randint(-8, 9, (B, H, 1, D)).expand(B, H, lkv, D).to(dtype)
    v = torch.randint(-3, 4, (B, H, lkv, D)).to(dtype)
    assert torch.equal(eager.attention_k_mean(k), k[:, :, 0].float())
    out = eager.flash_attention_fp8_qk(torch.randn(B, H, 33, D).to(dtype), k, v)
    assert torch.equal(out, v.double().mean(2, keepdim=True).float().to(dtype).expand_as(out))
