"""The e4m3 attention kernels (csrc/attention_fp8.hip) on the GPU, called through
ops.hip_ext() so that nothing can fall back to eager. K and V are always the
strided halves of a fused to_kv output; "chunked" cases read them from NC = 3
stale-KV slots of LC = 40 tokens with NaN between the slots.

Run on an MI355X box: pytest tests/test_fp8_attention_gpu.py -m gpu -q -s"""

import pytest
import torch

from distrifuser_amd import ops
from distrifuser_amd.ops import eager

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300),
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")]

B, H, D = 2, 2, 64
DTYPES = [torch.bfloat16, torch.float16]
# (Lkv, chunks): every tail, slab and block boundary of the 128-token tile
KV_SHAPES = [(n, 1) for n in (1, 31, 64, 127, 128, 129, 257)] + [(120, 3)]


def attention64(q, k, v):
    """float64 softmax(q k^T / sqrt(d)) v -> (o, sum p|v| / sum p); [B,H,L,D] in."""
    q, k, v = q.double(), k.double(), v.double()
    p = torch.softmax(torch.einsum("bhqd,bhkd->bhqk", q, k) * q.shape[-1] ** -0.5, dim=-1)
    return p @ v, p @ v.abs()


def run_fp8(q, k, v, chunks):
    """q [B,H,Lq,D], k/v [B,H,Lkv,D] on the CPU -> the kernel's [B,H,Lq,D] there.
    K and V reach the kernel as views of one [chunks, B, LC, 2*H*D] buffer."""
    lkv, dev = k.shape[2], "cuda:0"
    kv = torch.cat([k.transpose(1, 2).reshape(B, lkv, H * D),
                    v.transpose(1, 2).reshape(B, lkv, H * D)], dim=-1)
    slot = B * (lkv // chunks) * 2 * H * D
    buf = torch.full((chunks, slot + 64), float("nan"), dtype=q.dtype, device=dev)
    buf[:, :slot] = kv.view(B, chunks, lkv // chunks, -1).transpose(0, 1).reshape(chunks, slot)
    view = buf[:, :slot].view(chunks, B, lkv // chunks, 2 * H * D)
    kg, vg = (t.unflatten(-1, (H, D)).permute(1, 3, 0, 2, 4)
              for t in (view[..., :H * D], view[..., H * D:]))
    if chunks == 1:
        kg, vg = kg[:, :, 0], vg[:, :, 0]
    # q as the strided slice of a fused projection, like k and v
    qg = torch.cat([q, q], dim=-1).to(dev)[..., :D]
    return ops.hip_ext().flash_attention_fp8(qg, kg, vg).cpu()


def block_scaled_ints(lkv, dtype, zeros=True):
    """V [B,H,lkv,D]: integers in [-3, 3] (without 0 if not zeros) times 2^e, e
    in [-6, 6] drawn per (channel, 32-token block): exact in e4m3 under the
    block scale, and any sum of them over <= 512 tokens is exact in fp32
    (12 + 2 + 9 bits)."""
    nb = -(-lkv // 32)
    e = torch.randint(-6, 7, (B, H, nb, 1, D)).expand(B, H, nb, 32, D).reshape(B, H, nb * 32, D)
    n = torch.randint(-3, 4, (B, H, lkv, D))
    if not zeros:
        n = torch.where(n == 0, torch.ones_like(n), n)
    return torch.ldexp(n.float(), e[:, :, :lkv]).to(dtype)


@pytest.mark.parametrize("opsel_a,opsel_b", [(0, 0), (1, 2), (2, 3), (3, 1)])
def test_scaled_mfma_layout(opsel_a, opsel_b):
    """A[row = l&31][k = 32*(j>>4) + 16*(l>>5) + (j&15)] for byte j of lane l, B
    likewise by column; k-block b (32 k-elements) takes byte op_sel of the
    scale dword of the lane in half b; D as the bf16 32x32 MFMA. Scale
    exponents: a per-row part in [-6, 4] plus 0..2 per k-block, so every D
    element is exact in fp32."""
    torch.manual_seed(opsel_a * 4 + opsel_b)
    frag, scale, mats = [], [], []
    for opsel in (opsel_a, opsel_b):
        x = torch.randint(-3, 4, (32, 64)).float()
        e = torch.randint(-6, 5, (32, 1)) + torch.randint(0, 3, (32, 2))  # [row, k-block]
        mats.append(torch.ldexp(x, e.repeat_interleave(32, dim=1)).double())
        lanes = x.view(32, 2, 2, 16).permute(2, 0, 1, 3).reshape(64, 32)  # [half, row][block, 16]
        frag.append(lanes.to(torch.float8_e4m3fn).view(torch.uint8).view(torch.int32))
        sb = torch.full((64, 4), 127 + 7, dtype=torch.uint8)  # the bytes not selected
        sb[:, opsel] = (e.t().reshape(64) + 127).to(torch.uint8)
        scale.append(sb.view(torch.int32).reshape(64))
    d = ops.hip_ext().mfma_probe_fp8(*(t.contiguous().cuda() for t in (*frag, *scale)),
                                     opsel_a, opsel_b)[0].cpu()
    want = mats[0] @ mats[1].t()
    lane, r = torch.arange(64)[:, None], torch.arange(16)[None, :]
    assert torch.equal(d.double(), want[(r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), lane & 31])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lkv,chunks", KV_SHAPES)
def test_uniform_softmax_is_the_exact_mean(lkv, chunks, dtype):
    """Q = 0: every p is 1 (256 in e4m3, exact), so O is the mean of V, every
    sum exact, one correctly rounded division and the output rounding."""
    torch.manual_seed(lkv)
    v = block_scaled_ints(lkv, dtype)
    k = torch.randn(B, H, lkv, D).to(dtype)
    out = run_fp8(torch.zeros(B, H, 33, D, dtype=dtype), k, v, chunks)
    want = (v.double().mean(dim=2, keepdim=True)).float().to(dtype).expand_as(out)
    assert torch.equal(out, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lkv,chunks", [(129, 1), (257, 1), (120, 3)])
def test_exact_gather(lkv, chunks, dtype):
    """K rows in {-1, 1}^64 and q = 16 k_sel (all e4m3-exact): the selected
    token's scaled score leads every other by >= 40 nats, so its p is 1, the
    others' are 0 in e4m3 and in the fp32 sum, and O is V[sel] bit for bit. sel
    runs over the first / last token of a 32-block, a 64-slab, the tile, the
    tail and the stale chunks. V has no zero: what the online softmax summed
    before it met the selected token stays in O under an fp32 factor below
    e^-40, far under half an ulp of any entry but a zero."""
    torch.manual_seed(lkv + 1)
    sel = [t for t in (0, 31, 32, 63, 64, 39, 40, 79, 80, 127, 128, 255, 256, lkv - 1) if t < lkv]
    sel = torch.tensor((sel * 33)[:33])
    k = (torch.randint(0, 2, (B, H, lkv, D)) * 2 - 1).to(dtype)
    q = 16 * k[:, :, sel]
    v = block_scaled_ints(lkv, dtype, zeros=False)
    s = torch.einsum("bhqd,bhkd->bhqk", q.double(), k.double()) / 8
    top2 = s.topk(2, dim=-1).values
    assert (top2[..., 0] - top2[..., 1] >= 40).all(), "the inputs do not separate the scores"
    assert torch.equal(run_fp8(q, k, v, chunks), v[:, :, sel])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lkv,chunks", KV_SHAPES)
@pytest.mark.parametrize("lq", [1, 33, 257])
def test_bounded_against_float64_on_the_twins_operands(lq, lkv, chunks, dtype):
    """randn inputs against float64 attention on the operands the twin
    dequantises. Per element, from the rule: e4m3 rounding of p (relative 2^-4)
    plus fp32 score / exp error (2^-10); p below the e4m3 subnormal half step
    (2^-18 each, Lkv of them); the output rounding (2^-8 relative):
    |o - o64| <= (2^-4 + 2^-10) sum p|v| / sum p + Lkv 2^-18 max|v| + 2^-8 |o64|."""
    torch.manual_seed(lq * 1000 + lkv)
    q, k, v = (torch.randn(B, H, n, D).to(dtype) for n in (lq, lkv, lkv))
    qd, kd, vd = eager.fp8_attention_operands(q, k, v)
    o64, pav = attention64(qd, kd, vd)
    bound = (2.0 ** -4 + 2.0 ** -10) * pav + lkv * 2.0 ** -18 * vd.abs().max() + 2.0 ** -8 * o64.abs()
    err = (run_fp8(q, k, v, chunks).double() - o64).abs()
    print(f"lq={lq} lkv={lkv}x{chunks}: max err {err.max():.5f}, mean bound {bound.mean():.5f}")
    assert (err <= bound).all()


def test_faithful_to_true_attention():
    """rel-L2 to float64 attention on the ORIGINAL inputs, L = 512: the kernel
    within 1.25 x the twin's own distance (exp-ulp flips of an e4m3 rounding,
    summation order)."""
    torch.manual_seed(512)
    q, k, v = (torch.randn(B, H, 512, D).to(torch.bfloat16) for _ in range(3))
    o64, _ = attention64(q, k, v)
    dist = [((o.double() - o64).norm() / o64.norm()).item()
            for o in (run_fp8(q, k, v, 1), eager.flash_attention_fp8(q, k, v))]
    print(f"rel-L2 to float64 attention: kernel {dist[0]:.5f}, twin {dist[1]:.5f}")
    assert dist[0] <= 1.25 * dist[1]


def test_dispatch_reaches_the_kernel():
    """ops.flash_attention(compute_dtype="fp8") and the chunked entry return
    the kernel's bits for bf16 head_dim 64 on the GPU."""
    torch.manual_seed(3)
    q = torch.randn(B, 40, H * D, device="cuda:0", dtype=torch.bfloat16)
    kv = torch.randn(3, B, 40, 2 * H * D, device="cuda:0", dtype=torch.bfloat16)
    q4 = q.view(B, 40, H, D).transpose(1, 2)
    k, v = (t.unflatten(-1, (H, D)).permute(1, 3, 0, 2, 4)
            for t in (kv[..., :H * D], kv[..., H * D:]))
    want = ops.hip_ext().flash_attention_fp8(q4, k, v)
    got = ops.flash_attention_chunked(q, kv, H, D, compute_dtype="fp8")
    assert torch.equal(got, want.transpose(1, 2).reshape(B, 40, H * D))
    assert torch.equal(ops.flash_attention(q4, k[:, :, 0], v[:, :, 0], compute_dtype="fp8"),
                       ops.hip_ext().flash_attention_fp8(q4, k[:, :, 0], v[:, :, 0]))
