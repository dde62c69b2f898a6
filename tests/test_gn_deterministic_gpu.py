"""GroupNorm moments are the same bits on every run (csrc/groupnorm.hip: the
blocks of a group store per-chunk sums, and a second kernel adds the chunks in
a fixed order; atomic adds would land in scheduling order). The img2img and
inpaint init latents come from the VAE encoder on every rank, and one last-bit
difference in a moment is enough to move them, so the encoder is held to the
same.

Shapes walk the reduction's paths: one chunk (no second kernel), a few chunks,
more chunks than the 64 lanes of the reducing wave, and the element-wise
(group length not a multiple of the vector width) path. Every group has its
own offset, so a sum filed under the wrong group or chunk slot is far outside
the bound.

Bound against the float64 reference: recursive summation of n fp32 terms in
ANY order errs by at most (n - 1) * u * sum|x_i|, u = 2^-24; the mean adds one
rounding of 1/n, one of the product and one of the output. So
|mean - ref| <= u * sum|x_i| + (2u + u_out) * |ref|, and the same with x_i^2
(whose squares add one more u, inside the first term's slack of a factor n)
for the second moment.

Run on an MI355X box: pytest tests/test_gn_deterministic_gpu.py -m gpu -q"""

import functools

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

DEV = "cuda:0"
U = 2.0 ** -24

# (shape, groups, dtype, chunks the launcher picks: min(ceil(2048 / (N*G)), ceil(nvec / 256)))
CASES = [
    pytest.param((2, 8, 4, 4), 4, torch.float32, 1, id="one-chunk"),
    pytest.param((2, 32, 96, 96), 8, torch.float32, 36, id="36-chunks"),
    pytest.param((1, 8, 256, 256), 1, torch.float32, 512, id="512-chunks"),
    pytest.param((1, 8, 256, 256), 1, torch.bfloat16, 256, id="256-chunks-bf16"),
    pytest.param((1, 6, 33, 35), 2, torch.float32, 14, id="element-wise-14-chunks"),
]


def _chunks(shape, groups, dtype):
    n, c, h, w = shape
    group_len = c // groups * h * w
    v = 16 // torch.empty((), dtype=dtype).element_size()
    nvec = group_len // v if group_len % v == 0 else group_len
    return max(1, min(-(-2048 // (n * groups)), -(-nvec // 256)))


@functools.lru_cache(maxsize=None)
def _case(shape, groups, dtype):
    """Wide dynamic range, so the order of the adds shows in the last bits, and
    a different offset per (sample, group). Shared: never modified."""
    gen = torch.Generator().manual_seed(sum(shape) + groups)
    n, c, h, w = shape
    x = torch.randn(shape, generator=gen) * torch.exp(2 * torch.randn(shape, generator=gen))
    off = torch.arange(1, n * groups + 1, dtype=torch.float32).reshape(n, groups, 1, 1, 1) * 3
    x = (x.reshape(n, groups, c // groups, h, w) + off).reshape(shape).to(dtype)
    xg = x.double().reshape(n, groups, -1)
    return x.to(DEV), xg


@pytest.mark.parametrize("shape,groups,dtype,chunks", CASES)
def test_cases_take_the_paths_they_name(shape, groups, dtype, chunks):
    assert _chunks(shape, groups, dtype) == chunks


@requires_gpu
@pytest.mark.parametrize("shape,groups,dtype,chunks", CASES)
def test_group_norm_stats_same_bits_every_run_and_within_the_order_free_bound(
        shape, groups, dtype, chunks):
    from distrifuser_amd.ops.dispatch import hip_ext

    x, xg = _case(shape, groups, dtype)
    n = shape[0]
    runs = [hip_ext().group_norm_stats(x, groups) for _ in range(20)]
    torch.cuda.synchronize()
    for r in runs[1:]:
        assert torch.equal(r, runs[0]), "moments differ between two runs on the same input"
    got = runs[0].double().cpu().reshape(2, n, groups)
    ref_mean, ref_msq = xg.mean(-1), (xg * xg).mean(-1)
    # the sum, then 1/n (rounded) times it (rounded), then the output's own rounding
    out_u = U if dtype == torch.float32 else 2.0 ** -8
    tol_mean = U * xg.abs().sum(-1) + (2 * U + out_u) * ref_mean.abs()
    tol_msq = U * (xg * xg).sum(-1) + (2 * U + out_u) * ref_msq.abs()
    assert ((got[0] - ref_mean).abs() <= tol_mean).all()
    assert ((got[1] - ref_msq).abs() <= tol_msq).all()


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_two_encoders_give_the_same_moments_bit_for_bit(dtype):
    """Two VAE encoders with the same weights, as two ranks (or two pipelines)
    hold them, encode one image to the same bits, call after call."""
    from distrifuser_amd.models.vae import TINY_VAE, VAEEncoder

    encs = []
    for _ in range(2):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(11)
            encs.append(VAEEncoder(TINY_VAE).to(DEV, dtype).eval())
    x = (torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(2)) * 2 - 1)
    x = x.to(DEV, dtype)
    with torch.no_grad():
        outs = [torch.cat(e.encode_moments(x), dim=1) for e in encs for _ in range(4)]
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0].float()).all()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
