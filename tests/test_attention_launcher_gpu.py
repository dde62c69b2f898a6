"""The two bindings of the plain flash-attention kernel reach one launcher and
one instantiation: flash_attention(q, k, v) and flash_attention_ext(q, k, v,
1, False)[0] must agree bit for bit. Shapes: one row and more than one block
of queries; KV below, above and at a multiple of the 128-token tile; padded
and full head dims of the smallest and the largest DPAD.

Run on an MI355X box: pytest tests/test_attention_launcher_gpu.py -m gpu -q"""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

if torch.cuda.is_available():
    from distrifuser_amd import ops
else:  # collected on CPU boxes but never run
    ops = None

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_flash_attention_equals_ext_one_split(dtype):
    ext = ops.hip_ext()
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    for lq in (1, 257):
        for lkv in (127, 129, 384):
            for d in (40, 64, 160):
                q = torch.randn(1, 2, lq, d, device=dev).to(dtype)
                k = torch.randn(1, 2, lkv, d, device=dev).to(dtype)
                v = torch.randn(1, 2, lkv, d, device=dev).to(dtype)
                a = ext.flash_attention(q, k, v)
                b = ext.flash_attention_ext(q, k, v, 1, False)[0]
                assert a.shape == b.shape == (1, 2, lq, d) and a.dtype == dtype
                assert torch.isfinite(a.float()).all(), (lq, lkv, d)
                assert torch.equal(a, b), (lq, lkv, d)
