"""fp16 through the whole model on one GPU: a DistriUNet forward makes the same
native kernel calls in fp16 as in bf16 (no new fallback) and is no further
from an fp32 eager run of the same weights; the tiny SDXL pipeline runs in
fp16 with a hipGraph.

Run on an MI355X box: pytest tests/test_fp16_pipeline_gpu.py -m gpu -q -s"""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

COUNTED = ("flash_attention", "flash_attention_ext", "conv3x3", "layer_norm", "add_layer_norm")


@requires_gpu
def test_unet_fp16_runs_the_same_native_kernels_as_bf16(monkeypatch):
    from distrifuser_amd import DistriConfig, ops
    from distrifuser_amd.models import DistriUNet
    from distrifuser_amd.models.unet import UNetConfig

    # the two-block U-Net of tests/test_gpu_pipeline.py: 64-wide heads, so the
    # flash kernel is on the path
    cfg_model = UNetConfig(
        block_out_channels=(64, 128),
        down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"),
        layers_per_block=1,
        transformer_layers_per_block=(1, 1),
        num_attention_heads=(1, 2),
        cross_attention_dim=64,
        norm_num_groups=8,
        use_linear_projection=True,
        addition_embed_type=None,
        sample_size=16,
    )
    ext = ops.hip_ext()
    counts = {}
    for name in COUNTED:
        real = getattr(ext, name)

        def counted(*a, _real=real, _name=name, **kw):
            counts[_name] = counts.get(_name, 0) + 1
            return _real(*a, **kw)

        monkeypatch.setattr(ext, name, counted)

    cfg = DistriConfig(height=128, width=128, do_classifier_free_guidance=False,
                       use_cuda_graph=False, device="cuda:0")
    torch.manual_seed(0)
    weights = DistriUNet(cfg_model, cfg).state_dict()  # fp32, shared by the three runs
    x32 = torch.randn(1, 4, 16, 16, device="cuda:0",
                      generator=torch.Generator("cuda:0").manual_seed(1))
    ehs32 = torch.randn(1, 7, 64, device="cuda:0",
                        generator=torch.Generator("cuda:0").manual_seed(2))

    def run(dtype, eager):
        if eager:
            monkeypatch.setenv("DFA_FORCE_EAGER", "1")
        else:
            monkeypatch.delenv("DFA_FORCE_EAGER", raising=False)
        unet = DistriUNet(cfg_model, cfg)
        unet.load_state_dict(weights)
        unet = unet.to(device="cuda:0", dtype=dtype).eval()
        counts.clear()
        with torch.no_grad():
            unet.set_counter(0)
            out = unet(x32.to(dtype), 500.0, ehs32.to(dtype), None).float()
        return out, dict(counts)

    ref, ref_counts = run(torch.float32, eager=True)
    assert not ref_counts, f"the eager run reached native kernels: {ref_counts}"
    out_b, counts_b = run(torch.bfloat16, eager=False)
    out_h, counts_h = run(torch.float16, eager=False)
    print(f"native calls bf16 {counts_b}  fp16 {counts_h}")
    assert counts_b.get("conv3x3", 0) > 0 and counts_b.get("flash_attention", 0) > 0
    assert counts_b.get("layer_norm", 0) + counts_b.get("add_layer_norm", 0) > 0
    assert counts_h == counts_b, "fp16 fell off a native kernel that bf16 takes"
    assert torch.isfinite(out_h).all()
    err_b = (out_b - ref).abs().max().item()
    err_h = (out_h - ref).abs().max().item()
    print(f"U-Net vs fp32 eager: fp16 err {err_h:.5f}  bf16 err {err_b:.5f}")
    assert err_h <= err_b, f"fp16 U-Net err {err_h} above bf16's {err_b}"


@requires_gpu
def test_tiny_sdxl_fp16_graph_vs_eager():
    """As test_tiny_sdxl_gpu_graph_vs_eager of tests/test_gpu_pipeline.py, with
    torch_dtype=torch.float16: finite latents, and the hipGraph replay held to
    the same 0.05 against the eager fp16 steps."""
    from distrifuser_amd import DistriConfig, DistriSDXLPipeline

    outs = {}
    for use_graph in (False, True):
        cfg = DistriConfig(height=128, width=128, use_cuda_graph=use_graph, device="cuda:0")
        torch.manual_seed(0)
        pipe = DistriSDXLPipeline.from_pretrained(cfg, preset="tiny", torch_dtype=torch.float16)
        g = torch.Generator().manual_seed(5)
        out = pipe("graph parity", num_inference_steps=4, output_type="latent", generator=g)
        assert out.dtype == torch.float16 and out.shape == (1, 4, 16, 16)
        outs[use_graph] = out.float()
        assert torch.isfinite(outs[use_graph]).all()
    err = (outs[True] - outs[False]).abs().max().item()
    print(f"fp16 graph vs eager: {err:.5f}")
    assert err < 0.05, f"graph-replay output drifted from eager: {err}"
