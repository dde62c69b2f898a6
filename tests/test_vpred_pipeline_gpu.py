"""v-prediction with guidance_rescale through both pipelines on one GPU: finite
latents, and every denoise step makes one factor call and one fused step call
on the extension (none of the factor at guidance_rescale=0).

Run on an MI355X box: pytest tests/test_vpred_pipeline_gpu.py -m gpu -q -s"""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

STEPS = 4
STEP_OPS = ("cfg_affine_step", "cfg_dpm_step", "masked_affine_step", "masked_dpm_step")


def _counted(monkeypatch):
    from distrifuser_amd import ops

    ext = ops.hip_ext()
    counts = {}
    for name in ("guidance_rescale_factor", *STEP_OPS):
        real = getattr(ext, name)

        def counted(*a, _real=real, _name=name, **kw):
            counts[_name] = counts.get(_name, 0) + 1
            return _real(*a, **kw)

        monkeypatch.setattr(ext, name, counted)
    return counts


@requires_gpu
@pytest.mark.parametrize("scheduler,step_op", [("ddim", "cfg_affine_step"),
                                               ("dpm-solver", "cfg_dpm_step")])
@pytest.mark.parametrize("sdxl", [False, True], ids=["sd", "sdxl"])
def test_v_prediction_with_guidance_rescale(sdxl, scheduler, step_op, monkeypatch):
    from distrifuser_amd import DistriConfig, DistriSDPipeline, DistriSDXLPipeline

    monkeypatch.delenv("DFA_FORCE_EAGER", raising=False)
    cls = DistriSDXLPipeline if sdxl else DistriSDPipeline
    cfg = DistriConfig(height=64, width=64, use_cuda_graph=False, device="cuda:0")
    torch.manual_seed(0)
    pipe = cls.from_pretrained(cfg, preset="tiny", torch_dtype=torch.bfloat16,
                               scheduler=scheduler, prediction_type="v_prediction")
    assert pipe.scheduler.prediction_type == "v_prediction"
    counts = _counted(monkeypatch)

    def run(**kw):
        counts.clear()
        out = pipe("a prompt", num_inference_steps=STEPS, output_type="latent",
                   generator=torch.Generator().manual_seed(3), **kw)
        assert out.dtype == torch.bfloat16 and out.shape == (1, 4, 8, 8)
        assert torch.isfinite(out.float()).all()
        return out.float(), dict(counts)

    plain, plain_counts = run(guidance_rescale=0.0)
    assert plain_counts == {step_op: STEPS}, plain_counts
    rescaled, rescaled_counts = run(guidance_rescale=0.7)
    assert rescaled_counts == {"guidance_rescale_factor": STEPS, step_op: STEPS}, rescaled_counts
    assert not torch.equal(rescaled, plain)
    print(f"{cls.__name__}/{scheduler}: |rescaled - plain| max "
          f"{(rescaled - plain).abs().max().item():.4f}")


@requires_gpu
def test_inpaint_with_guidance_rescale(monkeypatch):
    from distrifuser_amd import DistriConfig, DistriSDPipeline

    monkeypatch.delenv("DFA_FORCE_EAGER", raising=False)
    cfg = DistriConfig(height=64, width=64, use_cuda_graph=False, device="cuda:0")
    torch.manual_seed(0)
    pipe = DistriSDPipeline.from_pretrained(cfg, preset="tiny", torch_dtype=torch.bfloat16,
                                            prediction_type="v_prediction")
    counts = _counted(monkeypatch)
    image = torch.rand(3, 64, 64, generator=torch.Generator().manual_seed(1))
    mask = torch.zeros(64, 64)
    mask[:32] = 1.0
    out = pipe("a prompt", num_inference_steps=STEPS, output_type="latent", image=image,
               mask=mask, generator=torch.Generator().manual_seed(3), guidance_rescale=0.7)
    assert torch.isfinite(out.float()).all()
    assert counts == {"guidance_rescale_factor": STEPS, "masked_affine_step": STEPS}, counts
