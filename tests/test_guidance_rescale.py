"""guidance_rescale on the CPU: the eager factor against diffusers'
``rescale_noise_cfg`` written out with torch.std, and the plumbing through
both pipelines (the argument, the scheduler config file, the overrides)."""

import json
import os

import pytest
import torch

from distrifuser_amd import DistriConfig, DistriSDPipeline, DistriSDXLPipeline, ops
from distrifuser_amd.ops import eager


def _pair(seed=0, shape=(2, 4, 8, 8), mean=0.0, std=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std + mean


def _rescale_noise_cfg_factor(noise, g, phi):
    """diffusers rescale_noise_cfg in float64: the factor that multiplies cfg."""
    nu, nc = noise.double().chunk(2)
    cfg = nu + g * (nc - nu)
    std_text = nc.std(dim=list(range(1, nc.ndim)), keepdim=True)
    std_cfg = cfg.std(dim=list(range(1, cfg.ndim)), keepdim=True)
    rescaled = cfg * (std_text / std_cfg)
    mixed = phi * rescaled + (1 - phi) * cfg
    return mixed, (phi * std_text / std_cfg + (1 - phi)).reshape(1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mean,std", [(0.0, 1.0), (3.0, 0.5)])
def test_eager_factor_is_rescale_noise_cfg(dtype, mean, std):
    noise = _pair(1, mean=mean, std=std).to(dtype)
    mixed, want = _rescale_noise_cfg_factor(noise, 7.5, 0.7)
    got = ops.guidance_rescale_factor(noise, 7.5, 0.7)
    assert got.dtype == torch.float32 and got.shape == (1,)
    assert abs(float(got) - float(want)) <= 2.0 ** -23 * float(want)
    # and factor * cfg is the rescaled output itself
    eps = eager._cfg_eps(noise, noise[:1], 7.5, got)
    assert torch.allclose(eps.double(), mixed, rtol=1e-5, atol=1e-5)


def test_factor_is_one_where_nothing_is_rescaled():
    noise = _pair(2)
    assert float(ops.guidance_rescale_factor(noise, 7.5, 0.0)) == 1.0
    same = torch.cat([noise[:1], noise[:1]])
    assert float(ops.guidance_rescale_factor(same, 1.0, 0.7)) == pytest.approx(1.0, abs=2e-7)
    with pytest.raises(ValueError):
        ops.guidance_rescale_factor(noise[:1], 7.5, 0.7)
    with pytest.raises(ValueError):  # no CFG pair to take the factor from
        eager._cfg_eps(noise[:1], noise[:1], 7.5, torch.ones(1))


# ---- pipelines ------------------------------------------------------------------------


def _tiny(cls, scheduler="ddim", pretrained=None, **kw):
    size = 128 if cls is DistriSDXLPipeline else 64
    cfg_kw = {k: kw.pop(k) for k in ("do_classifier_free_guidance",) if k in kw}
    cfg = DistriConfig(height=size, width=size, use_cuda_graph=False, device="cpu", **cfg_kw)
    torch.manual_seed(0)
    if pretrained is not None:
        kw["pretrained_model_name_or_path"] = pretrained
    return cls.from_pretrained(cfg, preset="tiny", torch_dtype=torch.float32,
                               scheduler=scheduler, **kw)


def _run(pipe, **kw):
    return pipe("a prompt", num_inference_steps=3, output_type="latent",
                generator=torch.Generator().manual_seed(4), **kw)


PIPES = pytest.mark.parametrize("cls", [DistriSDPipeline, DistriSDXLPipeline],
                                ids=["sd", "sdxl"])


@PIPES
@pytest.mark.parametrize("scheduler", ["ddim", "euler", "dpm-solver"])
def test_guidance_rescale_reaches_the_latents(cls, scheduler):
    # a pipeline per run: the same weights (seeded), no state from an earlier call
    fresh = lambda: _tiny(cls, scheduler, prediction_type="v_prediction")
    assert fresh().scheduler.prediction_type == "v_prediction"
    plain = _run(fresh())
    assert torch.equal(_run(fresh(), guidance_rescale=0.0), plain)
    rescaled = _run(fresh(), guidance_rescale=0.7)
    assert torch.isfinite(rescaled).all()
    assert not torch.equal(rescaled, plain)
    with pytest.raises(ValueError):
        _run(fresh(), guidance_rescale=-0.1)


@PIPES
def test_guidance_rescale_is_ignored_without_cfg(cls):
    pipe = _tiny(cls, do_classifier_free_guidance=False)
    plain = _run(pipe, guidance_scale=1)
    assert torch.equal(_run(pipe, guidance_scale=1, guidance_rescale=0.7), plain)
    with pytest.raises(ValueError):
        _run(pipe, guidance_scale=1, guidance_rescale=-1.0)


@PIPES
def test_inpaint_takes_guidance_rescale(cls):
    pipe = _tiny(cls)
    size = pipe.distri_config.height
    image = torch.rand(3, size, size, generator=torch.Generator().manual_seed(1))
    mask = torch.zeros(size, size)
    mask[: size // 2] = 1.0
    plain = _run(pipe, image=image, mask=mask)
    rescaled = _run(pipe, image=image, mask=mask, guidance_rescale=0.7)
    assert torch.equal(_run(pipe, image=image, mask=mask, guidance_rescale=0.0), plain)
    assert torch.isfinite(rescaled).all() and not torch.equal(rescaled, plain)


@PIPES
def test_scheduler_config_round_trip(cls, tmp_path):
    pipe = _tiny(cls, "euler", prediction_type="v_prediction", timestep_spacing="trailing",
                 rescale_betas_zero_snr=True)
    out = str(tmp_path / "ckpt")
    pipe.save_pretrained(out)
    path = os.path.join(out, "scheduler", "scheduler_config.json")
    with open(path, encoding="utf-8") as f:
        on_file = json.load(f)
    assert on_file["prediction_type"] == "v_prediction"
    assert on_file["timestep_spacing"] == "trailing"
    assert on_file["rescale_betas_zero_snr"] is True
    assert on_file["num_train_timesteps"] == 1000 and on_file["steps_offset"] == 1

    back = _tiny(cls, "ddim", pretrained=out)
    s = back.scheduler
    assert (s.prediction_type, s.timestep_spacing, s.rescale_betas_zero_snr) == (
        "v_prediction", "trailing", True)
    assert torch.equal(s.alphas_cumprod, pipe.scheduler.alphas_cumprod)

    over = _tiny(cls, "ddim", pretrained=out, prediction_type="epsilon")
    assert over.scheduler.prediction_type == "epsilon"
    assert over.scheduler.timestep_spacing == "trailing"  # the file's, not overridden

    # the betas and the offset are read from the file too
    on_file.update(beta_start=0.0001, beta_end=0.02, steps_offset=0)
    with open(path, "w", encoding="utf-8") as f:
        json.dump(on_file, f)
    edited = _tiny(cls, "ddim", pretrained=out, rescale_betas_zero_snr=False).scheduler
    assert (edited.beta_start, edited.beta_end, edited.steps_offset) == (0.0001, 0.02, 0)
    assert not torch.equal(edited.alphas_cumprod[:10], pipe.scheduler.alphas_cumprod[:10])


def test_a_checkpoint_without_the_file_keeps_the_defaults(tmp_path):
    pipe = _tiny(DistriSDPipeline)
    out = str(tmp_path / "ckpt")
    pipe.save_pretrained(out)
    os.remove(os.path.join(out, "scheduler", "scheduler_config.json"))
    s = _tiny(DistriSDPipeline, pretrained=out).scheduler
    assert (s.prediction_type, s.timestep_spacing, s.rescale_betas_zero_snr) == (
        "epsilon", "leading", False)
