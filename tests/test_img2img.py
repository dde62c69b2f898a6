"""img2img on the CPU: scheduler add_noise and part-way start, strength ->
steps, the tiny pipelines with image=, RNG isolation of the lazily built
encoder, multi-rank runs over gloo and the checkpoint round trip."""

import math

import numpy as np
import pytest
import torch

from distrifuser_amd import DistriConfig, DistriSDPipeline, DistriSDXLPipeline
from distrifuser_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler,
                                        EulerDiscreteScheduler)
from distrifuser_amd.schedulers.common import img2img_start

from conftest import run_distributed


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- add_noise -------------------------------------------------------------------


@pytest.mark.parametrize("cls", [DDIMScheduler, DPMSolverMultistepScheduler])
def test_add_noise_closed_form_vp(cls):
    s = cls()
    s.set_timesteps(10)
    x, n = _randn(1, 4, 8, 8, seed=1), _randn(1, 4, 8, 8, seed=2)
    for idx in (0, 5, 9):
        t = s.timesteps[idx]
        acp = s.alphas_cumprod[int(t)].double()
        want = acp.sqrt() * x.double() + (1 - acp).sqrt() * n.double()
        got = s.add_noise(x, n, t)
        assert got.dtype == x.dtype
        assert torch.allclose(got.double(), want, rtol=0, atol=1e-6)


def test_add_noise_closed_form_euler():
    s = EulerDiscreteScheduler()
    s.set_timesteps(10)
    x, n = _randn(1, 4, 8, 8, seed=1), _randn(1, 4, 8, 8, seed=2)
    for idx in (0, 5, 9):
        t = s.timesteps[idx]
        acp = s.alphas_cumprod[int(t)].double()
        sigma = ((1 - acp) / acp).sqrt()
        want = x.double() + sigma * n.double()   # no init_noise_sigma on this path
        got = s.add_noise(x, n, t)
        assert torch.allclose(got.double(), want, rtol=0, atol=1e-5 * max(1.0, float(sigma)))
    assert s.init_noise_sigma > 2  # and it would have shown


def test_add_noise_keeps_a_16_bit_dtype():
    s = DDIMScheduler()
    s.set_timesteps(4)
    out = s.add_noise(_randn(1, 4, 4, 4).bfloat16(), _randn(1, 4, 4, 4, seed=1), s.timesteps[1])
    assert out.dtype == torch.bfloat16


# ---- strength -> steps -------------------------------------------------------------


def test_img2img_start_rule():
    assert [img2img_start(10, s) for s in (0.3, 0.5, 0.99, 1.0)] == [7, 5, 1, 0]
    for bad in (0.0, 1.2, -0.5):
        with pytest.raises(ValueError):
            img2img_start(10, bad)
    with pytest.raises(ValueError):
        img2img_start(10, 0.05)  # int(0.5) = 0 steps: nothing to run


def _tiny_sd(scheduler="ddim", **cfg_kwargs):
    cfg = DistriConfig(height=64, width=64, use_cuda_graph=False, device="cpu", **cfg_kwargs)
    torch.manual_seed(0)
    return DistriSDPipeline.from_pretrained(cfg, preset="tiny", torch_dtype=torch.float32,
                                            scheduler=scheduler)


def _tiny_sdxl(**cfg_kwargs):
    cfg = DistriConfig(height=128, width=128, use_cuda_graph=False, device="cpu", **cfg_kwargs)
    torch.manual_seed(0)
    return DistriSDXLPipeline.from_pretrained(cfg, preset="tiny", torch_dtype=torch.float32)


def _image(h, w, seed=0):
    return torch.rand(3, h, w, generator=torch.Generator().manual_seed(seed))


def test_strength_sets_the_number_of_unet_calls():
    pipe = _tiny_sd()
    calls = []
    pipe.unet.register_forward_hook(lambda *a: calls.append(1))
    img = _image(64, 64)
    for strength, steps in ((0.3, 3), (0.5, 5), (0.99, 9), (1.0, 10)):
        calls.clear()
        out = pipe("a cat", image=img, strength=strength, num_inference_steps=10,
                   output_type="latent")
        assert len(calls) == steps, (strength, len(calls))
        assert len(pipe.scheduler.timesteps) == steps
        assert torch.isfinite(out).all()
    for bad in (0.0, 1.2):
        with pytest.raises(ValueError):
            pipe("a cat", image=img, strength=bad, num_inference_steps=10, output_type="latent")


def test_strength_one_still_noises_the_image():
    """Two different images at strength 1 give different results: the image
    latents are noised at the first timestep, not replaced by noise."""
    pipe = _tiny_sd()
    outs = [pipe("x", image=_image(64, 64, seed=s), strength=1.0, num_inference_steps=2,
                 output_type="latent", generator=torch.Generator().manual_seed(4))
            for s in (1, 2)]
    assert not torch.equal(outs[0], outs[1])


# ---- part-way start ------------------------------------------------------------------


def _fake_eps(x, t):
    return 0.25 * x + math.sin(float(t) / 100.0)


def _run(sched, x, guided):
    trace = []
    for t in sched.timesteps:
        trace.append(x)
        xin = sched.scale_model_input(x, t)
        eps = _fake_eps(xin, t)
        if guided:  # the CPU guided_step: CFG combine, then step
            x = sched.guided_step(torch.cat([eps - 0.5, eps]), t, x, 2.0)
        else:
            x = sched.step(eps, t, x)
    return x, trace


@pytest.mark.parametrize("guided", [False, True], ids=["step", "guided_step"])
@pytest.mark.parametrize("cls", [DDIMScheduler, EulerDiscreteScheduler])
def test_part_way_start_is_bitwise_the_tail_of_the_full_schedule(cls, guided):
    n, k = 10, 6
    full = cls()
    full.set_timesteps(n)
    all_t = full.timesteps.clone()
    final, trace = _run(full, _randn(1, 4, 8, 8, seed=3), guided)

    part = cls()
    part.set_timesteps(n)
    part.set_begin_index(k)
    assert torch.equal(part.timesteps, all_t[k:])
    got, _ = _run(part, trace[k], guided)
    assert torch.equal(got, final)
    if cls is EulerDiscreteScheduler:
        ref = cls()
        ref.set_timesteps(n)
        assert torch.equal(part.sigmas, ref.sigmas[k:]) and part._step_index == n - k
    # set_timesteps starts a full schedule again
    part.set_timesteps(n)
    assert torch.equal(part.timesteps, all_t)
    with pytest.raises(ValueError):
        part.set_begin_index(n)


def test_dpm_part_way_first_step_is_first_order_then_second():
    n, k = 10, 6
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(n)
    all_t = s.timesteps.clone()
    # give the solver a history, as a reused scheduler object has
    x = _randn(1, 4, 8, 8, seed=3)
    x = s.step(_fake_eps(x, all_t[0]), all_t[0], x)
    s.set_timesteps(n)
    s.set_begin_index(k)
    assert torch.equal(s.timesteps, all_t[k:]) and s._x0_prev is None

    def coeffs(t, tp):
        return (s.alpha_t[t], s.sigma_t[t], s.lambda_t[t],
                s.alpha_t[tp], s.sigma_t[tp], s.lambda_t[tp])

    x0 = _randn(1, 4, 8, 8, seed=5)
    t0, t1, t2 = int(all_t[k]), int(all_t[k + 1]), int(all_t[k + 2])
    e0 = _fake_eps(x0, t0)
    x1 = s.step(e0, all_t[k], x0)
    a_t, s_t, l_t, a_p, s_p, l_p = coeffs(t0, t1)
    d0 = (x0 - s_t * e0) / a_t
    h = l_p - l_t
    assert torch.equal(x1, (s_p / s_t) * x0 - a_p * (torch.exp(-h) - 1.0) * d0)

    e1 = _fake_eps(x1, t1)
    x2 = s.step(e1, all_t[k + 1], x1)
    a_t, s_t, l_t, a_p, s_p, l_p = coeffs(t1, t2)
    d1_0 = (x1 - s_t * e1) / a_t
    h = l_p - l_t
    r0 = (l_t - s.lambda_t[t0]) / h
    want = ((s_p / s_t) * x1 - a_p * (torch.exp(-h) - 1.0) * d1_0
            - 0.5 * a_p * (torch.exp(-h) - 1.0) * ((d1_0 - d0) / r0))
    assert torch.allclose(x2, want, rtol=0, atol=1e-6)  # the 2M update, from its history
    first_order = (s_p / s_t) * x1 - a_p * (torch.exp(-h) - 1.0) * d1_0
    assert (x2 - first_order).abs().max() > 1e-3


# ---- pipelines -----------------------------------------------------------------------


def test_tiny_sdxl_img2img():
    pipe = _tiny_sdxl()
    assert pipe._vae_encoder is None  # nothing allocated before the first image=
    img = _image(128, 128, seed=1)
    kw = dict(num_inference_steps=4, strength=0.5, output_type="latent")
    a = pipe("a photo", image=img, generator=torch.Generator().manual_seed(7), **kw)
    b = pipe("a photo", image=img, generator=torch.Generator().manual_seed(7), **kw)
    t2i = pipe("a photo", num_inference_steps=4, output_type="latent",
               generator=torch.Generator().manual_seed(7))
    assert a.shape == (1, 4, 16, 16) and torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert not torch.equal(a, t2i)
    # the other accepted input types give the same latents as the tensor
    u8 = (img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()
    c = pipe("a photo", image=u8, generator=torch.Generator().manual_seed(7), **kw)
    d = pipe("a photo", image=torch.from_numpy(u8).permute(2, 0, 1)[None].float() / 255.0,
             generator=torch.Generator().manual_seed(7), **kw)
    assert torch.equal(c, d)
    out = pipe("a photo", image=img, num_inference_steps=4, strength=0.5, output_type="np")
    assert out.shape == (1, 128, 128, 3) and out.dtype == np.uint8
    for bad in (_image(64, 128), _image(128, 136), torch.zeros(2, 3, 128, 128),
                np.zeros((128, 128, 3), dtype=np.float32)):
        with pytest.raises(ValueError):
            pipe("a photo", image=bad, **kw)


@pytest.mark.parametrize("scheduler", ["ddim", "euler", "dpm-solver"])
def test_tiny_sd_img2img(scheduler):
    pipe = _tiny_sd(scheduler)
    img = _image(64, 64, seed=2)
    kw = dict(num_inference_steps=6, strength=0.5, output_type="latent")
    a = pipe("a cat", image=img, generator=torch.Generator().manual_seed(1), **kw)
    b = pipe("a cat", image=img, generator=torch.Generator().manual_seed(1), **kw)
    t2i = pipe("a cat", num_inference_steps=6, output_type="latent",
               generator=torch.Generator().manual_seed(1))
    assert a.shape == (1, 4, 8, 8) and torch.isfinite(a).all()
    assert torch.equal(a, b) and not torch.equal(a, t2i)
    with pytest.raises(ValueError):
        pipe("a cat", image=_image(32, 64), **kw)


def test_pil_image_when_pillow_is_importable():
    Image = pytest.importorskip("PIL.Image")
    pipe = _tiny_sd()
    u8 = (_image(64, 64, seed=3).permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()
    kw = dict(num_inference_steps=4, strength=0.5, output_type="latent")
    a = pipe("x", image=Image.fromarray(u8), **kw)
    b = pipe("x", image=u8, **kw)
    assert torch.equal(a, b)


# ---- RNG isolation -------------------------------------------------------------------


def test_lazy_encoder_leaves_the_global_rng_alone():
    pipe = _tiny_sdxl()
    state = torch.get_rng_state()
    enc = pipe.vae_encoder
    assert torch.equal(torch.get_rng_state(), state)
    assert pipe.vae_encoder is enc
    # its random init is a fixed stream of its own, whatever the global seed
    torch.manual_seed(12345)
    other = _tiny_sdxl().vae_encoder
    for (k, a), (_, b) in zip(enc.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a, b), k


def test_text_to_image_is_bit_identical_around_an_img2img_call():
    pipe = _tiny_sdxl()
    kw = dict(num_inference_steps=3, output_type="latent")
    before = pipe("hello", generator=torch.Generator().manual_seed(7), **kw)
    pipe("hello", image=_image(128, 128), strength=0.7,
         generator=torch.Generator().manual_seed(7), **kw)
    after = pipe("hello", generator=torch.Generator().manual_seed(7), **kw)
    assert torch.equal(before, after)
    # and equals a pipeline that never built an encoder
    fresh = _tiny_sdxl()("hello", generator=torch.Generator().manual_seed(7), **kw)
    assert torch.equal(before, fresh)


# ---- multi-rank ----------------------------------------------------------------------

_MR_STEPS = 10


def _img2img_worker(rank, world_size, mode, strength):
    cfg = DistriConfig(height=128, width=128, mode=mode, warmup_steps=2,
                       do_classifier_free_guidance=False, use_cuda_graph=False, device="cpu")
    assert cfg.n_device_per_batch == world_size  # the ranks split the image into patches
    torch.manual_seed(0)
    pipe = DistriSDXLPipeline.from_pretrained(cfg, preset="tiny", torch_dtype=torch.float32)
    out = pipe("a scenic mountain", image=_image(128, 128, seed=4), strength=strength,
               num_inference_steps=_MR_STEPS, guidance_scale=1, output_type="latent",
               generator=torch.Generator().manual_seed(3))
    return out.clone()


def test_img2img_patch_full_sync_matches_single_ws2():
    cfg = DistriConfig(height=128, width=128, warmup_steps=2, do_classifier_free_guidance=False,
                       use_cuda_graph=False, device="cpu")
    torch.manual_seed(0)
    pipe = DistriSDXLPipeline.from_pretrained(cfg, preset="tiny", torch_dtype=torch.float32)
    ref = pipe("a scenic mountain", image=_image(128, 128, seed=4), strength=0.5,
               num_inference_steps=_MR_STEPS, guidance_scale=1, output_type="latent",
               generator=torch.Generator().manual_seed(3))
    out = run_distributed(2, _img2img_worker, ("full_sync", 0.5))
    for r in (0, 1):
        # the tolerance test_pipelines.py holds full_sync to against one process
        assert torch.allclose(out[r], ref, atol=1e-3), (
            f"rank {r}: max err {(out[r] - ref).abs().max()}")


@pytest.mark.parametrize("strength,steps", [(0.1, 1), (0.5, 5)],
                         ids=["below-warmup", "above-warmup"])
def test_img2img_displaced_runs_ws2(strength, steps):
    assert int(_MR_STEPS * strength) == steps and (steps < 2 or steps > 2)  # warmup_steps = 2
    out = run_distributed(2, _img2img_worker, ("corrected_async_gn", strength))
    assert out[0].shape == (1, 4, 16, 16)
    assert torch.isfinite(out[0]).all() and torch.equal(out[0], out[1])


# ---- checkpoint round trip -----------------------------------------------------------


def test_save_and_load_round_trips_the_encoder(tmp_path):
    from safetensors.torch import load_file

    pipe = _tiny_sd()
    pipe.save_pretrained(str(tmp_path / "plain"))
    plain = load_file(str(tmp_path / "plain" / "vae" / "diffusion_pytorch_model.safetensors"))
    assert not any(k.startswith(("encoder.", "quant_conv.")) for k in plain)

    enc = pipe.vae_encoder
    with torch.no_grad():
        for p in enc.parameters():  # move off the fixed random init
            p.add_(0.125)
    pipe.save_pretrained(str(tmp_path / "full"))
    full = load_file(str(tmp_path / "full" / "vae" / "diffusion_pytorch_model.safetensors"))
    assert "encoder.conv_in.weight" in full and "quant_conv.bias" in full
    assert all(torch.equal(full[k], v) for k, v in plain.items())  # decoder keys unchanged

    cfg = DistriConfig(height=64, width=64, use_cuda_graph=False, device="cpu")
    torch.manual_seed(5)
    loaded = DistriSDPipeline.from_pretrained(
        cfg, preset="tiny", torch_dtype=torch.float32,
        pretrained_model_name_or_path=str(tmp_path / "full"))
    assert loaded._vae_encoder is None  # still lazy
    got, want = loaded.vae_encoder.state_dict(), enc.state_dict()
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
