"""Inpainting on the CPU (fp32, tiny presets): the schedulers' masked_step
against the hand composition step -> add_noise -> blend, the exact known
region, RNG order, mask preprocessing, the 9-channel U-Net input, a ws=2 gloo
run, and the unchanged text-to-image / img2img paths."""

import dataclasses
import math

import numpy as np
import pytest
import torch

from distrifuser_amd import DistriConfig, DistriSDPipeline, DistriSDXLPipeline
from distrifuser_amd.models.unet import (SD15_INPAINT_UNET, SD15_UNET, SDXL_INPAINT_UNET,
                                         SDXL_UNET, TINY_UNET)
from distrifuser_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler,
                                        EulerDiscreteScheduler)

from conftest import run_distributed

SCHEDULERS = [DDIMScheduler, EulerDiscreteScheduler, DPMSolverMultistepScheduler]
NAMES = ["ddim", "euler", "dpm-solver"]


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _image(h, w, seed=0):
    return torch.rand(3, h, w, generator=torch.Generator().manual_seed(seed))


def _half_mask(h, w):
    m = torch.zeros(h, w)
    m[:, : w // 2] = 1.0  # repaint the left half
    return m


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _tiny_sd(scheduler="ddim", unet_config=None, **cfg_kwargs):
    cfg = DistriConfig(height=64, width=64, use_cuda_graph=False, device="cpu", **cfg_kwargs)
    torch.manual_seed(0)
    kw = {} if unet_config is None else {"unet_config": unet_config}
    return DistriSDPipeline.from_pretrained(cfg, preset="tiny", torch_dtype=torch.float32,
                                            scheduler=scheduler, **kw)


def _tiny_sdxl(scheduler="ddim", unet_config=None, **cfg_kwargs):
    cfg = DistriConfig(height=128, width=128, use_cuda_graph=False, device="cpu", **cfg_kwargs)
    torch.manual_seed(0)
    kw = {} if unet_config is None else {"unet_config": unet_config}
    return DistriSDXLPipeline.from_pretrained(cfg, preset="tiny", torch_dtype=torch.float32,
                                              scheduler=scheduler, **kw)


TINY_INPAINT_UNET = dataclasses.replace(TINY_UNET, in_channels=9)


# ---- schedulers ----------------------------------------------------------------------


def _fake_eps(x, t):
    return 0.25 * x + math.sin(float(t) / 100.0)


@pytest.mark.parametrize("guided", [False, True], ids=["no-cfg", "cfg-pair"])
@pytest.mark.parametrize("cls", SCHEDULERS)
def test_masked_step_is_step_then_add_noise_then_blend(cls, guided):
    n = 6
    masked, plain = cls(), cls()
    masked.set_timesteps(n)
    plain.set_timesteps(n)
    init, noise = _randn(1, 4, 8, 8, seed=1), _randn(1, 4, 8, 8, seed=2)
    m = (torch.rand(1, 1, 8, 8, generator=_gen(3)) >= 0.5).float()
    x = _randn(1, 4, 8, 8, seed=4) * masked.init_noise_sigma
    xh = x.clone()
    for i, t in enumerate(masked.timesteps):
        eps = _fake_eps(masked.scale_model_input(x, t), t)
        eps_h = _fake_eps(plain.scale_model_input(xh, t), t)
        last = i == n - 1
        if guided:
            x = masked.masked_step(torch.cat([eps - 0.5, eps]), t, x, 2.0, m, init, noise)
            stepped = plain.guided_step(torch.cat([eps_h - 0.5, eps_h]), t, xh, 2.0)
        else:
            x = masked.masked_step(eps, t, x, 1.0, m, init, noise)
            stepped = plain.step(eps_h, t, xh)
        known = init if last else plain.add_noise(init, noise, plain.timesteps[i + 1])
        xh = m * stepped + (1 - m) * known
        scale = max(1.0, float(xh.abs().max()))
        assert torch.allclose(x, xh, rtol=0, atol=1e-6 * scale), (i, (x - xh).abs().max())
    # the last step's known region is the clean init, not acp[0]-noised
    assert torch.equal(torch.where(m == 0, x, init), init)
    # state: as after an unmasked run
    for attr in ("_step_index", "_t_prev"):
        assert getattr(masked, attr, None) == getattr(plain, attr, None), attr
    if cls is DPMSolverMultistepScheduler:
        assert torch.allclose(masked._x0_prev, plain._x0_prev, rtol=0, atol=1e-5)
        assert masked._step_index == n


@pytest.mark.parametrize("cls", SCHEDULERS)
def test_known_coefficients_describe_the_next_timestep(cls):
    s = cls()
    s.set_timesteps(10)
    s.set_begin_index(4)  # the running list
    init, noise = _randn(1, 4, 4, 4, seed=1), _randn(1, 4, 4, 4, seed=2)
    sa, sb = s._known_coeffs(s.timesteps[0])
    want = s.add_noise(init, noise, s.timesteps[1])
    assert torch.allclose(sa * init + sb * noise, want, rtol=0, atol=1e-5)
    if cls is EulerDiscreteScheduler:
        assert sa == 1.0 and sb == pytest.approx(float(s.sigmas[1]))
        s._step_index = len(s.timesteps) - 1
    assert s._known_coeffs(s.timesteps[-1]) == (1.0, 0.0)


# ---- pipelines -----------------------------------------------------------------------


def _posterior_sample(pipe, img, seed):
    return pipe.vae_encoder.encode(pipe._prepare_image(img), generator=_gen(seed))


@pytest.mark.parametrize("scheduler", NAMES)
@pytest.mark.parametrize("make,size", [(_tiny_sd, 64), (_tiny_sdxl, 128)], ids=["sd", "sdxl"])
def test_all_zero_mask_returns_the_encoded_image(make, size, scheduler):
    pipe = make(scheduler)
    img = _image(size, size, seed=1)
    out = pipe("x", image=img, mask=torch.zeros(size, size), num_inference_steps=4,
               output_type="latent", generator=_gen(5))
    assert torch.equal(out, _posterior_sample(pipe, img, 5))


@pytest.mark.parametrize("scheduler", NAMES)
def test_all_one_mask_is_img2img_bit_for_bit(scheduler):
    """Pins the RNG order (posterior sample, then noise) and the start from
    the noised image for strength < 1."""
    pipe = _tiny_sd(scheduler)
    img = _image(64, 64, seed=2)
    kw = dict(image=img, strength=0.5, num_inference_steps=6, output_type="latent")
    a = pipe("a cat", mask=torch.ones(64, 64), generator=_gen(1), **kw)
    b = pipe("a cat", generator=_gen(1), **kw)
    assert torch.equal(a, b)


def test_all_one_mask_is_img2img_bit_for_bit_sdxl():
    pipe = _tiny_sdxl()
    img = _image(128, 128, seed=2)
    kw = dict(image=img, strength=0.5, num_inference_steps=4, output_type="latent")
    a = pipe("a cat", mask=torch.ones(1, 128, 128), generator=_gen(1), **kw)
    b = pipe("a cat", generator=_gen(1), **kw)
    assert torch.equal(a, b)


@pytest.mark.parametrize("scheduler", NAMES)
def test_half_mask_keeps_the_known_half_exactly(scheduler):
    pipe = _tiny_sd(scheduler)
    img = _image(64, 64, seed=3)
    out = pipe("a cat", image=img, mask=_half_mask(64, 64), strength=1.0,
               num_inference_steps=4, output_type="latent", generator=_gen(2))
    init = _posterior_sample(pipe, img, 2)
    assert torch.isfinite(out).all()
    assert torch.equal(out[..., 4:], init[..., 4:])
    assert (out[..., :4] != init[..., :4]).float().mean() > 0.9
    # strength defaults to 1.0 with a mask
    dflt = pipe("a cat", image=img, mask=_half_mask(64, 64), num_inference_steps=4,
                output_type="latent", generator=_gen(2))
    assert torch.equal(dflt, out)
    # and the decoded output has the pipeline's shape
    arr = pipe("a cat", image=img, mask=_half_mask(64, 64), num_inference_steps=2,
               output_type="np")
    assert arr.shape == (1, 64, 64, 3) and arr.dtype == np.uint8


# ---- mask preprocessing --------------------------------------------------------------


def test_mask_input_types_binarisation_and_nearest_sampling():
    pipe = _tiny_sd()
    g = _gen(7)
    u8 = torch.randint(0, 256, (64, 64), generator=g, dtype=torch.uint8)
    u8[0, 0], u8[0, 8], u8[8, 0], u8[8, 8] = 127, 128, 255, 0  # 127/255 < 0.5 <= 128/255
    f = u8.float() / 255.0
    want_pix = (f >= 0.5).float().reshape(1, 1, 64, 64)
    pix = pipe._prepare_mask(f)
    assert pix.dtype == torch.float32 and torch.equal(pix, want_pix)
    assert set(pix.unique().tolist()) == {0.0, 1.0}
    for other in (f[None], f[None, None], u8.numpy()):
        assert torch.equal(pipe._prepare_mask(other), pix)
    lat = pipe._latent_mask(pix)
    assert lat.shape == (1, 1, 8, 8)
    for i in range(8):
        for j in range(8):
            assert lat[0, 0, i, j] == want_pix[0, 0, 8 * i, 8 * j]
    assert lat[0, 0, 0, 0] == 0 and lat[0, 0, 0, 1] == 1 and lat[0, 0, 1, 0] == 1
    # what F.interpolate's nearest mode gives
    assert torch.equal(lat, torch.nn.functional.interpolate(pix, size=(8, 8)))
    # a soft 0.5 is repainted
    assert pipe._prepare_mask(torch.full((64, 64), 0.5)).min() == 1


def test_pil_mask_when_pillow_is_importable():
    Image = pytest.importorskip("PIL.Image")
    pipe = _tiny_sd()
    u8 = torch.randint(0, 256, (64, 64), generator=_gen(8), dtype=torch.uint8).numpy()
    assert torch.equal(pipe._prepare_mask(Image.fromarray(u8, mode="L")),
                       pipe._prepare_mask(u8))


def test_mask_validation():
    pipe = _tiny_sd()
    img = _image(64, 64)
    kw = dict(num_inference_steps=2, output_type="latent")
    with pytest.raises(ValueError):
        pipe("x", mask=torch.ones(64, 64), **kw)  # no image
    for bad in (torch.ones(32, 64), torch.ones(64, 72), torch.ones(2, 64, 64),
                np.zeros((64, 32), dtype=np.uint8), np.zeros((64, 64), dtype=np.float32),
                torch.ones(64, 64, dtype=torch.int64)):
        with pytest.raises(ValueError):
            pipe("x", image=img, mask=bad, **kw)
    nine = _tiny_sd(unet_config=dataclasses.replace(pipe.unet.config, in_channels=9))
    with pytest.raises(ValueError):
        nine("x", **kw)
    with pytest.raises(ValueError):
        nine("x", image=img, **kw)


# ---- 9-channel U-Nets ----------------------------------------------------------------


def test_inpaint_presets_have_nine_input_channels():
    assert SDXL_INPAINT_UNET == dataclasses.replace(SDXL_UNET, in_channels=9)
    assert SD15_INPAINT_UNET == dataclasses.replace(SD15_UNET, in_channels=9)


@pytest.mark.parametrize("scheduler", ["ddim", "euler"])
@pytest.mark.parametrize("do_cfg", [True, False], ids=["cfg", "no-cfg"])
def test_nine_channel_unet_input(scheduler, do_cfg):
    pipe = _tiny_sdxl(scheduler, TINY_INPAINT_UNET, do_classifier_free_guidance=do_cfg)
    conv_in = pipe.unet.unet.conv_in
    seen, samples, scales = [], [], []
    conv_in.register_forward_pre_hook(lambda mod, args: seen.append(args[0].clone()))
    real = pipe.scheduler.masked_step

    def spy(noise, t, sample, *a):
        samples.append(sample.clone())
        scales.append(pipe.scheduler.model_input_scale(t))
        return real(noise, t, sample, *a)

    pipe.scheduler.masked_step = spy
    img, mask = _image(128, 128, seed=4), _half_mask(128, 128)
    steps = 3
    out = pipe("x", image=img, mask=mask, num_inference_steps=steps, output_type="latent",
               guidance_scale=5.0 if do_cfg else 1, generator=_gen(6))
    assert out.shape == (1, 4, 16, 16) and torch.isfinite(out).all()
    assert len(seen) == len(samples) == steps

    pix = pipe._prepare_mask(mask)
    lat_mask = pipe._latent_mask(pix)
    g = _gen(6)
    pixels = pipe._prepare_image(img)
    init = pipe.vae_encoder.encode(pixels, generator=g)
    masked_lat = pipe.vae_encoder.encode(pixels * (pix < 0.5), generator=g)  # the second draw
    for x, sample, scale in zip(seen, samples, scales):
        assert x.shape == (2 if do_cfg else 1, 9, 16, 16)
        for copy in x:
            assert torch.equal(copy[4:5], lat_mask[0])
            assert torch.equal(copy[5:9], masked_lat[0])
            assert torch.equal(copy[0:4], (sample / scale)[0])
    if scheduler == "euler":
        assert scales[0] > 2 and scales[0] > scales[-1] > 1
    else:
        assert scales == [1.0] * steps
    assert torch.equal(out[..., 8:], init[..., 8:])


def test_nine_channel_conv_in_round_trips(tmp_path):
    pipe = _tiny_sdxl(unet_config=TINY_INPAINT_UNET)
    pipe.save_pretrained(str(tmp_path / "ckpt"))
    cfg = DistriConfig(height=128, width=128, use_cuda_graph=False, device="cpu")
    torch.manual_seed(9)
    loaded = DistriSDXLPipeline.from_pretrained(
        cfg, preset="tiny", torch_dtype=torch.float32, unet_config=TINY_INPAINT_UNET,
        pretrained_model_name_or_path=str(tmp_path / "ckpt"))
    sd, want = loaded.unet.unet.state_dict(), pipe.unet.unet.state_dict()
    key = [k for k in want if k.startswith("conv_in") and k.endswith("weight")]
    assert len(key) == 1
    assert tuple(sd[key[0]].shape) == (TINY_UNET.block_out_channels[0], 9, 3, 3)
    assert torch.equal(sd[key[0]], want[key[0]])


# ---- multi-rank ----------------------------------------------------------------------

_MR_STEPS = 6


def _inpaint_call(pipe):
    return pipe("a scenic mountain", image=_image(128, 128, seed=4), mask=_half_mask(128, 128),
                num_inference_steps=_MR_STEPS, guidance_scale=1, output_type="latent",
                generator=_gen(3))


def _inpaint_worker(rank, world_size, mode):
    cfg = DistriConfig(height=128, width=128, mode=mode, warmup_steps=2,
                       do_classifier_free_guidance=False, use_cuda_graph=False, device="cpu")
    assert cfg.n_device_per_batch == world_size  # the ranks split the image into patches
    torch.manual_seed(0)
    pipe = DistriSDXLPipeline.from_pretrained(cfg, preset="tiny", torch_dtype=torch.float32)
    return _inpaint_call(pipe).clone()


def test_inpaint_patch_full_sync_matches_single_ws2():
    cfg = DistriConfig(height=128, width=128, warmup_steps=2, do_classifier_free_guidance=False,
                       use_cuda_graph=False, device="cpu")
    torch.manual_seed(0)
    pipe = DistriSDXLPipeline.from_pretrained(cfg, preset="tiny", torch_dtype=torch.float32)
    ref = _inpaint_call(pipe)
    out = run_distributed(2, _inpaint_worker, ("full_sync",))
    for r in (0, 1):
        # the tolerance test_img2img.py holds its full_sync pipeline run to
        assert torch.allclose(out[r], ref, atol=1e-3), (
            f"rank {r}: max err {(out[r] - ref).abs().max()}")
    assert torch.equal(out[0], out[1])


# ---- mask omitted: nothing changes ---------------------------------------------------


def _parent_denoise(pipe, latents, embeds, added, steps, guidance_scale, t_start=0):
    """The denoise loop as it was before mask= existed."""
    sched = pipe.scheduler
    sched.set_timesteps(steps, device=None)
    if t_start:
        sched.set_begin_index(t_start)
    pipe.unet.set_counter(0)
    for t in sched.timesteps:
        latent_in = sched.scale_model_input(torch.cat([latents] * 2), t)
        noise = pipe.unet(latent_in, t, embeds, added)
        latents = sched.guided_step(noise, t, latents, guidance_scale)
    return latents


@pytest.mark.parametrize("scheduler", NAMES)
def test_mask_omitted_runs_the_unmasked_path(monkeypatch, scheduler):
    def boom(*a, **kw):
        raise AssertionError("masked_step called without a mask")

    for cls in SCHEDULERS:
        monkeypatch.setattr(cls, "masked_step", boom)
    pipe = _tiny_sdxl(scheduler)
    img = _image(128, 128, seed=5)
    kw = dict(num_inference_steps=4, output_type="latent")
    sigma0 = pipe.scheduler.init_noise_sigma  # what the first call's initial latents see
    t2i = pipe("hello", generator=_gen(7), **kw)
    i2i = pipe("hello", image=img, generator=_gen(7), **kw)  # strength defaults to 0.3
    assert torch.equal(i2i, pipe("hello", image=img, strength=0.3, generator=_gen(7), **kw))
    assert torch.isfinite(pipe("hello", mask=None, strength=None, **kw)).all()

    with torch.no_grad():
        embeds, pooled = pipe.encode_prompt("hello", None, True)
        added = pipe._added_cond(embeds.shape[0], pooled)
        lat = torch.randn(1, 4, 16, 16, generator=_gen(7)) * sigma0
        assert torch.equal(t2i, _parent_denoise(pipe, lat, embeds, added, 4, 5.0))
        g = _gen(7)
        init = pipe.vae_encoder.encode(pipe._prepare_image(img), generator=g)
        noise = torch.randn(init.shape, generator=g)
        pipe.scheduler.set_timesteps(4)
        lat = pipe.scheduler.add_noise(init, noise, pipe.scheduler.timesteps[3])
        assert torch.equal(i2i, _parent_denoise(pipe, lat, embeds, added, 4, 5.0, t_start=3))
