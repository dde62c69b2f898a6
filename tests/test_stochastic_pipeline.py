"""The stochastic samplers through both pipelines on the CPU (tiny presets):
the noise seed is drawn from the caller's generator right after the latents,
a deterministic scheduler draws nothing, and every rank adds the same noise."""

import pytest
import torch
from conftest import run_distributed

from distrifuser_amd import DistriConfig, DistriSDPipeline, DistriSDXLPipeline

PIPES = pytest.mark.parametrize("cls", [DistriSDPipeline, DistriSDXLPipeline],
                                ids=["sd", "sdxl"])
CFG = pytest.mark.parametrize("do_cfg", [True, False], ids=["cfg", "nocfg"])
SAMPLERS = {
    "euler-a": ("euler-a", {}),
    "ddim-eta1": ("ddim", {"eta": 1.0}),
    "dpm-sde": ("dpm-solver", {"algorithm_type": "sde-dpmsolver++"}),
}
NAMES = pytest.mark.parametrize("sampler", list(SAMPLERS))
STEPS = 3


def _size(cls):
    return 128 if cls is DistriSDXLPipeline else 64


def _tiny(cls, sampler, do_cfg=True):
    name, extra = SAMPLERS.get(sampler, (sampler, {}))
    cfg = DistriConfig(height=_size(cls), width=_size(cls), use_cuda_graph=False, device="cpu",
                       do_classifier_free_guidance=do_cfg)
    torch.manual_seed(0)
    pipe = cls.from_pretrained(cfg, preset="tiny", torch_dtype=torch.float32, scheduler=name,
                               **extra)
    # Euler's init_noise_sigma is known once a schedule is set: without this a
    # pipeline's first call would scale its initial latents by 1.0
    pipe.scheduler.set_timesteps(STEPS)
    return pipe


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _run(pipe, seed=4, **kw):
    scale = {} if pipe.distri_config.do_classifier_free_guidance else {"guidance_scale": 1}
    return pipe("a prompt", num_inference_steps=STEPS, output_type="latent",
                generator=None if seed is None else _gen(seed), **scale, **kw)


def _image(size, seed=1):
    return torch.rand(3, size, size, generator=_gen(seed))


def _half_mask(size):
    mask = torch.zeros(size, size)
    mask[: size // 2] = 1.0
    return mask


@CFG
@NAMES
@PIPES
def test_runs_are_finite_and_reproducible_from_the_generator_seed(cls, sampler, do_cfg):
    pipe = _tiny(cls, sampler, do_cfg)
    assert pipe.scheduler.stochastic
    a = _run(pipe, 4)
    seed_a = pipe.scheduler._noise_seed
    b = _run(pipe, 4)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and pipe.scheduler._noise_seed == seed_a
    c = _run(pipe, 5)
    assert not torch.equal(a, c) and pipe.scheduler._noise_seed != seed_a
    # the same latents without the steps' noise: it reaches the result
    deterministic = _run(_tiny(cls, SAMPLERS[sampler][0].replace("euler-a", "euler"), do_cfg), 4)
    assert not torch.equal(a, deterministic)


@NAMES
@PIPES
def test_the_seed_is_one_draw_after_the_latents(cls, sampler):
    pipe = _tiny(cls, sampler)
    g = _gen(11)
    pipe("a prompt", num_inference_steps=STEPS, output_type="latent", generator=g)
    twin = _gen(11)
    torch.randn(1, 4, _size(cls) // 8, _size(cls) // 8, generator=twin)
    want = int(torch.randint(0, 2**63 - 1, (1,), generator=twin))
    assert pipe.scheduler._noise_seed == want
    assert torch.equal(g.get_state(), twin.get_state())
    # generator=None: the fixed-seed generator the latents fall back to
    default = _run(pipe, None)
    assert torch.equal(default, _run(pipe, 0))
    assert pipe.scheduler._noise_seed != want


@pytest.mark.parametrize("scheduler", ["ddim", "euler", "dpm-solver"])
@PIPES
def test_a_deterministic_scheduler_draws_nothing_extra(cls, scheduler):
    """The generator ends where the initial latents left it, the scheduler's
    seed is untouched, and the output is the plain denoise loop's."""
    pipe = _tiny(cls, scheduler)
    assert not pipe.scheduler.stochastic
    sigma0 = pipe.scheduler.init_noise_sigma
    g = _gen(7)
    out = pipe("hello", num_inference_steps=STEPS, output_type="latent", generator=g)
    twin = _gen(7)
    lat = torch.randn(1, 4, _size(cls) // 8, _size(cls) // 8, generator=twin) * sigma0
    assert torch.equal(g.get_state(), twin.get_state())
    assert pipe.scheduler._noise_seed == 0
    with torch.no_grad():
        if cls is DistriSDXLPipeline:
            embeds, pooled = pipe.encode_prompt("hello", None, True)
            added = pipe._added_cond(embeds.shape[0], pooled)
            scale = 5.0
        else:
            embeds, added, scale = pipe.encode_prompt("hello", None, True), None, 7.5
        sched = pipe.scheduler
        sched.set_timesteps(STEPS)
        pipe.unet.set_counter(0)
        for t in sched.timesteps:
            noise = pipe.unet(sched.scale_model_input(torch.cat([lat] * 2), t), t, embeds, added)
            lat = sched.guided_step(noise, t, lat, scale)
    assert torch.equal(out, lat)


@CFG
@NAMES
@PIPES
def test_img2img_and_inpaint_run(cls, sampler, do_cfg):
    pipe = _tiny(cls, sampler, do_cfg)
    size = _size(cls)
    image, mask = _image(size), _half_mask(size)
    plain = _run(pipe)
    i2i = _run(pipe, image=image, strength=0.7)
    assert torch.isfinite(i2i).all() and torch.equal(i2i, _run(pipe, image=image, strength=0.7))
    assert not torch.equal(i2i, plain)
    inp = _run(pipe, image=image, mask=mask)
    assert torch.isfinite(inp).all() and torch.equal(inp, _run(pipe, image=image, mask=mask))
    assert not torch.equal(inp, _run(pipe, 5, image=image, mask=mask))
    # the known region (mask 0: the lower half) comes out as the encoded image
    g = _gen(4)
    init = pipe.vae_encoder.encode(pipe._prepare_image(image), generator=g).float()
    half = size // 16
    assert torch.equal(inp[:, :, half:], init[:, :, half:])
    assert not torch.equal(inp[:, :, :half], init[:, :, :half])


# ---- multi-rank ----------------------------------------------------------------------


def _mr_call(pipe):
    return pipe("a scenic mountain", num_inference_steps=STEPS, guidance_scale=1,
                output_type="latent", generator=_gen(3))


def _mr_config(**kw):
    return DistriConfig(height=128, width=128, warmup_steps=2, do_classifier_free_guidance=False,
                        use_cuda_graph=False, device="cpu", **kw)


def _mr_worker(rank, world_size, mode):
    cfg = _mr_config(mode=mode)
    assert cfg.n_device_per_batch == world_size  # the ranks split the image into patches
    torch.manual_seed(0)
    pipe = DistriSDXLPipeline.from_pretrained(cfg, preset="tiny", torch_dtype=torch.float32,
                                              scheduler="euler-a")
    out = _mr_call(pipe).clone()
    return out, pipe.scheduler._noise_seed


def test_every_rank_adds_the_same_noise_full_sync_ws2():
    torch.manual_seed(0)
    pipe = DistriSDXLPipeline.from_pretrained(_mr_config(), preset="tiny",
                                              torch_dtype=torch.float32, scheduler="euler-a")
    ref = _mr_call(pipe)
    out = run_distributed(2, _mr_worker, ("full_sync",))
    for r in (0, 1):
        latents, seed = out[r]
        assert seed == pipe.scheduler._noise_seed
        # the tolerance tests/test_unet_parallel.py holds full_sync to
        err = (latents - ref).abs().max().item()
        print(f"rank {r}: max err {err:.3e}")
        assert torch.allclose(latents, ref, atol=2e-4), f"rank {r}: max err {err}"
    assert torch.equal(out[0][0], out[1][0])
