"""Inpainting on one GPU: hipGraph replay against eager, the exact known
region in bf16, one native masked-step launch per step (and one input-assembly
launch with a 9-channel U-Net, whose conv_in rides the conv kernel), and the
other schedulers and fp16.

Run on an MI355X box: pytest tests/test_inpaint_gpu.py -m gpu -q -s"""

import dataclasses

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

DEV = "cuda:0"


def _image(h, w, seed=0):
    return torch.rand(3, h, w, generator=torch.Generator().manual_seed(seed))


def _half_mask(h, w):
    m = torch.zeros(h, w)
    m[:, : w // 2] = 1.0
    return m


def _spy_init(pipe):
    """The fp32 init latents the pipeline hands to every masked_step."""
    seen = []
    real = pipe.scheduler.masked_step

    def spy(noise, t, sample, g, mask, init, init_noise):
        seen.append(init)
        return real(noise, t, sample, g, mask, init, init_noise)

    pipe.scheduler.masked_step = spy
    return seen


def _tiny_sdxl(use_graph=False, unet_config=None, dtype=torch.bfloat16, scheduler="ddim"):
    from distrifuser_amd import DistriConfig, DistriSDXLPipeline

    cfg = DistriConfig(height=128, width=128, use_cuda_graph=use_graph, device=DEV)
    torch.manual_seed(0)
    kw = {} if unet_config is None else {"unet_config": unet_config}
    return DistriSDXLPipeline.from_pretrained(cfg, preset="tiny", torch_dtype=dtype,
                                              scheduler=scheduler, **kw)


@requires_gpu
def test_tiny_sdxl_inpaint_graph_vs_eager_and_known_region():
    """use_cuda_graph=True is within the 0.05 that the other graph-parity
    tests hold, and in both runs the known half is init.to(bf16) bit for bit."""
    img, mask = _image(128, 128, seed=2), _half_mask(128, 128)
    outs = {}
    for use_graph in (False, True):
        pipe = _tiny_sdxl(use_graph)
        inits = _spy_init(pipe)
        out = pipe("graph parity", image=img, mask=mask, num_inference_steps=8,
                   output_type="latent", generator=torch.Generator().manual_seed(5))
        assert out.shape == (1, 4, 16, 16) and out.dtype == torch.bfloat16
        assert torch.isfinite(out.float()).all()
        assert len(inits) == 8 and inits[0].dtype == torch.float32
        init = inits[0].to(torch.bfloat16)
        assert torch.equal(out[..., 8:], init[..., 8:])
        assert (out[..., :8] != init[..., :8]).float().mean() > 0.9
        outs[use_graph] = out.float()
    err = (outs[True] - outs[False]).abs().max().item()
    print(f"inpaint graph vs eager: {err:.5f}")
    assert err < 0.05, f"graph-replay output drifted from eager: {err}"


def _count(monkeypatch, ext, names):
    calls = {n: 0 for n in names}

    def wrap(name):
        real = getattr(ext, name)

        def f(*a, **kw):
            calls[name] += 1
            return real(*a, **kw)

        monkeypatch.setattr(ext, name, f)

    for n in names:
        wrap(n)
    return calls


@requires_gpu
@pytest.mark.parametrize("scheduler,step_op", [("ddim", "masked_affine_step"),
                                               ("euler", "masked_affine_step"),
                                               ("dpm-solver", "masked_dpm_step")])
def test_one_native_masked_step_per_denoise_step(monkeypatch, scheduler, step_op):
    from distrifuser_amd import ops

    monkeypatch.delenv("DFA_FORCE_EAGER", raising=False)
    calls = _count(monkeypatch, ops.hip_ext(),
                   ["masked_affine_step", "masked_dpm_step", "cfg_affine_step", "cfg_dpm_step",
                    "inpaint_unet_input"])
    pipe = _tiny_sdxl(scheduler=scheduler)
    steps = 5
    out = pipe("x", image=_image(128, 128), mask=_half_mask(128, 128),
               num_inference_steps=steps, output_type="latent")
    assert torch.isfinite(out.float()).all()
    want = {n: 0 for n in calls}
    want[step_op] = steps
    assert calls == want


@requires_gpu
@pytest.mark.parametrize("do_cfg", [True, False], ids=["cfg", "no-cfg"])
def test_nine_channel_unet_one_assembly_launch_per_step_native_conv_in(monkeypatch, do_cfg):
    from distrifuser_amd import DistriConfig, DistriSDXLPipeline, ops
    from distrifuser_amd.models.unet import TINY_UNET

    monkeypatch.delenv("DFA_FORCE_EAGER", raising=False)
    calls = _count(monkeypatch, ops.hip_ext(),
                   ["masked_affine_step", "cfg_affine_step", "inpaint_unet_input"])
    torch_convs = []
    real_f = F.conv2d

    def counted_f(x, weight, *a, **kw):
        torch_convs.append(tuple(weight.shape[2:]))
        return real_f(x, weight, *a, **kw)

    monkeypatch.setattr(F, "conv2d", counted_f)
    cfg = DistriConfig(height=128, width=128, use_cuda_graph=False, device=DEV,
                       do_classifier_free_guidance=do_cfg)
    torch.manual_seed(0)
    pipe = DistriSDXLPipeline.from_pretrained(
        cfg, preset="tiny", torch_dtype=torch.bfloat16, scheduler="euler",
        unet_config=dataclasses.replace(TINY_UNET, in_channels=9))
    inits = _spy_init(pipe)
    seen = []
    pipe.unet.unet.conv_in.register_forward_pre_hook(
        lambda mod, args: seen.append(tuple(args[0].shape)))
    steps = 4
    img = _image(128, 128, seed=3)
    out = pipe("x", image=img, mask=_half_mask(128, 128), num_inference_steps=steps,
               guidance_scale=5.0 if do_cfg else 1, output_type="latent",
               generator=torch.Generator().manual_seed(1))
    assert out.shape == (1, 4, 16, 16) and torch.isfinite(out.float()).all()
    assert calls == {"masked_affine_step": steps, "cfg_affine_step": 0,
                     "inpaint_unet_input": steps}
    assert seen == [(2 if do_cfg else 1, 9, 16, 16)] * steps
    assert (3, 3) not in torch_convs, f"3x3 convs through F.conv2d: {torch_convs}"
    assert torch.equal(out[..., 8:], inits[0].to(torch.bfloat16)[..., 8:])


@requires_gpu
@pytest.mark.parametrize("scheduler,dtype", [("euler", torch.bfloat16),
                                             ("dpm-solver", torch.bfloat16),
                                             ("ddim", torch.float16)],
                         ids=["euler-bf16", "dpm-bf16", "ddim-fp16"])
def test_tiny_sd_inpaint_schedulers_and_fp16(scheduler, dtype):
    from distrifuser_amd import DistriConfig, DistriSDPipeline

    cfg = DistriConfig(height=64, width=64, use_cuda_graph=False, device=DEV)
    torch.manual_seed(0)
    pipe = DistriSDPipeline.from_pretrained(cfg, preset="tiny", torch_dtype=dtype,
                                            scheduler=scheduler)
    img, mask = _image(64, 64, seed=3), _half_mask(64, 64)
    out = pipe("a cat", image=img, mask=mask, num_inference_steps=6, output_type="np")
    assert out.shape == (1, 64, 64, 3)
    lat = pipe("a cat", image=img, mask=mask, num_inference_steps=6, output_type="latent")
    assert lat.shape == (1, 4, 8, 8) and lat.dtype == dtype
    assert torch.isfinite(lat.float()).all()
