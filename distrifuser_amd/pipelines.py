"""DistriSDXLPipeline / DistriSDPipeline — the user-facing API.

Parity with the reference surface (reference pipelines.py): construction via
``from_pretrained(distri_config, **kw)``, generation via ``pipeline(prompt=
..., generator=...)``, ``prepare()`` runs the comm-buffer registration pass,
the buffer-filling pre-run, and hipGraph capture. Unlike the reference
(which wrapped diffusers' StableDiffusion*Pipeline), the scheduler loop,
prompt encoding, latent handling and VAE decode here are all owned natively.

No network in this environment: ``pretrained_model_name_or_path=None`` (the
default) builds random-init weights of the exact architecture; a local
diffusers-layout directory with safetensors files is loaded when given.
"""

from __future__ import annotations

import json
import os

import torch

from .models.clip import CLIP_VIT_L, OPEN_CLIP_BIG_G, TINY_CLIP, CLIPTextEncoder
from .models.distri_unet import DistriUNet
from .models.tokenizer import CLIPBPETokenizer, SimpleTokenizer, load_clip_tokenizer
from .models.unet import (SD15_INPAINT_UNET, SD15_UNET, SDXL_INPAINT_UNET, SDXL_UNET, TINY_UNET,
                          UNetConfig)
from .models.vae import SD_VAE, SDXL_VAE, TINY_VAE, VAEDecoder, VAEEncoder
from . import ops
from .models import weights as weight_io
from .schedulers import scheduler_class
from .schedulers.common import img2img_start
from .utils.comm import PatchParallelismCommManager
from .utils.config import DistriConfig


def _resolve_tokenizer(pretrained, vocab_size: int, subfolder: str = "tokenizer",
                       pad_with_zero: bool = False, allow_simple: bool = False):
    """Real-checkpoint tokenizer policy: a checkpoint directory
    must ship CLIP BPE files (``<subfolder>/vocab.json`` + ``merges.txt``) —
    hash-token ids against real weights silently break text conditioning.
    Our own ``save_pretrained`` leaves a SimpleTokenizer marker so random-init
    round-trips keep working; anything else must opt in explicitly."""
    if pretrained is None:
        return SimpleTokenizer(vocab_size=vocab_size)
    tok = load_clip_tokenizer(pretrained, subfolder, pad_with_zero=pad_with_zero)
    if tok is not None:
        return tok
    marker = os.path.join(pretrained, subfolder, "tokenizer_config.json")
    marker_simple = False
    if os.path.isfile(marker):
        try:
            with open(marker, encoding="utf-8") as f:
                marker_simple = json.load(f).get("tokenizer_class") == "SimpleTokenizer"
        except (OSError, ValueError):
            pass
    if marker_simple or allow_simple:
        return SimpleTokenizer(vocab_size=vocab_size)
    raise FileNotFoundError(
        f"checkpoint {pretrained!r} has no {subfolder}/vocab.json+merges.txt: pairing real "
        "weights with the hash SimpleTokenizer would feed garbage token ids to the text "
        "encoders (conditioning silently broken). Ship the CLIP BPE files, or pass "
        "allow_simple_tokenizer=True for random-init/debug checkpoints.")


_SCHEDULER_FILE_KEYS = ("prediction_type", "timestep_spacing", "rescale_betas_zero_snr",
                        "beta_start", "beta_end", "steps_offset", "num_train_timesteps")
_SCHEDULER_KWARGS = _SCHEDULER_FILE_KEYS[:3]
# what one scheduler class alone takes (its extra_config_keys)
_SCHEDULER_CLASS_KWARGS = ("eta", "algorithm_type")


def _load_scheduler(name: str, pretrained, kwargs: dict):
    """The scheduler ``name`` configured from the checkpoint's
    ``scheduler/scheduler_config.json`` (the keys above, where present) and
    from ``prediction_type=`` / ``timestep_spacing=`` /
    ``rescale_betas_zero_snr=`` in ``kwargs`` (popped), which win over the
    file. A v-prediction checkpoint run as epsilon-prediction gives noise, so
    the file is read whenever it is there.

    ``eta`` (ddim) and ``algorithm_type`` (dpm-solver) belong to one class
    each: the file's value is taken only by that class, so a file saved with
    one sampler loads into another, and as a keyword (popped) it raises
    ``ValueError`` for a scheduler that lacks it."""
    cls = scheduler_class(name)
    file_keys = _SCHEDULER_FILE_KEYS + cls.extra_config_keys
    config = {}
    if pretrained is not None:
        path = os.path.join(pretrained, "scheduler", "scheduler_config.json")
        if os.path.isfile(path):
            with open(path, encoding="utf-8") as f:
                on_file = json.load(f)
            config = {k: on_file[k] for k in file_keys if k in on_file}
    for key in _SCHEDULER_KWARGS + _SCHEDULER_CLASS_KWARGS:
        if key in kwargs:
            if key in _SCHEDULER_CLASS_KWARGS and key not in cls.extra_config_keys:
                raise ValueError(f"scheduler {name!r} ({cls.__name__}) takes no {key!r}")
            config[key] = kwargs.pop(key)
    return cls(**config)


def _check_guidance_rescale(guidance_rescale: float) -> float:
    if guidance_rescale < 0:
        raise ValueError(f"guidance_rescale must be >= 0, got {guidance_rescale}")
    return float(guidance_rescale)


def _maybe_tqdm(iterable, enabled: bool):
    if not enabled:
        return iterable
    try:
        from tqdm import tqdm

        return tqdm(iterable)
    except ImportError:  # pragma: no cover
        return iterable


class _DistriPipelineBase:
    is_sdxl = False
    # img2img: the VAE encoder is built on first use (the vae_encoder
    # accessor), so a text-to-image pipeline allocates nothing for it
    _vae_encoder: VAEEncoder | None = None
    _pretrained_path: str | None = None  # from_pretrained's checkpoint directory
    _ENCODER_SEED = 0x1E2C0DE  # random-init stream of the encoder, its own

    def __init__(
        self,
        distri_config: DistriConfig,
        unet: DistriUNet,
        vae: VAEDecoder,
        scheduler,
        tokenizer: SimpleTokenizer,
    ):
        self.distri_config = distri_config
        self.unet = unet
        self.vae = vae
        self.scheduler = scheduler
        self.tokenizer = tokenizer
        self.comm_manager: PatchParallelismCommManager | None = None
        self._progress = distri_config.rank == 0 and distri_config.verbose
        self.prepare()

    @staticmethod
    def _load_components(pretrained, components: dict, device, torch_dtype) -> list:
        """Load each named component from the checkpoint directory (when one
        is given), then move it to device / dtype in eval mode. ``components``
        maps checkpoint subfolder -> module; the modules come back in order."""
        if pretrained is not None:
            for comp, model in components.items():
                path = weight_io.find_component_weights(pretrained, comp)
                if path is not None:
                    # the checkpoint holds the plain U-Net inside the DistriUNet wrapper
                    target = model.unet if isinstance(model, DistriUNet) else model
                    weight_io.load_into(target, weight_io.load_safetensors(path))
        return [m.to(device=device, dtype=torch_dtype).eval() for m in components.values()]

    # -- reference-API conveniences -----------------------------------------

    def set_progress_bar_config(self, disable: bool = False, **kwargs):
        self._progress = not disable and self.distri_config.rank == 0

    def save_pretrained(self, out_dir: str) -> None:
        """Write a diffusers-layout safetensors directory loadable by
        ``from_pretrained(pretrained_model_name_or_path=out_dir)``."""
        import os

        from safetensors.torch import save_file

        from .models.weights import export_diffusers_state_dict

        components = {"unet": self.unet.unet, "vae": self.vae}
        # the encoder's keys share the vae file, once an encoder has been built
        extra = {"vae": self._vae_encoder} if self._vae_encoder is not None else {}
        if hasattr(self, "text_encoder"):
            components["text_encoder"] = self.text_encoder
        if hasattr(self, "text_encoder_2"):
            components["text_encoder_2"] = self.text_encoder_2
        for name, model in components.items():
            os.makedirs(os.path.join(out_dir, name), exist_ok=True)
            sd = {k: v.contiguous().cpu() for k, v in export_diffusers_state_dict(model).items()}
            if name in extra:
                sd.update({k: v.contiguous().cpu()
                           for k, v in export_diffusers_state_dict(extra[name]).items()})
            # diffusers repo layout: unet/vae use diffusion_pytorch_model.*,
            # text encoders use model.* (ADVICE r1 — keeps the export loadable
            # by upstream diffusers, not just our own from_pretrained).
            fname = ("diffusion_pytorch_model.safetensors"
                     if name in ("unet", "vae") else "model.safetensors")
            save_file(sd, os.path.join(out_dir, name, fname))
        tokenizers = {"tokenizer": self.tokenizer}
        if getattr(self, "tokenizer_2", None) is not None:
            tokenizers["tokenizer_2"] = self.tokenizer_2
        for sub, tok in tokenizers.items():
            tdir = os.path.join(out_dir, sub)
            os.makedirs(tdir, exist_ok=True)
            with open(os.path.join(tdir, "tokenizer_config.json"), "w", encoding="utf-8") as f:
                json.dump({"tokenizer_class": type(tok).__name__}, f)
            if isinstance(tok, CLIPBPETokenizer):
                import shutil
                shutil.copy(tok.vocab_path, os.path.join(tdir, "vocab.json"))
                shutil.copy(tok.merges_path, os.path.join(tdir, "merges.txt"))
        # the prediction type and the schedule travel with the weights
        sdir = os.path.join(out_dir, "scheduler")
        os.makedirs(sdir, exist_ok=True)
        with open(os.path.join(sdir, "scheduler_config.json"), "w", encoding="utf-8") as f:
            json.dump({"_class_name": type(self.scheduler).__name__, **self.scheduler.config()},
                      f, indent=2)

    @property
    def device(self):
        return self.distri_config.device

    # -- core helpers --------------------------------------------------------

    def _unet_dtype(self) -> torch.dtype:
        return next(self.unet.parameters()).dtype

    def _prepare_latents(self, batch_size: int, generator,
                         channels: int | None = None) -> torch.Tensor:
        """Initial noise with the VAE's latent channels, or with ``channels``
        (the U-Net's input width for the static graph inputs: a 9-channel
        inpaint U-Net takes more than the latents)."""
        cfg = self.distri_config
        if channels is None:
            channels = self.vae.config.latent_channels
        shape = (batch_size, channels, cfg.height // 8, cfg.width // 8)
        if generator is None:
            # Cross-rank determinism: every rank MUST sample identical initial
            # latents (they denoise the same image). Default to a fixed seed.
            generator = torch.Generator().manual_seed(0)
        device = generator.device if hasattr(generator, "device") else torch.device("cpu")
        latents = torch.randn(shape, generator=generator, dtype=torch.float32, device=device)
        latents = latents.to(device=cfg.device, dtype=self._unet_dtype())
        return latents * self.scheduler.init_noise_sigma

    # -- img2img ---------------------------------------------------------------

    @property
    def vae_encoder(self) -> VAEEncoder:
        """The VAE encoder, built on first access.

        It is built inside ``torch.random.fork_rng`` from a fixed seed of its
        own, so building it never advances the global CPU or GPU generators
        (``from_pretrained``'s seeded construction order is untouched), and it
        loads the checkpoint's ``encoder.*`` / ``quant_conv.*`` weights when
        the pipeline came from a checkpoint directory."""
        if self._vae_encoder is None:
            with torch.random.fork_rng(devices=[]):
                # the CPU generator only: modules are initialised on the CPU
                torch.default_generator.manual_seed(self._ENCODER_SEED)
                enc = VAEEncoder(self.vae.config)
            if self._pretrained_path is not None:
                path = weight_io.find_component_weights(self._pretrained_path, "vae")
                if path is not None:
                    weight_io.load_into(enc, weight_io.load_safetensors(path))
            ref = next(self.vae.parameters())
            self._vae_encoder = enc.to(device=ref.device, dtype=ref.dtype).eval()
        return self._vae_encoder

    def _prepare_image(self, image) -> torch.Tensor:
        """A float tensor [3,H,W] / [1,3,H,W] in [0, 1], a uint8 HWC numpy
        array or a PIL image -> [1,3,H,W] in [-1, 1] on the model device. H, W
        must be DistriConfig's: nothing is resized."""
        cfg = self.distri_config
        if not torch.is_tensor(image):
            import numpy as np

            if not isinstance(image, np.ndarray):
                try:
                    from PIL import Image
                except ImportError:
                    Image = None
                if Image is None or not isinstance(image, Image.Image):
                    raise TypeError(f"image: unsupported type {type(image).__name__}")
                image = np.array(image.convert("RGB"))
            if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
                raise ValueError("image: a numpy image must be uint8 [H, W, 3], got "
                                 f"{image.dtype} {image.shape}")
            image = torch.from_numpy(np.ascontiguousarray(image)).permute(2, 0, 1).float() / 255.0
        elif not image.is_floating_point():
            raise ValueError("image: a tensor image must be floating point in [0, 1]")
        if image.dim() == 3:
            image = image[None]
        if image.dim() != 4 or image.shape[0] != 1 or image.shape[1] != 3:
            raise ValueError(f"image: expected [3,H,W] or [1,3,H,W], got {tuple(image.shape)}")
        if tuple(image.shape[2:]) != (cfg.height, cfg.width):
            raise ValueError(
                f"image is {image.shape[2]}x{image.shape[3]} but the pipeline is built for "
                f"{cfg.height}x{cfg.width} (DistriConfig); resize it first")
        image = image.float() * 2.0 - 1.0
        return image.to(device=cfg.device, dtype=next(self.vae.parameters()).dtype)

    def _img2img_latents(self, image, strength: float, num_inference_steps: int, generator):
        """Encode ``image``, sample the posterior, and noise it to the first
        executed timestep. Returns (latents, t_start). Every rank encodes the
        full image (replicated work, as decode is) and, drawing from equal
        generators, holds identical latents. The posterior sample is drawn
        first and the noise after it, from the same generator."""
        t_start = img2img_start(num_inference_steps, strength)
        pixels = self._prepare_image(image)
        if generator is None:
            generator = torch.Generator().manual_seed(0)  # same on every rank
        from .utils.tracing import trace_range

        with trace_range("vae_encode"):
            init = self.vae_encoder.encode(pixels, generator=generator)
        device = generator.device if hasattr(generator, "device") else torch.device("cpu")
        noise = torch.randn(init.shape, generator=generator, dtype=torch.float32, device=device)
        self.scheduler.set_timesteps(num_inference_steps, device=None)
        # strength = 1 still noises the image at the first timestep; and no
        # init_noise_sigma here: add_noise already lands on sigma_t
        latents = self.scheduler.add_noise(init.float(), noise.to(init.device),
                                           self.scheduler.timesteps[t_start])
        return latents.to(self._unet_dtype()), t_start

    # -- inpainting ------------------------------------------------------------

    def _prepare_mask(self, mask) -> torch.Tensor:
        """A float tensor [H,W] / [1,H,W] / [1,1,H,W] in [0, 1], a uint8 [H,W]
        numpy array (0..255) or a PIL image (converted to "L") -> the binary
        pixel mask, fp32 [1,1,H,W] on the model device: 1 (values >= 0.5)
        means repaint. H, W must be DistriConfig's: nothing is resized."""
        cfg = self.distri_config
        if not torch.is_tensor(mask):
            import numpy as np

            if not isinstance(mask, np.ndarray):
                try:
                    from PIL import Image
                except ImportError:
                    Image = None
                if Image is None or not isinstance(mask, Image.Image):
                    raise TypeError(f"mask: unsupported type {type(mask).__name__}")
                mask = np.array(mask.convert("L"))
            if mask.dtype != np.uint8 or mask.ndim != 2:
                raise ValueError("mask: a numpy mask must be uint8 [H, W], got "
                                 f"{mask.dtype} {mask.shape}")
            mask = torch.from_numpy(np.ascontiguousarray(mask)).float() / 255.0
        elif not mask.is_floating_point():
            raise ValueError("mask: a tensor mask must be floating point in [0, 1]")
        if mask.dim() not in (2, 3, 4) or any(s != 1 for s in mask.shape[:-2]):
            raise ValueError(f"mask: expected [H,W], [1,H,W] or [1,1,H,W], got {tuple(mask.shape)}")
        if tuple(mask.shape[-2:]) != (cfg.height, cfg.width):
            raise ValueError(
                f"mask is {mask.shape[-2]}x{mask.shape[-1]} but the pipeline is built for "
                f"{cfg.height}x{cfg.width} (DistriConfig); resize it first")
        mask = mask.reshape(1, 1, cfg.height, cfg.width)
        return (mask.float() >= 0.5).float().to(cfg.device)

    @staticmethod
    def _latent_mask(pixel_mask: torch.Tensor) -> torch.Tensor:
        """The mask at latent resolution by nearest sampling: latent pixel
        (i, j) takes mask pixel (8i, 8j), which is what ``F.interpolate`` to
        (H/8, W/8) in its default nearest mode gives (the diffusers rule)."""
        return pixel_mask[..., ::8, ::8].contiguous()

    def _inpaint_latents(self, image, mask, strength: float, num_inference_steps: int,
                         generator):
        """Returns (latents, t_start, inpaint): the start latents, the first
        executed step and what every step's blend needs. One generator gives,
        in this order, the posterior sample of ``image``, the posterior sample
        of the masked image (9-channel U-Nets only) and the noise. strength < 1
        starts as img2img does, from the image noised to the first executed
        timestep; strength = 1 starts from pure noise, and the same noise
        tensor re-noises the known region at every step."""
        t_start = img2img_start(num_inference_steps, strength)
        pixels = self._prepare_image(image)
        pixel_mask = self._prepare_mask(mask)
        if generator is None:
            generator = torch.Generator().manual_seed(0)  # same on every rank
        from .utils.tracing import trace_range

        dtype = self._unet_dtype()
        inpaint = {"mask": self._latent_mask(pixel_mask)}
        with trace_range("vae_encode"):
            inpaint["init"] = self.vae_encoder.encode(pixels, generator=generator).float()
            if self.unet.config.in_channels == 9:
                keep = (pixel_mask < 0.5).to(pixels.dtype)
                masked = self.vae_encoder.encode(pixels * keep, generator=generator)
                inpaint["masked_latents"] = masked.to(dtype)
                inpaint["mask_in"] = inpaint["mask"].to(dtype)
        init = inpaint["init"]
        device = generator.device if hasattr(generator, "device") else torch.device("cpu")
        noise = torch.randn(init.shape, generator=generator, dtype=torch.float32, device=device)
        inpaint["init_noise"] = noise.to(init.device)
        self.scheduler.set_timesteps(num_inference_steps, device=None)
        if strength < 1:
            latents = self.scheduler.add_noise(init, inpaint["init_noise"],
                                               self.scheduler.timesteps[t_start]).to(dtype)
        else:
            latents = inpaint["init_noise"].to(dtype) * self.scheduler.init_noise_sigma
        return latents, t_start, inpaint

    def _denoise(self, latents, prompt_embeds, added_cond_kwargs, num_inference_steps,
                 guidance_scale, t_start: int = 0, inpaint: dict | None = None,
                 guidance_rescale: float = 0.0):
        """``t_start > 0`` (img2img) runs the last n - t_start steps only. The
        U-Net counter is 0 at the first step that actually runs, so the
        ``warmup_steps`` synchronous steps of displaced patch parallelism are
        counted from there, and the captured graphs and ``_graph_counters``
        are the text-to-image ones.

        ``inpaint`` (from ``_inpaint_latents``) ends every step in the
        scheduler's ``masked_step`` and, with a 9-channel U-Net, assembles the
        U-Net input with ``ops.inpaint_unet_input``. Every rank holds the full
        latents, so the blend is replicated work like the step itself.

        ``guidance_rescale`` > 0 goes to the scheduler's ``guided_step`` /
        ``masked_step`` (the factor op and the fused step with it: three
        launches on GPU); 0, or classifier-free guidance off, makes the calls
        made without it."""
        cfg = self.distri_config
        do_cfg = cfg.do_classifier_free_guidance
        # keyword passed only when set: a plain step is the call it always was
        rescale = {"guidance_rescale": guidance_rescale} if do_cfg and guidance_rescale > 0 else {}
        from .utils.tracing import trace_range

        self.scheduler.set_timesteps(num_inference_steps, device=None)
        if t_start:
            self.scheduler.set_begin_index(t_start)
        self.unet.set_counter(0)
        for i, t in enumerate(_maybe_tqdm(self.scheduler.timesteps, self._progress)):
            with trace_range(f"denoise_step_{i}"):
                if inpaint is not None and "masked_latents" in inpaint:
                    latent_in = ops.inpaint_unet_input(
                        latents, inpaint["mask_in"], inpaint["masked_latents"],
                        self.scheduler.model_input_scale(t), 2 if do_cfg else 1)
                else:
                    latent_in = torch.cat([latents] * 2) if do_cfg else latents
                    latent_in = self.scheduler.scale_model_input(latent_in, t)
                noise = self.unet(
                    latent_in,
                    t.to(cfg.device) if torch.is_tensor(t) else t,
                    prompt_embeds,
                    added_cond_kwargs,
                )
                if inpaint is not None:
                    latents = self.scheduler.masked_step(
                        noise, t, latents, guidance_scale, inpaint["mask"], inpaint["init"],
                        inpaint["init_noise"], **rescale)
                elif do_cfg and hasattr(self.scheduler, "guided_step"):
                    latents = self.scheduler.guided_step(noise, t, latents, guidance_scale,
                                                         **rescale)
                else:
                    if do_cfg:
                        n_uncond, n_cond = noise.chunk(2)
                        noise = n_uncond + guidance_scale * (n_cond - n_uncond)
                    latents = self.scheduler.step(noise, t, latents)
        return latents

    def _generate(self, embeds, added_cond_kwargs, num_inference_steps, guidance_scale,
                  generator, output_type, image, strength, mask=None,
                  guidance_rescale: float = 0.0):
        """The tail both pipelines share once the prompt is encoded: initial
        (or img2img, or inpaint) latents -> denoise -> decode. ``strength``
        None is 0.3 for img2img and 1.0 for inpainting."""
        guidance_rescale = _check_guidance_rescale(guidance_rescale)
        if mask is not None and image is None:
            raise ValueError("mask= needs image=: inpainting repaints part of an image")
        if self.unet.config.in_channels == 9 and mask is None:
            raise ValueError("a 9-channel inpaint U-Net needs image= and mask=")
        t_start, inpaint = 0, None
        stochastic = getattr(self.scheduler, "stochastic", False)
        if stochastic and generator is None:
            # the fixed-seed generator the latents fall back to, kept to draw
            # the noise seed after them (the same on every rank)
            generator = torch.Generator().manual_seed(0)
        if image is None:
            latents = self._prepare_latents(1, generator)
        elif mask is None:
            latents, t_start = self._img2img_latents(
                image, 0.3 if strength is None else strength, num_inference_steps, generator)
        else:
            latents, t_start, inpaint = self._inpaint_latents(
                image, mask, 1.0 if strength is None else strength, num_inference_steps,
                generator)
        if stochastic:
            # one draw seeds every step's noise (a counter-based generator in
            # the fused step kernels): every rank, holding an equal generator,
            # adds the same noise. A deterministic scheduler draws nothing.
            device = generator.device if hasattr(generator, "device") else torch.device("cpu")
            seed = torch.randint(0, 2**63 - 1, (1,), generator=generator, device=device)
            self.scheduler.set_noise_seed(int(seed))
        latents = self._denoise(latents, embeds, added_cond_kwargs, num_inference_steps,
                                guidance_scale, t_start, inpaint, guidance_rescale)
        return self._decode(latents, output_type)

    def _decode(self, latents: torch.Tensor, output_type: str):
        # High-resolution decode: the VAE mid-attention is O(L^2) in latent
        # tokens, so >= 2048^2 outputs use tiled decode automatically
        # (diffusers enable_tiling parity; ~0.7 s at 3840^2 vs ~30 min full)
        if latents.shape[-1] >= 256 or latents.shape[-2] >= 256:
            self.vae.enable_tiling()
        if output_type == "latent":
            return latents
        images = self.vae.decode(latents.to(self._unet_dtype()))
        if output_type == "pt":
            return images
        arr = ((images.float() / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8)
        arr = arr.permute(0, 2, 3, 1).cpu().numpy()
        if output_type == "np":
            return arr
        try:  # "pil"
            from PIL import Image

            return [Image.fromarray(a) for a in arr]
        except ImportError:
            return arr  # no pillow in this environment; numpy HWC uint8

    # -- prepare: registration pass, comm buffer, pre-run, hipGraph capture --

    @torch.no_grad()
    def prepare(self):
        cfg = self.distri_config
        unet = self.unet

        if cfg.device.type == "cuda":
            # MIOpen find mode for whichever convs still ride torch ops: the
            # immediate-mode default picks im2col paths at large resolutions
            # (profiles/rocprof_3840_r01.md). Applies to every entry point,
            # not just bench.py.
            torch.backends.cudnn.benchmark = True

        needs_comm = cfg.parallelism == "patch" and cfg.n_device_per_batch > 1
        wants_graphs = cfg.use_cuda_graph and cfg.device.type == "cuda"
        if not needs_comm and not wants_graphs:
            return  # nothing to warm up
        batch_size = 2 if cfg.do_classifier_free_guidance else 1

        static = self._build_static_inputs(batch_size)

        if needs_comm:
            self.comm_manager = PatchParallelismCommManager(cfg)
            unet.set_comm_manager(self.comm_manager)
            # registration pass: sizes every stale-activation slot
            unet.set_counter(0)
            unet(**static, record=True)
            self.comm_manager.create_buffer()

        # pre-run: modules grab their buffer views and fill them
        unet.set_counter(0)
        unet(**static, record=True)
        if self.comm_manager is not None:
            self.comm_manager.clear()

        if cfg.use_cuda_graph and cfg.device.type == "cuda":
            self._capture_graphs(static)

    def _graph_counters(self) -> list[int]:
        cfg = self.distri_config
        if cfg.world_size == 1 or cfg.n_device_per_batch == 1:
            return [0]
        if cfg.parallelism == "patch":
            return [0, cfg.warmup_steps + 1, cfg.warmup_steps + 2]
        if cfg.parallelism == "naive_patch" and cfg.split_scheme == "alternate":
            return [0, 1]
        return [0]

    def _capture_graphs(self, static):
        import torch.distributed as dist

        unet = self.unet
        cfg = self.distri_config
        graphs, outputs = [], []
        ok = True
        try:
            torch.cuda.synchronize()
            for counter in self._graph_counters():
                g = torch.cuda.CUDAGraph()
                unet.set_counter(counter)
                with torch.cuda.graph(g):
                    out = unet(**static, record=True)
                graphs.append(g)
                outputs.append(out)
        except Exception as exc:  # pragma: no cover - depends on RCCL graph support
            ok = False
            if cfg.rank == 0:
                print(f"[distrifuser_amd] hipGraph capture failed ({exc}); running eager")
        # Consensus: if ANY rank failed to capture, all ranks must run eager,
        # otherwise collective counts diverge and the job deadlocks.
        if cfg.world_size > 1 and dist.is_initialized():
            flag = torch.tensor([0 if ok else 1], device=cfg.device)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            ok = flag.item() == 0
        if ok:
            unet.setup_cuda_graph(outputs, graphs)
        else:
            unet.setup_cuda_graph(None, None)
            if self.comm_manager is not None:
                self.comm_manager.clear()

    def _build_static_inputs(self, batch_size: int) -> dict:
        raise NotImplementedError


class DistriSDXLPipeline(_DistriPipelineBase):
    is_sdxl = True

    def __init__(self, distri_config, unet, vae, text_encoder, text_encoder_2, scheduler,
                 tokenizer, tokenizer_2=None):
        self.text_encoder = text_encoder
        self.text_encoder_2 = text_encoder_2
        self.tokenizer_2 = tokenizer_2
        super().__init__(distri_config, unet, vae, scheduler, tokenizer)

    @staticmethod
    def from_pretrained(distri_config: DistriConfig, **kwargs):
        pretrained = kwargs.pop("pretrained_model_name_or_path", None)
        torch_dtype = kwargs.pop("torch_dtype", torch.bfloat16)
        scheduler = _load_scheduler(kwargs.pop("scheduler", "ddim"), pretrained, kwargs)
        preset = kwargs.pop("preset", "sdxl")
        allow_simple = kwargs.pop("allow_simple_tokenizer", False)

        if preset == "tiny":
            unet_cfg, vae_cfg = TINY_UNET, TINY_VAE
            clip1_cfg, clip2_cfg = TINY_CLIP, TINY_CLIP
        else:
            unet_cfg = SDXL_INPAINT_UNET if preset == "sdxl-inpaint" else SDXL_UNET
            vae_cfg = SDXL_VAE
            clip1_cfg, clip2_cfg = CLIP_VIT_L, OPEN_CLIP_BIG_G
        tokenizer = _resolve_tokenizer(pretrained, clip1_cfg.vocab_size,
                                       allow_simple=allow_simple)
        # SDXL's second tokenizer (open-CLIP) pads with 0 ("!"), not eos.
        tokenizer_2 = _resolve_tokenizer(pretrained, clip2_cfg.vocab_size,
                                         subfolder="tokenizer_2", pad_with_zero=True,
                                         allow_simple=allow_simple)
        unet_cfg = kwargs.pop("unet_config", unet_cfg)

        unet = DistriUNet(unet_cfg, distri_config)
        vae = VAEDecoder(vae_cfg)
        te1 = CLIPTextEncoder(clip1_cfg)
        te2 = CLIPTextEncoder(clip2_cfg)
        unet, vae, te1, te2 = _DistriPipelineBase._load_components(
            pretrained, {"unet": unet, "vae": vae, "text_encoder": te1, "text_encoder_2": te2},
            distri_config.device, torch_dtype)
        pipeline = DistriSDXLPipeline(distri_config, unet, vae, te1, te2,
                                      scheduler, tokenizer,
                                      tokenizer_2=tokenizer_2)
        pipeline._pretrained_path = pretrained  # for the lazily built VAE encoder
        return pipeline

    @torch.no_grad()
    def encode_prompt(self, prompt, negative_prompt=None, do_classifier_free_guidance=True):
        """Returns (prompt_embeds [B,77,2048], pooled [B,1280]) per branch,
        concatenated [uncond; cond] when CFG is on."""
        device = self.distri_config.device
        tok2 = self.tokenizer_2 if self.tokenizer_2 is not None else self.tokenizer
        ids1 = self.tokenizer(prompt, device=device)
        ids2 = tok2(prompt, device=device)
        emb1, _ = self.text_encoder(ids1, hidden_state_index=-2)
        emb2, pooled = self.text_encoder_2(ids2, hidden_state_index=-2)
        embeds = torch.cat([emb1, emb2], dim=-1)
        if not do_classifier_free_guidance:
            return embeds, pooled
        neg = negative_prompt if negative_prompt is not None else ""
        nids = self.tokenizer(neg, device=device)
        nids2 = tok2(neg, device=device)
        nemb1, _ = self.text_encoder(nids, hidden_state_index=-2)
        nemb2, npooled = self.text_encoder_2(nids2, hidden_state_index=-2)
        nembeds = torch.cat([nemb1, nemb2], dim=-1)
        return torch.cat([nembeds, embeds]), torch.cat([npooled, pooled])

    def _added_cond(self, batch_size: int, pooled: torch.Tensor) -> dict:
        cfg = self.distri_config
        time_ids = torch.tensor(
            [[cfg.height, cfg.width, 0, 0, cfg.height, cfg.width]],
            device=cfg.device, dtype=pooled.dtype,
        ).repeat(batch_size, 1)
        return {"text_embeds": pooled, "time_ids": time_ids}

    def _build_static_inputs(self, batch_size: int) -> dict:
        embeds, pooled = self.encode_prompt("", do_classifier_free_guidance=False)
        embeds = embeds.repeat(batch_size, 1, 1).to(self._unet_dtype())
        pooled = pooled.repeat(batch_size, 1).to(self._unet_dtype())
        latents = self._prepare_latents(batch_size, None, self.unet.config.in_channels)
        return {
            "sample": latents,
            "timestep": torch.zeros((), dtype=torch.float32, device=self.distri_config.device),
            "encoder_hidden_states": embeds,
            "added_cond_kwargs": self._added_cond(batch_size, pooled),
        }

    @torch.no_grad()
    def __call__(
        self,
        prompt: str = "",
        negative_prompt: str | None = None,
        num_inference_steps: int = 50,
        guidance_scale: float = 5.0,
        generator: torch.Generator | None = None,
        output_type: str = "pil",
        image=None,
        strength: float | None = None,
        mask=None,
        guidance_rescale: float = 0.0,
        **kwargs,
    ):
        """Text-to-image, or with ``image=`` img2img (SDEdit): the image (a
        float tensor [3,H,W] / [1,3,H,W] in [0, 1], a uint8 HWC numpy array
        or a PIL image, at DistriConfig's height x width) is encoded, noised
        to ``strength`` and denoised over the last ``int(steps * strength)``
        steps. The displaced-patch warmup counts from the first step that
        runs (see ``_denoise``). The added time ids are the text-to-image
        ones; there is no refiner aesthetic score.

        With ``mask=`` as well it inpaints: the mask (a float tensor [H,W] /
        [1,H,W] / [1,1,H,W] in [0, 1], a uint8 [H,W] numpy array or a PIL
        image, at the same size) is binarised at 0.5, 1 meaning repaint, and
        taken to latent resolution by nearest sampling (``mask[::8, ::8]``).
        After every step the known region is replaced by the image latents
        noised to the next timestep (and by the clean ones after the last),
        so it comes out as encoded. A 9-channel inpaint U-Net (preset
        ``"sdxl-inpaint"``) is also fed the mask and the masked-image
        latents. ``strength`` defaults to 0.3 for img2img and to 1.0, a start
        from pure noise, with a mask.

        ``guidance_rescale`` (Lin et al., section 3.4; 0.7 is the usual value
        for v-prediction and zero-terminal-SNR checkpoints) scales the guided
        model output towards the cond branch's standard deviation before every
        step. 0 is off; with classifier-free guidance off it is ignored, as
        in diffusers; a negative value raises ``ValueError``. The prediction
        type itself belongs to the scheduler: ``from_pretrained(...,
        prediction_type="v_prediction")`` or the checkpoint's
        ``scheduler/scheduler_config.json``."""
        assert "height" not in kwargs and "width" not in kwargs, (
            "height/width are fixed by DistriConfig (the comm buffers and "
            "graphs are sized for them)"
        )
        cfg = self.distri_config
        if not cfg.do_classifier_free_guidance:
            assert guidance_scale == 1 or guidance_scale is None
            guidance_scale = 1
        do_cfg = cfg.do_classifier_free_guidance

        embeds, pooled = self.encode_prompt(prompt, negative_prompt, do_cfg)
        embeds = embeds.to(self._unet_dtype())
        pooled = pooled.to(self._unet_dtype())
        added = self._added_cond(embeds.shape[0], pooled)
        return self._generate(embeds, added, num_inference_steps, guidance_scale, generator,
                              output_type, image, strength, mask, guidance_rescale)


class DistriSDPipeline(_DistriPipelineBase):
    """SD 1.x/2.x pipeline (single text encoder, no added conditions)."""

    def __init__(self, distri_config, unet, vae, text_encoder, scheduler, tokenizer):
        self.text_encoder = text_encoder
        super().__init__(distri_config, unet, vae, scheduler, tokenizer)

    @staticmethod
    def from_pretrained(distri_config: DistriConfig, **kwargs):
        pretrained = kwargs.pop("pretrained_model_name_or_path", None)
        torch_dtype = kwargs.pop("torch_dtype", torch.bfloat16)
        scheduler = _load_scheduler(kwargs.pop("scheduler", "ddim"), pretrained, kwargs)
        preset = kwargs.pop("preset", "sd15")
        allow_simple = kwargs.pop("allow_simple_tokenizer", False)

        if preset == "tiny":
            unet_cfg = UNetConfig(
                block_out_channels=(32, 64),
                down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
                layers_per_block=1,
                transformer_layers_per_block=(1, 1),
                num_attention_heads=(2, 4),
                cross_attention_dim=16,
                norm_num_groups=8,
                use_linear_projection=False,
                addition_embed_type=None,
                sample_size=8,
            )
            vae_cfg, clip_cfg = TINY_VAE, TINY_CLIP
        elif preset in ("sd21", "sd2"):
            from .models.clip import OPEN_CLIP_VIT_H
            from .models.unet import SD21_UNET

            unet_cfg, vae_cfg, clip_cfg = SD21_UNET, SD_VAE, OPEN_CLIP_VIT_H
        else:
            unet_cfg = SD15_INPAINT_UNET if preset == "sd15-inpaint" else SD15_UNET
            vae_cfg, clip_cfg = SD_VAE, CLIP_VIT_L
        tokenizer = _resolve_tokenizer(pretrained, clip_cfg.vocab_size,
                                       allow_simple=allow_simple)
        unet_cfg = kwargs.pop("unet_config", unet_cfg)

        unet = DistriUNet(unet_cfg, distri_config)
        vae = VAEDecoder(vae_cfg)
        te = CLIPTextEncoder(clip_cfg)
        unet, vae, te = _DistriPipelineBase._load_components(
            pretrained, {"unet": unet, "vae": vae, "text_encoder": te},
            distri_config.device, torch_dtype)
        pipeline = DistriSDPipeline(distri_config, unet, vae, te, scheduler, tokenizer)
        pipeline._pretrained_path = pretrained  # for the lazily built VAE encoder
        return pipeline

    @torch.no_grad()
    def encode_prompt(self, prompt, negative_prompt=None, do_classifier_free_guidance=True):
        device = self.distri_config.device
        ids = self.tokenizer(prompt, device=device)
        emb, _ = self.text_encoder(ids, hidden_state_index=-1)
        if not do_classifier_free_guidance:
            return emb
        neg = negative_prompt if negative_prompt is not None else ""
        nids = self.tokenizer(neg, device=device)
        nemb, _ = self.text_encoder(nids, hidden_state_index=-1)
        return torch.cat([nemb, emb])

    def _build_static_inputs(self, batch_size: int) -> dict:
        embeds = self.encode_prompt("", do_classifier_free_guidance=False)
        embeds = embeds.repeat(batch_size, 1, 1).to(self._unet_dtype())
        latents = self._prepare_latents(batch_size, None, self.unet.config.in_channels)
        return {
            "sample": latents,
            "timestep": torch.zeros((), dtype=torch.float32, device=self.distri_config.device),
            "encoder_hidden_states": embeds,
            "added_cond_kwargs": None,
        }

    @torch.no_grad()
    def __call__(
        self,
        prompt: str = "",
        negative_prompt: str | None = None,
        num_inference_steps: int = 50,
        guidance_scale: float = 7.5,
        generator: torch.Generator | None = None,
        output_type: str = "pil",
        image=None,
        strength: float | None = None,
        mask=None,
        guidance_rescale: float = 0.0,
        **kwargs,
    ):
        """Text-to-image, img2img with ``image=`` / ``strength=``, or
        inpainting with ``mask=`` as well (see ``DistriSDXLPipeline.__call__``,
        also for ``guidance_rescale``; the 9-channel preset here is
        ``"sd15-inpaint"``)."""
        assert "height" not in kwargs and "width" not in kwargs
        cfg = self.distri_config
        if not cfg.do_classifier_free_guidance:
            guidance_scale = 1
        do_cfg = cfg.do_classifier_free_guidance
        embeds = self.encode_prompt(prompt, negative_prompt, do_cfg).to(self._unet_dtype())
        return self._generate(embeds, None, num_inference_steps, guidance_scale, generator,
                              output_type, image, strength, mask, guidance_rescale)
