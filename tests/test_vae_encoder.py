"""VAEEncoder on the CPU: shapes, the forward against an independent functional
oracle that reads the exported diffusers-layout state dict (which also checks
the key map), the weight round trip, posterior sampling and tiled encode."""

import functools

import pytest
import torch
import torch.nn.functional as F

from distrifuser_amd.models import weights as weight_io
from distrifuser_amd.models.vae import SD_VAE, TINY_VAE, VAEEncoder


@functools.lru_cache(maxsize=None)
def _tiny_encoder():
    """Shared and never modified (tiling is switched on copies of its state)."""
    torch.manual_seed(11)
    enc = VAEEncoder(TINY_VAE).eval()
    # default init leaves logvar near 0 and the attention nearly uniform; widen
    # the weights a little so the oracle comparison exercises every layer
    with torch.no_grad():
        for p in enc.parameters():
            p.mul_(1.5)
    return enc


def _fresh_tiny():
    enc = VAEEncoder(TINY_VAE).eval()
    enc.load_state_dict(_tiny_encoder().state_dict())
    return enc


def _image(b, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(b, 3, h, w, generator=g) * 2 - 1


# ---- the oracle: F.pad / F.conv2d / F.group_norm / F.silu / softmax only --------


def _oracle_moments(sd, cfg, x):
    groups = cfg.norm_num_groups

    def conv(p, t, stride=1, padding=1):
        return F.conv2d(t, sd[p + ".weight"], sd[p + ".bias"], stride=stride, padding=padding)

    def norm(p, t):
        return F.group_norm(t, groups, sd[p + ".weight"], sd[p + ".bias"], eps=1e-6)

    def resnet(p, t):
        h = conv(p + ".conv1", F.silu(norm(p + ".norm1", t)))
        h = conv(p + ".conv2", F.silu(norm(p + ".norm2", h)))
        if p + ".conv_shortcut.weight" in sd:
            t = conv(p + ".conv_shortcut", t, padding=0)
        return t + h

    def attention(p, t):
        b, c, hh, ww = t.shape
        n = norm(p + ".group_norm", t).permute(0, 2, 3, 1).reshape(b, hh * ww, c)
        lin = lambda name: n @ sd[f"{p}.{name}.weight"].T + sd[f"{p}.{name}.bias"]
        q, k, v = lin("to_q"), lin("to_k"), lin("to_v")
        probs = torch.softmax(q @ k.transpose(1, 2) * c ** -0.5, dim=-1)
        o = (probs @ v) @ sd[p + ".to_out.0.weight"].T + sd[p + ".to_out.0.bias"]
        return t + o.reshape(b, hh, ww, c).permute(0, 3, 1, 2)

    h = conv("encoder.conv_in", x)
    nblocks = len(cfg.block_out_channels)
    for i in range(nblocks):
        for j in range(cfg.layers_per_block):
            h = resnet(f"encoder.down_blocks.{i}.resnets.{j}", h)
        if i < nblocks - 1:
            h = conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", F.pad(h, (0, 1, 0, 1)),
                     stride=2, padding=0)
    h = resnet("encoder.mid_block.resnets.0", h)
    h = attention("encoder.mid_block.attentions.0", h)
    h = resnet("encoder.mid_block.resnets.1", h)
    h = conv("encoder.conv_out", F.silu(norm("encoder.conv_norm_out", h)))
    h = conv("quant_conv", h, padding=0)
    mean, logvar = h.chunk(2, dim=1)
    return mean, logvar.clamp(-30.0, 20.0)


# ---- shapes ------------------------------------------------------------------------


def test_shapes_tiny_and_sd():
    enc = _tiny_encoder()
    assert enc.encode(_image(2, 64, 48), sample=False).shape == (2, 4, 8, 6)
    torch.manual_seed(0)
    sd_enc = VAEEncoder(SD_VAE).eval()
    out = sd_enc.encode(_image(1, 32, 32), generator=torch.Generator().manual_seed(0))
    assert out.shape == (1, 4, 4, 4) and torch.isfinite(out).all()


def test_presets_keep_their_decoder_meaning():
    from distrifuser_amd.models.vae import SDXL_VAE, VAEDecoder

    assert (SDXL_VAE.latent_channels, SDXL_VAE.out_channels, SDXL_VAE.scaling_factor) == \
        (4, 3, 0.13025)
    assert SD_VAE.scaling_factor == 0.18215 and SD_VAE.block_out_channels == (128, 256, 512, 512)
    assert TINY_VAE.block_out_channels == (16, 16, 32, 32) and TINY_VAE.layers_per_block == 1
    assert VAEDecoder(TINY_VAE)(torch.zeros(1, 4, 2, 2)).shape == (1, 3, 16, 16)


def test_asym_pad_conv_keeps_a_plain_state_dict():
    from distrifuser_amd.ops import NativeConv2d

    m = NativeConv2d(4, 8, 3, stride=2, padding=0, asym_pad=True)
    assert sorted(m.state_dict()) == ["bias", "weight"]
    x = torch.randn(1, 4, 6, 8)
    want = F.conv2d(F.pad(x, (0, 1, 0, 1)), m.weight, m.bias, stride=2)
    assert torch.equal(m(x), want)
    with pytest.raises(ValueError):
        NativeConv2d(4, 8, 3, stride=1, padding=0, asym_pad=True)


# ---- forward vs oracle, key map ------------------------------------------------------


def test_forward_matches_functional_oracle():
    enc = _tiny_encoder()
    sd = weight_io.export_diffusers_state_dict(enc)
    x = _image(2, 40, 56, seed=3)
    mean, logvar = enc.encode_moments(x)
    o_mean, o_logvar = _oracle_moments(sd, TINY_VAE, x)
    scale = max(o_mean.abs().max().item(), o_logvar.abs().max().item(), 1.0)
    # fp32 round-off through ~20 layers: a few hundred ulp of the largest value
    tol = 512 * torch.finfo(torch.float32).eps * scale
    assert (mean - o_mean).abs().max().item() <= tol
    assert (logvar - o_logvar).abs().max().item() <= tol
    assert o_mean.abs().max() > 1e-3  # not a vacuous all-zero comparison


def test_diffusers_key_names():
    keys = set(weight_io.export_diffusers_state_dict(_tiny_encoder()))
    for k in ("encoder.conv_in.weight", "encoder.down_blocks.0.resnets.0.conv1.weight",
              "encoder.down_blocks.2.downsamplers.0.conv.bias",
              "encoder.mid_block.resnets.1.norm2.weight",
              "encoder.mid_block.attentions.0.to_out.0.weight",
              "encoder.mid_block.attentions.0.group_norm.bias",
              "encoder.conv_norm_out.weight", "encoder.conv_out.bias", "quant_conv.weight"):
        assert k in keys, k
    assert not any("downsamplers" in k for k in keys if k.startswith("encoder.down_blocks.3"))
    assert all(k.startswith(("encoder.", "quant_conv.")) for k in keys)


def test_export_load_round_trip_is_bit_exact():
    src = _tiny_encoder()
    sd = weight_io.export_diffusers_state_dict(src)
    torch.manual_seed(99)
    dst = VAEEncoder(TINY_VAE)
    native, missing = weight_io.state_dict_to_native(dst, sd)
    assert missing == []
    weight_io.load_into(dst, sd)
    want = src.state_dict()
    got = dst.state_dict()
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


# ---- sampling ----------------------------------------------------------------------


def test_sampling_mode_determinism_and_clamp():
    enc = _tiny_encoder()
    x = _image(1, 32, 32, seed=5)
    mean, logvar = enc.encode_moments(x)
    assert torch.equal(enc.encode(x, sample=False), mean * TINY_VAE.scaling_factor)
    a = enc.encode(x, generator=torch.Generator().manual_seed(1))
    b = enc.encode(x, generator=torch.Generator().manual_seed(1))
    c = enc.encode(x, generator=torch.Generator().manual_seed(2))
    assert torch.equal(a, b) and not torch.equal(a, c)
    # the sample is mean + std * N(0, 1) from that generator, drawn in fp32
    n = torch.randn(mean.shape, generator=torch.Generator().manual_seed(1))
    want = (mean + torch.exp(0.5 * logvar) * n) * TINY_VAE.scaling_factor
    assert torch.allclose(a, want, rtol=0, atol=1e-5)


def test_logvar_is_clamped():
    enc = _fresh_tiny()
    with torch.no_grad():
        enc.quant_conv.bias[:4] = 0.0
        enc.quant_conv.bias[4:6] = 1000.0   # logvar channels 0, 1
        enc.quant_conv.bias[6:] = -1000.0   # logvar channels 2, 3
    _, logvar = enc.encode_moments(_image(1, 16, 16))
    assert (logvar[:, :2] == 20.0).all() and (logvar[:, 2:] == -30.0).all()


# ---- tiling --------------------------------------------------------------------------


def test_tiled_equals_untiled_when_one_tile_holds_the_image():
    enc = _fresh_tiny()
    x = _image(1, 32, 32, seed=7)
    ref = enc.encode_moments(x)
    enc.enable_tiling(tile_latent_size=4, tile_overlap=1)  # 32 px tile
    got = enc.encode_moments(x)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert enc.use_tiling  # an explicit enable_tiling is not undone


def test_tiled_2x2_unblended_positions_equal_their_tile():
    """Tile 4 latents (32 px), overlap 1, stride 3 (24 px); a 56-px image has
    tiles at 0 and 24 px on each axis, both full. Output latent rows / cols
    0..2 come from the first tile and 3..6 from the second, whose first row /
    col is the blend ramp: everything else must be the tile's own encode."""
    enc = _fresh_tiny()
    x = _image(1, 56, 56, seed=8)
    enc.enable_tiling(tile_latent_size=4, tile_overlap=1)
    mean, logvar = enc.encode_moments(x)
    assert mean.shape == (1, 4, 7, 7)
    plain = _tiny_encoder()
    tile = {(y0, x0): plain.encode_moments(x[:, :, y0 : y0 + 32, x0 : x0 + 32])
            for y0 in (0, 24) for x0 in (0, 24)}
    for k, got in enumerate((mean, logvar)):
        # first tile: its kept 3x3 block is untouched
        assert torch.allclose(got[:, :, :3, :3], tile[(0, 0)][k][:, :, :3, :3], atol=1e-5)
        # last tile: rows/cols 1.. of the tile (output 4..6) are past the ramp
        assert torch.allclose(got[:, :, 4:, 4:], tile[(24, 24)][k][:, :, 1:, 1:], atol=1e-5)
        assert torch.allclose(got[:, :, :3, 4:], tile[(0, 24)][k][:, :, :3, 1:], atol=1e-5)
        assert torch.allclose(got[:, :, 4:, :3], tile[(24, 0)][k][:, :, 1:, :3], atol=1e-5)
    # the ramp starts at weight 0 for the new tile: column 3 still is the left tile's
    assert torch.allclose(mean[:, :, :3, 3], tile[(0, 0)][0][:, :, :3, 3], atol=1e-5)


def test_tiled_ragged_size():
    enc = _fresh_tiny()
    enc.enable_tiling(tile_latent_size=4, tile_overlap=1)
    mean, logvar = enc.encode_moments(_image(1, 72, 40, seed=9))
    assert mean.shape == logvar.shape == (1, 4, 9, 5)
    assert torch.isfinite(mean).all() and torch.isfinite(logvar).all()
    out = enc.encode(_image(1, 72, 40, seed=9), sample=False)
    assert out.shape == (1, 4, 9, 5)


def test_auto_tiling_restores_the_state_it_found():
    enc = _fresh_tiny()
    assert VAEEncoder.auto_tiling_min_latent == 256  # the decode trigger
    enc.auto_tiling_min_latent = 16  # same code path at a CPU-sized image
    calls = []
    real = enc._encode_tiled
    enc._encode_tiled = lambda t: (calls.append((enc.use_tiling, enc.tile_latent_size,
                                                 enc.tile_overlap)), real(t))[1]
    enc.tile_latent_size, enc.tile_overlap = 5, 2   # stale settings from an earlier use
    x = _image(1, 128, 776, seed=10)                # latent 16 x 97: one side over the tile
    mean, _ = enc.encode_moments(x)
    assert mean.shape == (1, 4, 16, 97)
    assert calls == [(True, 96, 16)]                # tiled, with the default settings
    assert (enc.use_tiling, enc.tile_latent_size, enc.tile_overlap) == (False, 5, 2)
    # below the trigger nothing tiles
    enc.encode_moments(_image(1, 64, 64))
    assert len(calls) == 1
