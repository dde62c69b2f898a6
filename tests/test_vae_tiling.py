"""Tiled VAE decode on the CPU, exactly: the shared tiling function against
``_decode_one`` of each tile's latent slice and the documented linear blend,
both written out here. (The encoder's twins are in test_vae_encoder.py.)

Geometry of the 2x2 and ragged cases: tile 8 latents (64 px), overlap 2
(16 px), stride 6 (48 px). Tiles start at latent 0 and 6 on each axis; every
tile but the last of a row / column keeps its first 48 px, and the first
16 px of a later tile are the blend ramp with its predecessor's last 16.
"""

import functools

import torch

from distrifuser_amd.models.vae import TINY_VAE, VAEDecoder

TS, OV = 8, 2
PX, OV_PX, ST_PX = TS * 8, OV * 8, (TS - OV) * 8


@functools.lru_cache(maxsize=None)
def _decoder():
    """Shared; tests switch tiling on and off but never touch the weights."""
    torch.manual_seed(21)
    dec = VAEDecoder(TINY_VAE).eval()
    with torch.no_grad():
        for p in dec.parameters():
            p.mul_(1.5)  # the default init leaves the attention nearly uniform
    return dec


def _latent(h, w, seed):
    return torch.randn(1, TINY_VAE.latent_channels, h, w,
                       generator=torch.Generator().manual_seed(seed))


def _post_quant(dec, latents):
    """What decode() hands to _decode_one / _decode_tiled."""
    return dec.post_quant_conv(latents / dec.config.scaling_factor)


def _tiled(dec, latents):
    dec.enable_tiling(tile_latent_size=TS, tile_overlap=OV)
    try:
        return dec.decode(latents)
    finally:
        dec.disable_tiling()


def test_one_tile_holds_the_latent():
    dec = _decoder()
    lat = _latent(8, 8, seed=1)
    ref = dec.decode(lat)
    assert torch.equal(_tiled(dec, lat), ref)
    # decode() does not tile a latent that fits one tile; the tiling itself
    # must also return that single tile untouched
    dec.enable_tiling(tile_latent_size=TS, tile_overlap=OV)
    try:
        assert torch.equal(dec._decode_tiled(_post_quant(dec, lat)), ref)
    finally:
        dec.disable_tiling()


def test_2x2_tiles_unblended_pixels_and_vertical_band():
    dec = _decoder()
    lat = _latent(14, 14, seed=2)
    out = _tiled(dec, lat)
    assert out.shape == (1, 3, 112, 112)
    assert out.abs().max() > 1e-3  # not a vacuous all-zero comparison
    z = _post_quant(dec, lat)
    # all four tiles are full-size and the batch is 1, so they decode as one
    # batched _decode_one pass, in row-major tile order
    starts = [(y0, x0) for y0 in (0, 6) for x0 in (0, 6)]
    dec_all = dec._decode_one(torch.cat([z[:, :, y0 : y0 + TS, x0 : x0 + TS]
                                         for (y0, x0) in starts]))
    tile = {s: dec_all[i : i + 1] for i, s in enumerate(starts)}
    assert tile[(0, 0)].shape == (1, 3, PX, PX)
    # the batched pass is the per-slice decode up to fp32 round-off
    for (y0, x0) in starts:
        one = dec._decode_one(z[:, :, y0 : y0 + TS, x0 : x0 + TS])
        assert torch.allclose(tile[(y0, x0)], one, rtol=0, atol=1e-5)

    lo, hi = ST_PX, ST_PX + OV_PX  # output 48..64 is the band on either axis
    assert torch.equal(out[:, :, :lo, :lo], tile[(0, 0)][:, :, :lo, :lo])
    assert torch.equal(out[:, :, :lo, hi:], tile[(0, 6)][:, :, :lo, OV_PX:])
    assert torch.equal(out[:, :, hi:, :lo], tile[(6, 0)][:, :, OV_PX:, :lo])
    assert torch.equal(out[:, :, hi:, hi:], tile[(6, 6)][:, :, OV_PX:, OV_PX:])
    # vertical band of the left column (its columns 0..47 take no horizontal
    # blend): the upper tile's last 16 rows fade into the lower tile's first 16
    w = torch.linspace(0, 1, OV_PX).view(1, 1, OV_PX, 1)
    want = tile[(0, 0)][:, :, PX - OV_PX :, :lo] * (1 - w) + tile[(6, 0)][:, :, :OV_PX, :lo] * w
    assert torch.equal(out[:, :, lo:hi, :lo], want)
    # the ramp starts at weight 0 for the new tile and ends at weight 1
    assert torch.equal(out[:, :, lo, :lo], tile[(0, 0)][:, :, PX - OV_PX, :lo])
    assert torch.equal(out[:, :, hi - 1, :lo], tile[(6, 0)][:, :, OV_PX - 1, :lo])
    # and the right column's band, right of the horizontal ramp
    want = tile[(0, 6)][:, :, PX - OV_PX :, OV_PX:] * (1 - w) + tile[(6, 6)][:, :, :OV_PX, OV_PX:] * w
    assert torch.equal(out[:, :, lo:hi, hi:], want)


def test_ragged_latent():
    dec = _decoder()
    lat = _latent(11, 13, seed=3)
    out = _tiled(dec, lat)
    assert out.shape == (1, 3, 88, 104)
    z = _post_quant(dec, lat)
    # only tile (0, 0) is full-size, so every tile decodes on its own
    hi = ST_PX + OV_PX
    first = dec._decode_one(z[:, :, :TS, :TS])
    assert torch.equal(out[:, :, :ST_PX, :ST_PX], first[:, :, :ST_PX, :ST_PX])
    last = dec._decode_one(z[:, :, 6:, 6:])  # 5 x 7 latents
    assert last.shape == (1, 3, 40, 56)
    assert torch.equal(out[:, :, hi:, hi:], last[:, :, OV_PX:, OV_PX:])
