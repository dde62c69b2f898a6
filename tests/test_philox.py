"""The Philox4x32-10 normal generator of the stochastic samplers, eager twin
(CPU): ops.eager.philox4x32 / philox_normal, the oracle of the native op.

Z_TOL. The float64 values below are the rule of csrc/philox.h evaluated in
float64 by a stand-alone Python Philox. The fp32 evaluation differs from them
by the error of the precise fp32 log / sqrt / sin / cos (a couple of ulp each)
and by the rounding of 2*pi*u2 near 6.28, up to 2.4e-7 in sin / cos; with a
radius of at most sqrt(48 ln 2) ~ 5.77 that is about 3e-6, and Z_TOL is three
times that."""

import math

import pytest
import torch

from distrifuser_amd import ops
from distrifuser_amd.ops import eager

Z_TOL = 1e-5


def _words(counter, key):
    return [int(w) for w in eager.philox4x32(*counter, *key)]


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
], ids=["zeros", "ones", "pi"])
def test_philox_words_match_the_random123_known_answers(counter, key, want):
    assert " ".join(f"{w:08x}" for w in _words(counter, key)) == want


def test_philox_words_are_elementwise():
    c0 = torch.tensor([0, 0xFFFFFFFF, 0x243F6A88])
    got = eager.philox4x32(c0, 0, 0, 0, 7, 9)
    for i, c in enumerate(c0.tolist()):
        assert [int(w[i]) for w in got] == _words((c, 0, 0, 0), (7, 9))


def test_normals_match_the_float64_rule():
    want = torch.tensor([0.33950952, -0.25030605, 0.01561981, -0.8754559, -1.53537316,
                         0.6684846, 0.95610474, -0.74321232], dtype=torch.float64)
    got = eager.philox_normal(8, 233, 0)
    assert got.dtype == torch.float32 and got.shape == (8,)
    diff = (got.double() - want).abs().max().item()
    print(f"max |z - float64 rule| = {diff:.3e}")
    assert diff <= Z_TOL


def test_normals_follow_the_rule_from_the_raw_words():
    """Element i is lane i & 3 of block i >> 2 with counter (q, 0, draw, 0) and
    key (lo32(seed), hi32(seed)): checked in float64 from the raw words."""
    seed, draw = (0x1234 << 32) | 0x89ABCDEF, 5
    got = eager.philox_normal(12, seed, draw).double()
    for q in range(3):
        r = _words((q, 0, draw, 0), (seed & 0xFFFFFFFF, seed >> 32))
        for pair in range(2):
            u1 = ((r[2 * pair] >> 8) + 1) * 2.0 ** -24
            u2 = (r[2 * pair + 1] >> 8) * 2.0 ** -24
            rad = math.sqrt(-2.0 * math.log(u1))
            want = (rad * math.cos(2 * math.pi * u2), rad * math.sin(2 * math.pi * u2))
            for k in range(2):
                assert abs(float(got[4 * q + 2 * pair + k]) - want[k]) <= Z_TOL


def test_mean_and_std():
    n = 65536
    z = eager.philox_normal(n, 233, 3)
    mean, std = z.double().mean().item(), z.double().std().item()
    print(f"mean {mean:.5f} std {std:.5f}")  # the float64 rule: -0.00046, 0.9979
    assert torch.isfinite(z).all() and z.abs().max() <= math.sqrt(48 * math.log(2))
    assert abs(mean) < 4 / math.sqrt(n)
    assert abs(std - 1) < 4 / math.sqrt(2 * n)


def test_draws_and_seeds_give_different_streams():
    base = eager.philox_normal(256, 233, 0)
    assert torch.equal(base, eager.philox_normal(256, 233, 0))
    for other in (eager.philox_normal(256, 233, 1), eager.philox_normal(256, 234, 0),
                  eager.philox_normal(256, 233 + (1 << 32), 0)):
        assert (other != base).float().mean() > 0.99


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 7, 141])
def test_offset_returns_the_stream_from_element_k(k):
    whole = eager.philox_normal(160, 99, 2)
    for n in (1, 5, 16):
        assert torch.equal(eager.philox_normal(n, 99, 2, offset=k), whole[k:k + n])


def test_offset_reaches_the_high_counter_word():
    """offset = 2^34 is block 2^32: counter word c1 = 1, c0 = 0."""
    off = 1 << 34
    got = eager.philox_normal(8, 233, 0, offset=off)
    assert not torch.equal(got, eager.philox_normal(8, 233, 0))
    r = _words((0, 1, 0, 0), (233, 0))
    u1 = ((r[0] >> 8) + 1) * 2.0 ** -24
    u2 = (r[1] >> 8) * 2.0 ** -24
    assert abs(float(got[0]) - math.sqrt(-2 * math.log(u1)) * math.cos(2 * math.pi * u2)) <= Z_TOL
    assert torch.equal(eager.philox_normal(5, 233, 0, offset=off + 3), got[3:])
    # a range that straddles the carry into the high word
    across = eager.philox_normal(8, 233, 0, offset=off - 4)
    assert torch.equal(across[4:], got[:4])
    assert torch.equal(across[:4], eager.philox_normal(4, 233, 0, offset=off - 4))


def test_dispatch_on_the_cpu_is_the_eager_twin():
    assert torch.equal(ops.philox_normal(37, 5, 1, offset=2), eager.philox_normal(37, 5, 1, 2))
    assert ops.philox_normal(0, 5, 1).shape == (0,)
    for bad in ((-1, 0, 0, 0), (4, -1, 0, 0), (4, 1 << 64, 0, 0), (4, 0, 1 << 32, 0),
                (4, 0, 0, -1)):
        with pytest.raises(ValueError):
            eager.philox_normal(*bad)
