"""Transformer boundary on the CPU: the eager fallbacks of the token-layout
GroupNorm and of tokens_add_nchw equal the torch compositions they replace,
the tiny SDXL-style transformer gives the same output with and without
DFA_NO_BOUNDARY_FUSE, and PatchGroupNorm(tokens=True) equals its NCHW output
permuted on the distributed branches (warm-up, steady state, sync all-reduce).
Everything is torch.equal: the values are the same, only their order moves."""

import pytest
import torch

from distrifuser_amd import ops
from distrifuser_amd.ops import eager


def _to_tokens(x):
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n, h * w, c).contiguous()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("silu", [False, True])
def test_eager_group_norm_tokens(dtype, silu):
    torch.manual_seed(0)
    n, c, g, h, w = 2, 24, 4, 5, 7
    x = torch.randn(n, c, h, w).to(dtype)
    wt, b = torch.randn(c).to(dtype), torch.randn(c).to(dtype)
    for fn in (eager.group_norm_silu, ops.group_norm_silu):
        ref = fn(x, g, wt, b, 1e-6, silu)
        got = fn(x, g, wt, b, 1e-6, silu, tokens=True)
        assert got.shape == (n, h * w, c) and got.is_contiguous()
        assert torch.equal(got, _to_tokens(ref))
    stats = eager.group_norm_stats(x, g)
    for fn in (eager.group_norm_apply, ops.group_norm_apply):
        ref = fn(x, stats[0], stats[1], wt, b, 1e-6, silu)
        got = fn(x, stats[0], stats[1], wt, b, 1e-6, silu, tokens=True)
        assert got.shape == (n, h * w, c) and got.is_contiguous()
        assert torch.equal(got, _to_tokens(ref))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_eager_tokens_add_nchw(dtype):
    torch.manual_seed(1)
    n, c, h, w = 2, 24, 5, 7
    y = torch.randn(n, h * w, c).to(dtype)
    wide = torch.randn(n, c + 8, h, w + 3).to(dtype)
    for res in (wide[:, :c, :, :w].contiguous(), wide[:, 4 : 4 + c, :, :w]):
        ref = y.reshape(n, h, w, c).permute(0, 3, 1, 2) + res
        for fn in (eager.tokens_add_nchw, ops.tokens_add_nchw):
            got = fn(y, res)
            assert got.shape == (n, c, h, w) and got.is_contiguous()
            assert torch.equal(got, ref)


def _tiny_transformer(monkeypatch, no_fuse):
    from distrifuser_amd.models.layers import LayerFactory
    from distrifuser_amd.models.transformer import Transformer2DModel
    from distrifuser_amd.parallel.state import ParallelState
    from distrifuser_amd.utils.config import DistriConfig

    if no_fuse:
        monkeypatch.setenv("DFA_NO_BOUNDARY_FUSE", "1")
    else:
        monkeypatch.delenv("DFA_NO_BOUNDARY_FUSE", raising=False)
    cfg = DistriConfig(height=64, width=96, use_cuda_graph=False, device="cpu")
    torch.manual_seed(0)
    model = Transformer2DModel(64, 2, 32, 1, 32, factory=LayerFactory(ParallelState(cfg))).eval()
    assert model.boundary_fuse == (not no_fuse)
    return model


def test_tiny_transformer_switch_cpu(monkeypatch):
    old = _tiny_transformer(monkeypatch, True)
    new = _tiny_transformer(monkeypatch, False)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 8, 12, generator=g)
    ehs = torch.randn(2, 7, 32, generator=g)
    with torch.no_grad():
        a, b = old(x, ehs), new(x, ehs)
    assert b.shape == x.shape and b.is_contiguous()
    assert torch.equal(a, b)


def test_conv_projection_path_never_fuses(monkeypatch):
    """The SD1.5 / SD2.1 1x1-conv path keeps its composition."""
    from distrifuser_amd.models.layers import LayerFactory
    from distrifuser_amd.models.transformer import Transformer2DModel
    from distrifuser_amd.parallel.state import ParallelState
    from distrifuser_amd.utils.config import DistriConfig

    monkeypatch.delenv("DFA_NO_BOUNDARY_FUSE", raising=False)
    cfg = DistriConfig(height=64, width=64, use_cuda_graph=False, device="cpu")
    model = Transformer2DModel(64, 2, 32, 1, 32, factory=LayerFactory(ParallelState(cfg)),
                               use_linear_projection=False)
    assert not model.boundary_fuse


def _patch_gn_sequence(mode, tokens, rank):
    from distrifuser_amd.parallel.patch_ops import PatchGroupNorm
    from distrifuser_amd.parallel.state import ParallelState
    from distrifuser_amd.utils.comm import PatchParallelismCommManager
    from distrifuser_amd.utils.config import DistriConfig

    cfg = DistriConfig(height=128, width=128, do_classifier_free_guidance=False, mode=mode,
                       warmup_steps=1, use_cuda_graph=False, device="cpu")
    assert cfg.n_device_per_batch == 2
    state = ParallelState(cfg)
    comm = PatchParallelismCommManager(cfg)
    state.comm_manager = comm
    gn = PatchGroupNorm(4, 16, eps=1e-6, state=state)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        gn.weight.copy_(torch.randn(16, generator=g))
        gn.bias.copy_(torch.randn(16, generator=g))
    x = torch.randn(2, 16, 3, 6, generator=torch.Generator().manual_seed(10 + rank))
    outs = []
    with torch.no_grad():
        state.recording = True
        gn(x, tokens=tokens)  # registration pass
        comm.create_buffer()
        state.recording = False
        for step in range(4):  # counter 0, 1: warm-up composition; 2, 3: steady state
            state.set_counter(step)
            outs.append(gn(x * (1.0 + 0.25 * step) + 0.1 * step, tokens=tokens).clone())
        comm.clear()
    return outs


def _patch_gn_worker(rank, world_size, mode):
    return _patch_gn_sequence(mode, False, rank), _patch_gn_sequence(mode, True, rank)


@pytest.mark.parametrize("mode", ["corrected_async_gn", "sync_gn"])
def test_patch_group_norm_tokens_ws2(distributed_runner, mode):
    out = distributed_runner(2, _patch_gn_worker, (mode,))
    for rank in (0, 1):
        nchw, tok = out[rank]
        assert len(nchw) == len(tok) == 4
        for a, b in zip(nchw, tok):
            assert b.shape == (2, 18, 16) and b.is_contiguous()
            assert torch.equal(b, _to_tokens(a))
    # the ranks hold different patches: the stats really were merged
    assert not torch.equal(out[0][0][0], out[1][0][0])
