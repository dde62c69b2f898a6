"""GPU numerics: every gfx950 kernel vs the plain-PyTorch fp32 reference
(ops/eager.py), at randn inputs and a tolerance. The MFMA kernels have
exact edge-shape suites of their own:
* tests/test_attention_tiles_gpu.py: flash-attention tile structure;
* tests/test_conv3x3_edges_gpu.py: conv3x3 with integer and impulse data,
  bit-identical to float64 in all three launch configs (wide/small/stride 2,
  vectorised and scalar staging, partial tiles, halo and strided views);
* tests/test_vae_attention_edges_gpu.py: VAE attention as an exact row
  gather at L around the 32-token tile, and peaked/stepped scores that pin
  the tail mask, the split-K d-slices and the running-max rescale.
The element-wise kernels have float64-bounded edge suites (bounds derived
from the kernel source, never from its output):
* tests/test_layernorm_edges_gpu.py: rows known to the bit at every VPT
  dispatch boundary, the once-rounded add_layer_norm sum, a NaN arena, and a
  mean/std conditioning ladder;
* tests/test_groupnorm_apply_edges_gpu.py: GroupNorm apply with supplied
  moments on both paths, every dtype, and a second grid-stride trip;
* tests/test_geglu_edges_gpu.py: every finite 16-bit gate, NaN containment,
  which half is which, and a second grid-stride trip.

Run on an MI355X box: pytest tests -m gpu -x -q"""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

if torch.cuda.is_available():
    from distrifuser_amd import ops
    from distrifuser_amd.ops import eager
    from distrifuser_amd.ops.dispatch import hip_ext
else:  # collected on CPU boxes but never run
    ops = eager = hip_ext = None

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")


def _dev():
    return torch.device("cuda:0")


@requires_gpu
def test_extension_loads():
    ext = hip_ext()
    for fn in ("group_norm_stats", "group_norm_apply", "group_norm_silu", "geglu",
               "flash_attention", "mfma_probe"):
        assert hasattr(ext, fn)


@requires_gpu
def test_mfma_fragment_layout():
    """Verify the A/B fragment maps assumed by attention.hip:
    A[row=l&15][k=(l>>4)*8+j], B[k=(l>>4)*8+j][col=l&15],
    D[row=(l>>4)*4+r][col=l&15]."""
    torch.manual_seed(0)
    # values exactly representable in bf16
    a_frag = torch.randint(-8, 8, (64, 8), dtype=torch.float32, device=_dev())
    b_frag = torch.randint(-8, 8, (64, 8), dtype=torch.float32, device=_dev())
    (d,) = hip_ext().mfma_probe(a_frag, b_frag)
    d = d.cpu()

    A = torch.zeros(16, 32)
    B = torch.zeros(32, 16)
    for lane in range(64):
        lo, hi = lane & 15, lane >> 4
        for j in range(8):
            A[lo, hi * 8 + j] = a_frag[lane, j]
            B[hi * 8 + j, lo] = b_frag[lane, j]
    D = A @ B
    for lane in range(64):
        lo, hi = lane & 15, lane >> 4
        for r in range(4):
            assert abs(d[lane, r].item() - D[hi * 4 + r, lo].item()) < 1e-3, (
                f"lane {lane} r {r}: got {d[lane, r]}, want {D[hi * 4 + r, lo]}"
            )


@requires_gpu
def test_mfma32_fragment_layout():
    """mfma_f32_32x32x16_bf16: A[row=l&31][k=(l>>5)*8+j],
    B[k=(l>>5)*8+j][col=l&31], D[row=(r&3)+8*(r>>2)+4*(l>>5)][col=l&31]
    (C/D map verified in the CDNA4 guide §3; A/B checked here)."""
    torch.manual_seed(1)
    a_frag = torch.randint(-8, 8, (64, 8), dtype=torch.float32, device=_dev())
    b_frag = torch.randint(-8, 8, (64, 8), dtype=torch.float32, device=_dev())
    (d,) = hip_ext().mfma_probe32(a_frag, b_frag)
    d = d.cpu()

    A = torch.zeros(32, 16)
    B = torch.zeros(16, 32)
    for lane in range(64):
        lo, hi = lane & 31, lane >> 5
        for j in range(8):
            A[lo, hi * 8 + j] = a_frag[lane, j]
            B[hi * 8 + j, lo] = b_frag[lane, j]
    D = A @ B
    for lane in range(64):
        lo, hi = lane & 31, lane >> 5
        for r in range(16):
            row = (r & 3) + 8 * (r >> 2) + 4 * hi
            assert abs(d[lane, r].item() - D[row, lo].item()) < 1e-3, (
                f"lane {lane} r {r}: got {d[lane, r]}, want {D[row, lo]}"
            )


def _attn_ref(q, k, v):
    return eager.flash_attention(q.float(), k.float(), v.float())


@requires_gpu
@pytest.mark.parametrize(
    "b,h,lq,lkv",
    [(1, 2, 64, 64), (1, 4, 100, 200), (2, 10, 1024, 1024), (1, 5, 4096, 4096), (1, 2, 37, 77)],
)
def test_flash_attention_vs_fp32(b, h, lq, lkv):
    torch.manual_seed(0)
    dev = _dev()
    q = torch.randn(b, h, lq, 64, device=dev, dtype=torch.bfloat16)
    k = torch.randn(b, h, lkv, 64, device=dev, dtype=torch.bfloat16)
    v = torch.randn(b, h, lkv, 64, device=dev, dtype=torch.bfloat16)
    out = ops.flash_attention(q, k, v).float()
    ref = _attn_ref(q, k, v)
    err = (out - ref).abs().max().item()
    assert err < 0.03, f"max err {err}"


@requires_gpu
@pytest.mark.parametrize("d", [40, 80, 96, 128, 160])
@pytest.mark.parametrize("lq,lkv", [(256, 256), (100, 333)])
def test_flash_attention_head_dims(d, lq, lkv):
    """SD1.5 head dims (40/80/160) + other padded-DPAD shapes vs fp32."""
    torch.manual_seed(0)
    dev = _dev()
    q = torch.randn(1, 3, lq, d, device=dev, dtype=torch.bfloat16)
    k = torch.randn(1, 3, lkv, d, device=dev, dtype=torch.bfloat16)
    v = torch.randn(1, 3, lkv, d, device=dev, dtype=torch.bfloat16)
    out = ops.flash_attention(q, k, v).float()
    ref = _attn_ref(q, k, v)
    err = (out - ref).abs().max().item()
    assert err < 0.03, f"d={d} lq={lq} lkv={lkv}: max err {err}"


@requires_gpu
def test_flash_attention_chunked_matches_cat():
    """5-D chunked KV (the stale-KV flat-buffer layout) == concatenated KV."""
    torch.manual_seed(0)
    dev = _dev()
    b, heads, dim_head, l, n = 1, 4, 64, 256, 4
    inner = heads * dim_head
    q = torch.randn(b, l, inner, device=dev, dtype=torch.bfloat16)
    # emulate the flat buffer: [n, numel_slot + pad] rows
    slot = b * l * 2 * inner
    buf = torch.randn(n, slot + 64, device=dev, dtype=torch.bfloat16)
    kv_chunks = buf[:, :slot].view(n, b, l, 2 * inner)
    out = ops.flash_attention_chunked(q, kv_chunks, heads, dim_head).float()

    full = kv_chunks.permute(1, 0, 2, 3).reshape(b, n * l, 2 * inner).float()
    kf, vf = full.split(inner, dim=-1)
    qf = q.float().view(b, l, heads, dim_head).transpose(1, 2)
    kf = kf.view(b, n * l, heads, dim_head).transpose(1, 2)
    vf = vf.view(b, n * l, heads, dim_head).transpose(1, 2)
    ref = eager.flash_attention(qf, kf, vf).transpose(1, 2).reshape(b, l, inner)
    err = (out - ref).abs().max().item()
    assert err < 0.03, f"max err {err}"


@requires_gpu
def test_flash_attention_chunked_batch2():
    """CFG-unsplit patch case: batch 2 rides the same chunked buffer."""
    torch.manual_seed(1)
    dev = _dev()
    b, heads, dim_head, l, n = 2, 4, 64, 128, 2
    inner = heads * dim_head
    q = torch.randn(b, l, inner, device=dev, dtype=torch.bfloat16)
    slot = b * l * 2 * inner
    buf = torch.randn(n, slot + 8, device=dev, dtype=torch.bfloat16)
    kv_chunks = buf[:, :slot].view(n, b, l, 2 * inner)
    out = ops.flash_attention_chunked(q, kv_chunks, heads, dim_head).float()

    full = kv_chunks.permute(1, 0, 2, 3).reshape(b, n * l, 2 * inner).float()
    kf, vf = full.split(inner, dim=-1)
    qf = q.float().view(b, l, heads, dim_head).transpose(1, 2)
    kf = kf.view(b, n * l, heads, dim_head).transpose(1, 2)
    vf = vf.view(b, n * l, heads, dim_head).transpose(1, 2)
    ref = eager.flash_attention(qf, kf, vf).transpose(1, 2).reshape(b, l, inner)
    assert (out - ref).abs().max().item() < 0.03


@requires_gpu
def test_group_norm_stats_gpu():
    torch.manual_seed(0)
    x = torch.randn(2, 64, 33, 40, device=_dev(), dtype=torch.bfloat16)
    out = ops.group_norm_stats(x, 32).float()
    ref = eager.group_norm_stats(x.float().cpu(), 32)
    assert out.shape == (2, 2, 32, 1, 1, 1)
    assert (out.cpu() - ref).abs().max() < 5e-3


@requires_gpu
def test_group_norm_apply_gpu():
    torch.manual_seed(0)
    dev = _dev()
    x = torch.randn(2, 64, 16, 24, device=dev, dtype=torch.bfloat16)
    w = torch.randn(64, device=dev, dtype=torch.bfloat16)
    b = torch.randn(64, device=dev, dtype=torch.bfloat16)
    stats = ops.group_norm_stats(x, 8)
    for silu in (False, True):
        out = ops.group_norm_apply(x, stats[0], stats[1], w, b, 1e-5, silu=silu).float()
        ref = eager.group_norm_apply(
            x.float().cpu(), stats[0].float().cpu(), stats[1].float().cpu(),
            w.float().cpu(), b.float().cpu(), 1e-5, silu=silu,
        )
        assert (out.cpu() - ref).abs().max() < 0.05


@requires_gpu
def test_group_norm_silu_fused_gpu():
    torch.manual_seed(0)
    dev = _dev()
    for shape, g in [((1, 320, 64, 64), 32), ((2, 64, 15, 30), 8), ((1, 8, 3, 3), 4)]:
        x = torch.randn(*shape, device=dev, dtype=torch.bfloat16)
        w = torch.randn(shape[1], device=dev, dtype=torch.bfloat16)
        b = torch.randn(shape[1], device=dev, dtype=torch.bfloat16)
        out = ops.group_norm_silu(x, g, w, b, 1e-6, silu=True).float()
        ref = eager.group_norm_silu(x.float().cpu(), g, w.float().cpu(), b.float().cpu(),
                                    1e-6, silu=True)
        err = (out.cpu() - ref).abs().max().item()
        assert err < 0.05, f"{shape} g={g}: max err {err}"


@requires_gpu
def test_gn_merge_stats_gpu():
    """Fused stale/fresh GN moment merge vs the eager composition
    (corrected estimator + negative-variance guard + in-slot staging)."""
    torch.manual_seed(0)
    dev = _dev()
    n, N, G = 4, 1, 32
    ng = N * G
    row = 2 * ng + 24
    buffer = torch.rand(n, row, device=dev, dtype=torch.bfloat16) + 0.5
    slot_off = 8
    own = 2
    fresh = (torch.rand(2, N, G, 1, 1, 1, device=dev, dtype=torch.bfloat16) + 0.5)
    buf0 = buffer.clone()

    for corrected in (True, False):
        buffer.copy_(buf0)
        out = hip_ext().gn_merge_stats(buffer, slot_off, own, fresh, corrected).cpu().float()
        stale = buf0[:, slot_off : slot_off + 2 * ng].view(n, 2, ng).cpu().float()
        f = fresh.view(2, ng).cpu().float()
        if corrected:
            full = stale.mean(0) + (f - stale[own])
            var = full[1] - full[0] ** 2
            local_var = f[1] - f[0] ** 2
            full[1] = torch.where(var < 0, full[0] ** 2 + local_var, full[1])
        else:
            sub = stale.clone()
            sub[own] = f
            full = sub.mean(0)
        assert torch.allclose(out, full, atol=2e-2), (
            f"corrected={corrected} max err {(out - full).abs().max()}"
        )
        # fresh staged into own slot
        staged = buffer[own, slot_off : slot_off + 2 * ng].view(2, ng).cpu()
        assert torch.equal(staged, fresh.view(2, ng).cpu())


@requires_gpu
def test_geglu_gpu():
    torch.manual_seed(0)
    for shape in [(2, 128, 256), (1, 77, 48), (3, 5, 10)]:
        h = torch.randn(*shape, device=_dev(), dtype=torch.bfloat16)
        out = ops.geglu(h).float()
        ref = eager.geglu(h.float().cpu())
        assert (out.cpu() - ref).abs().max() < 0.02, shape


@requires_gpu
def test_ddim_cfg_step_gpu():
    from distrifuser_amd.schedulers import DDIMScheduler

    torch.manual_seed(0)
    dev = _dev()
    s = DDIMScheduler()
    s.set_timesteps(50)
    noise = torch.randn(2, 4, 64, 64, device=dev, dtype=torch.bfloat16)
    x = torch.randn(1, 4, 64, 64, device=dev, dtype=torch.bfloat16)
    t = s.timesteps[7]
    fused = s.guided_step(noise, t, x, 5.0).float().cpu()
    nu, nc = noise.float().cpu().chunk(2)
    eps = nu + 5.0 * (nc - nu)
    ref = s.step(eps, t, x.float().cpu())
    assert (fused - ref).abs().max() < 0.03


@requires_gpu
def test_gpu_ops_fail_loudly_without_ext(monkeypatch):
    """On a GPU box, a missing extension must raise, not fall back silently."""
    from distrifuser_amd.ops import dispatch

    monkeypatch.setattr(dispatch, "_EXT", None)
    monkeypatch.setattr(dispatch, "_EXT_ERR", ImportError("simulated"))
    x = torch.randn(1, 8, 4, 4, device=_dev(), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="extension"):
        dispatch.group_norm_silu(x, 2, None, None, 1e-5)

# ---- conv3x3 implicit-GEMM kernel ------------------------------------------


@requires_gpu
@pytest.mark.parametrize(
    "cin,cout,h,w,stride,halos",
    [
        (320, 320, 30, 120, 1, True),    # interior ResBlock conv with halos
        (320, 640, 16, 60, 1, False),    # channel change, zero-pad borders
        (64, 64, 129, 130, 1, True),     # multi-block x and y, odd sizes
        (4, 320, 32, 96, 1, False),      # conv_in (cin << 64 zero-pad path)
        (48, 40, 20, 50, 1, True),       # non-multiple cin/cout tails
        (320, 4, 12, 40, 1, False),      # conv_out (cout tail only)
        (320, 640, 32, 120, 2, True),    # downsample stride 2 with top halo
        (128, 128, 64, 250, 2, False),   # stride 2 multi-block
    ],
)
def test_conv3x3_vs_fp32(cin, cout, h, w, stride, halos):
    from distrifuser_amd.ops import conv as conv_ops
    from distrifuser_amd.ops import eager

    torch.manual_seed(0)
    dev = "cuda"
    x = torch.randn(2, cin, h, w, device=dev, dtype=torch.bfloat16) * 0.5
    weight = torch.randn(cout, cin, 3, 3, device=dev, dtype=torch.bfloat16) * (cin * 9) ** -0.5
    bias = torch.randn(cout, device=dev, dtype=torch.bfloat16)
    top = bot = None
    if halos:
        top = torch.randn(2, cin, 1, w, device=dev, dtype=torch.bfloat16) * 0.5
        if stride == 1:
            bot = torch.randn(2, cin, 1, w, device=dev, dtype=torch.bfloat16) * 0.5

    packed = conv_ops.pack_conv3x3_weight(weight)
    got = conv_ops.conv3x3_halo(x, weight, bias, stride, top, bot, packed=packed)

    ref = eager.conv3x3_halo(
        x.float(), weight.float(), bias.float(), stride,
        top.float() if top is not None else None,
        bot.float() if bot is not None else None,
    )
    assert got.shape == ref.shape
    err = (got.float() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= 0.02 * max(scale, 1.0), f"max err {err} vs scale {scale}"


@requires_gpu
def test_conv3x3_channel_slice_view():
    """TPConv2d passes a channel-slice view; the kernel must accept it."""
    from distrifuser_amd.ops import conv as conv_ops
    from distrifuser_amd.ops import eager

    torch.manual_seed(1)
    full = torch.randn(1, 128, 24, 48, device="cuda", dtype=torch.bfloat16)
    x = full[:, 32:96]  # non-contiguous channel slice, contiguous rows
    weight = torch.randn(96, 64, 3, 3, device="cuda", dtype=torch.bfloat16) * 0.04
    packed = conv_ops.pack_conv3x3_weight(weight)
    got = conv_ops.conv3x3_halo(x, weight, None, 1, packed=packed)
    ref = eager.conv3x3_halo(x.float(), weight.float(), None, 1)
    err = (got.float() - ref).abs().max().item()
    assert err <= 0.02 * max(ref.abs().max().item(), 1.0)


@requires_gpu
def test_native_conv2d_module_matches_eager():
    from distrifuser_amd.ops import NativeConv2d

    torch.manual_seed(2)
    m = NativeConv2d(96, 160, 3, padding=1).to("cuda", torch.bfloat16)
    x = torch.randn(2, 96, 40, 72, device="cuda", dtype=torch.bfloat16)
    got = m(x)
    ref = torch.nn.functional.conv2d(
        x.float(), m.weight.float(), m.bias.float(), padding=1)
    err = (got.float() - ref).abs().max().item()
    assert err <= 0.02 * max(ref.abs().max().item(), 1.0)


# ---- VAE mid-attention (single head, d=512) --------------------------------


@requires_gpu
@pytest.mark.parametrize("b,l", [(1, 256), (2, 1000), (1, 4096)])
def test_vae_attention_vs_fp32(b, l):
    from distrifuser_amd import ops
    from distrifuser_amd.ops import eager

    torch.manual_seed(0)
    q = torch.randn(b, l, 512, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(b, l, 512, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(b, l, 512, device="cuda", dtype=torch.bfloat16)
    got = ops.hip_ext().vae_attention(q, k, v)
    ref = eager.vae_attention(q.float(), k.float(), v.float())
    err = (got.float() - ref).abs().max().item()
    assert err <= 0.03, f"max err {err}"


# ---- fused (residual +) LayerNorm ------------------------------------------


@requires_gpu
@pytest.mark.parametrize("rows,c", [(64, 320), (100, 640), (33, 1280), (17, 2048)])
def test_layer_norm_gpu(rows, c):
    import torch.nn.functional as F

    from distrifuser_amd import ops

    torch.manual_seed(0)
    x = torch.randn(rows, c, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(c, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(c, device="cuda", dtype=torch.bfloat16)
    got = ops.hip_ext().layer_norm(x, w, b, 1e-5)
    ref = F.layer_norm(x.float(), (c,), w.float(), b.float(), 1e-5)
    assert (got.float() - ref).abs().max().item() < 0.05


@requires_gpu
def test_add_layer_norm_gpu():
    import torch.nn.functional as F

    from distrifuser_amd import ops

    torch.manual_seed(1)
    x = torch.randn(50, 1280, device="cuda", dtype=torch.bfloat16)
    r = torch.randn(50, 1280, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(1280, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(1280, device="cuda", dtype=torch.bfloat16)
    s, y = ops.hip_ext().add_layer_norm(x, r, w, b, 1e-5)
    sref = (x.float() + r.float())
    yref = F.layer_norm(sref, (1280,), w.float(), b.float(), 1e-5)
    assert (s.float() - sref).abs().max().item() < 0.05
    assert (y.float() - yref).abs().max().item() < 0.05


@requires_gpu
def test_cfg_dpm_step_gpu_matches_eager():
    """Fused cfg_dpm_step over a full DPM trajectory vs the eager compose."""
    import os

    from distrifuser_amd.schedulers import get_scheduler

    torch.manual_seed(4)
    a = get_scheduler("dpm-solver")
    b = get_scheduler("dpm-solver")
    a.set_timesteps(6)
    b.set_timesteps(6)
    x_a = torch.randn(1, 4, 16, 16, device="cuda", dtype=torch.bfloat16)
    x_b = x_a.clone()
    g = 5.0
    for t in a.timesteps:
        noise = torch.randn(2, 4, 16, 16, device="cuda", dtype=torch.bfloat16)
        x_a = a.guided_step(noise, int(t), x_a, g)  # fused kernel path
        os.environ["DFA_FORCE_EAGER"] = "1"
        x_b = b.guided_step(noise, int(t), x_b, g)  # eager compose + step
        del os.environ["DFA_FORCE_EAGER"]
        assert (x_a.float() - x_b.float()).abs().max().item() < 0.05, int(t)


@requires_gpu
def test_conv3x3_row_band_views():
    """conv_in sliced path: interior is a row-slice VIEW of the full latent
    and the halos are adjacent-row views — must equal the full conv's band."""
    import torch.nn.functional as F

    from distrifuser_amd.ops import NativeConv2d

    torch.manual_seed(5)
    full = torch.randn(2, 4, 64, 96, device="cuda", dtype=torch.bfloat16)
    m = NativeConv2d(4, 320, 3, padding=1).to("cuda", torch.bfloat16)
    ref = F.conv2d(full.float(), m.weight.float(), m.bias.float(), padding=1)
    for h0, h1 in ((0, 16), (16, 48), (48, 64)):
        band = full[:, :, h0:h1]
        top = full[:, :, h0 - 1 : h0] if h0 > 0 else None
        bot = full[:, :, h1 : h1 + 1] if h1 < 64 else None
        got = m(band, top=top, bot=bot)
        err = (got.float() - ref[:, :, h0:h1]).abs().max().item()
        assert err <= 0.02 * max(ref.abs().max().item(), 1.0), (h0, h1, err)


@requires_gpu
def test_conv3x3_residual_epilogue(monkeypatch):
    from distrifuser_amd.ops import conv as conv_ops
    from distrifuser_amd.ops import eager

    monkeypatch.setenv("DFA_CONV_RESID", "1")
    torch.manual_seed(6)
    x = torch.randn(2, 64, 24, 48, device="cuda", dtype=torch.bfloat16)
    res = torch.randn(2, 96, 24, 48, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(96, 64, 3, 3, device="cuda", dtype=torch.bfloat16) * 0.04
    pk = conv_ops.pack_conv3x3_weight(w)
    got = conv_ops.conv3x3_halo(x, w, None, 1, packed=pk, residual=res)
    ref = eager.conv3x3_halo(x.float(), w.float(), None, 1) + res.float()
    err = (got.float() - ref).abs().max().item()
    assert err <= 0.03 * max(ref.abs().max().item(), 1.0)


@requires_gpu
def test_conv3x3_bias2_epilogue():
    """Per-(batch, channel) bias2 (the fused time-embedding add)."""
    from distrifuser_amd.ops import conv as conv_ops
    from distrifuser_amd.ops import eager

    torch.manual_seed(7)
    x = torch.randn(2, 64, 20, 40, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(96, 64, 3, 3, device="cuda", dtype=torch.bfloat16) * 0.04
    bias = torch.randn(96, device="cuda", dtype=torch.bfloat16)
    b2 = torch.randn(2, 96, device="cuda", dtype=torch.bfloat16)
    pk = conv_ops.pack_conv3x3_weight(w)
    got = conv_ops.conv3x3_halo(x, w, bias, 1, packed=pk, bias2=b2)
    ref = eager.conv3x3_halo(x.float(), w.float(), bias.float(), 1) \
        + b2.float()[:, :, None, None]
    err = (got.float() - ref).abs().max().item()
    assert err <= 0.03 * max(ref.abs().max().item(), 1.0)
