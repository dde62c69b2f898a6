"""Quick on-box kernel A/B: our gfx950 kernels vs the PyTorch-ROCm baselines.

Run on an MI355X: python scripts/kernel_bench.py > gpurun_out/kernel_bench.json
(--splitkv-only: just the split-KV attention sweep; --vae-downsample-only:
just the VAE-encoder downsample convs; --rescale-only: just the rescaled
DDIM step, native against the torch composition; --dtype {bf16,fp16}: the
element type of the attention, conv, LayerNorm and VAE-attention rows, default
bf16 — fp16 rows carry "dtype": "fp16")
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


import json
import sys
import time

import torch
import torch.nn.functional as F


def timeit(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1000  # ms


def splitkv_sweep(results, reps=5, iters=100):
    """Split-KV on the shapes whose plain grid (ceil(Lq/256) * B * H blocks)
    leaves most of the 512 d64 block slots idle: S = 1, 2, 4, 8 and the
    heuristic's choice, interleaved `reps` times per shape on the same box.
    Reports the median and the min..max spread of the repeats."""
    from distrifuser_amd import ops

    dev = "cuda:0"
    ext = ops.hip_ext()
    shapes = [("chunked", h, lq, n) for h, lq, n in
              [(10, 1024, 4), (20, 256, 4), (10, 7200, 8), (20, 3600, 4)]]
    shapes += [("plain", h, l, 1) for h, l in [(20, 1024), (10, 4096)]]
    for kind, h, lq, n in shapes:
        lkv = lq * n
        inner = h * 64
        q = torch.randn(1, h, lq, 64, device=dev, dtype=torch.bfloat16)
        if kind == "chunked":
            slot = lq * 2 * inner
            buf = torch.randn(n, slot + 64, device=dev, dtype=torch.bfloat16)
            kv = buf[:, :slot].view(n, 1, lq, 2 * inner)
            k = kv[..., :inner].unflatten(-1, (h, 64)).permute(1, 3, 0, 2, 4)
            v = kv[..., inner:].unflatten(-1, (h, 64)).permute(1, 3, 0, 2, 4)
        else:
            k = torch.randn(1, h, lkv, 64, device=dev, dtype=torch.bfloat16)
            v = torch.randn(1, h, lkv, 64, device=dev, dtype=torch.bfloat16)
        auto = ops.attention_kv_splits(1, h, lq, lkv, 64, dev)
        configs = [("S1", 1), ("S2", 2), ("S4", 4), ("S8", 8), ("auto", auto)]
        ms = {name: [] for name, _ in configs}
        for _ in range(reps):
            for name, s in configs:
                if s == 1:  # the entry the default path takes
                    ms[name].append(timeit(lambda: ext.flash_attention(q, k, v), iters=iters))
                else:
                    ms[name].append(
                        timeit(lambda: ext.flash_attention_ext(q, k, v, s, False), iters=iters))
        row = {"op": "flash_attention_splitkv", "kind": kind, "heads": h, "Lq": lq, "Lkv": lkv,
               "n_chunks": n, "blocks_S1": -(-lq // 256) * h, "auto_S": auto, "reps": reps}
        for name, _ in configs:
            t = sorted(ms[name])
            row[f"ms_{name}"] = t[len(t) // 2]
            row[f"spread_{name}"] = [t[0], t[-1]]
        results.append(row)
        print(json.dumps(row), flush=True)


def vae_downsample_rows(results, dt, tag, batches=(1, 25), reps=3):
    """The three SDXL-VAE encoder downsample convs (3x3, stride 2, padded on
    the bottom and right only) for 768^2 tiles: the kernel's pad_lo=0 mode
    against F.pad + F.conv2d, interleaved `reps` times. Batch 25 is the
    full-tile batch of a tiled 3840^2 encode. Reports the median and the
    min..max spread of the repeats."""
    from distrifuser_amd import ops

    dev = "cuda:0"
    for b in batches:
        for c, hw in [(128, 768), (256, 384), (512, 192)]:
            x = torch.randn(b, c, hw, hw, device=dev, dtype=dt) * 0.5
            wt = torch.randn(c, c, 3, 3, device=dev, dtype=dt) * (c * 9) ** -0.5
            bias = torch.randn(c, device=dev, dtype=dt)
            packed = ops.pack_conv3x3_weight(wt, dt)
            ours = lambda: ops.conv3x3_halo(x, wt, bias, 2, packed=packed, pad_lo=0)
            ref = lambda: F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, bias, stride=2)
            err = (ours().float() - ref().float()).abs().max().item()
            ms = {"ours": [], "miopen": []}
            for _ in range(reps):
                ms["ours"].append(timeit(ours))
                ms["miopen"].append(timeit(ref))
            flops = 2.0 * b * c * (hw // 2) ** 2 * c * 9
            row = {**tag, "op": "conv3x3_pad_lo0", "batch": b, "c": c, "hw": hw, "reps": reps,
                   "max_abs_diff": err}
            for name, t in ms.items():
                t = sorted(t)
                row[f"ms_{name}"] = t[len(t) // 2]
                row[f"spread_{name}"] = [t[0], t[-1]]
                row[f"tflops_{name}"] = flops / t[len(t) // 2] / 1e9
            results.append(row)
            print(json.dumps(row), flush=True)


def _count_launches(fn):
    """Device kernels one call of fn launches, from the profiler's trace."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events()
               if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower())


def rescale_step_rows(results, reps=5, iters=200):
    """One DDIM step with guidance_rescale=0.7 on a bf16 CFG pair, outside any
    graph: the three native launches (moments, finalize, RESCALE step)
    against the torch composition of the same maths (chunk, CFG, two std,
    scale, affine update). Median and range of `reps` timings of `iters`
    back-to-back calls each."""
    from distrifuser_amd import ops

    g, phi, ca, cb = 7.5, 0.7, 1.02, -0.05
    ext = ops.hip_ext()
    for hw in (128, 480):
        noise = torch.randn(2, 4, hw, hw, device="cuda:0", dtype=torch.bfloat16)
        x = torch.randn(1, 4, hw, hw, device="cuda:0", dtype=torch.bfloat16)

        def native():
            f = ext.guidance_rescale_factor(noise, g, phi)
            return ext.cfg_affine_step(noise, x, g, ca, cb, f)

        def composed():
            nu, nc = noise.float().chunk(2)
            cfg = nu + g * (nc - nu)
            r = phi * (nc.std() / cfg.std()) + (1 - phi)
            return (ca * x.float() + cb * (r * cfg)).to(x.dtype)

        err = (native().float() - composed().float()).abs().max().item()
        row = {"op": "rescaled_ddim_step", "shape": [1, 4, hw, hw], "dtype": "bf16",
               "max_abs_diff": err,
               "launches_native": _count_launches(native),
               "launches_torch": _count_launches(composed)}
        for name, fn in (("native", native), ("torch", composed)):
            us = sorted(timeit(fn, iters=iters, warmup=20) * 1000 for _ in range(reps))
            row[f"us_{name}"] = us[len(us) // 2]
            row[f"us_{name}_range"] = [us[0], us[-1]]
        results.append(row)
        print(json.dumps(row), flush=True)


def main():
    assert torch.cuda.is_available()
    from distrifuser_amd import ops

    dev = "cuda:0"
    results = []
    argv = sys.argv[1:]
    dtype_name = argv[argv.index("--dtype") + 1] if "--dtype" in argv else "bf16"
    assert dtype_name in ("bf16", "fp16"), "--dtype takes bf16 or fp16"
    dt = torch.float16 if dtype_name == "fp16" else torch.bfloat16
    tag = {"dtype": "fp16"} if dtype_name == "fp16" else {}  # bf16 rows: as ever

    if "--splitkv-only" in sys.argv[1:]:
        splitkv_sweep(results)
        with open("kernel_bench_splitkv.json", "w") as f:
            json.dump(results, f, indent=1)
        return 0

    if "--rescale-only" in sys.argv[1:]:
        rescale_step_rows(results)
        return 0

    if "--vae-downsample-only" in sys.argv[1:]:
        torch.backends.cudnn.benchmark = True
        vae_downsample_rows(results, dt, tag)
        return 0

    # ---- flash attention at SDXL shapes (B=1 CFG-split branch) ----
    #   (heads, L): 1024^2 -> (10, 4096) and (20, 1024)
    #   3840^2 -> (10, 57600) and (20, 14400)
    for h, l in [(20, 1024), (10, 4096), (20, 14400), (10, 57600)]:
        q = torch.randn(1, h, l, 64, device=dev, dtype=dt)
        k = torch.randn(1, h, l, 64, device=dev, dtype=dt)
        v = torch.randn(1, h, l, 64, device=dev, dtype=dt)
        ms_ours = timeit(lambda: ops.hip_ext().flash_attention(q, k, v))
        ms_sdpa = timeit(lambda: F.scaled_dot_product_attention(q, k, v))
        flops = 4.0 * l * l * 64 * h
        results.append({
            **tag,
            "op": "flash_attention", "heads": h, "L": l,
            "ms_ours": ms_ours, "ms_sdpa": ms_sdpa,
            "tflops_ours": flops / ms_ours / 1e9,
            "tflops_sdpa": flops / ms_sdpa / 1e9,
        })
        print(json.dumps(results[-1]), flush=True)

    # ---- displaced-patch shape: local Q x full stale KV (8 chunks) ----
    for h, lq, n in [(10, 7200, 8), (20, 3600, 4)]:
        lkv = lq * n
        inner = h * 64
        q = torch.randn(1, h, lq, 64, device=dev, dtype=dt)
        slot = lq * 2 * inner
        buf = torch.randn(n, slot + 64, device=dev, dtype=dt)
        kv = buf[:, :slot].view(n, 1, lq, 2 * inner)
        k5 = kv[..., :inner].unflatten(-1, (h, 64)).permute(1, 3, 0, 2, 4)
        v5 = kv[..., inner:].unflatten(-1, (h, 64)).permute(1, 3, 0, 2, 4)
        ms_ours = timeit(lambda: ops.hip_ext().flash_attention(q, k5, v5))
        kc = kv.permute(1, 0, 2, 3).reshape(1, lkv, 2 * inner)
        kcat = kc[..., :inner].view(1, lkv, h, 64).transpose(1, 2).contiguous()
        vcat = kc[..., inner:].view(1, lkv, h, 64).transpose(1, 2).contiguous()
        ms_sdpa = timeit(lambda: F.scaled_dot_product_attention(q, kcat, vcat))
        flops = 4.0 * lq * lkv * 64 * h
        results.append({
            **tag,
            "op": "flash_attention_stale_chunked", "heads": h, "Lq": lq, "Lkv": lkv,
            "n_chunks": n, "ms_ours": ms_ours, "ms_sdpa_precat": ms_sdpa,
            "tflops_ours": flops / ms_ours / 1e9,
            "tflops_sdpa_precat": flops / ms_sdpa / 1e9,
        })
        print(json.dumps(results[-1]), flush=True)

    # ---- split-KV on the under-filled shapes ----
    splitkv_sweep(results)

    # ---- implicit-GEMM conv3x3 at SDXL 3840^2 shapes (2-sample CFG batch) ----
    torch.backends.cudnn.benchmark = True
    conv_shapes = [
        (4, 320, 480, 480, 1),      # conv_in
        (320, 320, 480, 480, 1),    # down0 ResBlock
        (320, 320, 240, 240, 2),    # downsample
        (640, 640, 240, 240, 1),
        (1280, 1280, 120, 120, 1),  # mid/up ResBlocks
        (2560, 1280, 120, 120, 1),  # up-block concat conv
        (960, 320, 480, 480, 1),
    ]
    for cin, cout, h, w, s in conv_shapes:
        x = torch.randn(2, cin, h, w, device=dev, dtype=dt) * 0.5
        wt = torch.randn(cout, cin, 3, 3, device=dev, dtype=dt) * (cin * 9) ** -0.5
        bias = torch.randn(cout, device=dev, dtype=dt)
        packed = ops.pack_conv3x3_weight(wt, dt)
        ms_ours = timeit(lambda: ops.conv3x3_halo(x, wt, bias, s, packed=packed))
        ms_ref = timeit(lambda: F.conv2d(x, wt, bias, stride=s, padding=1))
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        flops = 2.0 * 2 * cout * ho * wo * cin * 9
        results.append({
            **tag,
            "op": "conv3x3", "cin": cin, "cout": cout, "h": h, "w": w, "stride": s,
            "ms_ours": ms_ours, "ms_miopen": ms_ref,
            "tflops_ours": flops / ms_ours / 1e9,
            "tflops_miopen": flops / ms_ref / 1e9,
        })
        print(json.dumps(results[-1]), flush=True)

    # ---- the VAE encoder's downsample convs (pad_lo=0) ----
    vae_downsample_rows(results, dt, tag)

    # ---- rescaled-CFG DDIM step: three native launches vs the torch ops ----
    rescale_step_rows(results)

    # ---- fused GN+SiLU at SDXL shapes ----
    for c, hw in [(320, 480), (640, 240), (1280, 120), (320, 128), (640, 64)]:
        x = torch.randn(2, c, hw, hw, device=dev, dtype=torch.bfloat16)
        w = torch.randn(c, device=dev, dtype=torch.bfloat16)
        b = torch.randn(c, device=dev, dtype=torch.bfloat16)
        ms_ours = timeit(lambda: ops.group_norm_silu(x, 32, w, b, 1e-5, silu=True))
        ms_ref = timeit(lambda: F.silu(F.group_norm(x, 32, w, b, 1e-5)))
        gb = x.numel() * 2 * 2 / 1e9  # read + write
        results.append({
            "op": "gn_silu", "C": c, "HW": hw,
            "ms_ours": ms_ours, "ms_torch": ms_ref,
            "tbps_ours": gb / ms_ours, "tbps_torch": gb / ms_ref,
        })
        print(json.dumps(results[-1]), flush=True)

    # ---- GEGLU ----
    for rows, inner in [(4096, 2560), (14400, 5120), (57600, 2560)]:
        x = torch.randn(1, rows, 2 * inner, device=dev, dtype=torch.bfloat16)
        ms_ours = timeit(lambda: ops.geglu(x))
        def ref():
            a, g = x.chunk(2, dim=-1)
            return a * F.gelu(g)
        ms_ref = timeit(ref)
        gb = x.numel() * 2 * 1.5 / 1e9
        results.append({
            "op": "geglu", "rows": rows, "inner": inner,
            "ms_ours": ms_ours, "ms_torch": ms_ref,
            "tbps_ours": gb / ms_ours, "tbps_torch": gb / ms_ref,
        })
        print(json.dumps(results[-1]), flush=True)

    # ---- fused (residual+)LayerNorm at SDXL transformer shapes ----
    for rows, c in [(57600, 640), (14400, 1280), (4096, 640)]:
        x = torch.randn(1, rows, c, device=dev, dtype=dt)
        r = torch.randn(1, rows, c, device=dev, dtype=dt)
        w = torch.randn(c, device=dev, dtype=dt)
        b = torch.randn(c, device=dev, dtype=dt)
        ms_ours = timeit(lambda: ops.hip_ext().add_layer_norm(x, r, w, b, 1e-5))
        def ref():
            s2 = x + r
            return s2, F.layer_norm(s2, (c,), w, b, 1e-5)
        ms_ref = timeit(ref)
        gb = x.numel() * 2 * 4 / 1e9  # 2 reads + 2 writes
        results.append({
            **tag,
            "op": "add_layer_norm", "rows": rows, "C": c,
            "ms_ours": ms_ours, "ms_torch": ms_ref,
            "tbps_ours": gb / ms_ours, "tbps_torch": gb / ms_ref,
        })
        print(json.dumps(results[-1]), flush=True)

    # ---- VAE 512-dim single-head mid attention ----
    for l in (4096, 16384):
        q = torch.randn(1, l, 512, device=dev, dtype=dt)
        k = torch.randn(1, l, 512, device=dev, dtype=dt)
        v = torch.randn(1, l, 512, device=dev, dtype=dt)
        ms_ours = timeit(lambda: ops.hip_ext().vae_attention(q, k, v), iters=5, warmup=2)
        flops = 4.0 * l * l * 512
        results.append({
            **tag,
            "op": "vae_attention", "L": l, "ms_ours": ms_ours,
            "tflops_ours": flops / ms_ours / 1e9,
        })
        print(json.dumps(results[-1]), flush=True)

    with open("gpurun_out/kernel_bench.json", "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    sys.exit(main())
