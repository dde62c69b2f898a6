// Fused CFG-combine + scheduler update (gfx950): one elementwise pass
// replaces the chunk/lerp/axpy torch ops between denoise steps (they run
// OUTSIDE the captured graphs, so their launch overhead is exposed every
// step). Deterministic eta=0 updates are affine in (x, eps):
//
//   eps = nu + g * (nc - nu)              (classifier-free guidance)
//   x'  = ca * x + cb * eps
//
// DDIM:  ca = sqrt(a_prev/a_t), cb = sqrt(1-a_prev) - ca * sqrt(1-a_t)
// Euler: ca = 1,                cb = sigma_next - sigma
// Reference numerics: schedulers/{ddim,euler}.py + pipelines._denoise.
//
// Inpainting (the MASKED axis of both step kernels) blends the step's result
// with the known region, the init latents re-noised to the next timestep:
//
//   known = sa * init + sb * init_noise
//   out   = m * x' + (1 - m) * known      (fp32, rounded once to T)
//
// In this form m == 1 returns x' and m == 0 returns known, and sa = 1, sb = 0
// makes known == init: exactly for finite inputs, up to the sign of a zero (a
// -0.0 comes out as +0.0, since the term that vanishes is +0), while a
// non-finite value on the vanishing side gives NaN (0 * inf). init, init_noise
// (one fp32 value per latent element) and m (one per pixel, shared by the
// channels) are read-only. A masked step also runs without a CFG pair:
// noise_c null means eps = nu.
//
// guidance_rescale (the RESCALE axis of both step kernels) scales the CFG
// result towards the cond branch's standard deviation, both taken over the
// one sample (C, H, W):
//
//   r     = phi * std(nc) / std(eps) + (1 - phi)
//   eps_r = r * eps                        (a rounding of its own)
//
// and the step is formed from eps_r. r comes from two launches before the
// step: cfg_moments_kernel writes each CHUNK's four partial sums to its own
// workspace row, cfg_rescale_finalize_kernel adds the rows in index order.
// No atomics, and a block count that depends on the element count alone: the
// factor is the same bits on every run and every device.
//
// The stochastic samplers (the NOISE axis of both step kernels) add one term
// to the same affine step, before any blend:
//
//   x' = fma(cn, z, x')                    z ~ N(0, 1)
//
// Euler ancestral: cn = sigma_up; DDIM with eta > 0: cn = the DDIM sigma;
// DPM-Solver++ SDE: cn = s_p * sqrt(1 - e^-2h). z is the Philox4x32-10 normal
// of (seed, draw, the element's index in the sample), philox.h: the same bits
// for every element type, for the 16-byte and the element-wise path and for
// every launch geometry. A vector thread computes whole Philox blocks (two for
// eight 16-bit elements, one for four fp32), the element-wise paths one block
// per element, of which they take their lane. Like MASKED, a NOISE step runs
// without a CFG pair (noise_c null: eps = nu). cn == 0 takes NOISE = false:
// every deterministic step runs the instantiation it ran before the axis
// existed.

#include "dispatch.h"
#include "philox.h"

// elements per block of cfg_moments_kernel, a constant of the arithmetic (it
// fixes the summation tree): 8 blocks at 1024^2, 113 at 3840^2
constexpr int64_t CFG_MOMENTS_CHUNK = 8192;
constexpr int CFG_MOMENTS_BLOCK = 256;

namespace {

// V consecutive fp32 values, 16 bytes at a time (p 16-byte aligned)
template <int V>
__device__ __forceinline__ void load_f32(float (&dst)[V], const float* __restrict__ p) {
#pragma unroll
    for (int q = 0; q < V / 4; ++q)
        *reinterpret_cast<float4*>(&dst[q * 4]) = *reinterpret_cast<const float4*>(p + q * 4);
}

// eps and x' of the masked kernels, with every rounding written out: m == 1
// must return the unmasked step bit for bit, so they round where the unmasked
// instantiation of the same (T, VEC) rounds (tests/test_inpaint_ops_gpu.py
// holds the two together). eps is one fma everywhere; x' is
// fma(ca, x, round(cb*eps)) when FUSED (the affine kernel's 16-byte path, which
// the unmasked launcher takes for every [1,4,h,w] fp32 tensor, and the 16-bit
// kernels) and round(ca*x) + round(cb*eps) when not (the fp32 DPM kernel, and
// x0 of every DPM kernel).
__device__ __forceinline__ float cfg_eps(float nu, float nc, float g) {
    return __builtin_fmaf(g, nc - nu, nu);
}
template <bool FUSED>
__device__ __forceinline__ float affine_xp(float ca, float x, float cb, float eps) {
#pragma clang fp contract(off)
    const float t = cb * eps;
    if constexpr (FUSED) return __builtin_fmaf(ca, x, t);
    const float s = ca * x;
    return s + t;
}

// eps_r of the RESCALE kernels: never contracted into the step's products, so
// f == 1 returns eps and with it the instantiation without RESCALE
__device__ __forceinline__ float rescale_eps(float f, float eps) {
#pragma clang fp contract(off)
    const float r = f * eps;
    return r;
}

// x' of a NOISE step, fma(cn, z, x') rounded to fp32. The empty asm keeps the
// value in a register as it is: without it the compiler folds this fma and the
// conversion to fp16 that follows into one v_fma_mixlo_f16, which rounds the
// exact sum straight to fp16, while a masked step (the blend comes between)
// rounds to fp32 first; m == 1 would then miss the unmasked step by one fp16
// ulp near a tie. Rounded to fp32 first, as the eager reference does.
__device__ __forceinline__ float add_step_noise(float cn, float z, float xp) {
    float r = __builtin_fmaf(cn, z, xp);
    asm volatile("" : "+v"(r));
    return r;
}

__device__ __forceinline__ float mask_blend(float xp, float m, float init, float init_noise,
                                            float sa, float sb) {
    const float known = sa * init + sb * init_noise;
    return m * xp + (1.f - m) * known;
}

// VEC && MASKED: hw % V == 0, so a vector never straddles a plane. MASKED,
// RESCALE and NOISE share the explicitly rounded form; RESCALE reads *factor,
// noise_c is then never null. NOISE: element i of the sample draws z(i).
template <typename T, bool VEC, bool MASKED, bool RESCALE, bool NOISE>
__global__ void cfg_affine_step_kernel(const T* __restrict__ noise_u,
                                       const T* __restrict__ noise_c, const T* __restrict__ x,
                                       T* __restrict__ out, float g, float ca, float cb,
                                       int64_t total, MaskBlend bl,
                                       const float* __restrict__ factor, float cn,
                                       PhiloxKey key) {
    constexpr int V = VEC ? VecN<T>::value : 1;
    constexpr bool EXPLICIT = MASKED || RESCALE || NOISE;
    float f = 1.f;
    if constexpr (RESCALE) f = *factor;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t vid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; vid * V < total;
         vid += stride) {
        const int64_t i = vid * V;
        if (VEC) {
            uint4 ur = *reinterpret_cast<const uint4*>(noise_u + i);
            uint4 cr = ur;
            if (!(MASKED || NOISE) || noise_c) cr = *reinterpret_cast<const uint4*>(noise_c + i);
            uint4 xr = *reinterpret_cast<const uint4*>(x + i);
            const T* u = reinterpret_cast<const T*>(&ur);
            const T* c = reinterpret_cast<const T*>(&cr);
            const T* xi = reinterpret_cast<const T*>(&xr);
            uint4 orw;
            T* o = reinterpret_cast<T*>(&orw);
            if constexpr (EXPLICIT) {
                alignas(16) float iv[V], nv[V], mv[V];
                if constexpr (MASKED) {
                    load_f32<V>(iv, bl.init + i);
                    load_f32<V>(nv, bl.init_noise + i);
                    load_f32<V>(mv, bl.mask + i % bl.hw);
                }
                float zv[(V + 3) / 4][4];  // i % 4 == 0: whole blocks
                if constexpr (NOISE) {
#pragma unroll
                    for (int b = 0; b < V / 4; ++b)
                        philox_normal4(key, (uint64_t)(i >> 2) + b, zv[b]);
                }
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float nu = to_f32(u[j]);
                    float eps = noise_c ? cfg_eps(nu, to_f32(c[j]), g) : nu;
                    if constexpr (RESCALE) eps = rescale_eps(f, eps);
                    float xp = affine_xp<true>(ca, to_f32(xi[j]), cb, eps);
                    if constexpr (NOISE) xp = add_step_noise(cn, zv[j / 4][j % 4], xp);
                    if constexpr (MASKED) xp = mask_blend(xp, mv[j], iv[j], nv[j], bl.sa, bl.sb);
                    o[j] = from_f32<T>(xp);
                }
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float nu = to_f32(u[j]);
                    const float eps = nu + g * (to_f32(c[j]) - nu);
                    o[j] = from_f32<T>(ca * to_f32(xi[j]) + cb * eps);
                }
            }
            *reinterpret_cast<uint4*>(out + i) = orw;
        } else if constexpr (EXPLICIT) {
            const float nu = to_f32(noise_u[i]);
            float eps = noise_c ? cfg_eps(nu, to_f32(noise_c[i]), g) : nu;
            if constexpr (RESCALE) eps = rescale_eps(f, eps);
            float xp = affine_xp<true>(ca, to_f32(x[i]), cb, eps);
            if constexpr (NOISE) xp = add_step_noise(cn, philox_normal1(key, (uint64_t)i), xp);
            if constexpr (MASKED)
                xp = mask_blend(xp, bl.mask[i % bl.hw], bl.init[i], bl.init_noise[i], bl.sa,
                                bl.sb);
            out[i] = from_f32<T>(xp);
        } else {
            const float nu = to_f32(noise_u[i]);
            const float eps = nu + g * (to_f32(noise_c[i]) - nu);
            out[i] = from_f32<T>(ca * to_f32(x[i]) + cb * eps);
        }
    }
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// Whether a step takes its NOISE instantiation: cn != 0, or the one call that
// has no instantiation without it (no CFG pair and no blend: the plain kernels
// always read noise_c), which then adds 0 * z.
bool step_draws(const StepNoise* noise, const void* noise_c, const MaskBlend* blend) {
    return noise != nullptr && (noise->cn != 0.f || (noise_c == nullptr && blend == nullptr));
}

PhiloxKey philox_key(const StepNoise* noise) {
    if (noise == nullptr) return PhiloxKey{0u, 0u, 0u};
    return PhiloxKey{(uint32_t)noise->seed, (uint32_t)(noise->seed >> 32), noise->draw};
}

}  // namespace

void launch_cfg_affine_step(const void* noise_u, const void* noise_c, const void* x, void* out,
                            float g, float ca, float cb, int64_t total, int dtype,
                            hipStream_t stream, const MaskBlend* blend, const float* factor,
                            const StepNoise* noise) {
    const int block = 256;
    const bool noisy = step_draws(noise, noise_c, blend);
    const float cn = noisy ? noise->cn : 0.f;
    const PhiloxKey key = philox_key(noisy ? noise : nullptr);
    dispatch_dtype(dtype, [&]<typename T>(std::type_identity<T>) {
        dispatch_bool(blend != nullptr, [&]<bool MASKED>(std::bool_constant<MASKED>) {
            bool vec = total % VecN<T>::value == 0;
            if (noisy)  // noise_c may be null: aligned16(nullptr) holds
                vec = vec && aligned16(noise_u) && aligned16(noise_c) && aligned16(x) &&
                      aligned16(out);
            if constexpr (MASKED)
                vec = blend->hw % VecN<T>::value == 0 && aligned16(noise_u) &&
                      aligned16(noise_c) && aligned16(x) && aligned16(out) &&
                      aligned16(blend->init) && aligned16(blend->init_noise) &&
                      aligned16(blend->mask);
            dispatch_bool(vec, [&]<bool VEC>(std::bool_constant<VEC>) {
                dispatch_bool(factor != nullptr, [&]<bool RESCALE>(std::bool_constant<RESCALE>) {
                    dispatch_bool(noisy, [&]<bool NOISE>(std::bool_constant<NOISE>) {
                        const int grid = grid_for(total / (VEC ? VecN<T>::value : 1), block);
                        cfg_affine_step_kernel<T, VEC, MASKED, RESCALE, NOISE>
                            <<<grid, block, 0, stream>>>(
                                (const T*)noise_u, (const T*)noise_c, (const T*)x, (T*)out, g, ca,
                                cb, total, MASKED ? *blend : MaskBlend{}, factor, cn, key);
                    });
                });
            });
        });
    });
}

namespace {

// DPM-Solver++(2M): x' = ca*x + cb*eps + cc*x0_prev, also emits
// x0 = cx*x + ce*eps for the next step (x0_prev null on the first step).
// x0 state kept in fp32: it reaches ~1/alpha_t * x magnitudes early in the
// trajectory, where bf16 granularity visibly perturbs the 2M correction.
// MASKED blends out alone: x0_out is the unmasked kernel's, bit for bit.
// NOISE: prev += cn * z(i) after the x0_prev term and before the blend; x0_out
// is the noise-free call's, bit for bit.
template <typename T, bool MASKED, bool RESCALE, bool NOISE>
__global__ void cfg_dpm_step_kernel(const T* __restrict__ noise_u, const T* __restrict__ noise_c,
                                    const T* __restrict__ x, const float* __restrict__ x0_prev,
                                    T* __restrict__ out, float* __restrict__ x0_out, float g,
                                    float ca, float cb, float cc, float cx, float ce,
                                    int64_t total, MaskBlend bl,
                                    const float* __restrict__ factor, float cn, PhiloxKey key) {
    float f = 1.f;
    if constexpr (RESCALE) f = *factor;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const float nu = to_f32(noise_u[i]);
        const float xf = to_f32(x[i]);
        if constexpr (MASKED || RESCALE || NOISE) {
            float eps = noise_c ? cfg_eps(nu, to_f32(noise_c[i]), g) : nu;
            if constexpr (RESCALE) eps = rescale_eps(f, eps);
            float prev = affine_xp<sizeof(T) == 2>(ca, xf, cb, eps);
            if (x0_prev) prev = __builtin_fmaf(cc, x0_prev[i], prev);
            if constexpr (NOISE) prev = add_step_noise(cn, philox_normal1(key, (uint64_t)i), prev);
            if constexpr (MASKED)
                prev = mask_blend(prev, bl.mask[i % bl.hw], bl.init[i], bl.init_noise[i], bl.sa,
                                  bl.sb);
            out[i] = from_f32<T>(prev);
            x0_out[i] = affine_xp<false>(cx, xf, ce, eps);
        } else {
            const float eps = nu + g * (to_f32(noise_c[i]) - nu);
            float prev = ca * xf + cb * eps;
            if (x0_prev) prev += cc * x0_prev[i];
            out[i] = from_f32<T>(prev);
            x0_out[i] = cx * xf + ce * eps;
        }
    }
}

}  // namespace

void launch_cfg_dpm_step(const void* nu, const void* nc, const void* x, const void* x0_prev,
                         void* out, void* x0_out, float g, float ca, float cb, float cc,
                         float cx, float ce, int64_t total, int dtype, hipStream_t stream,
                         const MaskBlend* blend, const float* factor, const StepNoise* noise) {
    const int block = 256;
    const int grid = grid_for(total, block);
    const bool noisy = step_draws(noise, nc, blend);
    const float cn = noisy ? noise->cn : 0.f;
    const PhiloxKey key = philox_key(noisy ? noise : nullptr);
    dispatch_dtype(dtype, [&]<typename T>(std::type_identity<T>) {
        dispatch_bool(blend != nullptr, [&]<bool MASKED>(std::bool_constant<MASKED>) {
            dispatch_bool(factor != nullptr, [&]<bool RESCALE>(std::bool_constant<RESCALE>) {
                dispatch_bool(noisy, [&]<bool NOISE>(std::bool_constant<NOISE>) {
                    cfg_dpm_step_kernel<T, MASKED, RESCALE, NOISE><<<grid, block, 0, stream>>>(
                        (const T*)nu, (const T*)nc, (const T*)x, (const float*)x0_prev, (T*)out,
                        (float*)x0_out, g, ca, cb, cc, cx, ce, total,
                        MASKED ? *blend : MaskBlend{}, factor, cn, key);
                });
            });
        });
    });
}

namespace {

// One thread per Philox block of the absolute stream: block q covers elements
// 4q .. 4q + 3, of which those in [offset, offset + numel) are stored.
__global__ void philox_normal_kernel(float* __restrict__ out, int64_t numel, int64_t offset,
                                     int64_t nblocks, PhiloxKey key) {
    const int64_t first = offset >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nblocks; b += stride) {
        float z[4];
        philox_normal4(key, (uint64_t)(first + b), z);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t e = ((first + b) << 2) + j - offset;
            if (e >= 0 && e < numel) out[e] = z[j];
        }
    }
}

}  // namespace

void launch_philox_normal(float* out, int64_t numel, int64_t offset, uint64_t seed,
                          uint32_t draw, hipStream_t stream) {
    if (numel <= 0) return;
    const int block = 256;
    const int64_t nblocks = ((offset + numel - 1) >> 2) - (offset >> 2) + 1;
    const StepNoise noise{1.f, seed, draw};
    philox_normal_kernel<<<grid_for(nblocks, block), block, 0, stream>>>(out, numel, offset,
                                                                         nblocks, philox_key(&noise));
}

namespace {

// Partial moments of the cond branch and of the CFG result for guidance_rescale.
// Block b reduces elements [b*CHUNK, min((b+1)*CHUNK, total)) and stores
// (sum nc, sum nc^2, sum eps, sum eps^2) to ws[b][0..3], fp32. A thread takes
// groups of V = 16 bytes / sizeof(T) elements, 256 groups apart, with one
// 16-byte load per branch (VEC: total % V == 0, both pointers 16-byte aligned)
// or element by element; the groups and the order of the adds are the same, so
// the two forms give the same bits.
template <typename T, bool VEC>
__global__ void __launch_bounds__(CFG_MOMENTS_BLOCK)
cfg_moments_kernel(const T* __restrict__ noise_u, const T* __restrict__ noise_c, float g,
                   int64_t total, float* __restrict__ ws) {
    constexpr int V = VecN<T>::value;
    __shared__ float lds[2][2 * CFG_MOMENTS_BLOCK / WAVE_SIZE];
    const int64_t base = (int64_t)blockIdx.x * CFG_MOMENTS_CHUNK;
    const int64_t end = base + CFG_MOMENTS_CHUNK < total ? base + CFG_MOMENTS_CHUNK : total;
    float sc = 0.f, qc = 0.f, sg = 0.f, qg = 0.f;
    for (int64_t i = base + (int64_t)threadIdx.x * V; i < end;
         i += (int64_t)CFG_MOMENTS_BLOCK * V) {
        alignas(16) T u[V], c[V];
        if constexpr (VEC) {
            *reinterpret_cast<uint4*>(u) = *reinterpret_cast<const uint4*>(noise_u + i);
            *reinterpret_cast<uint4*>(c) = *reinterpret_cast<const uint4*>(noise_c + i);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const bool in = i + j < end;
                u[j] = in ? noise_u[i + j] : from_f32<T>(0.f);
                c[j] = in ? noise_c[i + j] : from_f32<T>(0.f);
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (VEC || i + j < end) {
                const float nc = to_f32(c[j]);
                const float eps = cfg_eps(to_f32(u[j]), nc, g);
                sc += nc;
                qc = __builtin_fmaf(nc, nc, qc);
                sg += eps;
                qg = __builtin_fmaf(eps, eps, qg);
            }
        }
    }
    block_reduce_sum2(sc, qc, lds[0]);
    block_reduce_sum2(sg, qg, lds[1]);
    if (threadIdx.x == 0) {
        float* row = ws + (int64_t)blockIdx.x * 4;
        row[0] = sc;
        row[1] = qc;
        row[2] = sg;
        row[3] = qg;
    }
}

// One wave: lane k < 4 adds column k of ws [nblocks][4] in row order, lane 0
// forms both variances (n * var = sum x^2 - (sum x)^2 / n; n cancels in the
// ratio) and stores r = phi * std(nc) / std(eps) + (1 - phi).
__global__ void cfg_rescale_finalize_kernel(const float* __restrict__ ws, int nblocks,
                                            float inv_n, float phi, float* __restrict__ factor) {
    const int lane = threadIdx.x;
    float acc = 0.f;
    if (lane < 4)
        for (int b = 0; b < nblocks; ++b) acc += ws[(int64_t)b * 4 + lane];
    const float sc = __shfl(acc, 0, WAVE_SIZE), qc = __shfl(acc, 1, WAVE_SIZE);
    const float sg = __shfl(acc, 2, WAVE_SIZE), qg = __shfl(acc, 3, WAVE_SIZE);
    if (lane == 0) {
        const float var_c = fmaxf(qc - sc * sc * inv_n, 0.f);
        const float var_g = fmaxf(qg - sg * sg * inv_n, 0.f);
        factor[0] = phi * sqrtf(var_c / var_g) + (1.f - phi);
    }
}

}  // namespace

int cfg_moments_blocks(int64_t total) {
    return (int)((total + CFG_MOMENTS_CHUNK - 1) / CFG_MOMENTS_CHUNK);
}

void launch_guidance_rescale_factor(const void* noise_u, const void* noise_c, float g, float phi,
                                    int64_t total, float* ws, float* factor, int dtype,
                                    hipStream_t stream) {
    const int nblocks = cfg_moments_blocks(total);
    dispatch_dtype(dtype, [&]<typename T>(std::type_identity<T>) {
        const bool vec = total % VecN<T>::value == 0 && aligned16(noise_u) && aligned16(noise_c);
        dispatch_bool(vec, [&]<bool VEC>(std::bool_constant<VEC>) {
            cfg_moments_kernel<T, VEC><<<nblocks, CFG_MOMENTS_BLOCK, 0, stream>>>(
                (const T*)noise_u, (const T*)noise_c, g, total, ws);
        });
    });
    cfg_rescale_finalize_kernel<<<1, WAVE_SIZE, 0, stream>>>(ws, nblocks, 1.0f / (float)total,
                                                             phi, factor);
}

namespace {

// out [copies, 9, hw]: channels 0..3 latents / scale (rounded once), channel 4
// the mask and 5..8 the masked-image latents, both copied bit for bit; every
// copy is the same. VEC: hw % V == 0, a vector stays inside one channel plane.
template <typename T, bool VEC>
__global__ void inpaint_unet_input_kernel(const T* __restrict__ latents,
                                          const T* __restrict__ mask,
                                          const T* __restrict__ masked, T* __restrict__ out,
                                          float scale, int64_t hw, int copies) {
    constexpr int V = VEC ? VecN<T>::value : 1;
    const int64_t per_copy = 9 * hw;
    const int64_t total = per_copy * copies;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t vid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; vid * V < total;
         vid += stride) {
        const int64_t i = vid * V;
        const int64_t r = i % per_copy;  // offset inside one copy
        const int c = (int)(r / hw);
        const T* src = c < 4 ? latents + r : (c == 4 ? mask + (r - 4 * hw) : masked + (r - 5 * hw));
        if (VEC) {
            uint4 raw = *reinterpret_cast<const uint4*>(src);
            if (c < 4) {
                T* e = reinterpret_cast<T*>(&raw);
#pragma unroll
                for (int j = 0; j < V; ++j) e[j] = from_f32<T>(to_f32(e[j]) / scale);
            }
            *reinterpret_cast<uint4*>(out + i) = raw;
        } else {
            out[i] = c < 4 ? from_f32<T>(to_f32(*src) / scale) : *src;
        }
    }
}

}  // namespace

void launch_inpaint_unet_input(const void* latents, const void* mask, const void* masked,
                               void* out, float scale, int64_t hw, int copies, int dtype,
                               hipStream_t stream) {
    const int block = 256;
    const int64_t total = 9 * hw * copies;
    dispatch_dtype(dtype, [&]<typename T>(std::type_identity<T>) {
        const bool vec = hw % VecN<T>::value == 0 && aligned16(latents) && aligned16(mask) &&
                         aligned16(masked) && aligned16(out);
        dispatch_bool(vec, [&]<bool VEC>(std::bool_constant<VEC>) {
            const int grid = grid_for(total / (VEC ? VecN<T>::value : 1), block);
            inpaint_unet_input_kernel<T, VEC><<<grid, block, 0, stream>>>(
                (const T*)latents, (const T*)mask, (const T*)masked, (T*)out, scale, hw, copies);
        });
    });
}
