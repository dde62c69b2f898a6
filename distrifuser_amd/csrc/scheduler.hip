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

#include "dispatch.h"

namespace {

template <typename T, bool VEC>
__global__ void cfg_affine_step_kernel(const T* __restrict__ noise_u,
                                       const T* __restrict__ noise_c, const T* __restrict__ x,
                                       T* __restrict__ out, float g, float ca, float cb,
                                       int64_t total) {
    constexpr int V = VEC ? VecN<T>::value : 1;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t vid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; vid * V < total;
         vid += stride) {
        const int64_t i = vid * V;
        if (VEC) {
            uint4 ur = *reinterpret_cast<const uint4*>(noise_u + i);
            uint4 cr = *reinterpret_cast<const uint4*>(noise_c + i);
            uint4 xr = *reinterpret_cast<const uint4*>(x + i);
            const T* u = reinterpret_cast<const T*>(&ur);
            const T* c = reinterpret_cast<const T*>(&cr);
            const T* xi = reinterpret_cast<const T*>(&xr);
            uint4 orw;
            T* o = reinterpret_cast<T*>(&orw);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float nu = to_f32(u[j]);
                const float eps = nu + g * (to_f32(c[j]) - nu);
                o[j] = from_f32<T>(ca * to_f32(xi[j]) + cb * eps);
            }
            *reinterpret_cast<uint4*>(out + i) = orw;
        } else {
            const float nu = to_f32(noise_u[i]);
            const float eps = nu + g * (to_f32(noise_c[i]) - nu);
            out[i] = from_f32<T>(ca * to_f32(x[i]) + cb * eps);
        }
    }
}

}  // namespace

void launch_cfg_affine_step(const void* noise_u, const void* noise_c, const void* x, void* out,
                            float g, float ca, float cb, int64_t total, int dtype,
                            hipStream_t stream) {
    const int block = 256;
    dispatch_dtype(dtype, [&]<typename T>(std::type_identity<T>) {
        dispatch_bool(total % VecN<T>::value == 0, [&]<bool VEC>(std::bool_constant<VEC>) {
            const int grid = grid_for(total / (VEC ? VecN<T>::value : 1), block);
            cfg_affine_step_kernel<T, VEC><<<grid, block, 0, stream>>>(
                (const T*)noise_u, (const T*)noise_c, (const T*)x, (T*)out, g, ca, cb, total);
        });
    });
}

namespace {

// DPM-Solver++(2M): x' = ca*x + cb*eps + cc*x0_prev, also emits
// x0 = cx*x + ce*eps for the next step (x0_prev null on the first step).
// x0 state kept in fp32: it reaches ~1/alpha_t * x magnitudes early in the
// trajectory, where bf16 granularity visibly perturbs the 2M correction.
template <typename T>
__global__ void cfg_dpm_step_kernel(const T* __restrict__ noise_u, const T* __restrict__ noise_c,
                                    const T* __restrict__ x, const float* __restrict__ x0_prev,
                                    T* __restrict__ out, float* __restrict__ x0_out, float g,
                                    float ca, float cb, float cc, float cx, float ce,
                                    int64_t total) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const float nu = to_f32(noise_u[i]);
        const float eps = nu + g * (to_f32(noise_c[i]) - nu);
        const float xf = to_f32(x[i]);
        float prev = ca * xf + cb * eps;
        if (x0_prev) prev += cc * x0_prev[i];
        out[i] = from_f32<T>(prev);
        x0_out[i] = cx * xf + ce * eps;
    }
}

}  // namespace

void launch_cfg_dpm_step(const void* nu, const void* nc, const void* x, const void* x0_prev,
                         void* out, void* x0_out, float g, float ca, float cb, float cc,
                         float cx, float ce, int64_t total, int dtype, hipStream_t stream) {
    const int block = 256;
    const int grid = grid_for(total, block);
    dispatch_dtype(dtype, [&]<typename T>(std::type_identity<T>) {
        cfg_dpm_step_kernel<T><<<grid, block, 0, stream>>>(
            (const T*)nu, (const T*)nc, (const T*)x, (const float*)x0_prev, (T*)out,
            (float*)x0_out, g, ca, cb, cc, cx, ce, total);
    });
}
