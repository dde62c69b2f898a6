// Fused GEGLU gate (gfx950): out[r, i] = in[r, i] * gelu(in[r, inner + i]).
// Memory-bound; 16 B/lane vector loads on both halves, erf-exact gelu
// (matches torch F.gelu default). Reference numerics: ops/eager.py geglu.

#include "dispatch.h"

namespace {

template <typename T, bool VEC>
__global__ void geglu_kernel(const T* __restrict__ in, T* __restrict__ out, int64_t rows,
                             int64_t inner) {
    constexpr int V = VEC ? VecN<T>::value : 1;
    const int64_t total_v = rows * inner / V;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t vid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; vid < total_v;
         vid += stride) {
        const int64_t i = vid * V;
        const int64_t r = i / inner;
        const int64_t col = i % inner;
        const T* a_ptr = in + r * 2 * inner + col;
        const T* g_ptr = a_ptr + inner;
        if (VEC) {
            uint4 araw = *reinterpret_cast<const uint4*>(a_ptr);
            uint4 graw = *reinterpret_cast<const uint4*>(g_ptr);
            const T* a = reinterpret_cast<const T*>(&araw);
            const T* g = reinterpret_cast<const T*>(&graw);
            uint4 oraw;
            T* o = reinterpret_cast<T*>(&oraw);
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = from_f32<T>(to_f32(a[j]) * geluf(to_f32(g[j])));
            *reinterpret_cast<uint4*>(out + i) = oraw;
        } else {
            out[i] = from_f32<T>(to_f32(*a_ptr) * geluf(to_f32(*g_ptr)));
        }
    }
}

}  // namespace

void launch_geglu(const void* in, void* out, int64_t rows, int64_t inner, int dtype,
                  hipStream_t stream) {
    const int block = 256;
    dispatch_dtype(dtype, [&]<typename T>(std::type_identity<T>) {
        dispatch_bool(inner % VecN<T>::value == 0, [&]<bool VEC>(std::bool_constant<VEC>) {
            const int grid = grid_for(rows * inner / (VEC ? VecN<T>::value : 1), block);
            geglu_kernel<T, VEC><<<grid, block, 0, stream>>>((const T*)in, (T*)out, rows, inner);
        });
    });
}
