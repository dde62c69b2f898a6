// Fused GroupNorm kernels (gfx950).
//
// Reference semantics: ops/eager.py group_norm_{stats,apply,silu}. The op is
// HBM-bandwidth-bound on MI355X (8 TB/s), so everything is vectorized to
// 16 B/lane and SiLU is fused into the normalization epilogue (every GN in an
// SD ResBlock is followed by SiLU — fusing halves the traffic of a separate
// activation pass). Stats use a grid-strided partial-reduction kernel: every
// block stores the sums of its chunk, and a second small kernel adds a group's
// chunks in a fixed order, so the moments are the same bits on every run and
// on every rank (atomic adds would land in scheduling order; one last-bit
// difference in the VAE encoder's moments is enough to move the img2img and
// inpaint init latents). Each (sample, group) slab is contiguous in NCHW.

#include "boundary_plan.h"
#include "dispatch.h"

namespace {

template <typename T, bool VEC>
__global__ void gn_stats_partial_kernel(const T* __restrict__ x, float* __restrict__ partial,
                                        int64_t group_len, int chunks, int ngt) {
    constexpr int V = VEC ? VecN<T>::value : 1;
    const int ng = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    // per-chunk range, V-aligned (VEC requires group_len % V == 0, host-checked)
    const int64_t nvec = group_len / V;
    const int64_t per = (nvec + chunks - 1) / chunks;
    const int64_t v0 = chunk * per;
    const int64_t v1 = min(v0 + per, nvec);
    const T* base = x + (int64_t)ng * group_len;

    float s = 0.f, ss = 0.f;
    for (int64_t iv = v0 + threadIdx.x; iv < v1; iv += blockDim.x) {
        if (VEC) {
            uint4 raw = *reinterpret_cast<const uint4*>(base + iv * V);
            const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                float f = to_f32(e[j]);
                s += f;
                ss += f * f;
            }
        } else {
            float f = to_f32(base[iv]);
            s += f;
            ss += f * f;
        }
    }
    __shared__ float lds[2 * 16];
    block_reduce_sum2(s, ss, lds);
    // partial: [2][ngt][chunks]
    if (threadIdx.x == 0) {
        partial[(int64_t)ng * chunks + chunk] = s;
        partial[((int64_t)ngt + ng) * chunks + chunk] = ss;
    }
}

// out[e] = sum over the chunks of ws[e][:], e in [0, 2*ngt): one wave per
// entry, lane-strided partial sums and a butterfly, the same order every time
__global__ void gn_reduce_chunks_kernel(const float* __restrict__ ws, float* __restrict__ out,
                                        int chunks, int entries) {
    const int e = blockIdx.x * (blockDim.x / WAVE_SIZE) + threadIdx.x / WAVE_SIZE;
    if (e >= entries) return;
    const int lane = threadIdx.x % WAVE_SIZE;
    float v = 0.f;
    for (int c = lane; c < chunks; c += WAVE_SIZE) v += ws[(int64_t)e * chunks + c];
    v = wave_all_reduce_sum(v);
    if (lane == 0) out[e] = v;
}

template <typename T>
__global__ void gn_finalize_kernel(const float* __restrict__ partial, T* __restrict__ out,
                                   float inv_count, int total) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * total) out[i] = from_f32<T>(partial[i] * inv_count);
}

// The GroupNorm arithmetic of every apply kernel, NCHW and token-layout alike:
// the per-channel scale / shift and the per-element value, each rounding step
// spelled out with contraction off, so the result is a property of this source
// and not of where an optimiser chooses to form fmas. There are two forms.
// FUSED takes `m * sc` and `x * sc` into fmas; the other rounds each product
// first. gn_fused() on the host picks the form from the tensor alone, so the
// NCHW kernel and both token tile paths give the same bits for the same tensor
// (tests/test_transformer_boundary_gpu.py holds them to that).
template <bool FUSED>
__device__ __forceinline__ void gn_scale_shift(float m, float msq, float eps, float wv, float bv,
                                               float& sc, float& sh) {
#pragma clang fp contract(off)  // every fma below is spelled out
    float var = __builtin_fmaf(-m, m, msq);
    var = var < 0.f ? 0.f : var;
    const float inv = rsqrtf(var + eps);
    sc = wv * inv;
    if (FUSED) {
        sh = __builtin_fmaf(-m, sc, bv);
    } else {
        const float ms = m * sc;
        sh = bv - ms;
    }
}
template <bool FUSED>
__device__ __forceinline__ float gn_norm(float x, float sc, float sh) {
#pragma clang fp contract(off)
    if (FUSED) return __builtin_fmaf(x, sc, sh);
    const float xs = x * sc;
    return xs + sh;
}

// Fused arithmetic iff HW is a whole number of 16-byte vectors: the tensors the
// NCHW kernel takes with vector accesses. The only place that decides the form.
template <typename T>
bool gn_fused(int64_t hw) {
    return hw % VecN<T>::value == 0;
}

template <typename T, bool SILU, bool VEC>
__global__ void gn_apply_kernel(const T* __restrict__ x, T* __restrict__ y,
                                const float* __restrict__ mean, const float* __restrict__ meansq,
                                const T* __restrict__ w, const T* __restrict__ b, float eps,
                                int64_t hw, int C, int G, int64_t total) {
    constexpr int V = VEC ? VecN<T>::value : 1;
    const int gs = C / G;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t vid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; vid * V < total;
         vid += stride) {
        const int64_t i = vid * V;
        const int64_t c = (i / hw) % C;
        const int64_t n = i / (hw * (int64_t)C);
        const int g = (int)(c / gs);
        float sc, sh;  // VEC is also the arithmetic form: gn_fused() chose both
        gn_scale_shift<VEC>(mean[n * G + g], meansq[n * G + g], eps, w ? to_f32(w[c]) : 1.f,
                            b ? to_f32(b[c]) : 0.f, sc, sh);
        if (VEC) {
            uint4 raw = *reinterpret_cast<const uint4*>(x + i);
            const T* e = reinterpret_cast<const T*>(&raw);
            uint4 outv;
            T* o = reinterpret_cast<T*>(&outv);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                float f = gn_norm<VEC>(to_f32(e[j]), sc, sh);
                if (SILU) f = siluf(f);
                o[j] = from_f32<T>(f);
            }
            *reinterpret_cast<uint4*>(y + i) = outv;
        } else {
            float f = gn_norm<VEC>(to_f32(x[i]), sc, sh);
            if (SILU) f = siluf(f);
            y[i] = from_f32<T>(f);
        }
    }
}

// ---- NCHW <-> token-major transposing kernels --------------------------------
// The transformer boundary: GroupNorm apply that writes [N, HW, C] (the layout
// proj_in reads) and the closing residual add that reads [N, HW, C] and writes
// NCHW. Both are tiled transposes through LDS; launch arithmetic is in
// boundary_plan.h.
//
// Vector path (16-bit types, HW % 8 == 0, C % 8 == 0): a block owns 64
// channels x 64 pixels. The LDS image is pixel-major, [64 pixels][64 channels]
// = 32 dwords per pixel row, each dword a pair of neighbouring channels. The
// 16-byte chunk q (8 channels) of pixel row p sits at chunk q ^ ((p >> 3) & 7):
//  - NCHW side, thread (cp = t >> 3, pv = t & 7) holds channels 2cp, 2cp+1 at
//    pixels 8pv..8pv+7 and moves 8 dwords, dword j at row 8pv + j. The 32
//    lanes of a b32 lane group have 4 consecutive cp of one chunk and all 8
//    pv, so ((q ^ pv) << 2 | cp & 3) covers the 32 banks once.
//  - token side, thread (p = t >> 3, q = t & 7) moves one 16-byte chunk; the 8
//    lanes of a pixel row cover its 32 dwords once.
constexpr int BT = BOUNDARY_VEC_TILE;

__device__ __forceinline__ int bt_dword(int prow, int cp) {
    return prow * (BT / 2) + (((cp >> 2) ^ ((prow >> 3) & 7)) << 2 | (cp & 3));
}
__device__ __forceinline__ int bt_chunk(int prow, int q) {
    return prow * (BT / 2) + ((q ^ ((prow >> 3) & 7)) << 2);
}

template <typename T>
__device__ __forceinline__ uint32_t bits16(T v) {
    return (uint32_t)__builtin_bit_cast(uint16_t, v);
}

template <typename T, bool SILU>
__global__ __launch_bounds__(BOUNDARY_THREADS) void gn_apply_tokens_vec_kernel(
    const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ mean,
    const float* __restrict__ meansq, const T* __restrict__ w, const T* __restrict__ b, float eps,
    int64_t hw, int C, int G) {
    static_assert(sizeof(T) == 2, "16-bit types only");
    __shared__ __attribute__((aligned(16))) uint32_t tile[BT * BT / 2];
    const int t = threadIdx.x;
    const int64_t n = blockIdx.z;
    const int c0 = blockIdx.y * BT;
    const int64_t p0 = (int64_t)blockIdx.x * BT;
    const int gs = C / G;
    {
        const int pv = t & 7, cp = t >> 3;
        const int c = c0 + 2 * cp;
        const int64_t p = p0 + pv * 8;
        uint32_t packed[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (c < C && p < hw) {  // C is even: channel c + 1 exists with c
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int ch = c + h;
                const int g = ch / gs;
                float sc, sh;  // HW % 8 == 0 here: the NCHW kernel's vector variant
                gn_scale_shift<true>(mean[n * G + g], meansq[n * G + g], eps,
                                     w ? to_f32(w[ch]) : 1.f, b ? to_f32(b[ch]) : 0.f, sc, sh);
                const uint4 raw = *reinterpret_cast<const uint4*>(x + (n * C + ch) * hw + p);
                const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float f = gn_norm<true>(to_f32(e[j]), sc, sh);
                    if (SILU) f = siluf(f);
                    packed[j] |= bits16(from_f32<T>(f)) << (16 * h);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) tile[bt_dword(pv * 8 + j, cp)] = packed[j];
    }
    __syncthreads();
    {
        const int q = t & 7;
        const int ch = c0 + q * 8;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int pr = (t >> 3) + 32 * pass;
            const int64_t pix = p0 + pr;
            const uint4 v = *reinterpret_cast<const uint4*>(&tile[bt_chunk(pr, q)]);
            if (pix < hw && ch < C) *reinterpret_cast<uint4*>(y + (n * hw + pix) * C + ch) = v;
        }
    }
}

// Any type, any HW, any C % G == 0: 32 x 32 elements per block through a padded
// fp32 tile (the value is rounded once, at the store, as in gn_apply_kernel).
template <typename T, bool SILU, bool FUSED>
__global__ __launch_bounds__(BOUNDARY_THREADS) void gn_apply_tokens_scalar_kernel(
    const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ mean,
    const float* __restrict__ meansq, const T* __restrict__ w, const T* __restrict__ b, float eps,
    int64_t hw, int C, int G) {
    constexpr int S = BOUNDARY_SCALAR_TILE;
    __shared__ float tile[S][S + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t n = blockIdx.z;
    const int c0 = blockIdx.y * S;
    const int64_t p0 = (int64_t)blockIdx.x * S;
    const int gs = C / G;
#pragma unroll
    for (int i = 0; i < S / 8; ++i) {
        const int cl = ty + 8 * i;
        const int c = c0 + cl;
        const int64_t p = p0 + tx;
        if (c < C && p < hw) {
            const int g = c / gs;
            float sc, sh;
            gn_scale_shift<FUSED>(mean[n * G + g], meansq[n * G + g], eps,
                                  w ? to_f32(w[c]) : 1.f, b ? to_f32(b[c]) : 0.f, sc, sh);
            float f = gn_norm<FUSED>(to_f32(x[(n * C + c) * hw + p]), sc, sh);
            if (SILU) f = siluf(f);
            tile[cl][tx] = f;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < S / 8; ++i) {
        const int pl = ty + 8 * i;
        const int64_t p = p0 + pl;
        const int c = c0 + tx;
        if (c < C && p < hw) y[(n * hw + p) * C + c] = from_f32<T>(tile[tx][pl]);
    }
}

// out[n, c, p] = round(float(y[n, p, c]) + float(res[n, c, p])): the mirror of
// gn_apply_tokens_vec_kernel. res has batch / channel strides rs_n / rs_c
// (elements) and a contiguous pixel plane; out is contiguous NCHW.
template <typename T>
__global__ __launch_bounds__(BOUNDARY_THREADS) void tokens_add_nchw_vec_kernel(
    const T* __restrict__ y, const T* __restrict__ res, T* __restrict__ out, int64_t hw, int C,
    int64_t rs_n, int64_t rs_c) {
    static_assert(sizeof(T) == 2, "16-bit types only");
    __shared__ __attribute__((aligned(16))) uint32_t tile[BT * BT / 2];
    const int t = threadIdx.x;
    const int64_t n = blockIdx.z;
    const int c0 = blockIdx.y * BT;
    const int64_t p0 = (int64_t)blockIdx.x * BT;
    // NCHW-side coordinates; the residual loads go out before the transpose
    const int pv = t & 7, cp = t >> 3;
    const int c = c0 + 2 * cp;
    const int64_t p = p0 + pv * 8;
    const bool live = c < C && p < hw;
    uint4 r[2] = {uint4{0, 0, 0, 0}, uint4{0, 0, 0, 0}};
    if (live) {
        r[0] = *reinterpret_cast<const uint4*>(res + n * rs_n + (int64_t)c * rs_c + p);
        r[1] = *reinterpret_cast<const uint4*>(res + n * rs_n + (int64_t)(c + 1) * rs_c + p);
    }
    {
        const int q = t & 7;
        const int ch = c0 + q * 8;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int pr = (t >> 3) + 32 * pass;
            const int64_t pix = p0 + pr;
            uint4 v{0, 0, 0, 0};
            if (pix < hw && ch < C) v = *reinterpret_cast<const uint4*>(y + (n * hw + pix) * C + ch);
            *reinterpret_cast<uint4*>(&tile[bt_chunk(pr, q)]) = v;
        }
    }
    __syncthreads();
    if (live) {
        uint32_t d[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = tile[bt_dword(pv * 8 + j, cp)];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const T* re = reinterpret_cast<const T*>(&r[h]);
            uint4 outv;
            T* o = reinterpret_cast<T*>(&outv);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const T yv = __builtin_bit_cast(T, (uint16_t)(d[j] >> (16 * h)));
                o[j] = from_f32<T>(to_f32(yv) + to_f32(re[j]));
            }
            *reinterpret_cast<uint4*>(out + (n * C + c + h) * hw + p) = outv;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(BOUNDARY_THREADS) void tokens_add_nchw_scalar_kernel(
    const T* __restrict__ y, const T* __restrict__ res, T* __restrict__ out, int64_t hw, int C,
    int64_t rs_n, int64_t rs_c) {
    constexpr int S = BOUNDARY_SCALAR_TILE;
    __shared__ float tile[S][S + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t n = blockIdx.z;
    const int c0 = blockIdx.y * S;
    const int64_t p0 = (int64_t)blockIdx.x * S;
#pragma unroll
    for (int i = 0; i < S / 8; ++i) {
        const int pl = ty + 8 * i;
        const int64_t p = p0 + pl;
        const int c = c0 + tx;
        if (c < C && p < hw) tile[pl][tx] = to_f32(y[(n * hw + p) * C + c]);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < S / 8; ++i) {
        const int cl = ty + 8 * i;
        const int c = c0 + cl;
        const int64_t p = p0 + tx;
        if (c < C && p < hw)
            out[(n * C + c) * hw + p] =
                from_f32<T>(tile[tx][cl] + to_f32(res[n * rs_n + (int64_t)c * rs_c + p]));
    }
}

template <typename T, bool CORRECTED>
__global__ void gn_merge_stats_kernel(T* __restrict__ buffer, int64_t row_stride,
                                      int64_t slot_off, int n_peers, int own,
                                      const T* __restrict__ fresh, float* __restrict__ out,
                                      int ng) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ng) return;
    // moments live as [mean[0..ng), meansq[ng..2ng)] within each peer slot
    float m_sum = 0.f, q_sum = 0.f;
    float m_own = 0.f, q_own = 0.f;
    for (int p = 0; p < n_peers; ++p) {
        const T* slot = buffer + p * row_stride + slot_off;
        float m = to_f32(slot[g]);
        float q = to_f32(slot[ng + g]);
        if (p == own) {
            m_own = m;
            q_own = q;
            if (!CORRECTED) {  // stale_gn substitutes the fresh slot
                m = to_f32(fresh[g]);
                q = to_f32(fresh[ng + g]);
            }
        }
        m_sum += m;
        q_sum += q;
    }
    float mean = m_sum / n_peers;
    float msq = q_sum / n_peers;
    const float f_m = to_f32(fresh[g]);
    const float f_q = to_f32(fresh[ng + g]);
    if (CORRECTED) {
        mean += f_m - m_own;
        msq += f_q - q_own;
        // negative-variance guard: fall back to the local slice variance
        // (reference pp/groupnorm.py:60-63)
        const float var = msq - mean * mean;
        if (var < 0.f) msq = mean * mean + (f_q - f_m * f_m);
    }
    out[g] = mean;
    out[ng + g] = msq;
    // stage fresh into our slot for the async all-gather
    T* own_slot = buffer + own * row_stride + slot_off;
    own_slot[g] = fresh[g];
    own_slot[ng + g] = fresh[ng + g];
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

void launch_gn_merge_stats(void* buffer, int64_t row_stride, int64_t slot_off, int n_peers,
                           int own, const void* fresh, float* out, int ng, bool corrected,
                           int dtype, hipStream_t stream) {
    const int block = 256;
    const int grid = (ng + block - 1) / block;
    dispatch_dtype(dtype, [&]<typename T>(std::type_identity<T>) {
        dispatch_bool(corrected, [&]<bool CORRECTED>(std::bool_constant<CORRECTED>) {
            gn_merge_stats_kernel<T, CORRECTED><<<grid, block, 0, stream>>>(
                (T*)buffer, row_stride, slot_off, n_peers, own, (const T*)fresh, out, ng);
        });
    });
}

int gn_stats_chunks(int64_t group_len, int ngt, int dtype) {
    int chunks = 1;
    dispatch_dtype(dtype, [&]<typename T>(std::type_identity<T>) {
        const int V = group_len % VecN<T>::value == 0 ? VecN<T>::value : 1;
        // size chunks so the chip is filled: >= 2048 blocks total
        chunks = (int)std::max<int64_t>(1, (2048 + ngt - 1) / ngt);
        // but never more chunks than work
        int64_t nvec = std::max<int64_t>(group_len / V, 1);
        chunks = (int)std::min<int64_t>(chunks, (nvec + 255) / 256);
        chunks = std::max(chunks, 1);
    });
    return chunks;
}

void launch_gn_stats_partial(const void* x, float* ws, float* partial, int64_t group_len, int ngt,
                             int dtype, hipStream_t stream) {
    const int chunks = gn_stats_chunks(group_len, ngt, dtype);
    dispatch_dtype(dtype, [&]<typename T>(std::type_identity<T>) {
        dispatch_bool(group_len % VecN<T>::value == 0, [&]<bool VEC>(std::bool_constant<VEC>) {
            // one chunk: the block's sums are the group's, straight into partial
            gn_stats_partial_kernel<T, VEC><<<dim3(ngt * chunks), 256, 0, stream>>>(
                (const T*)x, chunks == 1 ? partial : ws, group_len, chunks, ngt);
        });
    });
    if (chunks > 1) {
        const int waves = 4, entries = 2 * ngt;
        gn_reduce_chunks_kernel<<<(entries + waves - 1) / waves, waves * WAVE_SIZE, 0, stream>>>(
            ws, partial, chunks, entries);
    }
}

void launch_gn_finalize(const float* partial, void* out, float inv_count, int ngt, int dtype,
                        hipStream_t stream) {
    const int block = 256;
    const int grid = (2 * ngt + block - 1) / block;
    dispatch_dtype(dtype, [&]<typename T>(std::type_identity<T>) {
        gn_finalize_kernel<T><<<grid, block, 0, stream>>>(partial, (T*)out, inv_count, ngt);
    });
}

void launch_gn_apply(const void* x, void* y, const float* mean, const float* meansq,
                     const void* weight, const void* bias, float eps, int64_t hw, int C, int G,
                     int N, bool silu, int dtype, hipStream_t stream) {
    const int64_t total = (int64_t)N * C * hw;
    const int block = 256;
    dispatch_dtype(dtype, [&]<typename T>(std::type_identity<T>) {
        dispatch_bool(gn_fused<T>(hw), [&]<bool VEC>(std::bool_constant<VEC>) {
            const int grid = grid_for(total / (VEC ? VecN<T>::value : 1), block);
            dispatch_bool(silu, [&]<bool SILU>(std::bool_constant<SILU>) {
                gn_apply_kernel<T, SILU, VEC><<<grid, block, 0, stream>>>(
                    (const T*)x, (T*)y, mean, meansq, (const T*)weight, (const T*)bias, eps, hw,
                    C, G, total);
            });
        });
    });
}

void launch_gn_apply_tokens(const void* x, void* y, const float* mean, const float* meansq,
                            const void* weight, const void* bias, float eps, int64_t hw, int C,
                            int G, int N, bool silu, int dtype, hipStream_t stream) {
    dispatch_dtype(dtype, [&]<typename T>(std::type_identity<T>) {
        const BoundaryPlan pl =
            boundary_plan(N, C, hw, (int)sizeof(T), aligned16(x) && aligned16(y));
        if (!pl.ok) return;  // empty; the binding rejects an oversized grid
        const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y, (unsigned)pl.grid_z);
        dispatch_bool(silu, [&]<bool SILU>(std::bool_constant<SILU>) {
            // one argument list for the three kernels
            const auto launch = [&](auto kernel) {
                kernel<<<grid, BOUNDARY_THREADS, 0, stream>>>((const T*)x, (T*)y, mean, meansq,
                                                              (const T*)weight, (const T*)bias,
                                                              eps, hw, C, G);
            };
            if constexpr (sizeof(T) == 2) {
                if (pl.vec) return launch(gn_apply_tokens_vec_kernel<T, SILU>);
            }
            if (gn_fused<T>(hw))
                launch(gn_apply_tokens_scalar_kernel<T, SILU, true>);
            else
                launch(gn_apply_tokens_scalar_kernel<T, SILU, false>);
        });
    });
}

void launch_tokens_add_nchw(const void* y, const void* residual, void* out, int64_t hw, int C,
                            int N, int64_t res_stride_n, int64_t res_stride_c, int dtype,
                            hipStream_t stream) {
    dispatch_dtype(dtype, [&]<typename T>(std::type_identity<T>) {
        const bool al = aligned16(y) && aligned16(residual) && aligned16(out) &&
                        res_stride_n % 8 == 0 && res_stride_c % 8 == 0;
        const BoundaryPlan pl = boundary_plan(N, C, hw, (int)sizeof(T), al);
        if (!pl.ok) return;
        const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y, (unsigned)pl.grid_z);
        const auto launch = [&](auto kernel) {
            kernel<<<grid, BOUNDARY_THREADS, 0, stream>>>((const T*)y, (const T*)residual,
                                                          (T*)out, hw, C, res_stride_n,
                                                          res_stride_c);
        };
        if constexpr (sizeof(T) == 2) {
            if (pl.vec) return launch(tokens_add_nchw_vec_kernel<T>);
        }
        launch(tokens_add_nchw_scalar_kernel<T>);
    });
}
