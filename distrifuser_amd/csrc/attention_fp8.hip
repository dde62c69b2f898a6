// FP8 (OCP e4m3) self-attention forward, gfx950, head_dim 64, opt-in
// (ops.flash_attention(..., compute_dtype="fp8")). Q, K, V and P are e4m3 with
// power-of-two (E8M0) block scales that the scaled MFMA applies in hardware;
// scores, max, sum and O are fp32; the output is bf16 or fp16.
//
// Quantisation rule (the eager twin, ops/eager.py flash_attention_fp8, is the
// one written statement): x_hat = e4m3(x * 2^-e), e = ceil(log2(amax / 448)),
// e = 0 for an all-zero block.
//   Q: one e per row.   K: one e per token.   V: one e per (channel, block of
//   32 consecutive tokens).   P: e4m3(p * 2^8) with the B scale 2^-8.
// The row sum l is taken from the fp32 p; scale * log2(e) is applied to the
// MFMA result in fp32.
//
// Two kernels:
// * attn_quant_kv_kernel (pre-pass): one block per (128-token tile, b, h).
//   Reads K and V where the bf16 kernel reads them (any element strides, the
//   [B,H,NC,LC,64] stale-KV chunk views; the chunk walk lives here alone) and
//   writes one 16768-byte record per tile, zero beyond Lkv:
//     +0     K8  [128 t][64 d]            fp8, 16 B windows XOR-swizzled
//     +8192  V8T [2 slabs][64 d][64 t]    fp8, transposed, same swizzle form
//     +16384 K scale dwords [32 lo]       byte 2*slab + m
//     +16512 V scale dwords [64 lane]     byte 2*slab + dt
//   A record is the LDS image of its tile, so the attention kernel's staging
//   is a linear LDS-DMA copy, and a scale dword is what one lane hands to the
//   MFMA: op_sel picks the byte, no VALU unpacks anything.
// * flash_attn_fp8_kernel: the 8-wave block of 256 Q rows, 32 per wave, the
//   swapped QK^T and the lane-local online softmax of attention.hip. Per
//   64-token slab a wave issues 2 scaled MFMAs for S^T = K Q^T (each covers
//   all of d = 64; the bf16 kernel needs 8) and 2 for O^T += V^T P^T (bf16: 8).
//   KV records are staged by LDS-DMA into two buffers, one barrier per tile;
//   the tail is a tile like any other (the records are padded), masked.
//
// Row permutation instead of a P shuffle. MFMA (slab, m) takes as its A row
// rho the token
//     tok(m, rho) = 32*m + 16*((rho>>2)&1) + (rho&3) + 4*(rho>>3)
// of the slab (an LDS address, free). D register r of a lane in half hi is
// row rho = (r&3) + 8*(r>>2) + 4*hi, i.e. token 32*m + 16*hi + r. Byte
// j = 16*m + r of that lane's operand registers is k-element
// 32*m + 16*hi + r of the PV MFMA over the slab (layout below): the token
// itself. So P goes from the score registers to the B operand in register
// order with 16 cvt_pk_fp8 and nothing else (the bf16 kernel: 8 packs + 8
// permlane32_swap per 64 tokens), V8T keeps natural token order (a lane reads
// tokens 16*hi .. +15 and 32 + 16*hi .. +15 of its channel, two 16 B pieces),
// and a V scale block, k-elements 32*b .. +31, is 32 consecutive tokens.
//
// LDS banks (the 16-lane-group model of profiles/rocprof_3840_r06.md: one
// ds_read_b128 is served per 16 lanes, conflict-free iff their 16 B pieces
// fall in 16 different windows of the 256 B bank row). K8 and V8T rows are
// 64 B, four to a bank row, so the window of a piece is 4*(row&3) + w.
//   K: lanes lo = 0..15 of a group read rows tok(m, lo), row&3 = lo&3; the
//   four lanes that share it differ in lo bits 2,3 = token bits 4,2, so
//   w ^= ((t>>2)&1) | ((t>>4)&1)<<1 separates them.
//   V: the group reads rows d = d0 .. d0+15 at one window; the four lanes that
//   share d&3 differ in (d>>2)&3, so w ^= (d>>2)&3.
// Both XORs depend on the lane alone (not on m, slab, dt, tile): every
// fragment address is a per-lane base plus an immediate.
//
// Scaled-MFMA operand layout (v_mfma_scale_f32_32x32x64_f8f6f4, established on
// MI355X with launch_mfma_probe_fp8, held by tests/test_fp8_attention_gpu.py):
//   A[row = l&31][k], B[k][col = l&31] with k = 32*(j>>4) + 16*(l>>5) + (j&15),
//   j = 0..31 the byte order of the lane's 8 dwords: a lane's first 16 bytes
//   lie in k-block 0, its last 16 in k-block 1;
//   D[row = (r&3) + 8*(r>>2) + 4*(l>>5)][col = l&31];
//   the E8M0 scale of k-block b (k = 32*b .. +31) of a row / column is byte
//   op_sel of the scale dword of the lane in half b (l>>5 == b).
// (A scale that is the same for both k-blocks, Q rows and K tokens here, does
// not see the difference to "a lane's scale covers its own 32 bytes"; V's
// does.)

#include "dispatch.h"

namespace {

typedef int int8v __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int KVB = 128;                      // tokens per tile
constexpr int K8_BYTES = KVB * 64;            // 8192
constexpr int REC_V = K8_BYTES;               // V8T image
constexpr int REC_KS = 2 * K8_BYTES;          // K scale dwords
constexpr int REC_VS = REC_KS + 32 * 4;       // V scale dwords
constexpr int REC_BYTES = REC_VS + 64 * 4;    // 16768
static_assert(REC_BYTES == ATTN_FP8_TILE_BYTES);
constexpr int QW = 32, NW = 8, QBLK = QW * NW;

__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}

// E8M0 byte of 2^e, e = ceil(log2(amax / 448)): 448 = 1.75 * 2^8, so with
// amax = 1.f * 2^(E-127) the exponent is E - 135, one more when 1.f > 1.75
// (mantissa above 0x600000: the add carries into the exponent field). Clamped
// to [1, 254]; 127 (e = 0) for amax = 0.
__device__ __forceinline__ uint32_t e8m0_of_amax(float amax) {
    const uint32_t bits = __builtin_bit_cast(uint32_t, amax);
    const int byte = (int)((bits + 0x1FFFFFu) >> 23) - 8;
    return amax == 0.f ? 127u : (uint32_t)min(max(byte, 1), 254);
}
// 2^-e for the byte of 2^e
__device__ __forceinline__ float inv_scale_of(uint32_t byte) {
    return __builtin_bit_cast(float, (254u - byte) << 23);
}
// One v_mul_f32. The runs of independent multiplies in this file (quantise,
// O^T rescale) are written through it so that the vectoriser cannot pair them
// into packed fp32 instructions, which this file must not contain. The
// compiler does not see what an asm statement reads, so it keeps no wait
// state between a v_exp_f32 and a multiply by its result: after_trans() does.
__device__ __forceinline__ float mul1(float a, float b) {
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// v: the result of a transcendental instruction that asm statements go on to
// read. gfx950 needs one wait state between the two; the value the later
// statements use is the one that leaves here.
__device__ __forceinline__ float after_trans(float v) {
    asm volatile("s_nop 1" : "+v"(v));
    return v;
}
// four fp32 -> one dword of four e4m3 bytes, the first in the low byte
__device__ __forceinline__ uint32_t cvt4_fp8(float a, float b, float c, float d) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
    return (uint32_t)w;
}

template <int OPSEL_A, int OPSEL_B>
__device__ __forceinline__ float16v mfma_f8(int8v a, int8v b, float16v c, uint32_t sa,
                                            uint32_t sb) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, OPSEL_A, (int)sa,
                                                           OPSEL_B, (int)sb);
}

__device__ __forceinline__ float half_max(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    const uint32_t a = r[0], b = r[1];
    return fmaxf(__builtin_bit_cast(float, a), __builtin_bit_cast(float, b));
}
__device__ __forceinline__ float half_sum(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    const uint32_t a = r[0], b = r[1];
    return __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b);
}

// 32 consecutive 16-bit elements -> fp32
template <bool F16>
__device__ __forceinline__ void load32(const uint16_t* src, float (&x)[32]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint4 u = *reinterpret_cast<const uint4*>(src + i * 8);
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x[i * 8 + 2 * j] = b16_to_f32<F16>((uint16_t)(w[j] & 0xFFFFu));
            x[i * 8 + 2 * j + 1] = b16_to_f32<F16>((uint16_t)(w[j] >> 16));
        }
    }
}
// 32 fp32 (|x| * inv <= 448) -> 32 e4m3 bytes
__device__ __forceinline__ void quant32(const float (&x)[32], float inv, uint32_t (&w)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
        w[i] = cvt4_fp8(mul1(x[4 * i], inv), mul1(x[4 * i + 1], inv), mul1(x[4 * i + 2], inv),
                        mul1(x[4 * i + 3], inv));
}

// ---- pre-pass ------------------------------------------------------------------
// K: two threads per token, 32 channels each (the half row one attention lane
// reads). V: the tile goes through LDS as [128 t][64 d] 16-bit, then one
// thread per (channel, 32-token block) reads its column.
template <bool F16>
__global__ __launch_bounds__(256) void attn_quant_kv_kernel(FlashAttnParams p, uint8_t* ws) {
    __shared__ __attribute__((aligned(16))) uint16_t v_lds[KVB * 64];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x;
    const int bh = blockIdx.y;
    const int b = bh / p.H, h = bh % p.H;
    const int64_t Lkv = p.NC * p.LC;
    const int64_t n_tiles = gridDim.x;
    uint8_t* rec = ws + ((int64_t)bh * n_tiles + tile) * REC_BYTES;
    const uint16_t* kbase = p.k + b * p.k_sb + h * p.k_sh;
    const uint16_t* vbase = p.v + b * p.v_sb + h * p.v_sh;
    const int64_t t0 = (int64_t)tile * KVB;

    // V tile -> LDS (zeros beyond Lkv): 1024 16 B pieces, 4 per thread
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int piece = tid + i * 256;
        const int t = piece >> 3, c = piece & 7;
        const int64_t tg = t0 + t;
        uint4 u{0, 0, 0, 0};
        if (tg < Lkv) {
            const int64_t ch = tg / p.LC, tin = tg - ch * p.LC;
            u = *reinterpret_cast<const uint4*>(vbase + ch * p.v_sc + tin * p.v_sl + c * 8);
        }
        *reinterpret_cast<uint4*>(&v_lds[t * 64 + c * 8]) = u;
    }

    // K: token t, channels half*32 .. +31
    {
        const int t = tid >> 1, half = tid & 1;
        const int64_t tg = t0 + t;
        float x[32];
        float amax = 0.f;
        if (tg < Lkv) {
            const int64_t ch = tg / p.LC, tin = tg - ch * p.LC;
            load32<F16>(kbase + ch * p.k_sc + tin * p.k_sl + half * 32, x);
#pragma unroll
            for (int j = 0; j < 32; ++j) amax = fmaxf(amax, fabsf(x[j]));
        } else {
#pragma unroll
            for (int j = 0; j < 32; ++j) x[j] = 0.f;
        }
        amax = fmaxf(amax, __shfl_xor(amax, 1, WAVE_SIZE));
        const uint32_t sbyte = e8m0_of_amax(amax);
        uint32_t w[8];
        quant32(x, inv_scale_of(sbyte), w);
        const int swz = ((t >> 2) & 1) | (((t >> 4) & 1) << 1);
        uint8_t* row = rec + t * 64;
        *reinterpret_cast<uint4*>(row + (((2 * half) ^ swz) << 4)) = uint4{w[0], w[1], w[2], w[3]};
        *reinterpret_cast<uint4*>(row + (((2 * half + 1) ^ swz) << 4)) =
            uint4{w[4], w[5], w[6], w[7]};
        if (half == 0) {
            // token t = 64*slab + 32*m + 16*hi + r is A row rho of MFMA (slab, m)
            const int slab = t >> 6, m = (t >> 5) & 1, hi = (t >> 4) & 1, r = t & 15;
            const int rho = (r & 3) + 8 * (r >> 2) + 4 * hi;
            rec[REC_KS + rho * 4 + slab * 2 + m] = (uint8_t)sbyte;
        }
    }
    __syncthreads();

    // V: channel d, tokens blk*32 .. +31
    {
        const int d = tid & 63, blk = tid >> 6;
        float x[32];
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            x[j] = b16_to_f32<F16>(v_lds[(blk * 32 + j) * 64 + d]);
            amax = fmaxf(amax, fabsf(x[j]));
        }
        const uint32_t sbyte = e8m0_of_amax(amax);
        uint32_t w[8];
        quant32(x, inv_scale_of(sbyte), w);
        const int slab = blk >> 1, hi = blk & 1;
        const int swz = (d >> 2) & 3;
        uint8_t* row = rec + REC_V + slab * 4096 + d * 64;
        *reinterpret_cast<uint4*>(row + (((2 * hi) ^ swz) << 4)) = uint4{w[0], w[1], w[2], w[3]};
        *reinterpret_cast<uint4*>(row + (((2 * hi + 1) ^ swz) << 4)) =
            uint4{w[4], w[5], w[6], w[7]};
        rec[REC_VS + (hi * 32 + (d & 31)) * 4 + slab * 2 + (d >> 5)] = (uint8_t)sbyte;
    }
}

// ---- attention -------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(NW * WAVE_SIZE) __attribute__((amdgpu_waves_per_eu(4)))
void flash_attn_fp8_kernel(FlashAttnParams p, const uint8_t* __restrict__ ws, int n_tiles) {
    constexpr int NT = NW * WAVE_SIZE;
    constexpr int BUF = 2 * K8_BYTES;  // one buffer: K8 image, then V8T image
    __shared__ __attribute__((aligned(16))) char kv_lds[2 * BUF];

    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lo = lane & 31;
    const int hi = lane >> 5;
    const int bh = blockIdx.y;
    const int b = bh / p.H, h = bh % p.H;
    const int64_t q0 = (int64_t)blockIdx.x * QBLK;
    const int Lkv = (int)(p.NC * p.LC);
    const uint8_t* recs = ws + (int64_t)bh * n_tiles * REC_BYTES;

    // ---- Q: row q0 + wave*32 + lo, channels hi*32 .. +31, quantised in
    // registers; the row's amax is the max with the partner half ----
    const int64_t qrow = q0 + wave * QW + lo;
    const bool qvalid = qrow < p.Lq;
    int8v qf;
    uint32_t qs;
    {
        const uint16_t* qp = p.q + b * p.q_sb + h * p.q_sh + (qvalid ? qrow : (p.Lq - 1)) * p.q_sl;
        float x[32];
        load32<F16>(qp + hi * 32, x);
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 32; ++j) amax = fmaxf(amax, fabsf(x[j]));
        amax = half_max(amax);
        qs = e8m0_of_amax(amax);
        uint32_t w[8];
        quant32(x, inv_scale_of(qs), w);
#pragma unroll
        for (int i = 0; i < 8; ++i) qf[i] = (int)w[i];
    }

    // ---- fragment read bases (buffer 0). K: channels 32*hi .. +31 of row
    // tok(m, lo), windows 2*hi and 2*hi + 1, the second at base ^ 16. V:
    // tokens 16*hi .. +15 and 32 + 16*hi .. +15 of channel row lo, windows hi
    // and 2 + hi, the second at base ^ 32. (m, slab, dt) are immediates, a
    // buffer flip is ^ BUF ----
    int krd, vrd;
    {
        const int tok0 = 16 * ((lo >> 2) & 1) + (lo & 3) + 4 * (lo >> 3);  // tok(0, lo)
        const int kswz = ((lo >> 3) & 1) | (((lo >> 2) & 1) << 1);
        krd = tok0 * 64 + (((2 * hi) ^ kswz) << 4);
        vrd = REC_V + lo * 64 + ((hi ^ ((lo >> 2) & 3)) << 4);
    }
    auto frag = [&]<int SECOND>(std::integral_constant<int, SECOND>, int off) {
        const uint4 a = *reinterpret_cast<const uint4*>(&kv_lds[off]);
        const uint4 c = *reinterpret_cast<const uint4*>(&kv_lds[off ^ SECOND]);
        return int8v{(int)a.x, (int)a.y, (int)a.z, (int)a.w, (int)c.x, (int)c.y, (int)c.z, (int)c.w};
    };
    constexpr std::integral_constant<int, 16> K_FRAG{};
    constexpr std::integral_constant<int, 32> V_FRAG{};

    // ---- staging: a tile's K8 + V8T images are 16 KiB, linear; thread tid
    // moves the 16 B slots tid (K) and 512 + tid (V) by LDS-DMA. One asm
    // statement, as in attention.hip: unseen by the compiler's vmcnt counting
    // the loads stay in flight across the compute; M0 is saved and restored. --
    const uint32_t slot = (uint32_t)tid * 16;
    auto stage_dma = [&](int wbuf, int tile) {
        const uint64_t a = reinterpret_cast<uint64_t>(recs + (int64_t)tile * REC_BYTES);
        const u32x4 rs{(uint32_t)a, (uint32_t)(a >> 32) & 0xFFFFu, 0xFFFFFFFFu, 0x00020000u};
        const uint32_t piece = __builtin_amdgcn_readfirstlane(wave) * (WAVE_SIZE * 16);
        const uint32_t kd = lds_addr(&kv_lds[wbuf * BUF]) + piece;
        const uint32_t vd = kd + K8_BYTES;
        const uint32_t voff = K8_BYTES;
        uint32_t keep;
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %3\n\ts_nop 0\n\t"
            "buffer_load_dwordx4 %1, %2, 0 offen lds\n\t"
            "s_mov_b32 m0, %4\n\ts_nop 0\n\t"
            "buffer_load_dwordx4 %1, %2, %5 offen lds\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(slot), "s"(rs), "s"(kd), "s"(vd), "s"(voff)
            : "memory");
    };
    static_assert(NT * 16 == K8_BYTES);
    // the scale dwords of a tile: one K and one V dword per lane
    auto load_scales = [&](int tile, uint32_t& ks, uint32_t& vs) {
        const uint8_t* rec = recs + (int64_t)tile * REC_BYTES;
        ks = *reinterpret_cast<const uint32_t*>(rec + REC_KS + lo * 4);
        vs = *reinterpret_cast<const uint32_t*>(rec + REC_VS + lane * 4);
    };

    // Online softmax in the exp2 domain. c8 = 8 - m * scale2: p * 2^8 =
    // exp2(fma(s, scale2, c8)) is what the e4m3 pack takes, at most 256. l_run
    // sums those fp32 values over this lane's own tokens; the halves are added
    // once, in the epilogue, and the 2^8 leaves with the P scale byte 2^-8.
    float m_raw = -1e30f;
    float c8 = 8.f + 1e30f;
    float l_run = 0.f;
    float16v ot[2] = {};  // O^T: [dt] rows d = dt*32 + mfma32_row(r, hi), col q = lo
    const float scale2 = p.scale * 1.44269504088896340736f;
    constexpr uint32_t P_SCALE = 119;  // 2^-8

    uint32_t ks = 0, vs = 0;  // the scale dwords of the tile being computed

    auto qk_slab = [&]<int SLAB>(std::integral_constant<int, SLAB>, float16v (&s)[2]) {
        __builtin_amdgcn_s_setprio(1);
        s[0] = mfma_f8<SLAB * 2, 0>(frag(K_FRAG, krd + SLAB * 4096), qf, float16v{}, ks, qs);
        s[1] = mfma_f8<SLAB * 2 + 1, 0>(frag(K_FRAG, krd + SLAB * 4096 + 32 * 64), qf, float16v{},
                                        ks, qs);
        __builtin_amdgcn_s_setprio(0);
    };

    auto softmax_pv = [&]<int SLAB, bool MASK>(std::integral_constant<int, SLAB>,
                                               std::bool_constant<MASK>, float16v (&s)[2],
                                               int t0) {
        // s[m][r]: token t0 + 64*SLAB + 32*m + 16*hi + r of q column lo
        float tm = -1e30f;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (MASK) {
                    if (t0 + SLAB * 64 + 32 * m + 16 * hi + r >= Lkv) s[m][r] = -1e30f;
                }
                tm = fmaxf(tm, s[m][r]);
            }
        tm = half_max(tm);
        if (__any(tm > m_raw)) {
            const float m_new = fmaxf(m_raw, tm);
            const float c8_new = 8.f - m_new * scale2;
            const float corr = after_trans(__builtin_amdgcn_exp2f(c8_new - c8));
            m_raw = m_new;
            c8 = c8_new;
            l_run *= corr;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) ot[dt][r] = mul1(ot[dt][r], corr);
        }
        float pv[32];
        float tsum = 0.f;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            pv[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[j >> 4][j & 15], scale2, c8));
            tsum += pv[j];
        }
        l_run += tsum;
        // B fragment of the PV MFMA: byte j = 16*m + r is k-element (token)
        // 32*m + 16*hi + r
        int8v pb;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            pb[i] = (int)cvt4_fp8(pv[4 * i], pv[4 * i + 1], pv[4 * i + 2], pv[4 * i + 3]);
        __builtin_amdgcn_s_setprio(1);
        ot[0] = mfma_f8<SLAB * 2, 0>(frag(V_FRAG, vrd + SLAB * 4096), pb, ot[0], vs, P_SCALE);
        ot[1] = mfma_f8<SLAB * 2 + 1, 0>(frag(V_FRAG, vrd + SLAB * 4096 + 32 * 64), pb, ot[1], vs,
                                         P_SCALE);
        __builtin_amdgcn_s_setprio(0);
    };

    // one staged tile. A slab's 32 scores, its 32 p and O^T leave no room in
    // 128 registers for the next slab's scores (issuing them ahead spilled 93
    // registers), so MFMA and VALU overlap across the four waves of a SIMD,
    // not inside one.
    auto compute = [&]<bool MASK>(std::bool_constant<MASK> mask, int t0) {
        float16v s[2];
        qk_slab(std::integral_constant<int, 0>{}, s);
        softmax_pv(std::integral_constant<int, 0>{}, mask, s, t0);
        qk_slab(std::integral_constant<int, 1>{}, s);
        softmax_pv(std::integral_constant<int, 1>{}, mask, s, t0);
    };

    // ---- tile loop: two buffers, one barrier per tile (attention.hip's DMA
    // scheme without its register path: every tile is a linear record) ----
    // The vmcnt(0) is a builtin so that the compiler's own counting knows the
    // scale loads have landed: told by asm alone it re-waits for them, and with
    // them for the DMA just issued, in front of the tile's first MFMA.
    auto publish = [] {
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) only
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };
    if (n_tiles > 0) {
        stage_dma(0, 0);
        load_scales(0, ks, vs);
    }
    const int n_full = Lkv / KVB;  // mask-free tiles; the peeled tail follows them
    for (int tile = 0; tile < n_full; ++tile) {
        publish();
        uint32_t ks_n = 0, vs_n = 0;
        if (tile + 1 < n_tiles) {
            stage_dma((tile + 1) & 1, tile + 1);
            load_scales(tile + 1, ks_n, vs_n);
        }
        compute(std::false_type{}, tile * KVB);
        krd ^= BUF;
        vrd ^= BUF;
        ks = ks_n;
        vs = vs_n;
    }
    if (n_full < n_tiles) {
        publish();
        compute(std::true_type{}, n_full * KVB);
    }

    // ---- epilogue: O[q][d] = O^T / l, as the bf16 kernel stores it ----
    // A true division, once per element: with exact sums (integer-like V, p = 1
    // or 0) O is then the correctly rounded quotient, which the exact tests
    // hold it to; a reciprocal-multiply rounds twice.
    l_run = half_sum(l_run);
    const bool any = l_run > 0.f;
    const float l = any ? l_run * (1.f / 256.f) : 1.f;
    uint16_t* op = p.o + ((int64_t)b * p.Lq + (qvalid ? qrow : 0)) * (p.H * 64) + (int64_t)h * 64;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
        uint32_t ow[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
            ow[i] = pack2_b16<F16>(any ? ot[dt][2 * i] / l : 0.f, any ? ot[dt][2 * i + 1] / l : 0.f);
#pragma unroll
        for (int g = 0; g < 4; g += 2) {
            const auto rx = __builtin_amdgcn_permlane32_swap(ow[2 * g], ow[2 * g + 2], false, false);
            const auto ry =
                __builtin_amdgcn_permlane32_swap(ow[2 * g + 1], ow[2 * g + 3], false, false);
            const int d0 = dt * 32 + 8 * (g + hi);
            if (qvalid) *reinterpret_cast<uint4*>(op + d0) = uint4{rx[0], ry[0], rx[1], ry[1]};
        }
    }
}

// ---- fragment-layout probe: one wave, one scaled MFMA ------------------------------
template <int OA, int OB>
__global__ void mfma_probe_fp8_kernel(const int* __restrict__ a, const int* __restrict__ b,
                                      const int* __restrict__ sa, const int* __restrict__ sb,
                                      float* __restrict__ d) {
    const int lane = threadIdx.x;
    int8v af, bf;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        af[j] = a[lane * 8 + j];
        bf[j] = b[lane * 8 + j];
    }
    const float16v acc = mfma_f8<OA, OB>(af, bf, float16v{}, (uint32_t)sa[lane], (uint32_t)sb[lane]);
#pragma unroll
    for (int r = 0; r < 16; ++r) d[lane * 16 + r] = acc[r];
}

template <int OA>
void probe_opsel_b(int opsel_b, const int* a, const int* b, const int* sa, const int* sb, float* d,
                   hipStream_t stream) {
    switch (opsel_b) {
        case 0: mfma_probe_fp8_kernel<OA, 0><<<1, WAVE_SIZE, 0, stream>>>(a, b, sa, sb, d); break;
        case 1: mfma_probe_fp8_kernel<OA, 1><<<1, WAVE_SIZE, 0, stream>>>(a, b, sa, sb, d); break;
        case 2: mfma_probe_fp8_kernel<OA, 2><<<1, WAVE_SIZE, 0, stream>>>(a, b, sa, sb, d); break;
        default: mfma_probe_fp8_kernel<OA, 3><<<1, WAVE_SIZE, 0, stream>>>(a, b, sa, sb, d); break;
    }
}

}  // namespace

int64_t attn_fp8_num_tiles(int64_t lkv) { return (lkv + KVB - 1) / KVB; }

void launch_attn_quant_kv(const FlashAttnParams& p, uint8_t* ws, int dtype, hipStream_t stream) {
    const int64_t n_tiles = attn_fp8_num_tiles(p.NC * p.LC);
    if (n_tiles == 0 || p.B * p.H == 0) return;
    const dim3 grid((unsigned)n_tiles, (unsigned)(p.B * p.H));
    dispatch_f16(dtype, [&]<bool F16>(std::bool_constant<F16>) {
        attn_quant_kv_kernel<F16><<<grid, 256, 0, stream>>>(p, ws);
    });
}

void launch_flash_attention_fp8(const FlashAttnParams& p, const uint8_t* ws, int dtype,
                                hipStream_t stream) {
    if (p.Lq == 0 || p.B * p.H == 0) return;
    const int n_tiles = (int)attn_fp8_num_tiles(p.NC * p.LC);
    const dim3 grid((unsigned)((p.Lq + QBLK - 1) / QBLK), (unsigned)(p.B * p.H));
    dispatch_f16(dtype, [&]<bool F16>(std::bool_constant<F16>) {
        flash_attn_fp8_kernel<F16><<<grid, NW * WAVE_SIZE, 0, stream>>>(p, ws, n_tiles);
    });
}

void launch_mfma_probe_fp8(const int* a, const int* b, const int* scale_a, const int* scale_b,
                           int opsel_a, int opsel_b, float* d, hipStream_t stream) {
    switch (opsel_a) {
        case 0: probe_opsel_b<0>(opsel_b, a, b, scale_a, scale_b, d, stream); break;
        case 1: probe_opsel_b<1>(opsel_b, a, b, scale_a, scale_b, d, stream); break;
        case 2: probe_opsel_b<2>(opsel_b, a, b, scale_a, scale_b, d, stream); break;
        default: probe_opsel_b<3>(opsel_b, a, b, scale_a, scale_b, d, stream); break;
    }
}
