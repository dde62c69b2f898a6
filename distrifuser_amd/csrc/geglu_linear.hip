// Fused GEGLU projection, gfx950, bf16 or fp16 (K3/K9 of SURVEY §2.4a):
//   out[r][i] = round16( (x[r].W[i] + b[i]) * gelu_erf(x[r].W[inner+i] + b[inner+i]) )
// one 16-bit MFMA GEMM with the gate in its epilogue: the [rows, 2*inner]
// projection never exists in memory and is never rounded to 16 bits.
//
// Structure (the idioms of attention.hip and conv.hip):
// * SWAPPED operands: D[m = output i][n = token] = A[i][k] x B[k][token] via
//   mfma_f32_32x32x16, so a lane holds ONE token's outputs, 4 consecutive i
//   per register group; a permlane32_swap between the wave halves makes that
//   8 consecutive i = one 16 B store (the attention epilogue).
// * VALUE AND GATE IN ONE BLOCK: a block's weight tile is NT value rows plus
//   the NT gate rows of the same i range, and every wave accumulates both for
//   its own (token, i) sub-tile. The two accumulators have identical register
//   layouts, so a * gelu(g) is register to register.
// * Block = 4 waves, 128 tokens x 128 outputs (256 GEMM columns), K-step 64.
//   Wave (wm, wn) owns 64 tokens x 64 outputs: 2 token sub-tiles x 2 output
//   sub-tiles x {value, gate} = 8 MFMA tiles = 128 fp32 accumulators per
//   lane; per 16-k slice it reads 4 A and 2 B fragments for 8 MFMAs.
// * Weights are prepacked (ops.pack_geglu_weight) as the LDS image of their
//   A fragments: [column tile][k16 slice][vg*4 + sub][lane][8], so a K-step is
//   32 contiguous KiB that LDS-DMA (buffer_load ... lds, 1 KiB per wave
//   instruction) copies linearly, and an A fragment is one lane-linear
//   ds_read_b128. K and inner are zero-padded to whole tiles in the pack.
// * x rows are staged row-major, 128 B per row and K-step, the 16 B piece c of
//   row t at piece c ^ ((t >> 1) & 7). A B fragment is 8 consecutive k of one
//   token: one ds_read_b128, nothing transposed. Bank model (64 banks of 4 B,
//   16-lane groups {0-3, 12-15, 20-27}.. per b128 read): the 16 rows of a
//   group read the same piece; row parity picks the half of the 256 B bank
//   row and (t >> 1) & 7 takes 8 different values over each parity, so the
//   16 lanes touch 16 different 16 B windows: conflict-free. The staging
//   write has the 8 pieces of one row in 8 consecutive lanes (a whole 128 B
//   row per b128 write group). x goes through registers (loaded before the
//   MFMA phase, written after it) behind a buffer descriptor that ends with
//   the tile's last row: rows past the end and the k tail of the last K-step
//   read zero in hardware (a tail piece is sent out of range, so nothing of
//   the next row is ever multiplied by the zero padding of the weights).
// * Two LDS stages (2 x 48 KiB), one barrier per K-step: the barrier that
//   publishes step s also says every wave is done with step s-1, whose
//   buffer the DMA and the register writes of step s+1 then fill.
// * Grid: the XCD-aware decode of conv.hip. The column tiles of one row tile
//   take consecutive slots of one XCD, so they run together and the x tile is
//   fetched into that XCD's L2 once.

#include "dispatch.h"

namespace {

constexpr int GL_MT = 128;                       // tokens per block
constexpr int GL_NT = 128;                       // outputs per block (x2 GEMM columns)
constexpr int GL_KSTEP = 64;                     // k per LDS stage
constexpr int GL_NW = 4;                         // waves per block: 2 (tokens) x 2 (outputs)
constexpr int GL_W_BYTES = 2 * GL_NT * GL_KSTEP * 2;  // weight image of one K-step
constexpr int GL_X_BYTES = GL_MT * GL_KSTEP * 2;      // x image of one K-step
constexpr int GL_XLD = GL_X_BYTES / (GL_NW * WAVE_SIZE * 16);  // x pieces per thread and step

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <bool F16>
__global__ __launch_bounds__(GL_NW * WAVE_SIZE) void geglu_linear_kernel(GegluLinearParams p) {
    constexpr int NTHR = GL_NW * WAVE_SIZE;
    __shared__ __attribute__((aligned(16))) char lds[2 * GL_W_BYTES + 2 * GL_X_BYTES];
    char* const w_lds = lds;
    char* const x_lds = lds + 2 * GL_W_BYTES;

    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lo = lane & 31;
    const int hi = lane >> 5;
    const int wm = wave & 1;   // token half of the block tile
    const int wn = wave >> 1;  // output half

    // hardware sends dispatch D to XCD D % 8: the nct column tiles of one row
    // tile sit at consecutive D / 8 of the same D % 8
    const int D = blockIdx.x;
    const int ct = (D >> 3) % p.nct;
    const int64_t rt = (D & 7) + 8 * (int64_t)((D >> 3) / p.nct);
    const int64_t row0 = rt * GL_MT;
    if (row0 >= p.rows) return;
    const int nrows = (int)(p.rows - row0 < GL_MT ? p.rows - row0 : GL_MT);

    // ---- x staging: thread owns piece c = tid % 8 of rows tid / 8 + 32 * i.
    // The range ends with the last k of the tile's last row.
    const uint32_t x_bytes = (uint32_t)(((int64_t)(nrows - 1) * p.ld + p.K) * 2);
    const auto xrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint16_t*>(p.x + row0 * p.ld), 0, x_bytes, 0x00020000);
    const int xc = tid & 7;
    const int xr = tid >> 3;
    uint32_t xoff[GL_XLD];
#pragma unroll
    for (int i = 0; i < GL_XLD; ++i)
        xoff[i] = (uint32_t)(xr + 32 * i) * (uint32_t)(p.ld * 2) + xc * 16;
    // 32 rows change neither XOR term
    const int xwr = xr * (GL_KSTEP * 2) + ((xc ^ ((xr >> 1) & 7)) << 4);
    uint4 xreg[GL_XLD];
    auto load_x = [&](int ks) {
        // a piece at or beyond K (the last step of a K that is no multiple of
        // 64) is sent out of range: it reads zero
        const bool k_ok = ks * GL_KSTEP + xc * 8 < p.K;
#pragma unroll
        for (int i = 0; i < GL_XLD; ++i) {
            const uint32_t off = k_ok ? xoff[i] + (uint32_t)ks * (GL_KSTEP * 2) : x_bytes;
            xreg[i] = __builtin_bit_cast(
                uint4, __builtin_amdgcn_raw_buffer_load_b128(xrs, (int)off, 0, 0));
        }
    };
    auto write_x = [&](int buf) {
#pragma unroll
        for (int i = 0; i < GL_XLD; ++i)
            *reinterpret_cast<uint4*>(&x_lds[buf * GL_X_BYTES + xwr + i * 32 * (GL_KSTEP * 2)]) =
                xreg[i];
    };

    // ---- weight staging: the K-step's 32 KiB image, copied linearly by LDS-DMA
    // (buffer_load ... lds: wave-uniform LDS base in M0 + lane * 16). Thread
    // tid owns the 16 B slot tid of each 4 KiB pass. Written as assembly so
    // that the compiler keeps no count of these loads: it would wait for them
    // in front of the first fragment read, and the barrier below is what
    // publishes them.
    const uint64_t wa = reinterpret_cast<uint64_t>(p.wp + (int64_t)ct * p.nks * (GL_W_BYTES / 2));
    const u32x4 wrs{(uint32_t)wa, (uint32_t)(wa >> 32) & 0xFFFFu, (uint32_t)p.nks * GL_W_BYTES,
                    0x00020000u};
    const uint32_t wvoff = tid * 16;
    const uint32_t wdst = __builtin_amdgcn_readfirstlane(wave) * (WAVE_SIZE * 16);
    const uint32_t lds_base =
        (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)w_lds;
    auto stage_w = [&](int ks, int buf) {
        static_assert(GL_W_BYTES / (NTHR * 16) == 8);
        const uint32_t m0v = lds_base + wdst + buf * GL_W_BYTES;
        const uint32_t so0 = (uint32_t)ks * GL_W_BYTES;
        uint32_t keep, so;
#define GL_DMA "s_nop 0\n\tbuffer_load_dwordx4 %2, %3, %1 offen lds\n\t"
#define GL_NEXT "s_add_u32 m0, m0, 0x1000\n\ts_add_u32 %1, %1, 0x1000\n\t"
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %4\n\t"
            "s_mov_b32 %1, %5\n\t"
            GL_DMA GL_NEXT GL_DMA GL_NEXT GL_DMA GL_NEXT GL_DMA GL_NEXT
            GL_DMA GL_NEXT GL_DMA GL_NEXT GL_DMA GL_NEXT GL_DMA
            "s_mov_b32 m0, %0"
            : "=&s"(keep), "=&s"(so)
            : "v"(wvoff), "s"(wrs), "s"(m0v), "s"(so0)
            : "memory", "scc");
#undef GL_DMA
#undef GL_NEXT
    };
    // this wave's DMA and LDS writes retired, then the block barrier
    auto publish = [] { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); };

    // ---- fragment read addresses (the buffer offset is added per step)
    const int ard = (wn * 2 * WAVE_SIZE + lane) * 16;
    int xrd[GL_KSTEP / 16];
#pragma unroll
    for (int k16 = 0; k16 < GL_KSTEP / 16; ++k16)
        xrd[k16] = (wm * 64 + lo) * (GL_KSTEP * 2) + (((k16 * 2 + hi) ^ ((lo >> 1) & 7)) << 4);

    float16v acc[2][2][2] = {};  // [value / gate][output sub-tile][token sub-tile]
    auto compute = [&](int buf) {
        const char* wb = w_lds + buf * GL_W_BYTES + ard;
        const char* xb = x_lds + buf * GL_X_BYTES;
#pragma unroll
        for (int k16 = 0; k16 < GL_KSTEP / 16; ++k16) {
            short8 bfrag[2];
#pragma unroll
            for (int ts = 0; ts < 2; ++ts)
                bfrag[ts] = *reinterpret_cast<const short8*>(
                    xb + xrd[k16] + ts * 32 * (GL_KSTEP * 2));
#pragma unroll
            for (int vg = 0; vg < 2; ++vg) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const short8 afrag = *reinterpret_cast<const short8*>(
                        wb + ((k16 * 8 + vg * 4 + s) * WAVE_SIZE) * 16);
#pragma unroll
                    for (int ts = 0; ts < 2; ++ts)
                        acc[vg][s][ts] = mfma_32x32x16<F16>(afrag, bfrag[ts], acc[vg][s][ts]);
                }
            }
        }
    };

    load_x(0);
    stage_w(0, 0);
    write_x(0);
    for (int ks = 0; ks < p.nks; ++ks) {
        const int buf = ks & 1;
        publish();  // step ks visible; every wave done with step ks-1, buffer buf^1 free
        const bool more = ks + 1 < p.nks;
        if (more) {
            // x first: the compiler's own waits in front of these loads must
            // not find the DMA in flight
            load_x(ks + 1);
            stage_w(ks + 1, buf ^ 1);
        }
        compute(buf);
        if (more) write_x(buf ^ 1);
    }

    // ---- epilogue: fp32 bias, a * gelu(g), ONE rounding, 16 B stores.
    // Register group g of a lane is i = 8g + 4hi + 0..3 of the sub-tile; the
    // swap of groups g and g+1 between the halves leaves 8 consecutive i.
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int ibase = ct * GL_NT + (wn * 2 + s) * 32;
        float bv[4][4], bg[4][4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i0 = ibase + 8 * g + 4 * hi;
            uint2 rv{0, 0}, rg{0, 0};
            if (i0 < p.inner) {  // inner % 8 == 0: all four or none
                rv = *reinterpret_cast<const uint2*>(p.bias + i0);
                rg = *reinterpret_cast<const uint2*>(p.bias + p.inner + i0);
            }
            const uint32_t dv[2] = {rv.x, rv.y}, dg[2] = {rg.x, rg.y};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bv[g][e] = b16_to_f32<F16>((uint16_t)(dv[e >> 1] >> (16 * (e & 1))));
                bg[g][e] = b16_to_f32<F16>((uint16_t)(dg[e >> 1] >> (16 * (e & 1))));
            }
        }
#pragma unroll
        for (int ts = 0; ts < 2; ++ts) {
            const int64_t row = row0 + wm * 64 + ts * 32 + lo;
            const bool rvalid = row < p.rows;
            uint16_t* op = p.out + (rvalid ? row : 0) * p.inner;
            uint32_t ow[8];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a = acc[0][s][ts][4 * g + e] + bv[g][e];
                    const float gate = acc[1][s][ts][4 * g + e] + bg[g][e];
                    o[e] = a * geluf(gate);
                }
                // fp16: round to nearest even, beyond 65504 -> inf
                ow[2 * g] = pack2_b16<F16>(o[0], o[1]);
                ow[2 * g + 1] = pack2_b16<F16>(o[2], o[3]);
            }
#pragma unroll
            for (int g = 0; g < 4; g += 2) {
                const auto rx =
                    __builtin_amdgcn_permlane32_swap(ow[2 * g], ow[2 * g + 2], false, false);
                const auto ry =
                    __builtin_amdgcn_permlane32_swap(ow[2 * g + 1], ow[2 * g + 3], false, false);
                const int i0 = ibase + 8 * (g + hi);
                if (rvalid && i0 < p.inner)
                    *reinterpret_cast<uint4*>(op + i0) = uint4{rx[0], ry[0], rx[1], ry[1]};
            }
        }
    }
}

}  // namespace

int64_t geglu_linear_packed_numel(int K, int inner) {
    const int64_t nct = (inner + GL_NT - 1) / GL_NT;
    const int64_t nks = (K + GL_KSTEP - 1) / GL_KSTEP;
    return nct * nks * (GL_W_BYTES / 2);
}

void launch_geglu_linear(GegluLinearParams p, int dtype, hipStream_t stream) {
    if (p.rows <= 0 || p.inner <= 0) return;
    p.nct = (p.inner + GL_NT - 1) / GL_NT;
    p.nks = (p.K + GL_KSTEP - 1) / GL_KSTEP;
    const int64_t nrt = (p.rows + GL_MT - 1) / GL_MT;
    const unsigned blocks = (unsigned)(8 * p.nct * ((nrt + 7) / 8));
    dispatch_f16(dtype, [&]<bool F16>(std::bool_constant<F16>) {
        geglu_linear_kernel<F16><<<dim3(blocks), dim3(GL_NW * WAVE_SIZE), 0, stream>>>(p);
    });
}
