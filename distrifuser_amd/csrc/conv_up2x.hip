// 2x nearest upsample folded into the pad-1 3x3 conv that follows it, gfx950,
// bf16 or fp16, NCHW (K4/K5 of SURVEY §2.4a). The [B, Cin, 2H, 2W] tensor is
// never written: output pixel (2y+py, 2x+px) is a 2x2 conv on the INPUT grid
// with the parity's collapsed weights Wc[py][px][a][b] (ops.pack_upsample2x_
// conv3x3_weight adds the 3x3 taps that land on one input pixel), tap (a, b)
// reading input (y + a + py - 1, x + b + px - 1). 16 tap-GEMMs give four
// outputs where the two-op route spends 36.
//
// Design (the vocabulary of conv.hip, a different split of the work):
// * SWAPPED operands, D[cout 32][input pixel 32] = A[cout][cin 16] x B[cin][pixel]
//   via mfma_f32_32x32x16. A lane owns ONE input pixel; its four parities are
//   four accumulators with the same register layout, so the px = 0 and px = 1
//   results of that pixel pack to one dword in the lane, and a wave stores
//   32 consecutive dwords = 128 B runs of output row 2y+py.
// * Block = 8 waves, 8 input rows x 32 input px (16 x 64 outputs) x 64 couts.
//   Wave (wr, wc) owns the input-row PAIR 2wr, 2wr+1 and the 32-cout tile wc:
//   2 rows x 4 parities = 8 MFMA tiles = 128 fp32 accumulators per lane. The
//   pair is what pays: the two rows share their A fragments, and the 4 staged
//   rows x 3 column shifts they touch are 12 B fragments, so a 16-cin slice is
//   12 B reads + 16 A reads for 32 MFMAs, 0.875 LDS reads per MFMA (one row
//   per wave: 9 + 16 for 16, 1.56; conv.hip's narrow tile: 1.5).
// * The input tile with its one-pixel ring, 10 rows x 34 px x 16 cin, is
//   staged ONCE per cin slice, transposed to [row][px][cin] as in conv.hip
//   (128 B-coalesced b128 global reads behind a buffer descriptor, 8x8 DPP
//   transpose, one b128 LDS write per lane). Every tap of every parity is an
//   address offset (a + py - 1, b + px - 1) into that one image.
// * LDS image: a pixel is 32 B (16 cin), rows are unpadded (34 * 32 B); the
//   16 B half h (cin 8h..8h+7) of pixel xi sits at half h ^ ((xi >> 3) & 1).
//   Bank model (64 banks of 4 B; a ds_read_b128 is served per 16-lane group
//   {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, and the same + 32): a B
//   fragment read has lane (lo, hi) at pixel xi = lo + dx, half hi, i.e. 16 B
//   window 2 xi + (hi ^ bit 3 of xi) of the row, which mod 16 (the 256 B bank
//   row) is a bijection of xi mod 16. Both groups hold every residue of
//   lo mod 16 once, and so of xi mod 16 for each of the three shifts dx: 16
//   different windows, conflict-free. (Unswizzled, the 16 lanes of one hi
//   would share 8 even windows: 2-way. The row pitch, 68 windows, moves every
//   window of a read by the same amount.) The staging write (8 contiguous lanes
//   per b128 write group, 128 B bank row) has lanes at pixels {1..4, 9..12} or
//   {5..8, 13..16} + 8k of one half: windows mod 8 all different. A fragments
//   are lane-linear b128 reads of the packed image.
// * Weights are prepacked [4 parities][4 taps][KS][CT][64][8] in A-fragment
//   order (lane l: cout = ct*32 + (l&31), cin = ks*16 + (l>>5)*8 + j); the 32
//   fragments of a block and cin slice go to LDS by LDS-DMA, 1 KiB per wave
//   instruction, no registers.
// * Two LDS stages, one barrier per cin slice (conv.hip's pipeline): the
//   DMA and the global loads of slice t+1 are issued before the MFMAs of
//   slice t, the transposing LDS writes after them. LDS: 2 x (32 KiB weights
//   + 10.6 KiB input) = 85 KiB, one block of 8 waves per CU.
// * Grid: conv.hip's XCD-aware decode, so the cout blocks of one pixel tile
//   run together on one XCD and share the staged input in its L2.
// * Epilogue: bias in fp32, one rounding, 64 dword stores per lane. No
//   residual / bias2: no upsample call site has them.

#include "dispatch.h"

namespace {

constexpr int U_YB = 8;                  // input rows per block
constexpr int U_XB = 32;                 // input px per block
constexpr int U_NCT = 2;                 // 32-cout tiles per block
constexpr int U_NW = 8;                  // waves: 4 row pairs x 2 cout tiles
constexpr int U_CIN_T = 16;              // cins per staged slice
constexpr int U_YIN = U_YB + 2;          // staged rows
constexpr int U_XIN = U_XB + 2;          // staged px
constexpr int U_PIX_B = U_CIN_T * 2;     // bytes per staged pixel
constexpr int U_ROW_B = U_XIN * U_PIX_B;
constexpr int U_IN_SZ = U_YIN * U_ROW_B;
constexpr int U_NFRAG = 16 * U_NCT;      // weight fragments per slice
constexpr int U_W_SZ = U_NFRAG * WAVE_SIZE * 16;
constexpr int U_NXW = (U_XIN - 1 + 7) / 8;            // 8-px windows for xi >= 1
constexpr int U_NSLAB = U_YIN * (U_CIN_T / 8);        // (row, 8-cin group) per slice
constexpr int U_STRIP = (U_NSLAB + U_NW - 1) / U_NW;  // slabs per wave
constexpr uint32_t U_OOB = 0x7fffff00u;               // beyond every descriptor range

// byte offset of cin group cg (8 cins) of staged pixel (ry, xi)
__device__ __forceinline__ int up2x_lds_off(int ry, int xi, int cg) {
    return ry * U_ROW_B + xi * U_PIX_B + ((cg ^ ((xi >> 3) & 1)) << 4);
}

struct Up2xGrid {
    int nxb, nyb, npix, ncb;
    unsigned blocks;
};
__host__ __device__ __forceinline__ Up2xGrid up2x_grid(const ConvUp2xParams& p) {
    Up2xGrid g;
    g.nxb = (p.W + U_XB - 1) / U_XB;
    g.nyb = (p.H + U_YB - 1) / U_YB;
    g.npix = g.nxb * g.nyb * p.B;
    g.ncb = (p.CT + U_NCT - 1) / U_NCT;
    g.blocks = (unsigned)(8 * g.ncb * ((g.npix + 7) / 8));
    return g;
}

template <bool F16>
__global__ __launch_bounds__(U_NW * WAVE_SIZE) void conv_up2x_kernel(ConvUp2xParams p) {
    __shared__ __attribute__((aligned(16))) char in_lds[2 * U_IN_SZ];
    __shared__ __attribute__((aligned(16))) char w_lds[2 * U_W_SZ];

    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lo = lane & 31;
    const int hi = lane >> 5;
    const int wr = wave & 3;   // input rows 2wr, 2wr+1 of the tile
    const int wc = wave >> 2;  // cout tile of the block

    // hardware sends dispatch D to XCD D % 8: the ncb cout blocks of one pixel
    // tile sit at consecutive D / 8 of the same D % 8
    const Up2xGrid g = up2x_grid(p);
    const int D = blockIdx.x;
    const int cb = (D >> 3) % g.ncb;
    const int pp = (D & 7) + 8 * ((D >> 3) / g.ncb);
    if (pp >= g.npix) return;
    const int b = pp / (g.nxb * g.nyb);
    const int pt = pp % (g.nxb * g.nyb);
    const int xb0 = (pt % g.nxb) * U_XB;
    const int yb0 = (pt / g.nxb) * U_YB;

    const uint16_t* xin = p.x + (int64_t)b * p.x_sb;
    const uint16_t* top = p.top ? p.top + (int64_t)b * p.t_sb : nullptr;
    const uint16_t* bot = p.bot ? p.bot + (int64_t)b * p.b_sb : nullptr;

    // ---- input staging state, hoisted out of the cin loop. A wave stages slab
    // (ry, cg): 8 cins x 64 px, lane (gr, gw) loading the 8 px of window gw of
    // cin cg*8 + gr; after the transpose it owns px xi = 1 + gw*8 + gr, 8 cins.
    // The descriptor ends with the last row of the last channel, so channels
    // past Cin and windows past the view read zero in hardware.
    const int gr = (lane & 3) | ((lane & 8) >> 1);
    const int gw = ((lane >> 2) & 1) | (((lane >> 4) & 3) << 1);
    const auto desc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint16_t*>(xin), 0,
        (uint32_t)(((int64_t)(p.Cin - 1) * p.x_sc + (int64_t)p.H * p.W) * 2), 0x00020000);
    const uint32_t voff_inc = (uint32_t)(U_CIN_T * p.x_sc * 2);
    const int x0 = xb0 + gw * 8;                // image x of this lane's window
    const bool win_ok = gw < U_NXW && x0 < p.W;  // else: all zero
    const int rem = p.W - x0;                    // valid px of the window (may be > 8)
    uint32_t voff[U_STRIP];
    uint32_t interior_mask = 0, valid_mask = 0;
#pragma unroll
    for (int sit = 0; sit < U_STRIP; ++sit) {
        const int slab = sit * U_NW + wave;
        voff[sit] = U_OOB;
        if (slab >= U_NSLAB) continue;
        valid_mask |= 1u << sit;
        const int cg = slab & 1;
        const int y_in = yb0 - 1 + (slab >> 1);
        if (y_in < 0 || y_in >= p.H) continue;
        interior_mask |= 1u << sit;
        if (win_ok)
            voff[sit] = (uint32_t)(((int64_t)(cg * 8 + gr) * p.x_sc + (int64_t)y_in * p.W + x0) * 2);
    }

    auto stage_weights = [&](int cint, char* wb) {
#pragma unroll
        for (int it = 0; it < U_NFRAG / U_NW; ++it) {
            const int frag = it * U_NW + wave;  // (parity*4 + tap) * NCT + ct2
            const int ct = cb * U_NCT + (frag % U_NCT);
            char* ldst = wb + frag * (WAVE_SIZE * 16);
            if (ct < p.CT) {
                const uint16_t* src =
                    p.wp + ((((int64_t)(frag / U_NCT) * p.KS + cint) * p.CT + ct) * WAVE_SIZE + lane) * 8;
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) uint32_t*)src,
                    (__attribute__((address_space(3))) uint32_t*)ldst, 16, 0, 0);
            } else {
                *reinterpret_cast<uint4*>(ldst + lane * 16) = uint4{0, 0, 0, 0};
            }
        }
    };
    uint4 iregs[U_STRIP];
    auto load_input = [&]() {
#pragma unroll
        for (int sit = 0; sit < U_STRIP; ++sit) {
            iregs[sit] = uint4{0, 0, 0, 0};
            if (!p.vec || !((interior_mask >> sit) & 1)) continue;
            iregs[sit] = __builtin_bit_cast(
                uint4, __builtin_amdgcn_raw_buffer_load_b128(desc, (int)voff[sit], 0, 0));
            if (win_ok) voff[sit] += voff_inc;
        }
    };
    // 8 px of one row through guarded 2-byte loads: halo rows, and every row
    // of an input whose rows are not 16 B aligned
    auto load_row_scalar = [&](const uint16_t* rp) {
        uint16_t vals[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) vals[j] = (j < rem) ? rp[x0 + j] : (uint16_t)0;
        return *reinterpret_cast<const uint4*>(vals);
    };
    auto write_input = [&](int cint, char* inb) {
        const int cin0 = cint * U_CIN_T;
#pragma unroll
        for (int sit = 0; sit < U_STRIP; ++sit) {
            if (!((valid_mask >> sit) & 1)) continue;
            const int slab = sit * U_NW + wave;
            const int cg = slab & 1;
            const int ry = slab >> 1;
            const int y_in = yb0 - 1 + ry;
            const int cin = cin0 + cg * 8 + gr;
            uint4 raw = iregs[sit];
            if ((interior_mask >> sit) & 1) {
                // vec: W % 8 == 0, so a window is inside the row or beyond it
                if (!p.vec && win_ok && cin < p.Cin)
                    raw = load_row_scalar(xin + (int64_t)cin * p.x_sc + (int64_t)y_in * p.W);
            } else if (win_ok && cin < p.Cin) {
                if (y_in == -1 && top)
                    raw = load_row_scalar(top + (int64_t)cin * p.t_sc);
                else if (y_in == p.H && bot)
                    raw = load_row_scalar(bot + (int64_t)cin * p.b_sc);
            }
            const uint4 tr = transpose8x8_b16(raw, lane);
            const int xi = 1 + gw * 8 + gr;  // the lane now owns px xi, cins cg*8..+7
            if (xi < U_XIN) *reinterpret_cast<uint4*>(&inb[up2x_lds_off(ry, xi, cg)]) = tr;
        }
        // left ring column xi = 0 (x = xb0 - 1): 10 rows x 16 cins, scalar
        if (tid < U_YIN * U_CIN_T) {
            const int ci = tid % U_CIN_T;
            const int ry = tid / U_CIN_T;
            const int y_in = yb0 - 1 + ry;
            const int cin = cin0 + ci;
            uint16_t val = 0;
            if (xb0 > 0 && cin < p.Cin) {
                if (y_in >= 0 && y_in < p.H)
                    val = xin[(int64_t)cin * p.x_sc + (int64_t)y_in * p.W + xb0 - 1];
                else if (y_in == -1 && top)
                    val = top[(int64_t)cin * p.t_sc + xb0 - 1];
                else if (y_in == p.H && bot)
                    val = bot[(int64_t)cin * p.b_sc + xb0 - 1];
            }
            *reinterpret_cast<uint16_t*>(&inb[up2x_lds_off(ry, 0, ci >> 3) + (ci & 7) * 2]) = val;
        }
    };

    // acc[j][py*2 + px]: input row 2wr + j of the tile, output parity (py, px)
    float16v acc[2][4] = {};
    auto compute_tile = [&](const char* inb, const char* wb) {
        // staged rows 2wr .. 2wr+3 (input rows y-1 .. y+2 of the pair) x 3 shifts
        short8 bf[4][3];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx)
                bf[r][dx] = *reinterpret_cast<const short8*>(
                    &inb[up2x_lds_off(2 * wr + r, lo + dx, hi)]);
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int px = 0; px < 2; ++px)
#pragma unroll
                    for (int bb = 0; bb < 2; ++bb) {
                        const int frag = ((py * 2 + px) * 4 + a * 2 + bb) * U_NCT + wc;
                        const short8 af = *reinterpret_cast<const short8*>(
                            &wb[(frag * WAVE_SIZE + lane) * 16]);
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            acc[j][py * 2 + px] = mfma_32x32x16<F16>(
                                af, bf[j + a + py][bb + px], acc[j][py * 2 + px]);
                    }
    };

    const int n_cin_tiles = p.KS;  // KS 16-cin slices, zero padded in the pack
    stage_weights(0, w_lds);
    load_input();
    write_input(0, in_lds);
    for (int cint = 0; cint < n_cin_tiles; ++cint) {
        const int cur = cint & 1;
        __syncthreads();  // slice cint visible; the other stage is free
        const bool more = cint + 1 < n_cin_tiles;
        if (more) {
            stage_weights(cint + 1, w_lds + (cur ^ 1) * U_W_SZ);
            load_input();
        }
        compute_tile(in_lds + cur * U_IN_SZ, w_lds + cur * U_W_SZ);
        if (more) write_input(cint + 1, in_lds + (cur ^ 1) * U_IN_SZ);
    }

    // ---- epilogue: o[b][cout][2y+py][2x .. 2x+1] = round(acc + bias), one dword
    const int x = xb0 + lo;
    const int ct = cb * U_NCT + wc;
    if (x >= p.W || ct >= p.CT) return;
    const int64_t plane = (int64_t)4 * p.H * p.W;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int y = yb0 + 2 * wr + j;
        if (y >= p.H) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cout = ct * 32 + mfma32_row(r, hi);
            if (cout >= p.Cout) continue;
            const float bv = p.bias ? b16_to_f32<F16>(p.bias[cout]) : 0.f;
            uint16_t* orow = p.o + ((int64_t)b * p.Cout + cout) * plane +
                             (int64_t)(2 * y) * (2 * p.W) + 2 * x;
#pragma unroll
            for (int py = 0; py < 2; ++py)
                *reinterpret_cast<uint32_t*>(orow + py * 2 * p.W) =
                    pack2_b16<F16>(acc[j][py * 2][r] + bv, acc[j][py * 2 + 1][r] + bv);
        }
    }
}

}  // namespace

void launch_conv_up2x(const ConvUp2xParams& p, int dtype, hipStream_t stream) {
    dispatch_f16(dtype, [&]<bool F16>(std::bool_constant<F16>) {
        conv_up2x_kernel<F16>
            <<<dim3(up2x_grid(p).blocks), dim3(U_NW * WAVE_SIZE), 0, stream>>>(p);
    });
}
