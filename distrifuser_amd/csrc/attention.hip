// Flash-attention forward, gfx950, bf16 or fp16, head_dim 64 (K1/K2/K8 of SURVEY
// §2.4a): rectangular local-query x global-(stale)-KV attention.
//
// Structure (cdna_hip_programming.md §B "8-warp 32x32 ladder"; evolution and
// per-step measurements in profiles/attention_ladder_r01.md and
// profiles/attention_r03_notes.md):
// * 8-wave workgroup per (batch, head, 256-row Q tile); each wave owns 32 Q
//   rows held in registers (4 k-slice A/B fragments). Q-block size governs
//   KV re-read traffic (each KV tile is re-read Lq/QBLK times).
// * KV streamed in 128-token LDS tiles shared by the waves. K and V are
//   staged the same way: b128 global loads into a row-major [t][d] image,
//   zero-filled beyond Dh and beyond Lkv. K rows are padded by 8 B (XOR-
//   swizzled instead where the tile is filled by LDS-DMA, below); V rows
//   are unpadded with a 64 B-granular XOR (v_swz) that keeps the transposed
//   reads conflict-free.
// * Full 128-token tiles run mask-free; one peeled tail tile handles
//   Lkv % 128 (mask-free when the remainder is 64, per-element masked
//   otherwise).
// * SWAPPED QK^T: S^T = K_tile x Q^T via mfma_f32_32x32x16_bf16, so each
//   lane holds 16 score rows of ONE q column (q = lane&31) — the online-
//   softmax max/sum are 15 in-register ops + ONE permlane32_swap with the
//   partner half, instead of 30+ cross-lane shuffles per tile (guide
//   common-mistake #6 / §B "swapped QK^T").
// * P stays in registers: v_cvt_pk_bf16_f32 packs + 4 permlane32_swap per
//   32-token sub-tile build the PV B-fragments directly (guide T12), no P LDS
//   round-trip and no half select.
// * PV is also swapped: O^T = V^T x P^T accumulates in 2x16 registers per
//   lane; the V^T A-fragments come from the row-major V image through
//   ds_read_b64_tr_b16 (guide T10), two per fragment.
// * stale-KV chunking: KV tokens come from NC flat-comm-buffer chunks of LC
//   tokens (k_sc/v_sc strides) — the displaced-patch KV is consumed in place
//   with zero torch.cat. The (chunk, token-in-chunk)
//   position of the tile being staged is a wave-uniform cursor advanced per
//   tile, together with a K and a V pointer at that token. A full tile that
//   lies inside one chunk (a uniform compare) loads through a raw buffer
//   descriptor seated at those pointers plus a lane offset computed once
//   before the loop: no per-lane multiply, 64-bit arithmetic or exec-mask
//   branch (head dims whose staging pass covers whole rows: DPAD 64, 128).
//   Any other tile — one that straddles chunk boundaries, the tail, the
//   other head dims — has every token row resolve its own chunk from the
//   cursor; the tile loop holds no division either way.
// * Staging, head_dim 64 with all columns real (the SDXL kernels): LDS-DMA
//   into TWO KV buffers, ONE barrier per tile. A full tile inside one chunk is
//   fetched by four buffer_load_dwordx4 ... lds per wave (1 KiB each, lane-
//   linear in LDS) from the tile cursor into the buffer the previous tile was
//   read from: no staging registers, no ds_write. Per tile: vmcnt(0) for the
//   wave's own DMA, s_barrier (tile t visible, every wave done with tile
//   t-1), issue tile t+1, compute tile t. The LDS image is made on the source
//   side: each lane fetches the 16 B column whose swizzled place is its
//   linear slot. K rows are unpadded 128 B under a 16 B-window XOR
//   ((t >> 1) & 7) and read with one ds_read_b128 per fragment; V keeps
//   v_swz. A tile that straddles chunks and the tail go through registers
//   after the compute (load, ds_write into the other buffer) and are
//   published by the same barrier, so the two kinds alternate freely.
//   (profiles/attention_dma_notes.md)
// * SPLIT staging (guide T14), every other instantiation: one KV buffer; the
//   next tile's global loads are issued into
//   registers before the current tile's compute and written to LDS after the
//   barrier that ends it; the barriers are raw s_barrier + lgkmcnt-only
//   waits, so the loads stay in flight across them.
// * LSE / split-KV mode (template flag; the plain instantiations are
//   untouched by it): grid.z blocks share a Q block, each over a tile-aligned
//   slice of the KV range, and write a normalised fp32 partial plus the
//   slice's log-sum-exp; merge_attn_kernel combines them. Fills the GPU when
//   Lq is short against Lkv (profiles/attention_splitkv_notes.md).
//
// Fragment maps (verified on MI355X by tests/test_ops_gpu.py probes):
//   16x16x32: A[row=l&15][k=(l>>4)*8+j]  B[k][col=l&15]  D[row=(l>>4)*4+r][col=l&15]
//   32x32x16: A[row=l&31][k=(l>>5)*8+j]  B[k][col=l&31]
//             D[row=(r&3)+8*(r>>2)+4*(l>>5)][col=l&31]
//   ds_read_b64_tr_b16, per 16-lane group: lane 4q+p supplies the address of
//   block row q, columns 4p..4p+3; lane i receives column i, row q in
//   element q.

#include "dispatch.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int QW = 32;     // q rows per wave
constexpr int KVB = 128;   // kv tokens per LDS tile
// split staging (issue-early / write-late) measured +1 % at L=57.6k and
// +5-7 % on the chunked shapes against loading after the barrier; the
// register-staged instantiations have no other mode.
// waves per block is a template parameter: bigger Q blocks amortize the KV
// stream (each KV tile is re-read Lq/QBLK times), smaller blocks keep small
// Lq shapes filled. Measured: 4w->8w at L=57.6k was +53% (439->673 TF).
// DPAD (head_dim padded to a multiple of 32) is a template parameter and
// covers the SD-family head dims (SDXL/SD2: 64; SD1.5: 40->64, 80->96,
// 160). The real head_dim rides in FlashAttnParams.Dh; padding lanes carry
// zeros (exact for QK^T scores and O columns < Dh).

typedef short short4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) short4v lds_short4v;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// byte address of a __shared__ object inside the block's LDS
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}

template <int DPAD>
__device__ __forceinline__ int v_swz(int t) {
    // One tr read takes, per 32-lane half, rows 4n..4n+3 of a 64 B column
    // window. Conflict-free needs those four 64 B pieces in four different
    // quarters of the 256 B bank row (guide §2). Rows of 192/320 B already
    // step by 64 B (mod 256); 128 B rows need rows {4n,4n+1} and {4n+2,4n+3}
    // told apart, 256 B rows need all four.
    if constexpr (DPAD % 128 == 0)
        return (t & 3) << 6;
    else if constexpr (DPAD % 64 == 0)
        return ((t >> 1) & 1) << 6;
    else
        return 0;
}

__device__ __forceinline__ uint32_t cvt_pk_bf16(float a, float b) {
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// the fp16 twin: one instruction, round to nearest even, overflow to inf
__device__ __forceinline__ uint32_t cvt_pk_f16(float a, float b) {
    uint32_t r;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ void lds_barrier() {
    // raw barrier with an LDS-only wait: unlike __syncthreads() it leaves
    // outstanding global loads in flight (guide §5 "Pipelining across
    // barriers")
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// lanes l and l^32 both end up with op(own, partner): one permlane32_swap of
// a value with itself puts the lower half's value in r[0] and the upper
// half's in r[1]. (The elements are copied to scalars first:
// __builtin_bit_cast on r[1] itself reads element 0.)
__device__ __forceinline__ float half_max(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    const uint32_t a = r[0], b = r[1];
    // plain v_max_f32: fmaxf would first canonicalise both swap results
    // (two v_max_f32 x, x, x), and neither can be a NaN here
    float m;
    asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(a), "v"(b));
    return m;
}
__device__ __forceinline__ float half_sum(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    const uint32_t a = r[0], b = r[1];
    return __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b);
}

// head_dim 64 is held to 128 registers: two 8-wave blocks per CU
// DFULL: head_dim == DPAD, no 16 B column is padding
// LSE: the block also emits the softmax log-sum-exp of its rows, and
// blockIdx.z selects one of gridDim.z tile-aligned slices of the KV range
// (split-KV): with p.o_part set it writes its normalised partial output as
// fp32 for merge_attn_kernel, otherwise (one split) bf16 O as the plain mode.
// F16: q/k/v/o are IEEE fp16 instead of bf16 — the two MFMAs, the P pack and
// the output conversion change type; scores, max, sum, LSE and o_part stay
// fp32 either way.
template <int NW, int DPAD, bool DFULL, bool LSE, bool F16>
__global__ __launch_bounds__(NW * WAVE_SIZE)
__attribute__((amdgpu_waves_per_eu(DPAD == 64 ? 4 : 2))) void flash_attn_kernel(
    std::conditional_t<LSE, FlashAttnLseParams, FlashAttnParams> p, bool off32) {
    constexpr int NT = NW * WAVE_SIZE;
    constexpr int QBLK = QW * NW;
    // K rows padded by 8 B: row stride DPAD*2+8 gives gcd(stride/4, 32) = 2,
    // so the 32-consecutive-row column reads are 2-way (free) instead of the
    // 4-way floor of XOR-swizzled 128 B rows — same trick as the conv
    // kernel's staged tile (profiles/conv_ladder_r02.md v5). Reads/writes
    // are b64 pairs (rows are 8 B- but not 16 B-aligned).
    //
    // DMA instantiations (head_dim 64, all columns real) fill the tile by
    // LDS-DMA instead, one wave-instruction = 1 KiB = eight rows written
    // lane-linearly, so their K rows are unpadded 128 B rows under a
    // 16 B-window XOR (k_swz) applied on the SOURCE side, read back with one
    // ds_read_b128 per fragment, and both images exist twice.
    constexpr bool DMA = DFULL && DPAD == 64;
    constexpr int K_ROW = DMA ? DPAD * 2 : DPAD * 2 + 8;  // K LDS row bytes [t][d]
    constexpr int V_ROW = DPAD * 2;         // V LDS row bytes [t][d], v_swz'd
    constexpr int K_BYTES = KVB * K_ROW;    // one K image
    constexpr int V_BYTES = KVB * V_ROW;    // one V image
    constexpr int NBUF = DMA ? 2 : 1;
    constexpr int KS = DPAD / 16;           // QK^T k-slices
    constexpr int DT = DPAD / 32;           // PV / O^T d-tiles
    constexpr int KCOLS = DPAD / 8;         // 16 B pieces per K/V row
    constexpr int NLD = KVB * KCOLS / NT;   // b128 loads per thread per tile, K and V each
    static_assert(KVB * KCOLS % NT == 0);
    __shared__ __attribute__((aligned(16))) char k_lds[NBUF * K_BYTES];
    __shared__ __attribute__((aligned(16))) char v_lds[NBUF * V_BYTES];

    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lo = lane & 31;   // q column of this lane
    const int hi = lane >> 5;   // partner-half index

    const int bh = blockIdx.y;
    const int b = bh / p.H;
    const int h = bh % p.H;
    const int64_t q0 = (int64_t)blockIdx.x * QBLK;

    const int LC = (int)p.LC;
    const int Lkv = (int)(p.NC * p.LC);
    const uint16_t* qbase = p.q + b * p.q_sb + h * p.q_sh;
    const uint16_t* kbase = p.k + b * p.k_sb + h * p.k_sh;
    const uint16_t* vbase = p.v + b * p.v_sb + h * p.v_sh;

    // ---- Q fragments: qf[ks] = Q[q = q0 + wave*32 + lo][d = ks*16 + hi*8 ..]
    // (8-element chunks beyond Dh are zero — Dh % 8 == 0 host-checked) ----
    short8 qf[KS];
    const int64_t qrow = q0 + wave * QW + lo;
    const bool qvalid = qrow < p.Lq;
    {
        const uint16_t* qp = qbase + (qvalid ? qrow : (p.Lq - 1)) * p.q_sl;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int d0 = ks * 16 + hi * 8;
            if (DFULL || d0 + 8 <= p.Dh)
                qf[ks] = *reinterpret_cast<const short8*>(qp + d0);
            else
                qf[ks] = short8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }

    // ---- V^T A-fragment read addresses: the tr read of 16-lane group g
    // takes V rows t = tb + hi*8 + rr*4 + q (q = 0..3), columns
    // d = dt*32 + (g&1)*16 + 0..15, so lane i of the group supplies the
    // address of row q = i>>2, columns (g&1)*16 + (i&3)*4 .. +3 and receives
    // d = dt*32 + (lane&31) — the MFMA A row. tb is a multiple of 16, so
    // v_swz(t) depends on q alone and everything but this per-lane base is
    // an immediate offset. ----
    int vrd[DT];
    {
        const int i = lane & 15;
        const int q = i >> 2;
        const int col_b = ((lane >> 4) & 1) * 32 + (i & 3) * 8;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            vrd[dt] = (hi * 8 + q) * V_ROW + ((dt * 64 + col_b) ^ v_swz<DPAD>(q));
    }

    // ---- DMA K image: 16 B window w of row t sits at window w ^ k_swz(t).
    // Even and odd rows fall in the two halves of the 256 B bank row and
    // (t >> 1) & 7 spreads the 16 rows of a ds_read_b128 lane group over the 8
    // windows of each half: conflict-free. A sub-tile step is 32 rows, which
    // leaves k_swz alone, so the fragment addresses are these per-lane bases
    // plus immediates. krd/vrd also carry the offset of the buffer being read
    // and flip with it after every tile. ----
    auto k_swz = [](int t) { return (t >> 1) & 7; };
    int krd[DMA ? KS : 1];
    if constexpr (DMA) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) krd[ks] = lo * K_ROW + (((ks * 2 + hi) ^ k_swz(lo)) << 4);
    }

    // ---- staging: thread (t-row, 16 B column) moves one b128 piece of K and
    // one of V per pass. cur_chunk/cur_tin locate the first token of the tile
    // being loaded and kcur/vcur point at it; all four are wave-uniform and
    // advance monotonically, one tile at a time. ----
    int cur_chunk = 0, cur_tin = 0;
    const char* kcur = reinterpret_cast<const char*>(kbase);
    const char* vcur = reinterpret_cast<const char*>(vbase);
    // Split s of S owns tiles [s*T/S, (s+1)*T/S) of the T = ceil(Lkv/KVB)
    // tiles: tile-aligned, non-empty for S <= T (host-clamped), and only the
    // last split reaches the peeled tail. The cursor is seated at the split's
    // first token, which may lie mid-chunk: the one division of the kernel.
    int tile_lo = 0, tile_hi = 0;
    if constexpr (LSE) {
        const int n_tiles = (Lkv + KVB - 1) / KVB;
        const int n_splits = (int)gridDim.z, split = (int)blockIdx.z;
        tile_lo = (int)((int64_t)split * n_tiles / n_splits);
        tile_hi = (int)((int64_t)(split + 1) * n_tiles / n_splits);
        if (tile_lo > 0) {
            const int tok = tile_lo * KVB;
            cur_chunk = tok / LC;
            cur_tin = tok - cur_chunk * LC;
            kcur = reinterpret_cast<const char*>(kbase + cur_chunk * p.k_sc + cur_tin * p.k_sl);
            vcur = reinterpret_cast<const char*>(vbase + cur_chunk * p.v_sc + cur_tin * p.v_sl);
        }
    }
    uint4 kreg[NLD], vreg[NLD];
    // piece i of this thread: linear index tid + i*NT over [KVB][KCOLS]. Where
    // a pass covers whole rows the passes differ by a constant row step, which
    // keeps every LDS write address one base plus an immediate.
    constexpr bool ROWPASS = NT % KCOLS == 0;
    auto stage_row = [&](int i) {
        if constexpr (ROWPASS)
            return tid / KCOLS + i * (NT / KCOLS);
        else
            return (tid + i * NT) / KCOLS;
    };
    auto stage_col = [&](int i) {
        if constexpr (ROWPASS)
            return tid % KCOLS;
        else
            return (tid + i * NT) % KCOLS;
    };
    auto stage_d_ok = [&](int i) { return DFULL || stage_col(i) * 8 + 8 <= p.Dh; };
    // Byte offset of this thread's first piece from the tile's first token,
    // fixed for the whole kernel (32-bit: the host passes off32 only when a
    // tile's span fits); the later pieces add the uniform k_pass/v_pass. Only
    // whole-row passes (DPAD 64 and 128) have that form: the others would
    // hold NLD lane offsets per tensor, which DPAD 160 has no registers for.
    //
    // DMA instantiations: thread tid owns the linear 16 B slot tid + i*NT of
    // each image — where its wave's LDS-DMA puts lane data, and where the
    // register path writes — and fetches the source column whose swizzled
    // place that slot is. A pass is 64 rows, which changes neither XOR, so the
    // source column is the same for every pass.
    auto stage_kcol = [&](int i) {
        return DMA ? stage_col(i) ^ k_swz(stage_row(i)) : stage_col(i);
    };
    auto stage_vcol = [&](int i) {
        return DMA ? stage_col(i) ^ (v_swz<DPAD>(stage_row(i)) >> 4) : stage_col(i);
    };
    const uint32_t koff = (uint32_t)stage_row(0) * ((uint32_t)p.k_sl * 2) + stage_kcol(0) * 16;
    const uint32_t voff = (uint32_t)stage_row(0) * ((uint32_t)p.v_sl * 2) + stage_vcol(0) * 16;
    const int k_pass = (NT / KCOLS) * (int)p.k_sl * 2;
    const int v_pass = (NT / KCOLS) * (int)p.v_sl * 2;
    // raw buffer descriptor at the (uniform) tile cursor: the load is base in
    // SGPRs + 32-bit lane offset + scalar pass offset, no 64-bit lane
    // arithmetic. No range to check against: off32 bounds every offset.
    auto tile_rsrc = [](const char* cur) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(cur), 0, 0xFFFFFFFFu,
                                                 0x00020000);
    };
    // the cursor moves on by one tile
    auto advance_cursor = [&]() {
        cur_tin += KVB;
        kcur += KVB * p.k_sl * 2;
        vcur += KVB * p.v_sl * 2;
        if (cur_tin >= LC) {  // chunk crossing: re-seat the cursor
            do {
                cur_tin -= LC;
                ++cur_chunk;
            } while (cur_tin >= LC);
            kcur = reinterpret_cast<const char*>(kbase + cur_chunk * p.k_sc + cur_tin * p.k_sl);
            vcur = reinterpret_cast<const char*>(vbase + cur_chunk * p.v_sc + cur_tin * p.v_sl);
        }
    };
    // the (full) tile at the cursor lies inside one chunk
    auto in_chunk = [&](bool full) {
        return ROWPASS && full && off32 && cur_tin + KVB <= LC;
    };
    // `full`: every token of the tile is below Lkv (all tiles but the tail).
    // In a DMA instantiation the in-chunk tiles go through stage_dma instead.
    auto stage_load = [&](int t0, bool full) {
        if (!DMA && in_chunk(full)) {
            // The tile lies inside one chunk: uniform cursor + fixed lane
            // offset, and registers about to be overwritten are not zeroed.
            const auto krs = tile_rsrc(kcur);
            const auto vrs = tile_rsrc(vcur);
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                if constexpr (!DFULL) {
                    kreg[i] = uint4{0, 0, 0, 0};
                    vreg[i] = uint4{0, 0, 0, 0};
                }
                if (stage_d_ok(i)) {
                    kreg[i] = __builtin_bit_cast(
                        uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                   krs, (int)koff, i * k_pass, 0));
                    vreg[i] = __builtin_bit_cast(
                        uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                   vrs, (int)voff, i * v_pass, 0));
                }
            }
        } else {
            // A tile that straddles chunks (many of them when LC < KVB), the
            // tail, or a tensor too large for 32-bit offsets: every row
            // resolves its own chunk from the cursor.
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int t_local = stage_row(i);
                int tin = cur_tin + t_local;
                int ch = cur_chunk;
                while (tin >= LC) {
                    tin -= LC;
                    ++ch;
                }
                kreg[i] = uint4{0, 0, 0, 0};
                vreg[i] = uint4{0, 0, 0, 0};
                if (stage_d_ok(i) && t0 + t_local < Lkv) {
                    kreg[i] = *reinterpret_cast<const uint4*>(
                        kbase + ch * p.k_sc + tin * p.k_sl + stage_kcol(i) * 8);
                    vreg[i] = *reinterpret_cast<const uint4*>(
                        vbase + ch * p.v_sc + tin * p.v_sl + stage_vcol(i) * 8);
                }
            }
        }
        advance_cursor();
    };
    // LDS-DMA of the in-chunk tile at the cursor into buffer wbuf: per wave
    // and pass one 1 KiB piece of K and one of V, no register in between. The
    // wave's piece of pass i is rows i*64 + wave*8 .. +7, the linear slots of
    // its lanes; the descriptor, the lane offset and the pass step are those
    // of the register path.
    //
    // The four loads are one asm statement: through the builtin the compiler
    // counts an LDS-DMA as a store to LDS that any later ds_read may alias and
    // puts vmcnt(3..0) in front of the first QK^T reads of the tile being
    // computed, which drains the prefetch on the spot. Unseen by its counting
    // they stay in flight across the compute; the vmcnt(0) before the next
    // barrier retires them, and its own vmcnt waits can only come out stricter
    // than needed (loads return in order). M0, the LDS destination of the
    // wave-instruction, is the compiler's: saved and put back.
    auto stage_dma = [&](int wbuf) {
        static_assert(!DMA || NLD == 2);
        auto words = [](const char* cur) {
            const uint64_t a = reinterpret_cast<uint64_t>(cur);
            return u32x4{(uint32_t)a, (uint32_t)(a >> 32) & 0xFFFFu, 0xFFFFFFFFu, 0x00020000u};
        };
        const u32x4 krs = words(kcur);
        const u32x4 vrs = words(vcur);
        const uint32_t piece = __builtin_amdgcn_readfirstlane(wave) * (WAVE_SIZE * 16);
        const uint32_t kd0 = lds_addr(&k_lds[wbuf * K_BYTES]) + piece;
        const uint32_t vd0 = lds_addr(&v_lds[wbuf * V_BYTES]) + piece;
        const uint32_t kd1 = kd0 + NT * 16, vd1 = vd0 + NT * 16;
        uint32_t keep;
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %5\n\ts_nop 0\n\t"
            "buffer_load_dwordx4 %1, %3, 0 offen lds\n\t"
            "s_mov_b32 m0, %6\n\ts_nop 0\n\t"
            "buffer_load_dwordx4 %2, %4, 0 offen lds\n\t"
            "s_mov_b32 m0, %7\n\ts_nop 0\n\t"
            "buffer_load_dwordx4 %1, %3, %9 offen lds\n\t"
            "s_mov_b32 m0, %8\n\ts_nop 0\n\t"
            "buffer_load_dwordx4 %2, %4, %10 offen lds\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(koff), "v"(voff), "s"(krs), "s"(vrs), "s"(kd0), "s"(vd0), "s"(kd1), "s"(vd1),
              "s"(k_pass), "s"(v_pass)
            : "memory");
        advance_cursor();
    };
    // wbuf: the buffer written (DMA instantiations; the others have one)
    auto stage_write = [&](int wbuf) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            if constexpr (DMA) {
                const int slot = (tid + i * NT) * 16;
                *reinterpret_cast<uint4*>(&k_lds[wbuf * K_BYTES + slot]) = kreg[i];
                *reinterpret_cast<uint4*>(&v_lds[wbuf * V_BYTES + slot]) = vreg[i];
            } else {
                const int t_local = stage_row(i);
                const int d8 = stage_col(i);
                char* kdst = &k_lds[t_local * K_ROW + d8 * 16];
                *reinterpret_cast<uint2*>(kdst) = uint2{kreg[i].x, kreg[i].y};
                *reinterpret_cast<uint2*>(kdst + 8) = uint2{kreg[i].z, kreg[i].w};
                *reinterpret_cast<uint4*>(
                    &v_lds[t_local * V_ROW + ((d8 * 16) ^ v_swz<DPAD>(t_local))]) = vreg[i];
            }
        }
    };

    // Online softmax bookkeeping (exp2 domain, guide §B):
    //   m_raw   running max of RAW scores (max commutes with the positive
    //           scale, so per-element work is p = exp2(fma(s, scale2, -msc))
    //           — ONE v_fma + ONE v_exp per score element)
    //   msc     m_raw * scale2 (refreshed only when m_raw moves)
    //   defer-max (guide T13): skip the O/l rescale while the tile max stays
    //   within DEFER_THR (log2 units) of the running max. The decision sits
    //   before the exponentiation of the sub-tile it covers, and the previous
    //   sub-tile's PV is already issued — nothing pending at the old max.
    float m_raw = -1e30f;
    float msc = -1e30f;
    float l_run = 0.f;
    float16v ot[DT] = {};  // O^T tiles: [dt] -> rows d = dt*32 + crow(r,hi), col q=lo
    const float scale2 = p.scale * 1.44269504088896340736f;
    const float defer_raw = 11.0f / scale2;

    // T15 att[2] double-pipeline (guide): while subtile st's softmax/PV
    // runs on the VALU, subtile st+1's QK^T fills the OTHER score tile on
    // the MFMA pipe (separate pipes -> free overlap). Static two-state
    // ping-pong via full unroll (rule #20: no dynamic indexing).
    auto qk_tile = [&](int st) {
        float16v s = {};
        __builtin_amdgcn_s_setprio(1);  // favor the MFMA wave (guide T5)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            short8 kfrag;
            if constexpr (DMA) {
                // one b128 read from the swizzled 128 B rows
                kfrag = *reinterpret_cast<const short8*>(&k_lds[krd[ks] + st * 32 * K_ROW]);
            } else {
                const int t = st * 32 + lo;
                // lds_frag_b64x2 spelled out: through the helper the DPAD-64
                // plain kernels schedule their staging writes differently
                const char* ksrc = &k_lds[t * K_ROW + (ks * 16 + hi * 8) * 2];
                const uint2 k0 = *reinterpret_cast<const uint2*>(ksrc);
                const uint2 k1 = *reinterpret_cast<const uint2*>(ksrc + 8);
                const uint4 kk{k0.x, k0.y, k1.x, k1.y};
                kfrag = __builtin_bit_cast(short8, kk);
            }
            s = mfma_32x32x16<F16>(kfrag, qf[ks], s);
        }
        __builtin_amdgcn_s_setprio(0);
        return s;
    };

    // one staged tile: NST 32-token sub-tiles, tokens >= Lkv masked if MASK
    auto compute = [&]<int NST, bool MASK>(int t0) {
        float16v s_cur = qk_tile(0);
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            float16v s_nxt;
            if (st + 1 < NST) s_nxt = qk_tile(st + 1);
            const float16v s = s_cur;
            // lane holds S^T rows mfma32_row(r, hi) for q col lo
            float tm = -1e30f;
            float pv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = s[r];
                if (MASK) {
                    if (t0 + st * 32 + mfma32_row(r, hi) >= Lkv) v = -1e30f;
                }
                pv[r] = v;
                tm = fmaxf(tm, v);
            }
            tm = half_max(tm);  // partner holds the other 16 rows

            if (__any(m_raw == -1e30f || tm > m_raw + defer_raw)) {
                const float m_new = fmaxf(m_raw, tm);
                const float msc_new = m_new * scale2;
                const float corr = __builtin_amdgcn_exp2f(msc - msc_new);
                m_raw = m_new;
                msc = msc_new;
                l_run *= corr;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) ot[dt][r] *= corr;
            }
            float tsum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                pv[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(pv[r], scale2, -msc));
                tsum += pv[r];
            }
            l_run += half_sum(tsum);

            // ---- pack P to bf16 (fp16) B-fragments (guide T12: cvt_pk +
            // permlane32_swap); B frag j=0..7 -> P^T rows kt*16 + hi*8 + j.
            // Own word i holds regs {2i,2i+1} = rows {(2i&3)+8*(i>>1)+4*hi, +1}.
            // swap(a, b) leaves a = {lower: a, upper: lower's b} and
            // b = {lower: upper's a, upper: b}, so swapping word pairs 8 rows
            // apart gives hi=0 rows 0..7 and hi=1 rows 8..15 in order. ----
            uint32_t w[8];
#pragma unroll
            for (int i = 0; i < 8; ++i)
                w[i] = F16 ? cvt_pk_f16(pv[2 * i], pv[2 * i + 1])
                           : cvt_pk_bf16(pv[2 * i], pv[2 * i + 1]);
            short8 pb[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                const auto r0 = __builtin_amdgcn_permlane32_swap(w[4 * kt + 0], w[4 * kt + 2],
                                                                 false, false);
                const auto r1 = __builtin_amdgcn_permlane32_swap(w[4 * kt + 1], w[4 * kt + 3],
                                                                 false, false);
                const uint4 pw{r0[0], r1[0], r0[1], r1[1]};
                pb[kt] = __builtin_bit_cast(short8, pw);
            }

            // ---- O^T += V^T x P^T; A[d = lo][k = hi*8 + j] = V[t][d] with
            // t = st*32 + kt*16 + hi*8 + j: two transposed 4-row reads ----
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    const char* vsrc = &v_lds[vrd[dt] + (st * 32 + kt * 16) * V_ROW];
                    const short4v v0 =
                        __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4v*)vsrc);
                    const short4v v1 =
                        __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4v*)(vsrc + 4 * V_ROW));
                    const short8 vf = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
                    ot[dt] = mfma_32x32x16<F16>(vf, pb[kt], ot[dt]);
                }
            }
            __builtin_amdgcn_s_setprio(0);
            s_cur = s_nxt;
        }
    };

    // ---- tile loop: mask-free full tiles, then one peeled tail (in LSE mode
    // over this split's tiles; the tail belongs to the last split) ----
    const int tile0 = LSE ? tile_lo : 0;
    const int n_full = LSE ? min(tile_hi, Lkv / KVB) : Lkv / KVB;
    const int rem = LSE && tile_hi * KVB <= Lkv ? 0 : Lkv % KVB;
    if constexpr (DMA) {
        // Two buffers, one barrier per tile. Tile t is read from buffer rb
        // while tile t+1 goes into the other one: by LDS-DMA, issued right
        // behind the barrier, if it lies inside one chunk, else through
        // registers after the compute (load, then ds_write: that keeps the 16
        // staging registers out of the compute's live range; such tiles are
        // one in 28 at LC = 3600, none without chunks). The
        // barrier at the top of the next iteration, with this wave's DMA
        // (vmcnt) and LDS writes (lgkmcnt) retired in front of it, publishes
        // either kind and tells that every wave is done reading the buffer the
        // tile after that will land in; so the two kinds alternate freely.
        auto publish = [] {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        };
        int rb = 0;
        auto flip = [&]() {
            rb ^= 1;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) krd[ks] ^= K_BYTES;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) vrd[dt] ^= V_BYTES;
        };
        if (Lkv > 0) {
            if (in_chunk(tile0 < n_full)) {
                stage_dma(0);
            } else {
                stage_load(tile0 * KVB, tile0 < n_full);
                stage_write(0);
            }
        }
        // Q has landed: else the compiler carries the pending Q loads into the
        // loop and waits for them, and with them the DMA, at every first QK^T
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) only
        for (int tile = tile0; tile < n_full; ++tile) {
            const int t0 = tile * KVB;
            const bool next_full = tile + 1 < n_full;
            publish();
            const bool more = next_full || rem;
            const bool by_dma = more && in_chunk(next_full);
            if (by_dma) stage_dma(rb ^ 1);
            compute.template operator()<KVB / 32, false>(t0);
            if (more && !by_dma) {
                stage_load(t0 + KVB, next_full);
                stage_write(rb ^ 1);
            }
            flip();
        }
        if (rem) publish();
    } else {
        if (Lkv > 0) {
            stage_load(tile0 * KVB, tile0 < n_full);
            stage_write(0);
            lds_barrier();
        }
        // Q has landed: without this the compiler cannot count the conditional
        // loads behind the Q loads and drains the prefetch at the first QK^T
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) only
        for (int tile = tile0; tile < n_full; ++tile) {
            const int t0 = tile * KVB;
            const bool next_full = tile + 1 < n_full;
            // split staging: the next tile's loads are in flight across the compute
            auto load_next = [&]() {
                if (next_full || rem) stage_load(t0 + KVB, next_full);
            };
            load_next();
            compute.template operator()<KVB / 32, false>(t0);
            if (next_full || rem) {
                lds_barrier();  // every wave is done reading this tile
                stage_write(0);
                lds_barrier();
            }
        }
    }
    if (rem == 64)
        compute.template operator()<2, false>(n_full * KVB);
    else if (rem)
        compute.template operator()<KVB / 32, true>(n_full * KVB);

    // ---- epilogue: O[q][d] = O^T / l (only the real head_dim columns).
    // A lane holds 4 consecutive d per register group g (d = dt*32 + 8g +
    // 4hi ..); swapping groups g and g+1 between the halves (guide T21)
    // leaves each lane 8 consecutive d: one 16 B store instead of 8 shorts.
    const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
    if constexpr (LSE) {
        // ln sum exp(scale * s) = ln2 * (msc + log2 l): msc is the (possibly
        // deferred) exp2-domain offset l_run was accumulated against. Both
        // halves hold the row's value; the lower one stores it.
        const float lse = l_run > 0.f
                              ? 0.69314718055994530942f * (msc + __builtin_amdgcn_logf(l_run))
                              : -__builtin_inff();
        const int64_t sb = (int64_t)blockIdx.z * p.B + b;
        if (qvalid && hi == 0) p.lse[(sb * p.H + h) * p.Lq + qrow] = lse;
        if (p.o_part != nullptr) {
            // fp32 partial [S, B, Lq, H, Dh]: register group g of a lane is 4
            // consecutive d (dt*32 + 8g + 4hi ..), one 16 B store each
            float* op32 = p.o_part + (sb * p.Lq + (qvalid ? qrow : 0)) * (p.H * p.Dh) +
                          (int64_t)h * p.Dh;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int d0 = dt * 32 + 8 * g + 4 * hi;
                    if (qvalid && (DFULL || d0 + 4 <= p.Dh))
                        *reinterpret_cast<float4*>(op32 + d0) =
                            float4{ot[dt][4 * g] * inv, ot[dt][4 * g + 1] * inv,
                                   ot[dt][4 * g + 2] * inv, ot[dt][4 * g + 3] * inv};
                }
            }
            return;
        }
    }
    uint16_t* op = p.o + ((int64_t)b * p.Lq + (qvalid ? qrow : 0)) * (p.H * p.Dh) +
                   (int64_t)h * p.Dh;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        uint32_t ow[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if constexpr (F16)
                ow[i] = cvt_pk_f16(ot[dt][2 * i] * inv, ot[dt][2 * i + 1] * inv);
            else
                ow[i] = pack2_b16<false>(ot[dt][2 * i] * inv, ot[dt][2 * i + 1] * inv);
        }
#pragma unroll
        for (int g = 0; g < 4; g += 2) {
            const auto rx = __builtin_amdgcn_permlane32_swap(ow[2 * g], ow[2 * g + 2],
                                                             false, false);
            const auto ry = __builtin_amdgcn_permlane32_swap(ow[2 * g + 1], ow[2 * g + 3],
                                                             false, false);
            const int d0 = dt * 32 + 8 * (g + hi);
            if (qvalid && (DFULL || d0 + 8 <= p.Dh))
                *reinterpret_cast<uint4*>(op + d0) = uint4{rx[0], ry[0], rx[1], ry[1]};
        }
    }
}

// ---- merge of split-KV partials --------------------------------------------
// One thread per (row, 8 d): S x two 16 B fp32 loads, one 16 B bf16/fp16 store (or
// two fp32). Plain HBM-bound streaming; the S weights of a row are re-derived
// by each of its Dh/8 threads from the (cached) lse parts. Fixed summation
// order s = 0..S-1, no atomics.
template <int OUT>  // DfaDtype of the output
__global__ __launch_bounds__(256) void merge_attn_kernel(MergeAttnParams p) {
    const int dcols = p.Dh / 8;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rows = (int64_t)p.B * p.Lq * p.H;  // (b, q, h), the O row order
    if (idx >= rows * dcols) return;
    const int64_t row = idx / dcols;
    const int dc = (int)(idx - row * dcols);
    const int h = (int)(row % p.H);
    const int64_t bq = row / p.H;
    const int64_t qi = bq % p.Lq;
    const int64_t b = bq / p.Lq;
    const int64_t lse_row = (b * p.H + h) * p.Lq + qi;
    const int64_t lse_ss = (int64_t)p.B * p.H * p.Lq;
    const int64_t o_ss = rows * p.Dh;

    float m = -__builtin_inff();
    for (int s = 0; s < p.S; ++s) m = fmaxf(m, p.lse_parts[s * lse_ss + lse_row]);
    float acc[8] = {};
    float wsum = 0.f;
    if (m > -__builtin_inff()) {  // else every part is empty: zeros, lse = -inf
        const float* src = p.o_parts + row * p.Dh + dc * 8;
        for (int s = 0; s < p.S; ++s) {
            const float w = expf(p.lse_parts[s * lse_ss + lse_row] - m);  // exp(-inf) = 0
            const float4 a = *reinterpret_cast<const float4*>(src + s * o_ss);
            const float4 c = *reinterpret_cast<const float4*>(src + s * o_ss + 4);
            if (w > 0.f) {  // an empty part may hold anything
                wsum += w;
                acc[0] += w * a.x, acc[1] += w * a.y, acc[2] += w * a.z, acc[3] += w * a.w;
                acc[4] += w * c.x, acc[5] += w * c.y, acc[6] += w * c.z, acc[7] += w * c.w;
            }
        }
        const float inv = 1.f / wsum;  // wsum >= 1: the max part has weight 1
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] *= inv;
    }
    if (OUT != DFA_F32) {
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = pack2_b16<OUT == DFA_F16>(acc[2 * j], acc[2 * j + 1]);
        *reinterpret_cast<uint4*>(static_cast<uint16_t*>(p.out) + row * p.Dh + dc * 8) =
            uint4{w[0], w[1], w[2], w[3]};
    } else {
        float* dst = static_cast<float*>(p.out) + row * p.Dh + dc * 8;
        *reinterpret_cast<float4*>(dst) = float4{acc[0], acc[1], acc[2], acc[3]};
        *reinterpret_cast<float4*>(dst + 4) = float4{acc[4], acc[5], acc[6], acc[7]};
    }
    if (dc == 0 && p.lse != nullptr)
        p.lse[lse_row] = wsum > 0.f ? m + logf(wsum) : -__builtin_inff();
}

// the DfaDtype of an element type
template <typename T>
constexpr int dtype_of = std::is_same_v<T, bf16_t>  ? DFA_BF16
                         : std::is_same_v<T, f16_t> ? DFA_F16
                                                    : DFA_F32;

}  // namespace

void launch_merge_attention(const MergeAttnParams& p, hipStream_t stream) {
    const int64_t total = (int64_t)p.B * p.Lq * p.H * (p.Dh / 8);
    if (total == 0) return;
    const dim3 grid((unsigned)((total + 255) / 256));
    dispatch_dtype(p.out_dtype, [&]<typename T>(std::type_identity<T>) {
        merge_attn_kernel<dtype_of<T>><<<grid, 256, 0, stream>>>(p);
    });
}

namespace {

// the in-chunk staging path adds a 32-bit lane offset (a tile's rows and one
// row's columns) to the tile cursor; larger token strides stay on the general
// 64-bit path
template <int DPAD>
bool fits_off32(const FlashAttnParams& p) {
    const int64_t sl = p.k_sl > p.v_sl ? p.k_sl : p.v_sl;
    return sl >= 0 && sl * 2 * KVB + DPAD * 2 <= (int64_t)INT32_MAX;
}

// grid.z = splits; the plain (LSE = false) kernel takes the base slice of the
// params and one split
template <int DPAD, bool LSE, bool F16>
void launch_dpad(const FlashAttnLseParams& p, int splits, hipStream_t stream) {
    constexpr int NW = 8;
    const int qblk = QW * NW;
    const dim3 grid((unsigned)((p.Lq + qblk - 1) / qblk), (unsigned)(p.B * p.H),
                    (unsigned)splits);
    const dim3 block(NW * WAVE_SIZE);
    const bool off32 = fits_off32<DPAD>(p);
    const std::conditional_t<LSE, FlashAttnLseParams, FlashAttnParams>& kp = p;
    dispatch_bool(p.Dh == DPAD, [&]<bool DFULL>(std::bool_constant<DFULL>) {
        flash_attn_kernel<NW, DPAD, DFULL, LSE, F16><<<grid, block, 0, stream>>>(kp, off32);
    });
}

template <bool LSE, bool F16>
void launch_ladder(const FlashAttnLseParams& p, int splits, hipStream_t stream) {
    // 8-wave (256-row) blocks measured best across the SD-family shapes;
    // every Lkv takes 128-token tiles plus a peeled tail. DPAD covers the
    // SD-family head dims.
    if (p.Dh <= 64)
        launch_dpad<64, LSE, F16>(p, splits, stream);
    else if (p.Dh <= 96)
        launch_dpad<96, LSE, F16>(p, splits, stream);
    else if (p.Dh <= 128)
        launch_dpad<128, LSE, F16>(p, splits, stream);
    else
        launch_dpad<160, LSE, F16>(p, splits, stream);
}

}  // namespace

int flash_attention_num_splits(int64_t lkv, int splits) {
    const int64_t tiles = (lkv + KVB - 1) / KVB;
    return (int)std::max<int64_t>(1, std::min<int64_t>(splits, tiles));
}

void launch_flash_attention(const FlashAttnLseParams& p, int splits, int dtype,
                            hipStream_t stream) {
    dispatch_f16(dtype, [&]<bool F16>(std::bool_constant<F16>) {
        if (p.lse == nullptr && p.o_part == nullptr)
            launch_ladder<false, F16>(p, 1, stream);
        else
            launch_ladder<true, F16>(p, flash_attention_num_splits(p.NC * p.LC, splits), stream);
    });
}

// ---- fragment-layout probes (tests/test_ops_gpu.py) ------------------------
namespace {
__global__ void mfma_probe_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                  float* __restrict__ d) {
    const int lane = threadIdx.x;  // single wave
    short8 af, bf;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        af[j] = __builtin_bit_cast(short, __float2bfloat16(a[lane * 8 + j]));
        bf[j] = __builtin_bit_cast(short, __float2bfloat16(b[lane * 8 + j]));
    }
    float4v acc = {};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) d[lane * 4 + r] = acc[r];
}

__global__ void mfma_probe32_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                    float* __restrict__ d) {
    const int lane = threadIdx.x;
    short8 af, bf;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        af[j] = __builtin_bit_cast(short, __float2bfloat16(a[lane * 8 + j]));
        bf[j] = __builtin_bit_cast(short, __float2bfloat16(b[lane * 8 + j]));
    }
    float16v acc = {};
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) d[lane * 16 + r] = acc[r];
}
}  // namespace

void launch_mfma_probe(const float* a, const float* b, float* d, hipStream_t stream) {
    mfma_probe_kernel<<<1, WAVE_SIZE, 0, stream>>>(a, b, d);
}

void launch_mfma_probe32(const float* a, const float* b, float* d, hipStream_t stream) {
    mfma_probe32_kernel<<<1, WAVE_SIZE, 0, stream>>>(a, b, d);
}
