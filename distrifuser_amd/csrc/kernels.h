// Host-side launcher declarations (implemented in the .hip translation units).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

enum DfaDtype : int { DFA_BF16 = 0, DFA_F16 = 1, DFA_F32 = 2 };

// ---- GroupNorm family ------------------------------------------------------
// partial: fp32 [2, N*G], receives sum and sumsq (no initialisation needed).
// A group is summed by gn_stats_chunks() blocks; with more than one, they
// store into ws, fp32 [2, N*G, chunks], and a second launch adds the chunks
// in a fixed order: the same bits on every run. ws is not read with one chunk.
int gn_stats_chunks(int64_t group_len, int n_groups_total, int dtype);
void launch_gn_stats_partial(const void* x, float* ws, float* partial, int64_t group_len,
                             int n_groups_total, int dtype, hipStream_t stream);
// out: [2, N*G] in `dtype`; mean = partial/count.
void launch_gn_finalize(const float* partial, void* out, float inv_count,
                        int n_groups_total, int dtype, hipStream_t stream);
// normalize+affine(+SiLU) with externally supplied fp32 moments [N*G] each.
void launch_gn_apply(const void* x, void* y, const float* mean, const float* meansq,
                     const void* weight, const void* bias, float eps, int64_t hw,
                     int C, int G, int N, bool silu, int dtype, hipStream_t stream);

// launch_gn_apply with a token-major result: x [N, C, HW] contiguous in,
// y [N, HW, C] contiguous out; the same value per element (a tiled transpose
// through LDS). 16-byte accesses for 16-bit types when HW % 8 == 0, C % 8 == 0
// and both pointers are 16-byte aligned, else an element-wise tile; any dtype.
// The caller keeps C tiles and N within 65535 (boundary_plan.h).
void launch_gn_apply_tokens(const void* x, void* y, const float* mean, const float* meansq,
                            const void* weight, const void* bias, float eps, int64_t hw,
                            int C, int G, int N, bool silu, int dtype, hipStream_t stream);

// ---- token -> NCHW transposing residual add ---------------------------------
// out[n, c, p] = round(float(y[n, p, c]) + float(residual[n, c, p])); y [N, HW, C]
// and out [N, C, HW] contiguous, residual with batch / channel strides in
// elements and a contiguous pixel plane. Same vector / scalar split as above
// (the vector path also needs both residual strides to be multiples of 8).
void launch_tokens_add_nchw(const void* y, const void* residual, void* out, int64_t hw, int C,
                            int N, int64_t res_stride_n, int64_t res_stride_c, int dtype,
                            hipStream_t stream);

// ---- displaced-GN stat merge ------------------------------------------------
// Merge per-peer stale GroupNorm moments with this rank's fresh ones in ONE
// launch (replaces a ~10-kernel torch composition per GN layer):
//   corrected: full = mean(stale) + (fresh - stale_own)   [+ neg-var guard]
//   stale:     full = mean(stale with own slot := fresh)
// Also stages `fresh` into the rank's buffer slot (the enqueue needs it).
// buffer: bf16, n_peers rows of row_stride elements, moment block at
// buffer[row * row_stride + slot_off .. + 2*ng); fresh: bf16 [2*ng];
// out: fp32 [2*ng].
void launch_gn_merge_stats(void* buffer, int64_t row_stride, int64_t slot_off,
                           int n_peers, int own, const void* fresh, float* out,
                           int ng, bool corrected, int dtype, hipStream_t stream);

// ---- GEGLU ------------------------------------------------------------------
// in: [rows, 2*inner]; out: [rows, inner]; out = a * gelu(gate).
void launch_geglu(const void* in, void* out, int64_t rows, int64_t inner, int dtype,
                  hipStream_t stream);

// ---- inpaint blend of a masked scheduler step -------------------------------
// known = sa*init + sb*init_noise; out = m*x' + (1 - m)*known, in fp32, rounded
// once. init and init_noise: fp32 [C*hw], one value per latent element; mask:
// fp32 [hw], element i reads mask[i % hw] (broadcast over channels).
struct MaskBlend {
    const float* init;
    const float* init_noise;
    const float* mask;
    float sa, sb;
    int64_t hw;
};

// ---- the noise term of a stochastic scheduler step ----------------------------
// x' += cn * z, z the Philox normal of (seed, draw, element index): philox.h.
struct StepNoise {
    float cn;
    uint64_t seed;
    uint32_t draw;
};

// out[e] = the normal of element offset + e, e in [0, numel): fp32
void launch_philox_normal(float* out, int64_t numel, int64_t offset, uint64_t seed,
                          uint32_t draw, hipStream_t stream);

// ---- guidance_rescale factor ---------------------------------------------------
// factor[0] = phi * std(nc) / std(eps) + (1 - phi), eps = nu + g*(nc - nu), both
// standard deviations over the `total` elements of the one sample; fp32 sums.
// Two launches: cfg_moments_blocks(total) blocks each store four partial sums
// to a row of ws, fp32 [blocks][4] (no initialisation needed), and one block
// adds the rows in index order. The block count depends on total alone, so
// the factor is the same bits on every run and device.
int cfg_moments_blocks(int64_t total);
void launch_guidance_rescale_factor(const void* noise_u, const void* noise_c, float g, float phi,
                                    int64_t total, float* ws, float* factor, int dtype,
                                    hipStream_t stream);

// ---- fused CFG + scheduler step (affine: out = ca*x + cb*eps) ---------------
// blend != null: the masked step, total = C*hw; noise_c may then be null (no
// CFG pair: eps = noise_u, g is not read). Its 16-byte path needs hw a
// multiple of the vector width and 16-byte aligned pointers.
// factor != null (one fp32 on the device, noise_c not null): eps is replaced
// by round(factor[0] * eps) before the update. A factor of 1 gives the bits
// of the call without one.
// noise != null with cn != 0: out = fma(cn, z, x') before any blend, z indexed
// by the element's offset in the one sample; noise_c may then be null as well.
// cn == 0 runs the instantiation of the call without noise, except for the
// call that has none (no pair, no blend), which then adds 0 * z.
void launch_cfg_affine_step(const void* noise_u, const void* noise_c, const void* x, void* out,
                            float g, float ca, float cb, int64_t total, int dtype,
                            hipStream_t stream, const MaskBlend* blend = nullptr,
                            const float* factor = nullptr, const StepNoise* noise = nullptr);

// ---- inpaint U-Net input assembly --------------------------------------------
// out [copies, 9, hw]: channels 0..3 = latents [4, hw] / scale, channel 4 =
// mask [hw], channels 5..8 = masked [4, hw] (4..8 copied bit for bit).
void launch_inpaint_unet_input(const void* latents, const void* mask, const void* masked,
                               void* out, float scale, int64_t hw, int copies, int dtype,
                               hipStream_t stream);

// ---- Implicit-GEMM 3x3 conv (bf16 or fp16, NCHW, stride 1/2, pad 1) -----------------
// x: interior [B][Cin][H][W] (row-contiguous; x_sc = channel stride).
// top/bot: optional single halo rows [B][Cin][1][W] (e.g. comm-buffer views);
// null => zero padding at that border. Input row y_in=-1 reads top, y_in=H
// reads bot. o: [B][Cout][Ho][Wo] contiguous output.
// wp: weights prepacked in per-lane A-fragment order [9][KS][CT][64][8]
// (cout = ct*32 + (lane&31), cin = ks*16 + (lane>>5)*8 + j), KS*16 and CT*32
// zero-padded to multiples of 64/32. bias: [Cout] or null.
struct Conv3x3Params {
    const uint16_t* x;
    const uint16_t* top;
    const uint16_t* bot;
    const uint16_t* wp;
    const uint16_t* bias;
    const uint16_t* residual;  // optional [B][Cout][Ho][Wo]: o += residual
    const uint16_t* bias2;     // optional [B][Cout]: o += bias2 (time-emb add)
    uint16_t* o;
    int B, Cin, Cout, H, W, Ho, Wo;
    int KS, CT;
    int debug;  // 1 = skip input staging, 2 = skip MFMA (phase-cost probes)
    // 1: pad 1 on every side. 0 (stride 2 only): pad bottom/right alone, the
    // AutoencoderKL downsample; Ho = (H-2)/2 + 1, Wo = (W-2)/2 + 1, top null,
    // row H reads bot (or zero), column W is zero.
    int pad_lo;
    int64_t x_sb, x_sc;
    int64_t t_sb, t_sc;
    int64_t b_sb, b_sc;
};
// dtype: DFA_BF16 or DFA_F16 for x, halos, wp, bias, residual, bias2 and o alike
void launch_conv3x3(const Conv3x3Params& p, int stride, int dtype, hipStream_t stream);

// ---- fused CFG + DPM-Solver++(2M) step --------------------------------------
// out = ca*x + cb*eps + cc*x0_prev (x0_prev may be null); x0_out = cx*x + ce*eps
// blend != null: out is blended as in the masked affine step (nc may be null);
// x0_out is not. factor as in the affine step: out and x0_out both use eps_r.
// noise as in the affine step: added to out after the x0_prev term and before
// the blend; x0_out never sees it.
void launch_cfg_dpm_step(const void* nu, const void* nc, const void* x, const void* x0_prev,
                         void* out, void* x0_out, float g, float ca, float cb, float cc,
                         float cx, float ce, int64_t total, int dtype, hipStream_t stream,
                         const MaskBlend* blend = nullptr, const float* factor = nullptr,
                         const StepNoise* noise = nullptr);

// ---- fused (residual +) LayerNorm (bf16 or fp16, C <= 2048, C % 8 == 0) -------------
// y = LN(x [+ res]); when res != null and sum_out != null, x+res is also
// written to sum_out (the transformer residual add fused away).
void launch_layer_norm(const void* x, const void* res, void* y, void* sum_out,
                       const void* w, const void* b, float eps, int64_t rows, int C,
                       int dtype, hipStream_t stream);

// ---- VAE mid-block attention (bf16 or fp16, single head, head_dim 512) --------------
// q/k/v/o: [B][L][512] row-contiguous (sb = batch stride in elements).
struct VaeAttnParams {
    const uint16_t* q;
    const uint16_t* k;
    const uint16_t* v;
    uint16_t* o;
    int B;
    int64_t L, sb;
    float scale;
};
void launch_vae_attention(const VaeAttnParams& p, int dtype, hipStream_t stream);

// ---- Flash attention (bf16 or fp16, SD-family head dims) ----------------------------
// q: logical [B, H, Lq, 64]; k/v: logical [B, H, NC, LC, 64] (NC stale-KV
// chunks of LC tokens; NC=1 for plain attention). All strides in ELEMENTS,
// innermost head_dim contiguous. o: [B, Lq, H, 64] contiguous output.
struct FlashAttnParams {
    const uint16_t* q;
    const uint16_t* k;
    const uint16_t* v;
    uint16_t* o;
    int B, H;
    int Dh;  // real head_dim (kernel pads to a multiple of 32)
    int64_t Lq, NC, LC;  // Lkv = NC * LC
    int64_t q_sb, q_sh, q_sl;
    int64_t k_sb, k_sh, k_sc, k_sl;
    int64_t v_sb, v_sh, v_sc, v_sl;
    float scale;  // 1/sqrt(64)
};

// LSE / split-KV mode of the same kernel. lse: fp32 [S, B, H, Lq], the natural
// log of each row's sum of exp(scale * q.k) over the split's KV slice (-inf
// for an empty slice). o_part == null (S == 1 only): 16-bit O goes to `o` as in
// the plain mode. o_part != null: split s writes its normalised partial
// output as fp32 into o_part [S, B, Lq, H, Dh]; `o` is not touched.
struct FlashAttnLseParams : FlashAttnParams {
    float* lse;
    float* o_part;
};
// S the launcher uses for a request of `splits`: clamped to [1, ceil(Lkv/128)]
// (splits are tile-aligned and never empty).
int flash_attention_num_splits(int64_t lkv, int splits);
// lse == null and o_part == null: the plain kernel (one split, `splits` is not
// read); otherwise the LSE kernel over the clamped number of splits.
// dtype: DFA_BF16 or DFA_F16, the element type of q/k/v/o (the caller rejects
// DFA_F32); a template axis of the kernel, the parameter block is the same.
void launch_flash_attention(const FlashAttnLseParams& p, int splits, int dtype,
                            hipStream_t stream);

// ---- fragment-layout probes: one wave, a/b fp32 [64][8], d fp32 [64][4] / [64][16] ----
void launch_mfma_probe(const float* a, const float* b, float* d, hipStream_t stream);
void launch_mfma_probe32(const float* a, const float* b, float* d, hipStream_t stream);

// ---- merge of attention partials ----------------------------------------------
// out[b,q,h,:] = sum_s w_s o_parts[s,b,q,h,:] / sum_s w_s, w_s = exp(lse_s - max_s lse_s);
// lse = max + ln sum_s w_s (optional). A part with lse = -inf has weight 0; all
// parts -inf gives zeros and lse = -inf. o_parts fp32 [S, B, Lq, H, Dh],
// lse_parts fp32 [S, B, H, Lq], out [B, Lq, H, Dh] bf16, fp16 or fp32, Dh % 8 == 0.
struct MergeAttnParams {
    const float* o_parts;
    const float* lse_parts;
    void* out;
    float* lse;  // [B, H, Lq] or null
    int S, B, H, Dh;
    int64_t Lq;
    int out_dtype;  // DfaDtype of `out`
};
void launch_merge_attention(const MergeAttnParams& p, hipStream_t stream);
