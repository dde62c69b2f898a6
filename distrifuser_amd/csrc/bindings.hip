// Python bindings for the distrifuser_amd gfx950 kernels (module _C).
// Pure HIP + ATen/hip — no CUDA-compat layer; compiled by hipcc via
// torch.utils.cpp_extension with PYTORCH_ROCM_ARCH=gfx950.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include <array>

#include "boundary_plan.h"
#include "kernels.h"

namespace {

int dtype_of(const at::Tensor& t) {
    switch (t.scalar_type()) {
        case at::kBFloat16: return DFA_BF16;
        case at::kHalf: return DFA_F16;
        case at::kFloat: return DFA_F32;
        default: TORCH_CHECK(false, "unsupported dtype ", t.scalar_type());
    }
}

// the MFMA kernels and LayerNorm take bf16 or fp16 (a template axis each)
bool is_b16(const at::Tensor& t) {
    return t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kHalf;
}

hipStream_t cur_stream() { return at::hip::getCurrentHIPStream().stream(); }

// A 16-bit parameter of a 16-bit op, in ref's dtype: an fp32 master copy is
// cast as it always was, the other 16-bit type is a mix-up
at::Tensor b16_param(const at::Tensor& t, const at::Tensor& ref, const char* op,
                     const char* name) {
    TORCH_CHECK(t.scalar_type() == ref.scalar_type() || !is_b16(t), op, ": ", name,
                " must have x's dtype (", ref.scalar_type(), "), got ", t.scalar_type());
    return t.to(ref.scalar_type()).contiguous();
}

// fp32 [2, ngt] sum and sum of squares of x's ngt groups of group_len elements
at::Tensor gn_partial_stats(const at::Tensor& x, int64_t group_len, int ngt) {
    const auto f32 = x.options().dtype(at::kFloat);
    auto partial = at::empty({2, (long)ngt}, f32);
    const int chunks = gn_stats_chunks(group_len, ngt, dtype_of(x));
    at::Tensor ws;  // per-chunk sums, added in a fixed order (no atomics)
    if (chunks > 1) ws = at::empty({2, (long)ngt, (long)chunks}, f32);
    launch_gn_stats_partial(x.data_ptr(), chunks > 1 ? ws.data_ptr<float>() : nullptr,
                            partial.data_ptr<float>(), group_len, ngt, dtype_of(x),
                            cur_stream());
    return partial;
}

// Optional GroupNorm affine tensor in x's dtype, contiguous (kept alive in
// `keep`), or null
const void* gn_affine(const c10::optional<at::Tensor>& t, const at::Tensor& x, at::Tensor& keep) {
    if (!t.has_value()) return nullptr;
    keep = t->to(x.scalar_type()).contiguous();
    return keep.data_ptr();
}

// The apply pass of both GroupNorm entries: NCHW like x, or [N, HW, C] (tokens)
at::Tensor gn_apply_out(const at::Tensor& x, const float* mean, const float* meansq,
                        const void* wp, const void* bp, double eps, int g, bool silu,
                        bool tokens) {
    const int64_t n = x.size(0), c = x.size(1), hw = x.size(2) * x.size(3);
    if (!tokens) {
        auto y = at::empty_like(x);
        launch_gn_apply(x.data_ptr(), y.data_ptr(), mean, meansq, wp, bp, (float)eps, hw, (int)c,
                        g, (int)n, silu, dtype_of(x), cur_stream());
        return y;
    }
    auto y = at::empty({n, hw, c}, x.options());
    const BoundaryPlan pl = boundary_plan(n, c, hw, (int)x.element_size(), true);
    TORCH_CHECK(pl.ok || pl.empty, "group_norm tokens: shape too large for one launch");
    launch_gn_apply_tokens(x.data_ptr(), y.data_ptr(), mean, meansq, wp, bp, (float)eps, hw,
                           (int)c, g, (int)n, silu, dtype_of(x), cur_stream());
    return y;
}

at::Tensor group_norm_stats(const at::Tensor& x_, int64_t num_groups) {
    TORCH_CHECK(x_.is_cuda() && x_.dim() == 4, "x must be CUDA [N,C,H,W]");
    auto x = x_.contiguous();
    const int64_t n = x.size(0), c = x.size(1), hw = x.size(2) * x.size(3);
    TORCH_CHECK(c % num_groups == 0);
    const int64_t group_len = (c / num_groups) * hw;
    const int ngt = (int)(n * num_groups);
    auto partial = gn_partial_stats(x, group_len, ngt);
    auto out = at::empty({2, n, num_groups, 1, 1, 1}, x.options());
    launch_gn_finalize(partial.data_ptr<float>(), out.data_ptr(), 1.0f / (float)group_len, ngt,
                       dtype_of(x), cur_stream());
    return out;
}

at::Tensor group_norm_apply(const at::Tensor& x_, const at::Tensor& mean_,
                            const at::Tensor& meansq_, const c10::optional<at::Tensor>& w_,
                            const c10::optional<at::Tensor>& b_, double eps, bool silu,
                            bool tokens) {
    TORCH_CHECK(x_.is_cuda() && x_.dim() == 4);
    auto x = x_.contiguous();
    const int64_t n = x.size(0), c = x.size(1);
    auto mean = mean_.to(at::kFloat).contiguous().view({-1});
    auto meansq = meansq_.to(at::kFloat).contiguous().view({-1});
    TORCH_CHECK(mean.numel() % n == 0);
    const int g = (int)(mean.numel() / n);
    TORCH_CHECK(c % g == 0, "channels ", c, " not divisible by groups ", g);
    at::Tensor w, b;
    const void* wp = gn_affine(w_, x, w);
    const void* bp = gn_affine(b_, x, b);
    return gn_apply_out(x, mean.data_ptr<float>(), meansq.data_ptr<float>(), wp, bp, eps, g, silu,
                        tokens);
}

at::Tensor group_norm_silu(const at::Tensor& x_, int64_t num_groups,
                           const c10::optional<at::Tensor>& w_,
                           const c10::optional<at::Tensor>& b_, double eps, bool silu,
                           bool tokens) {
    TORCH_CHECK(x_.is_cuda() && x_.dim() == 4);
    auto x = x_.contiguous();
    const int64_t n = x.size(0), c = x.size(1), hw = x.size(2) * x.size(3);
    TORCH_CHECK(c % num_groups == 0);
    const int64_t group_len = (c / num_groups) * hw;
    const int ngt = (int)(n * num_groups);
    auto partial = gn_partial_stats(x, group_len, ngt);
    // finalize in fp32 (full precision straight into the apply)
    auto moments = at::empty({2, (long)ngt}, x.options().dtype(at::kFloat));
    launch_gn_finalize(partial.data_ptr<float>(), moments.data_ptr(), 1.0f / (float)group_len,
                       ngt, DFA_F32, cur_stream());
    at::Tensor w, b;
    const void* wp = gn_affine(w_, x, w);
    const void* bp = gn_affine(b_, x, b);
    return gn_apply_out(x, moments.data_ptr<float>(), moments.data_ptr<float>() + ngt, wp, bp, eps,
                        (int)num_groups, silu, tokens);
}

// y [N, HW, C] + residual [N, C, H, W] -> [N, C, H, W] contiguous. residual may
// have any batch and channel stride; its (H, W) plane must be contiguous.
at::Tensor tokens_add_nchw(const at::Tensor& y_, const at::Tensor& residual) {
    TORCH_CHECK(y_.is_cuda() && y_.dim() == 3 && residual.is_cuda() && residual.dim() == 4,
                "tokens_add_nchw: y [N,HW,C] and residual [N,C,H,W] on the GPU");
    TORCH_CHECK(y_.scalar_type() == residual.scalar_type(),
                "tokens_add_nchw: residual must have y's dtype (", y_.scalar_type(), "), got ",
                residual.scalar_type());
    const int64_t n = residual.size(0), c = residual.size(1);
    const int64_t hw = residual.size(2) * residual.size(3);
    TORCH_CHECK(y_.size(0) == n && y_.size(1) == hw && y_.size(2) == c,
                "tokens_add_nchw: y must be [N, H*W, C] of residual [N, C, H, W]");
    const int64_t sizes[4] = {n, c, residual.size(2), residual.size(3)};
    const int64_t strides[4] = {residual.stride(0), residual.stride(1), residual.stride(2),
                                residual.stride(3)};
    TORCH_CHECK(boundary_plane_contiguous(sizes, strides),
                "tokens_add_nchw: residual's (H, W) plane must be contiguous");
    auto y = y_.contiguous();
    auto out = at::empty({n, c, residual.size(2), residual.size(3)}, y.options());
    const BoundaryPlan pl = boundary_plan(n, c, hw, (int)y.element_size(), true);
    TORCH_CHECK(pl.ok || pl.empty, "tokens_add_nchw: shape too large for one launch");
    launch_tokens_add_nchw(y.data_ptr(), residual.data_ptr(), out.data_ptr(), hw, (int)c, (int)n,
                           strides[0], strides[1], dtype_of(y), cur_stream());
    return out;
}

at::Tensor gn_merge_stats(const at::Tensor& buffer, int64_t slot_off, int64_t own,
                          const at::Tensor& fresh_, bool corrected) {
    // buffer: [n_peers, row_stride] (the flat comm buffer); fresh: [2, N, G,...]
    TORCH_CHECK(buffer.is_cuda() && buffer.dim() == 2 && buffer.stride(1) == 1);
    auto fresh = fresh_.contiguous();
    const int ng = (int)(fresh.numel() / 2);
    TORCH_CHECK(fresh.scalar_type() == buffer.scalar_type());
    auto out = at::empty({2, (long)ng}, buffer.options().dtype(at::kFloat));
    launch_gn_merge_stats(buffer.data_ptr(), buffer.stride(0), slot_off,
                          (int)buffer.size(0), (int)own, fresh.data_ptr(),
                          out.data_ptr<float>(), ng, corrected, dtype_of(buffer),
                          cur_stream());
    return out;
}

at::Tensor geglu(const at::Tensor& h_) {
    TORCH_CHECK(h_.is_cuda());
    auto h = h_.contiguous();
    const int64_t inner = h.size(-1) / 2;
    TORCH_CHECK(h.size(-1) % 2 == 0);
    auto sizes = h.sizes().vec();
    sizes.back() = inner;
    auto out = at::empty(sizes, h.options());
    launch_geglu(h.data_ptr(), out.data_ptr(), h.numel() / (2 * inner), inner, dtype_of(h),
                 cur_stream());
    return out;
}

// The guidance_rescale factor of a step, or null: one fp32 on the GPU, for a
// [2,C,h,w] CFG pair and x [1,C,h,w] only
const float* rescale_factor(const char* op, const c10::optional<at::Tensor>& factor,
                            const at::Tensor& noise, const at::Tensor& x) {
    if (!factor.has_value()) return nullptr;
    TORCH_CHECK(factor->is_cuda() && factor->scalar_type() == at::kFloat && factor->numel() == 1,
                op, ": factor must be one fp32 value on the GPU");
    TORCH_CHECK(noise.dim() == 4 && noise.size(0) == 2 && noise.numel() == 2 * x.numel(), op,
                ": a rescale factor needs the [2,C,h,w] CFG pair as noise");
    TORCH_CHECK(x.dim() == 4 && x.size(0) == 1, op,
                ": a rescale factor needs x [1,C,h,w] (one sample)");
    return factor->data_ptr<float>();
}

// r = phi * std(nc) / std(nu + g*(nc - nu)) + (1 - phi) over the one sample of
// the [2,C,h,w] CFG pair -> fp32 [1]; two launches, the same bits on every run
at::Tensor guidance_rescale_factor(const at::Tensor& noise, double g, double phi) {
    TORCH_CHECK(noise.is_cuda() && noise.dim() == 4 && noise.size(0) == 2,
                "guidance_rescale_factor: noise must be the CUDA [2,C,h,w] CFG pair");
    auto n = noise.contiguous();
    const int64_t total = n.numel() / 2;
    TORCH_CHECK(total > 0, "guidance_rescale_factor: empty noise");
    const auto f32 = n.options().dtype(at::kFloat);
    auto ws = at::empty({(long)cfg_moments_blocks(total), 4}, f32);
    auto factor = at::empty({1}, f32);
    launch_guidance_rescale_factor(
        n.data_ptr(), reinterpret_cast<const char*>(n.data_ptr()) + total * n.element_size(),
        (float)g, (float)phi, total, ws.data_ptr<float>(), factor.data_ptr<float>(), dtype_of(n),
        cur_stream());
    return factor;
}

// noise=(cn, seed, draw) of a stochastic step, or nothing: x' += cn * z with z
// the Philox normal of (seed, draw, element index). The index is the element's
// offset in the one sample, so x must be [1,C,h,w].
using NoiseArg = std::optional<std::tuple<double, uint64_t, uint32_t>>;
struct StepNoiseArg {
    StepNoise value;
    bool given;
    const StepNoise* ptr() const { return given ? &value : nullptr; }
};
StepNoiseArg step_noise(const char* op, const NoiseArg& noise, const at::Tensor& x) {
    if (!noise.has_value()) return {{0.f, 0, 0}, false};
    TORCH_CHECK(x.dim() == 4 && x.size(0) == 1, op,
                ": a noisy step needs x [1,C,h,w] (one sample)");
    return {{(float)std::get<0>(*noise), std::get<1>(*noise), std::get<2>(*noise)}, true};
}

// The unmasked step ops take the [2,C,h,w] CFG pair, or with noise= also the
// single-branch output in x's shape; -> the cond half, null without a pair
const void* cond_half(const char* op, const at::Tensor& n, const at::Tensor& xc, bool noisy) {
    TORCH_CHECK(n.is_cuda() && xc.is_cuda() && n.scalar_type() == xc.scalar_type(), op,
                ": noise and x must be CUDA tensors of one dtype");
    if (noisy && n.numel() == xc.numel()) return nullptr;
    TORCH_CHECK(n.size(0) == 2 && xc.numel() * 2 == n.numel(), op,
                ": noise must be the [2,C,h,w] CFG pair",
                noisy ? " or, with noise=, the output [1,C,h,w] of one branch" : "");
    return reinterpret_cast<const char*>(n.data_ptr()) + xc.numel() * n.element_size();
}

at::Tensor cfg_affine_step(const at::Tensor& noise, const at::Tensor& x, double g, double ca,
                           double cb, const c10::optional<at::Tensor>& factor,
                           const NoiseArg& znoise) {
    // noise: [2, C, H, W] = [uncond; cond]; x: [1, C, H, W]; out = ca*x + cb*eps
    TORCH_CHECK(noise.is_cuda() && noise.dim() >= 1);
    auto n = noise.contiguous();
    auto xc = x.contiguous();
    const auto nz = step_noise("cfg_affine_step", znoise, x);
    const void* nc = cond_half("cfg_affine_step", n, xc, nz.given);
    const float* fp = rescale_factor("cfg_affine_step", factor, noise, x);
    auto out = at::empty_like(xc);
    launch_cfg_affine_step(n.data_ptr(), nc, xc.data_ptr(), out.data_ptr(), (float)g, (float)ca,
                           (float)cb, xc.numel(), dtype_of(xc), cur_stream(), nullptr, fp,
                           nz.ptr());
    return out;
}

// fp32 [numel]: the normals of elements offset .. offset + numel - 1 of the
// stream (seed, draw), csrc/philox.h
at::Tensor philox_normal(int64_t numel, uint64_t seed, uint32_t draw, int64_t offset,
                         int64_t device_index) {
    TORCH_CHECK(numel >= 0 && offset >= 0 && offset <= INT64_MAX - numel,
                "philox_normal: numel and offset must be >= 0 and their sum an int64");
    const c10::Device device(c10::kCUDA, (c10::DeviceIndex)device_index);
    const c10::DeviceGuard guard(device);  // the launch and its stream are that device's
    auto out = at::empty({numel}, at::TensorOptions().dtype(at::kFloat).device(device));
    launch_philox_normal(out.data_ptr<float>(), numel, offset, seed, draw, cur_stream());
    return out;
}

// The inputs of a masked (inpaint) step: x [1,C,h,w] and noise [2,C,h,w] (a
// CFG pair) or [1,C,h,w] (no guidance), one dtype; init and init_noise fp32
// [1,C,h,w], mask fp32 with h*w elements. The contiguous copies live as long
// as the struct; nc is null without a CFG pair.
struct MaskedStepArgs {
    at::Tensor n, x, init, init_noise, mask;
    const void* nc;
    MaskBlend blend;
};
MaskedStepArgs masked_step_args(const char* op, const at::Tensor& noise, const at::Tensor& x,
                                const at::Tensor& init, const at::Tensor& init_noise,
                                const at::Tensor& mask, double sa, double sb) {
    TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.size(0) == 1, op, ": x must be CUDA [1,C,h,w]");
    TORCH_CHECK(noise.is_cuda() && noise.scalar_type() == x.scalar_type() &&
                    (noise.numel() == x.numel() || noise.numel() == 2 * x.numel()),
                op, ": noise must be [2,C,h,w] or [1,C,h,w] in x's dtype");
    const int64_t hw = x.size(2) * x.size(3);
    auto f32_on_gpu = [&](const at::Tensor& t, int64_t numel, const char* name) {
        TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.numel() == numel, op, ": ",
                    name, " must be CUDA fp32 with ", numel, " elements");
        return t.contiguous();
    };
    MaskedStepArgs a{noise.contiguous(), x.contiguous(), f32_on_gpu(init, x.numel(), "init"),
                     f32_on_gpu(init_noise, x.numel(), "init_noise"),
                     f32_on_gpu(mask, hw, "mask"), nullptr, {}};
    if (noise.numel() == 2 * x.numel())
        a.nc = reinterpret_cast<const char*>(a.n.data_ptr()) + x.numel() * a.n.element_size();
    a.blend = {a.init.data_ptr<float>(), a.init_noise.data_ptr<float>(),
               a.mask.data_ptr<float>(), (float)sa, (float)sb, hw};
    return a;
}

// cfg_affine_step (or the plain affine step when noise has batch 1), then
// out = m*x' + (1 - m)*(sa*init + sb*init_noise), in one launch
at::Tensor masked_affine_step(const at::Tensor& noise, const at::Tensor& x,
                              const at::Tensor& init, const at::Tensor& init_noise,
                              const at::Tensor& mask, double g, double ca, double cb, double sa,
                              double sb, const c10::optional<at::Tensor>& factor,
                              const NoiseArg& znoise) {
    auto a = masked_step_args("masked_affine_step", noise, x, init, init_noise, mask, sa, sb);
    const float* fp = rescale_factor("masked_affine_step", factor, noise, x);
    const auto nz = step_noise("masked_affine_step", znoise, x);
    auto out = at::empty_like(a.x);
    launch_cfg_affine_step(a.n.data_ptr(), a.nc, a.x.data_ptr(), out.data_ptr(), (float)g,
                           (float)ca, (float)cb, a.x.numel(), dtype_of(a.x), cur_stream(),
                           &a.blend, fp, nz.ptr());
    return out;
}

// [copies, 9, h, w] = [latents / scale (4), mask (1), masked-image latents (4)]
at::Tensor inpaint_unet_input(const at::Tensor& latents, const at::Tensor& mask,
                              const at::Tensor& masked, double scale, int64_t copies) {
    TORCH_CHECK(latents.is_cuda() && latents.dim() == 4 && latents.size(0) == 1 &&
                    latents.size(1) == 4,
                "inpaint_unet_input: latents must be CUDA [1,4,h,w]");
    const int64_t h = latents.size(2), w = latents.size(3);
    TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == latents.scalar_type() &&
                    mask.numel() == h * w,
                "inpaint_unet_input: mask must be [1,1,h,w] in the latents' dtype");
    TORCH_CHECK(masked.is_cuda() && masked.scalar_type() == latents.scalar_type() &&
                    masked.numel() == 4 * h * w,
                "inpaint_unet_input: masked latents must be [1,4,h,w] in the latents' dtype");
    TORCH_CHECK(copies == 1 || copies == 2, "inpaint_unet_input: copies must be 1 or 2");
    TORCH_CHECK(scale > 0, "inpaint_unet_input: scale must be positive");
    auto l = latents.contiguous(), m = mask.contiguous(), ml = masked.contiguous();
    auto out = at::empty({copies, 9, h, w}, l.options());
    launch_inpaint_unet_input(l.data_ptr(), m.data_ptr(), ml.data_ptr(), out.data_ptr(),
                              (float)scale, h * w, (int)copies, dtype_of(l), cur_stream());
    return out;
}

// q: [B,H,Lq,D]; k/v: [B,H,Lkv,D] or [B,H,NC,LC,D] (stale-KV chunks): checks
// and everything of FlashAttnParams but the output pointer
FlashAttnParams flash_params(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v) {
    TORCH_CHECK(q.is_cuda() && is_b16(q), "flash_attention: bf16 or fp16 only");
    TORCH_CHECK(k.scalar_type() == q.scalar_type(), "flash_attention: k must have q's dtype (",
                q.scalar_type(), "), got ", k.scalar_type());
    TORCH_CHECK(v.scalar_type() == q.scalar_type(), "flash_attention: v must have q's dtype (",
                q.scalar_type(), "), got ", v.scalar_type());
    const int Dh = (int)q.size(-1);
    TORCH_CHECK(q.dim() == 4 && Dh % 8 == 0 && Dh <= 160,
                "head_dim must be a multiple of 8 and <= 160");
    TORCH_CHECK(q.stride(-1) == 1 && k.stride(-1) == 1 && v.stride(-1) == 1,
                "innermost dim must be contiguous");
    const int B = (int)q.size(0), H = (int)q.size(1);
    const int64_t Lq = q.size(2);

    FlashAttnParams p{};
    p.q = reinterpret_cast<const uint16_t*>(q.data_ptr());
    p.B = B;
    p.H = H;
    p.Lq = Lq;
    p.q_sb = q.stride(0);
    p.q_sh = q.stride(1);
    p.q_sl = q.stride(2);
    p.Dh = Dh;
    p.scale = 1.0f / std::sqrt((float)Dh);

    auto set_kv = [&](const at::Tensor& t, const uint16_t*& ptr, int64_t& sb, int64_t& sh,
                      int64_t& sc, int64_t& sl, int64_t& NC, int64_t& LC) {
        TORCH_CHECK((int)t.size(-1) == Dh, "k/v head_dim mismatch");
        ptr = reinterpret_cast<const uint16_t*>(t.data_ptr());
        sb = t.stride(0);
        sh = t.stride(1);
        if (t.dim() == 4) {
            NC = 1;
            LC = t.size(2);
            sc = 0;
            sl = t.stride(2);
        } else {
            TORCH_CHECK(t.dim() == 5);
            NC = t.size(2);
            LC = t.size(3);
            sc = t.stride(2);
            sl = t.stride(3);
            // V staging reads 8-token windows assuming they never straddle a
            // chunk boundary
            TORCH_CHECK(NC == 1 || LC % 8 == 0, "chunk length must be a multiple of 8");
        }
        TORCH_CHECK(sl % 8 == 0 && sc % 8 == 0 && sh % 8 == 0 && sb % 8 == 0,
                    "KV strides must be 16B-aligned (multiples of 8 elements)");
    };
    int64_t nc2, lc2;
    set_kv(k, p.k, p.k_sb, p.k_sh, p.k_sc, p.k_sl, p.NC, p.LC);
    set_kv(v, p.v, p.v_sb, p.v_sh, p.v_sc, p.v_sl, nc2, lc2);
    TORCH_CHECK(nc2 == p.NC && lc2 == p.LC, "k/v shape mismatch");
    TORCH_CHECK(p.q_sl % 8 == 0 && p.q_sb % 8 == 0 && p.q_sh % 8 == 0);
    return p;
}

// 16-bit output [B,Lq,H,D] for p, seated in p.o
at::Tensor flash_out(FlashAttnLseParams& p, const at::Tensor& q) {
    auto o = at::empty({(long)p.B, (long)p.Lq, (long)p.H, (long)p.Dh}, q.options());
    p.o = reinterpret_cast<uint16_t*>(o.data_ptr());
    return o;
}

// one split, no log-sum-exp: the plain kernel -> logical [B,H,Lq,D]
at::Tensor flash_plain(FlashAttnLseParams p, const at::Tensor& q) {
    auto o = flash_out(p, q);
    launch_flash_attention(p, 1, dtype_of(q), cur_stream());
    return o.permute({0, 2, 1, 3});
}

at::Tensor flash_attention(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v) {
    return flash_plain({flash_params(q, k, v)}, q);
}

// A split-KV request: the params, S = the number of splits actually used
// (kv_splits clamped to the number of 128-token tiles) and the fp32 workspace
// shapes that go with it, o_part [S,B,Lq,H,D] and lse_part [S,B,H,Lq]
struct SplitKv {
    FlashAttnLseParams p;
    int S;
    std::array<int64_t, 5> o_part;
    std::array<int64_t, 4> lse_part;
};
SplitKv split_kv(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                 int64_t kv_splits) {
    TORCH_CHECK(kv_splits >= 1, "kv_splits must be >= 1");
    const FlashAttnLseParams p{flash_params(q, k, v)};
    const int S = flash_attention_num_splits(p.NC * p.LC, (int)std::min<int64_t>(kv_splits, 1 << 16));
    return {p, S, {S, p.B, p.Lq, p.H, p.Dh}, {S, p.B, p.H, p.Lq}};
}

// Split-KV partials into caller-owned buffers: o_part fp32 [S,B,Lq,H,D] and
// lse_part fp32 [S,B,H,Lq]; S is returned.
int64_t flash_attention_partial(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                                int64_t kv_splits, at::Tensor o_part, at::Tensor lse_part) {
    auto [p, S, o_shape, lse_shape] = split_kv(q, k, v, kv_splits);
    TORCH_CHECK(o_part.is_cuda() && o_part.scalar_type() == at::kFloat && o_part.is_contiguous() &&
                    o_part.sizes() == at::IntArrayRef(o_shape),
                "o_part must be contiguous fp32 [S,B,Lq,H,D] with S = ", S);
    TORCH_CHECK(lse_part.is_cuda() && lse_part.scalar_type() == at::kFloat &&
                    lse_part.is_contiguous() && lse_part.sizes() == at::IntArrayRef(lse_shape),
                "lse_part must be contiguous fp32 [S,B,H,Lq] with S = ", S);
    p.o_part = o_part.data_ptr<float>();
    p.lse = lse_part.data_ptr<float>();
    launch_flash_attention(p, S, dtype_of(q), cur_stream());
    return S;
}

at::Tensor merge_attention_into(const at::Tensor& o_parts, const at::Tensor& lse_parts,
                                at::ScalarType out_dtype,
                                const c10::optional<at::Tensor>& lse_out) {
    TORCH_CHECK(o_parts.is_cuda() && o_parts.dim() == 5 && o_parts.scalar_type() == at::kFloat &&
                    o_parts.is_contiguous(),
                "merge_attention: o_parts must be contiguous fp32 [S,B,Lq,H,D]");
    MergeAttnParams m{};
    m.S = (int)o_parts.size(0);
    m.B = (int)o_parts.size(1);
    m.Lq = o_parts.size(2);
    m.H = (int)o_parts.size(3);
    m.Dh = (int)o_parts.size(4);
    TORCH_CHECK(m.S >= 1 && m.Dh % 8 == 0, "merge_attention: S >= 1 and head_dim % 8 == 0");
    TORCH_CHECK(lse_parts.is_cuda() && lse_parts.scalar_type() == at::kFloat &&
                    lse_parts.is_contiguous() &&
                    lse_parts.sizes() ==
                        (at::IntArrayRef{(long)m.S, (long)m.B, (long)m.H, (long)m.Lq}),
                "merge_attention: lse_parts must be contiguous fp32 [S,B,H,Lq]");
    auto out = at::empty({(long)m.B, (long)m.Lq, (long)m.H, (long)m.Dh},
                         o_parts.options().dtype(out_dtype));
    m.o_parts = o_parts.data_ptr<float>();
    m.lse_parts = lse_parts.data_ptr<float>();
    m.out = out.data_ptr();
    m.out_dtype = dtype_of(out);
    if (lse_out.has_value()) m.lse = lse_out->data_ptr<float>();
    launch_merge_attention(m, cur_stream());
    return out;
}

// parts stacked on dim 0 -> (out [B,Lq,H,D], lse [B,H,Lq]). out is bf16 or
// fp32 by out_bf16 unless out_dtype names one of bf16 / fp16 / fp32.
std::vector<at::Tensor> merge_attention(const at::Tensor& o_parts, const at::Tensor& lse_parts,
                                        bool out_bf16,
                                        const c10::optional<at::ScalarType>& out_dtype) {
    const at::ScalarType dt = out_dtype.value_or(out_bf16 ? at::kBFloat16 : at::kFloat);
    TORCH_CHECK(dt == at::kBFloat16 || dt == at::kHalf || dt == at::kFloat,
                "merge_attention: out_dtype must be bf16, fp16 or fp32");
    TORCH_CHECK(lse_parts.dim() == 4, "merge_attention: lse_parts must be [S,B,H,Lq]");
    auto lse = at::empty({lse_parts.size(1), lse_parts.size(2), lse_parts.size(3)},
                         lse_parts.options());
    auto out = merge_attention_into(o_parts, lse_parts, dt, lse);
    return {out, lse};
}

// flash_attention with split-KV and an optional log-sum-exp output. Returns
// {out [B,H,Lq,D] (a view of [B,Lq,H,D])} or {out, lse [B,H,Lq] fp32}.
// kv_splits > 1 (after clamping to the tile count) runs the partial kernel
// over grid.z = S and then the merge kernel, on the current stream; the fp32
// workspace comes from the caching allocator (safe under graph capture).
std::vector<at::Tensor> flash_attention_ext(const at::Tensor& q, const at::Tensor& k,
                                            const at::Tensor& v, int64_t kv_splits,
                                            bool return_lse) {
    auto [p, S, o_shape, lse_shape] = split_kv(q, k, v, kv_splits);
    const auto f32 = q.options().dtype(at::kFloat);
    const long B = p.B, H = p.H, Lq = p.Lq;
    if (S == 1) {
        if (!return_lse) return {flash_plain(p, q)};
        auto o = flash_out(p, q);
        auto lse = at::empty({B, H, Lq}, f32);
        p.lse = lse.data_ptr<float>();
        launch_flash_attention(p, 1, dtype_of(q), cur_stream());
        return {o.permute({0, 2, 1, 3}), lse};
    }
    auto o_part = at::empty(o_shape, f32);
    auto lse_part = at::empty(lse_shape, f32);
    p.o_part = o_part.data_ptr<float>();
    p.lse = lse_part.data_ptr<float>();
    launch_flash_attention(p, S, dtype_of(q), cur_stream());
    // the merge writes the input dtype
    if (!return_lse)
        return {merge_attention_into(o_part, lse_part, q.scalar_type(), c10::nullopt)
                    .permute({0, 2, 1, 3})};
    auto lse = at::empty({B, H, Lq}, f32);
    auto o = merge_attention_into(o_part, lse_part, q.scalar_type(), lse);
    return {o.permute({0, 2, 1, 3}), lse};
}

at::Tensor conv3x3(const at::Tensor& x, const at::Tensor& wp,
                   const c10::optional<at::Tensor>& bias, int64_t cout, int64_t stride,
                   const c10::optional<at::Tensor>& top, const c10::optional<at::Tensor>& bot,
                   const c10::optional<at::Tensor>& residual,
                   const c10::optional<at::Tensor>& bias2, int64_t pad_lo) {
    TORCH_CHECK(x.is_cuda() && x.dim() == 4 && is_b16(x),
                "x must be CUDA bf16 or fp16 [B,Cin,H,W]");
    const auto dt = x.scalar_type();
    TORCH_CHECK(x.stride(3) == 1 && x.stride(2) == x.size(3), "x rows must be contiguous");
    TORCH_CHECK(wp.is_cuda() && wp.dim() == 5 && wp.is_contiguous() && wp.size(0) == 9 &&
                wp.size(3) == 64 && wp.size(4) == 8,
                "wp must be packed [9][KS][CT][64][8]");
    TORCH_CHECK(wp.scalar_type() == dt, "conv3x3: wp must have x's dtype (", dt, "), got ",
                wp.scalar_type());
    TORCH_CHECK(stride == 1 || stride == 2);
    const int B = (int)x.size(0), Cin = (int)x.size(1), H = (int)x.size(2), W = (int)x.size(3);
    TORCH_CHECK(pad_lo == 0 || pad_lo == 1, "conv3x3: pad_lo must be 0 or 1, got ", pad_lo);
    if (pad_lo == 0) {
        // bottom/right-only padding (AutoencoderKL downsample)
        TORCH_CHECK(stride == 2, "conv3x3: pad_lo=0 needs stride 2, got ", stride);
        TORCH_CHECK(!top.has_value(), "conv3x3: pad_lo=0 takes no top halo row");
        TORCH_CHECK(H >= 2 && W >= 2, "conv3x3: pad_lo=0 needs H, W >= 2, got ", H, "x", W);
    }
    const int Ho = pad_lo ? (H - 1) / (int)stride + 1 : (H - 2) / 2 + 1;
    const int Wo = pad_lo ? (W - 1) / (int)stride + 1 : (W - 2) / 2 + 1;

    Conv3x3Params p{};
    p.x = reinterpret_cast<const uint16_t*>(x.data_ptr());
    p.wp = reinterpret_cast<const uint16_t*>(wp.data_ptr());
    p.B = B;
    p.Cin = Cin;
    p.Cout = (int)cout;
    p.H = H;
    p.W = W;
    p.Ho = Ho;
    p.Wo = Wo;
    p.KS = (int)wp.size(1);
    p.CT = (int)wp.size(2);
    p.pad_lo = (int)pad_lo;
    TORCH_CHECK(p.KS * 16 >= Cin && p.CT * 32 >= cout, "packed weight too small");
    p.x_sb = x.stride(0);
    p.x_sc = x.stride(1);
    if (const char* dbg = getenv("DFA_CONV_DEBUG")) p.debug = atoi(dbg);
    at::Tensor bias_c;
    if (bias.has_value()) {
        bias_c = b16_param(*bias, x, "conv3x3", "bias");
        TORCH_CHECK(bias_c.numel() == cout);
        p.bias = reinterpret_cast<const uint16_t*>(bias_c.data_ptr());
    }
    auto set_halo = [&](const c10::optional<at::Tensor>& h, const uint16_t*& ptr, int64_t& sb,
                        int64_t& sc) {
        if (!h.has_value()) return;
        const at::Tensor& t = *h;
        TORCH_CHECK(t.scalar_type() == dt, "conv3x3: top/bot halo must have x's dtype (", dt,
                    "), got ", t.scalar_type());
        TORCH_CHECK(t.is_cuda() && t.stride(-1) == 1 && t.size(-1) == W && t.size(1) == Cin,
                    "halo must be [B,Cin,(1,)W] with contiguous rows");
        ptr = reinterpret_cast<const uint16_t*>(t.data_ptr());
        sb = t.stride(0);
        sc = t.stride(1);
    };
    set_halo(top, p.top, p.t_sb, p.t_sc);
    set_halo(bot, p.bot, p.b_sb, p.b_sc);
    at::Tensor b2_c;
    if (bias2.has_value()) {
        b2_c = b16_param(*bias2, x, "conv3x3", "bias2");
        TORCH_CHECK(b2_c.numel() == (int64_t)B * cout, "bias2 must be [B, Cout]");
        p.bias2 = reinterpret_cast<const uint16_t*>(b2_c.data_ptr());
    }
    at::Tensor res_c;
    if (residual.has_value()) {
        res_c = residual->contiguous();
        TORCH_CHECK(res_c.scalar_type() == dt, "conv3x3: residual must have x's dtype (", dt,
                    "), got ", res_c.scalar_type());
        TORCH_CHECK(res_c.sizes() == (at::IntArrayRef{(long)B, (long)cout, (long)Ho, (long)Wo}),
                    "residual must be [B,Cout,Ho,Wo]");
        p.residual = reinterpret_cast<const uint16_t*>(res_c.data_ptr());
    }

    auto o = at::empty({(long)B, (long)cout, (long)Ho, (long)Wo}, x.options());
    p.o = reinterpret_cast<uint16_t*>(o.data_ptr());
    launch_conv3x3(p, (int)stride, dtype_of(x), cur_stream());
    return o;
}

// n / nc: the contiguous noise and its cond half (null: no CFG pair, masked
// only); xc contiguous. -> (prev, x0 fp32)
std::vector<at::Tensor> dpm_step(const at::Tensor& n, const void* nc, const at::Tensor& xc,
                                 const c10::optional<at::Tensor>& x0_prev, double g, double ca,
                                 double cb, double cc, double cx, double ce,
                                 const MaskBlend* blend, const float* factor,
                                 const StepNoise* noise) {
    const void* pp = nullptr;
    at::Tensor p;
    if (x0_prev.has_value()) {
        p = x0_prev->contiguous();
        TORCH_CHECK(p.is_cuda() && p.numel() == xc.numel() && p.scalar_type() == at::kFloat,
                    "x0_prev must be the fp32 state from the previous cfg_dpm_step");
        pp = p.data_ptr();
    }
    auto out = at::empty_like(xc);
    auto x0 = at::empty_like(xc, xc.options().dtype(at::kFloat));
    launch_cfg_dpm_step(n.data_ptr(), nc, xc.data_ptr(), pp, out.data_ptr(), x0.data_ptr(),
                        (float)g, (float)ca, (float)cb, (float)cc, (float)cx, (float)ce,
                        xc.numel(), dtype_of(xc), cur_stream(), blend, factor, noise);
    return {out, x0};
}

std::vector<at::Tensor> cfg_dpm_step(const at::Tensor& noise, const at::Tensor& x,
                                     const c10::optional<at::Tensor>& x0_prev, double g,
                                     double ca, double cb, double cc, double cx, double ce,
                                     const c10::optional<at::Tensor>& factor,
                                     const NoiseArg& znoise) {
    TORCH_CHECK(noise.is_cuda() && noise.dim() >= 1);
    auto n = noise.contiguous();
    auto xc = x.contiguous();
    const auto nz = step_noise("cfg_dpm_step", znoise, x);
    const void* nc = cond_half("cfg_dpm_step", n, xc, nz.given);
    return dpm_step(n, nc, xc, x0_prev, g, ca, cb, cc, cx, ce, nullptr,
                    rescale_factor("cfg_dpm_step", factor, noise, x), nz.ptr());
}

// cfg_dpm_step with the inpaint blend on prev; x0 is the unmasked step's
std::vector<at::Tensor> masked_dpm_step(const at::Tensor& noise, const at::Tensor& x,
                                        const c10::optional<at::Tensor>& x0_prev,
                                        const at::Tensor& init, const at::Tensor& init_noise,
                                        const at::Tensor& mask, double g, double ca, double cb,
                                        double cc, double cx, double ce, double sa, double sb,
                                        const c10::optional<at::Tensor>& factor,
                                        const NoiseArg& znoise) {
    auto a = masked_step_args("masked_dpm_step", noise, x, init, init_noise, mask, sa, sb);
    const auto nz = step_noise("masked_dpm_step", znoise, x);
    return dpm_step(a.n, a.nc, a.x, x0_prev, g, ca, cb, cc, cx, ce, &a.blend,
                    rescale_factor("masked_dpm_step", factor, noise, x), nz.ptr());
}

at::Tensor layer_norm(const at::Tensor& x_, const at::Tensor& w_, const at::Tensor& b_,
                      double eps) {
    TORCH_CHECK(x_.is_cuda() && is_b16(x_), "layer_norm: bf16 or fp16 only");
    auto x = x_.contiguous();
    const int C = (int)x.size(-1);
    TORCH_CHECK(C % 8 == 0 && C <= 2048, "layer_norm kernel: C % 8 == 0 and C <= 2048");
    auto w = b16_param(w_, x, "layer_norm", "weight");
    auto b = b16_param(b_, x, "layer_norm", "bias");
    auto y = at::empty_like(x);
    launch_layer_norm(x.data_ptr(), nullptr, y.data_ptr(), nullptr, w.data_ptr(), b.data_ptr(),
                      (float)eps, x.numel() / C, C, dtype_of(x), cur_stream());
    return y;
}

std::vector<at::Tensor> add_layer_norm(const at::Tensor& x_, const at::Tensor& res_,
                                       const at::Tensor& w_, const at::Tensor& b_, double eps) {
    TORCH_CHECK(x_.is_cuda() && is_b16(x_), "add_layer_norm: bf16 or fp16 only");
    auto x = x_.contiguous();
    auto res = res_.contiguous();
    TORCH_CHECK(res.scalar_type() == x.scalar_type(), "add_layer_norm: res must have x's dtype (",
                x.scalar_type(), "), got ", res.scalar_type());
    TORCH_CHECK(res.sizes() == x.sizes());
    const int C = (int)x.size(-1);
    TORCH_CHECK(C % 8 == 0 && C <= 2048, "add_layer_norm kernel: C % 8 == 0 and C <= 2048");
    auto w = b16_param(w_, x, "add_layer_norm", "weight");
    auto b = b16_param(b_, x, "add_layer_norm", "bias");
    auto y = at::empty_like(x);
    auto sum = at::empty_like(x);
    launch_layer_norm(x.data_ptr(), res.data_ptr(), y.data_ptr(), sum.data_ptr(), w.data_ptr(),
                      b.data_ptr(), (float)eps, x.numel() / C, C, dtype_of(x), cur_stream());
    return {sum, y};
}

at::Tensor vae_attention(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v) {
    TORCH_CHECK(q.is_cuda() && q.dim() == 3 && q.size(-1) == 512 && is_b16(q),
                "vae_attention: bf16 or fp16 [B, L, 512] only");
    TORCH_CHECK(k.scalar_type() == q.scalar_type(), "vae_attention: k must have q's dtype (",
                q.scalar_type(), "), got ", k.scalar_type());
    TORCH_CHECK(v.scalar_type() == q.scalar_type(), "vae_attention: v must have q's dtype (",
                q.scalar_type(), "), got ", v.scalar_type());
    auto qc = q.contiguous(), kc = k.contiguous(), vc = v.contiguous();
    TORCH_CHECK(kc.sizes() == qc.sizes() && vc.sizes() == qc.sizes());
    VaeAttnParams p{};
    p.q = reinterpret_cast<const uint16_t*>(qc.data_ptr());
    p.k = reinterpret_cast<const uint16_t*>(kc.data_ptr());
    p.v = reinterpret_cast<const uint16_t*>(vc.data_ptr());
    p.B = (int)qc.size(0);
    p.L = qc.size(1);
    p.sb = qc.stride(0);
    p.scale = 1.0f / std::sqrt(512.0f);
    auto o = at::empty_like(qc);
    p.o = reinterpret_cast<uint16_t*>(o.data_ptr());
    launch_vae_attention(p, dtype_of(q), cur_stream());
    return o;
}

std::vector<at::Tensor> mfma_probe(const at::Tensor& a, const at::Tensor& b) {
    TORCH_CHECK(a.is_cuda() && a.sizes() == (at::IntArrayRef{64, 8}));
    auto af = a.to(at::kFloat).contiguous(), bf = b.to(at::kFloat).contiguous();
    auto d = at::zeros({64, 4}, af.options());
    launch_mfma_probe(af.data_ptr<float>(), bf.data_ptr<float>(), d.data_ptr<float>(),
                      cur_stream());
    return {d};
}

std::vector<at::Tensor> mfma_probe32(const at::Tensor& a, const at::Tensor& b) {
    TORCH_CHECK(a.is_cuda() && a.sizes() == (at::IntArrayRef{64, 8}));
    auto af = a.to(at::kFloat).contiguous(), bf = b.to(at::kFloat).contiguous();
    auto d = at::zeros({64, 16}, af.options());
    launch_mfma_probe32(af.data_ptr<float>(), bf.data_ptr<float>(), d.data_ptr<float>(),
                        cur_stream());
    return {d};
}
}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("group_norm_stats", &group_norm_stats, "per-group moments [2,N,G,1,1,1]");
    m.def("group_norm_apply", &group_norm_apply,
          "normalize+affine(+SiLU) from given moments; tokens: write [N, HW, C]",
          pybind11::arg("x"), pybind11::arg("mean"), pybind11::arg("meansq"),
          pybind11::arg("weight"), pybind11::arg("bias"), pybind11::arg("eps"),
          pybind11::arg("silu"), pybind11::arg("tokens") = false);
    m.def("group_norm_silu", &group_norm_silu, "fused GroupNorm(+SiLU); tokens: write [N, HW, C]",
          pybind11::arg("x"), pybind11::arg("num_groups"), pybind11::arg("weight"),
          pybind11::arg("bias"), pybind11::arg("eps"), pybind11::arg("silu"),
          pybind11::arg("tokens") = false);
    m.def("tokens_add_nchw", &tokens_add_nchw,
          "y [N, HW, C] + residual [N, C, H, W] -> [N, C, H, W] (transposing residual add)");
    m.def("geglu", &geglu, "a * gelu(gate) over last-dim halves");
    m.def("gn_merge_stats", &gn_merge_stats,
          "merge stale peer GN moments with fresh local ones (one launch)");
    m.def("guidance_rescale_factor", &guidance_rescale_factor,
          "guidance_rescale factor phi*std(cond)/std(cfg) + 1 - phi of a CFG pair -> fp32 [1]");
    m.def("cfg_affine_step", &cfg_affine_step,
          "fused CFG combine + affine scheduler update; factor: the guidance_rescale factor",
          pybind11::arg("noise"), pybind11::arg("x"), pybind11::arg("g"), pybind11::arg("ca"),
          pybind11::arg("cb"), pybind11::arg("factor") = pybind11::none(),
          pybind11::arg("step_noise") = pybind11::none());
    m.def("philox_normal", &philox_normal,
          "Philox4x32-10 Box-Muller normals of elements offset.. of (seed, draw) -> fp32 [numel]",
          pybind11::arg("numel"), pybind11::arg("seed"), pybind11::arg("draw"),
          pybind11::arg("offset") = 0, pybind11::arg("device_index") = 0);
    m.def("flash_attention", &flash_attention, "bf16/fp16 flash attention (chunked stale KV)");
    m.def("flash_attention_ext", &flash_attention_ext,
          "flash attention with split-KV and optional log-sum-exp -> [out] or [out, lse]",
          pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"),
          pybind11::arg("kv_splits") = 1, pybind11::arg("return_lse") = false);
    m.def("flash_attention_partial", &flash_attention_partial,
          "split-KV partials into caller buffers (o_part fp32 [S,B,Lq,H,D], lse_part [S,B,H,Lq])");
    m.def("merge_attention", &merge_attention,
          "merge fp32 attention partials by their log-sum-exp -> [out, lse]",
          pybind11::arg("o_parts"), pybind11::arg("lse_parts"), pybind11::arg("out_bf16") = true,
          pybind11::arg("out_dtype") = pybind11::none());
    m.def("cfg_dpm_step", &cfg_dpm_step, "fused CFG + DPM-Solver++(2M) update -> (prev, x0)",
          pybind11::arg("noise"), pybind11::arg("x"), pybind11::arg("x0_prev"),
          pybind11::arg("g"), pybind11::arg("ca"), pybind11::arg("cb"), pybind11::arg("cc"),
          pybind11::arg("cx"), pybind11::arg("ce"), pybind11::arg("factor") = pybind11::none(),
          pybind11::arg("step_noise") = pybind11::none());
    m.def("masked_affine_step", &masked_affine_step,
          "inpaint: (CFG +) affine scheduler update blended with the re-noised init latents",
          pybind11::arg("noise"), pybind11::arg("x"), pybind11::arg("init"),
          pybind11::arg("init_noise"), pybind11::arg("mask"), pybind11::arg("g"),
          pybind11::arg("ca"), pybind11::arg("cb"), pybind11::arg("sa"), pybind11::arg("sb"),
          pybind11::arg("factor") = pybind11::none(), pybind11::arg("step_noise") = pybind11::none());
    m.def("masked_dpm_step", &masked_dpm_step,
          "inpaint: (CFG +) DPM-Solver++(2M) update, prev blended -> (prev, x0)",
          pybind11::arg("noise"), pybind11::arg("x"), pybind11::arg("x0_prev"),
          pybind11::arg("init"), pybind11::arg("init_noise"), pybind11::arg("mask"),
          pybind11::arg("g"), pybind11::arg("ca"), pybind11::arg("cb"), pybind11::arg("cc"),
          pybind11::arg("cx"), pybind11::arg("ce"), pybind11::arg("sa"), pybind11::arg("sb"),
          pybind11::arg("factor") = pybind11::none(), pybind11::arg("step_noise") = pybind11::none());
    m.def("inpaint_unet_input", &inpaint_unet_input,
          "inpaint U-Net input [copies,9,h,w] = [latents / scale, mask, masked-image latents]");
    m.def("layer_norm", &layer_norm, "bf16/fp16 fused LayerNorm");
    m.def("add_layer_norm", &add_layer_norm, "bf16/fp16 fused residual-add + LayerNorm -> (sum, y)");
    m.def("vae_attention", &vae_attention, "bf16/fp16 single-head d=512 VAE mid attention");
    m.def("conv3x3", &conv3x3,
          "bf16/fp16 implicit-GEMM 3x3 conv, stride 1/2, in-place halo rows; pad_lo=0 "
          "(stride 2) pads bottom/right only",
          pybind11::arg("x"), pybind11::arg("wp"), pybind11::arg("bias"), pybind11::arg("cout"), pybind11::arg("stride"),
          pybind11::arg("top"), pybind11::arg("bot"), pybind11::arg("residual"), pybind11::arg("bias2"),
          pybind11::arg("pad_lo") = 1);
    m.def("mfma_probe", &mfma_probe, "dump mfma_f32_16x16x32_bf16 fragment mapping");
    m.def("mfma_probe32", &mfma_probe32, "dump mfma_f32_32x32x16_bf16 fragment mapping");
}
