// C-ABI dispatch layer of libunetmi: validates arguments and picks the MFMA fast path or the
// generic kernel.  See include/unetmi.h for the contract of every entry point.
#include "kernels.h"
#include <stdio.h>
#include <stdlib.h>

static ConvFwdProblem fwd_problem(int N, int H, int W, int Ci, int Co, int R, int S, int stride, int pad, int Ho, int Wo, int ldx,
                                  int ldy, int in_dtype, int out_dtype, int flags, bool has_tx, bool has_bias, bool has_stats) {
    return ConvFwdProblem{N, H, W, Ci, Co, R, S, stride, pad, Ho, Wo, ldx, ldy, in_dtype, out_dtype, flags, has_tx, has_bias, has_stats};
}
// a 3x3 / stride 1 / pad 1 problem without bias or statistics: "is this on the 3x3 matrix-core kernel"
static ConvFwdProblem fwd_problem_3x3(int N, int H, int W, int Ci, int Co, int ldx, int ldy, int dtype, bool has_tx) {
    return fwd_problem(N, H, W, Ci, Co, 3, 3, 1, 1, H, W, ldx, ldy, dtype, dtype, 0, has_tx, false, false);
}

extern "C" int umi_version(void) { return 1; }
extern "C" const char* umi_arch(void) { return "gfx950"; }

// A ViT-block linear with its elementwise tail in the GEMM epilogue (reference vit_seg_modeling.py:113-119 Mlp, :177-187 Block):
//   epi 1: y = x W + b,  y2 = dropout(GELU(y)),  mask          (fc1; y stays for the GELU backward)
//   epi 2: y = dropout(x W + b) + aux,           mask          (fc2 / attention output projection + residual)
// x [M, Ci], y / y2 / aux [M, Co] fp16 rows (ld in elements), wp8 = umi_pack_kn8 of the [Co, Ci] weight, mask = M * Co bytes.
// Same values as umi_conv_fwd followed by umi_dropout_fused (same random stream and roundings).  UMI_ERR_UNSUPPORTED where
// the pointwise matrix-core kernel does not apply: run the two calls instead.
extern "C" int umi_linear_fused(const void* x, int ldx, const void* wp8, const float* bias, void* y, int ldy, long M, int Ci,
                                int Co, int epi, float p, unsigned seed, const unsigned* seed_dev, void* mask, const void* aux,
                                int ldaux, void* y2, int ldy2, int dtype, umi_stream_t stream) {
    if (!x || !wp8 || !y || !mask || M <= 0 || M >= (1L << 31) || Ci <= 0 || Co <= 0 || !(p >= 0.f && p <= 1.f)) return UMI_ERR_BADARG;
    if (epi != 1 && epi != 2) return UMI_ERR_BADARG;
    if ((epi == 1 && (!y2 || ldy2 % 8)) || (epi == 2 && (!aux || ldaux % 8))) return UMI_ERR_BADARG;
    const ConvFwdProblem pr = fwd_problem(1, 1, (int)M, Ci, Co, 1, 1, 1, 0, 1, (int)M, ldx, ldy, dtype, dtype, 0, false, bias != nullptr, false);
    if (umi_conv_fwd_path(pr) != FWD_MFMA1X1) return UMI_ERR_UNSUPPORTED;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)wp8 | (uintptr_t)y2 | (uintptr_t)aux) & 15 || ((uintptr_t)mask & 7)) return UMI_ERR_UNSUPPORTED;
    const UmiLinearEpi e{epi, p, seed, seed_dev, mask, aux, ldaux, y2, ldy2, nullptr, nullptr, nullptr};
    return umi_conv1x1_mfma(pr, x, nullptr, wp8, bias, y, 0, 0, 1, (int)M, (hipStream_t)stream, &e);
}

// A data gradient on the pointwise / tap-gather matrix-core kernel (ConvTranspose2d(2,2)'s = a stride-2 2x2 conv over d(up),
// reference Model.py:56-57 under autograd; plain 1x1 convs; UMI_CONV_DGRAD_STRIDED) that also emits stage 1 of the BatchNorm(+ReLU)
// backward of the layer whose activated output the gradient belongs to: part[rows][2][Co], rows = umi_conv_gather_bnred_rows(...)
// (0 = not on that kernel: run umi_conv_fwd and umi_bn_bwd_reduce).  No transform, no bias, no accumulation.
extern "C" int umi_conv_gather_bnred_rows(int N, int H, int W, int Ci, int Co, int R, int S, int stride, int pad, int Ho, int Wo,
                                          int ldx, int ldy, int dtype, int flags) {
    if (flags & (UMI_CONV_UPSAMPLE2 | UMI_CONV_ACCUMULATE | UMI_CONV_FORCE_GENERIC)) return 0;
    const ConvFwdProblem p = fwd_problem(N, H, W, Ci, Co, R, S, stride, pad, Ho, Wo, ldx, ldy, dtype, dtype, flags, false, false, false);
    // (a 3x3 / stride-1 data gradient has umi_conv_dgrad_bnred, with UMI_CONV_DGRAD_STRIDED set as without)
    if (umi_conv_fwd_path(p) != FWD_MFMA1X1 || umi_conv3x3_mfma_ok(p)) return 0;
    return umi_conv1x1_bnred_rows((long)N * Ho * Wo, Co);
}
extern "C" int umi_conv_gather_bnred(const void* x, int ldx, const void* wp8, void* y, int ldy, const void* ybn, int ldybn,
                                     const void* txbn, const float* rstd, float* part, int N, int H, int W, int Ci, int Co, int R,
                                     int S, int stride, int pad, int Ho, int Wo, int dtype, int flags, umi_stream_t stream) {
    if (!x || !wp8 || !y || !ybn || !txbn || !rstd || !part || N <= 0 || H <= 0 || W <= 0) return UMI_ERR_BADARG;
    if (umi_conv_gather_bnred_rows(N, H, W, Ci, Co, R, S, stride, pad, Ho, Wo, ldx, ldy, dtype, flags) <= 0 || ldybn % 8 || ldybn < Co)
        return UMI_ERR_UNSUPPORTED;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)wp8 | (uintptr_t)ybn) & 15) return UMI_ERR_BADARG;
    const UmiLinearEpi e{3, 0.f, 0u, nullptr, nullptr, ybn, ldybn, nullptr, 0, txbn, rstd, part};
    const ConvFwdProblem p = fwd_problem(N, H, W, Ci, Co, R, S, stride, pad, Ho, Wo, ldx, ldy, dtype, dtype, flags, false, false, false);
    return umi_conv1x1_mfma(p, x, nullptr, wp8, nullptr, y, 0, 0, Ho, Wo, (hipStream_t)stream, &e);
}

extern "C" int umi_conv_fwd_plan(int N, int H, int W, int Ci, int Co, int R, int S, int stride, int pad, int ldx,
                                 int ldy, int in_dtype, int out_dtype, int flags, int has_bias, int* layout,
                                 int* stat_rows) {
    if (N <= 0 || H <= 0 || W <= 0 || Ci <= 0 || Co <= 0 || R <= 0 || S <= 0 || stride <= 0) return UMI_ERR_BADARG;
    const bool ups = flags & UMI_CONV_UPSAMPLE2;
    const int Ho = ups ? H : (H + 2 * pad - R) / stride + 1, Wo = ups ? W : (W + 2 * pad - S) / stride + 1;
    // the plan is asked before the call's pointers exist: it answers for a call that wants statistics (the rows are only read
    // then; the packing does not depend on it)
    const ConvFwdPath path = umi_conv_fwd_path(fwd_problem(N, H, W, Ci, Co, R, S, stride, pad, Ho, Wo, ldx, ldy, in_dtype, out_dtype,
                                                           flags, false, has_bias != 0, true));
    if ((flags & UMI_CONV_ACCUMULATE) && path != FWD_MFMA1X1) return UMI_ERR_UNSUPPORTED;
    if (layout) *layout = (path == FWD_MFMA3X3 || path == FWD_MFMA1X1) ? 1 : 0;      // (the fp32 matrix-core kernels read layout 0)
    if (stat_rows)
        *stat_rows = path == FWD_MFMA3X3_F32 ? umi_conv3x3_f32_mfma_stat_rows(N, H, W)
                     : path == FWD_GEMM_F32 ? umi_gemm_f32_mfma_stat_rows((long)N * H * W)
                     : path == FWD_CONVT_F32 ? 0                      // it writes no statistics
                     : path == FWD_MFMA3X3 ? umi_conv3x3_mfma_stat_rows(N, H, W, Co)
                     : path == FWD_STEM  ? umi_stem_stat_rows(N, H, W)
                     : path == FWD_HEAD  ? umi_head_stat_rows((long)N * H * W, Ci)
                                         : umi_cdiv((long)N * Ho * Wo, 64);
    return UMI_OK;
}

// 3x3 / stride 1 / pad 1 data gradient (x = dy, Ci = the forward conv's Co, weights rotated + transposed as for umi_conv_fwd)
// fused with stage 1 of the BatchNorm+ReLU backward of the layer whose activated output the gradient belongs to:
// part[rows][2][Co] <- per-tile sums of dz and dz*xhat (rows = umi_conv_fwd_plan's stat_rows for this problem).
// UMI_ERR_UNSUPPORTED when the shape is not on the MFMA path: the caller then runs the separate kernels.
extern "C" int umi_conv_dgrad_bnred(const void* dy, int lddy, const void* wp8, void* da, int ldda, const void* ybn, int ldybn,
                                    const void* txbn, const float* rstd, float* part, int N, int H, int W, int Ci, int Co,
                                    int dtype, umi_stream_t stream) {
    if (!dy || !wp8 || !da || !ybn || !txbn || !rstd || !part || N <= 0 || H <= 0 || W <= 0) return UMI_ERR_BADARG;
    const ConvFwdProblem p = fwd_problem_3x3(N, H, W, Ci, Co, lddy, ldda, dtype, false);
    if (umi_conv_fwd_path(p) != FWD_MFMA3X3 || ldybn % 8 || ldybn < Co) return UMI_ERR_UNSUPPORTED;
    if (((uintptr_t)dy | (uintptr_t)da | (uintptr_t)wp8 | (uintptr_t)ybn) & 15) return UMI_ERR_BADARG;
    return umi_conv3x3_mfma_bnred(p, dy, wp8, da, ybn, ldybn, txbn, rstd, part, (hipStream_t)stream);
}

// The same fusion for the data gradient of a narrow pointwise conv (the segmentation head `OutConv`, reference Model.py:89-93:
// Ci <= 8 logit channels -> Co feature channels): da = dl * W^T plus stage 1 of the BatchNorm+ReLU backward of the layer whose
// activated output feeds the head.  rows = umi_head_dgrad_bnred_rows(P, Co).  wp = the generic [1][Ci][Co] fp16 packing.
static bool head_dgrad_ok(int Ci, int Co, int ldda, int dtype) {       // (the predicate reads no pixel counts and no ldx)
    return umi_smallk_fwd_ok(fwd_problem(1, 1, 1, Ci, Co, 1, 1, 1, 0, 1, 1, Ci, ldda, dtype, dtype, 0, false, false, false));
}
extern "C" int umi_head_dgrad_bnred_rows(long P, int Ci, int Co, int ldda, int dtype) {
    if (!head_dgrad_ok(Ci, Co, ldda, dtype)) return 0;
    return umi_smallk_bnred_rows(P, Co);
}
extern "C" int umi_head_dgrad_bnred(const void* dl, int lddl, const void* wp, void* da, int ldda, const void* ybn, int ldybn,
                                    const void* txbn, const float* rstd, float* part, long P, int Ci, int Co, int dtype,
                                    umi_stream_t stream) {
    if (!dl || !wp || !da || !ybn || !txbn || !rstd || !part || P <= 0) return UMI_ERR_BADARG;
    if (!head_dgrad_ok(Ci, Co, ldda, dtype) || ldybn % 8 || ldybn < Co || lddl < Ci) return UMI_ERR_UNSUPPORTED;
    return umi_smallk_fwd_bnred(dl, lddl, wp, da, ldda, ybn, ldybn, txbn, rstd, part, P, Ci, Co, (hipStream_t)stream);
}
// ... and the head's WEIGHT gradient as well (reference Model.py:89-93 under autograd: dW[k][c] = sum_p act(ybn)[p][c] * dl[p][k]; the
// head's input is the activated ybn): dW[k * s_co + c * s_ci] <- out_scale * that.  ws: umi_head_bwd_fused_ws_bytes(P, Ci, Co).
extern "C" size_t umi_head_bwd_fused_ws_bytes(long P, int Ci, int Co) {
    return (size_t)umi_smallk_bnred_rows(P, Co) * Co * Ci * sizeof(float);
}
extern "C" int umi_head_bwd_fused(const void* dl, int lddl, const void* wp, void* da, int ldda, const void* ybn, int ldybn,
                                  const void* txbn, const float* rstd, float* part, float* dW, long s_co, long s_ci, float out_scale,
                                  void* ws, size_t ws_bytes, long P, int Ci, int Co, int dtype, umi_stream_t stream) {
    if (!dl || !wp || !da || !ybn || !txbn || !rstd || !part || !dW || !ws || P <= 0) return UMI_ERR_BADARG;
    // (Co > 256: the weight-gradient rows of a workgroup no longer fit its LDS)
    if (!head_dgrad_ok(Ci, Co, ldda, dtype) || Co > 256 || ldybn % 8 || ldybn < Co || lddl < Ci) return UMI_ERR_UNSUPPORTED;
    return umi_smallk_fwd_bnred(dl, lddl, wp, da, ldda, ybn, ldybn, txbn, rstd, part, P, Ci, Co, (hipStream_t)stream, dW, s_co, s_ci,
                                out_scale, ws, ws_bytes);
}

// Inference form of conv3x3 + BatchNorm + ReLU (reference Model.py:15-22 under model.eval(), test_mc3serousv5.py:877-887):
// y = max(out_tx.scale * conv(tx(x), w) + out_tx.shift, out_tx.lo) stored activated, no statistics.  UMI_ERR_UNSUPPORTED
// when the shape is not on the matrix-core path (the caller then uses umi_conv_fwd and the consumer-side transform).
extern "C" int umi_conv3x3_fwd_act(const void* x, int ldx, const void* tx, const void* wp8, const void* out_tx, void* y, int ldy,
                                   int N, int H, int W, int Ci, int Co, int dtype, umi_stream_t stream) {
    if (!x || !wp8 || !out_tx || !y || N <= 0 || H <= 0 || W <= 0 || ldx < Ci || ldy < Co) return UMI_ERR_BADARG;
    const ConvFwdProblem p = fwd_problem_3x3(N, H, W, Ci, Co, ldx, ldy, dtype, tx != nullptr);
    if (umi_conv_fwd_path(p) != FWD_MFMA3X3) return UMI_ERR_UNSUPPORTED;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)wp8 | (uintptr_t)out_tx) & 15) return UMI_ERR_BADARG;
    return umi_conv3x3_mfma_act(p, x, tx, wp8, out_tx, y, (hipStream_t)stream);
}

// BatchNorm batch statistics of a stored fp16 tensor as partial rows part[rows][2][C] (sum, sum of squares) for umi_bn_finalize:
// for producers without a statistics epilogue (the pointwise MFMA convolution).  rows = umi_bn_stats_rows(M, C) (0: unsupported).
extern "C" int umi_bn_stats_rows(long M, int C) { return umi_colsum_rows_f16v(M, C); }
extern "C" int umi_bn_stats(const void* x, int ldx, float* part, long M, int C, int dtype, umi_stream_t stream) {
    if (!x || !part || M <= 0 || C <= 0 || ldx < C) return UMI_ERR_BADARG;
    if (dtype != UMI_F16 || !umi_bn_stats_f16v(x, ldx, part, M, C, (hipStream_t)stream)) return UMI_ERR_UNSUPPORTED;
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

// MaxPool2d(2) backward into `da` + stage 1 of the BatchNorm backward of the pooled layer (x = its raw output): only when
// this is the last contribution to `da`.  *rows receives the partial rows written (part[rows][2][C]).
extern "C" int umi_pool2_bwd_bnred(const void* dpool, int lddp, const void* x, int ldx, const void* tx, const float* rstd,
                                   void* da, int ldda, int accumulate, float* part, int N, int H, int W, int C, int dtype,
                                   umi_stream_t stream) {
    if (!dpool || !x || !tx || !rstd || !da || !part || N <= 0 || H <= 0 || W <= 0 || C <= 0) return UMI_ERR_BADARG;
    if (dtype != UMI_F16) return UMI_ERR_UNSUPPORTED;
    if (!umi_pool2_bwd_bnred_f16v(dpool, lddp, x, ldx, tx, rstd, da, ldda, accumulate, part, N, H, W, C, (hipStream_t)stream))
        return UMI_ERR_UNSUPPORTED;
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
extern "C" int umi_pool2_bwd_bnred_stat_rows(int N, int H, int W, int C) { return umi_pool2_bwd_bnred_rows(N, H, W, C); }

extern "C" int umi_bn_bwd_from_partials(const float* part, int rows, int C, float* sum_dz, float* sum_dzx, umi_stream_t stream) {
    if (!part || !sum_dz || !sum_dzx || rows <= 0 || C <= 0) return UMI_ERR_BADARG;
    umi_launch_reduce_rows2(part, rows, C, sum_dz, sum_dzx, 1.f, (hipStream_t)stream);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

// UMI_TRACE_GENERIC=1: report every conv that lands on the generic (non-MFMA) kernels -- a tuning aid, off by default
static bool trace_generic() {
    static const bool on = [] { const char* e = getenv("UMI_TRACE_GENERIC"); return e && e[0] == '1'; }();
    return on;
}
#define UMI_TRACE(kind)                                                                                                  \
    if (trace_generic())                                                                                                 \
        fprintf(stderr, "[umi generic %s] N=%d H=%d W=%d Ci=%d Co=%d R=%d stride=%d pad=%d flags=%d\n", kind, N, H, W, Ci, Co, R, \
                stride, pad, flags)

extern "C" int umi_conv_fwd(const void* x, int ldx, const void* tx, const void* wp, const float* bias, void* y, int ldy,
                            float* stat_part, int N, int H, int W, int Ci, int Co, int R, int S, int stride, int pad,
                            int Ho, int Wo, int off_h, int off_w, int out_H, int out_W, int in_dtype, int out_dtype,
                            int flags, umi_stream_t stream) {
    if (!x || !wp || !y || N <= 0 || H <= 0 || W <= 0 || Ci <= 0 || Co <= 0 || R <= 0 || S <= 0 || stride <= 0 ||
        Ho <= 0 || Wo <= 0 || ldx < Ci || ldy < Co || out_H <= 0 || out_W <= 0)
        return UMI_ERR_BADARG;
    ConvFwdProblem p = fwd_problem(N, H, W, Ci, Co, R, S, stride, pad, Ho, Wo, ldx, ldy, in_dtype, out_dtype, flags,
                                   tx != nullptr, bias != nullptr, stat_part != nullptr);
    const ConvFwdPath path = umi_conv_fwd_path(p);
    if (path != FWD_MFMA3X3_F32 && path != FWD_GEMM_F32 && path != FWD_CONVT_F32) p.flags = flags &= ~UMI_CONV_F32_OPT_IN;      // refused there: the call runs without the flags
    // only the pointwise / tap-gather MFMA kernel adds into y
    if ((flags & UMI_CONV_ACCUMULATE) && (stat_part || path != FWD_MFMA1X1)) return UMI_ERR_UNSUPPORTED;
    if (flags & UMI_CONV_DGRAD_STRIDED) {
        // x = dy of a strided conv (H x W), output grid = the conv's input image (Ho x Wo)
        if (flags & UMI_CONV_UPSAMPLE2) return UMI_ERR_BADARG;
        if (H != (Ho + 2 * pad - R) / stride + 1 || W != (Wo + 2 * pad - S) / stride + 1) return UMI_ERR_BADARG;
        if (out_H != Ho || out_W != Wo || off_h || off_w || stat_part) return UMI_ERR_BADARG;
    } else if (!(flags & UMI_CONV_UPSAMPLE2)) {
        if (Ho != (H + 2 * pad - R) / stride + 1 || Wo != (W + 2 * pad - S) / stride + 1) return UMI_ERR_BADARG;
        if (out_H != Ho || out_W != Wo || off_h || off_w) return UMI_ERR_BADARG;
    } else {
        if (Ho != H || Wo != W) return UMI_ERR_BADARG;
    }
    const hipStream_t s = (hipStream_t)stream;
    switch (path) {
    case FWD_MFMA3X3_F32: return umi_conv3x3_f32_mfma(p, x, tx, wp, y, stat_part, s);
    case FWD_GEMM_F32: return umi_gemm_f32_mfma(p, x, tx, wp, bias, y, stat_part, s);
    case FWD_CONVT_F32:
        // 16-byte alignment is one of this flag's conditions, and the flag-less kernel reads the same weight packing: ignored here too
        if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)wp | (uintptr_t)tx) & 15)
            return umi_conv_fwd(x, ldx, tx, wp, bias, y, ldy, stat_part, N, H, W, Ci, Co, R, S, stride, pad, Ho, Wo, off_h, off_w, out_H,
                                out_W, in_dtype, out_dtype, flags & ~UMI_CONV_F32_OPT_IN, stream);
        if (stat_part) return UMI_ERR_UNSUPPORTED;      // no BatchNorm follows a ConvTranspose2d, its data gradient fuses no reduction
        return umi_convt_f32_mfma(p, x, tx, wp, bias, y, off_h, off_w, out_H, out_W, s);
    case FWD_MFMA3X3:
        // the caller packed the weights for this path (umi_conv_fwd_plan said layout 1): misalignment is an error,
        // not a reason to silently reinterpret them
        if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)wp) & 15) return UMI_ERR_BADARG;
        return umi_conv3x3_mfma(p, x, tx, wp, y, stat_part, s);
    case FWD_MFMA1X1:
        if (stat_part) return UMI_ERR_UNSUPPORTED;      // no BatchNorm follows a pointwise conv on this path
        if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)wp) & 15) return UMI_ERR_BADARG;
        return umi_conv1x1_mfma(p, x, tx, wp, bias, y, off_h, off_w, out_H, out_W, s);
    case FWD_STEM: return umi_stem_fwd(p, x, tx, wp, y, stat_part, s);
    case FWD_HEAD: return umi_head_fwd(p, x, tx, wp, bias, y, stat_part, s);
    case FWD_SMALLK: return umi_smallk_fwd(p, x, wp, y, s);
    case FWD_ROOT: return umi_root_fwd(p, x, wp, y, s);
    case FWD_HEAD3: return umi_head3_fwd(p, x, tx, wp, bias, y, s);
    case FWD_GENERIC: break;
    }
    UMI_TRACE((flags & UMI_CONV_DGRAD_STRIDED) ? "dgrad_strided" : "fwd");
    return umi_conv_fwd_generic(p, x, tx, wp, bias, y, stat_part, off_h, off_w, out_H, out_W, s);
}

static WgradProblem wgrad_problem(int N, int H, int W, int Ci, int Co, int R, int S, int stride, int pad, int Ho, int Wo, int ldx,
                                  int lddy, int dtype, int flags, bool has_txa, bool has_txb) {
    return WgradProblem{N, H, W, Ci, Co, R, S, stride, pad, Ho, Wo, ldx, lddy, dtype, flags, has_txa, has_txb};
}

extern "C" size_t umi_conv_wgrad_ws_bytes(int N, int Ho, int Wo, int Ci, int Co, int R, int S, int dtype, int flags) {
    // the call picks its path from more arguments than this query has: size for whichever path could need most
    WgradProblem p = wgrad_problem(N, 0, 0, Ci, Co, R, S, 0, 0, Ho, Wo, 0, 0, dtype, flags, false, false);
    const size_t f32_mfma = umi_wgrad3x3_f32_mfma_ws_bound(p), f32_gemm = umi_wgrad_gemm_f32_mfma_ws_bound(p),
                 f32_convt = umi_wgrad_convt_f32_mfma_ws_bound(p);
    p.flags &= ~UMI_CONV_F32_OPT_IN;                     // the call may still find the flags refused (strides, a transform on dy)
    const size_t bounds[] = {f32_mfma, f32_gemm, f32_convt, umi_wgrad3x3_mfma_ws_bound(p), umi_wgrad1x1_mfma_ws_bound(p), umi_wgradT_mfma_ws_bound(p),
                             umi_wgrad_gather_mfma_ws_bound(p), umi_stem_wgrad_ws_bound(p), umi_head_wgrad_ws_bound(p),
                             umi_root_wgrad_ws_bound(p), umi_head3_wgrad_ws_bound(p), umi_conv_wgrad_generic_ws_bound(p)};
    size_t most = 0;
    for (size_t b : bounds) most = b > most ? b : most;
    return most;
}

// The weight gradient of problem `p` on `path` (= umi_conv_wgrad_path(p)), with the sinks of `o`.
static int conv_wgrad(const WgradProblem& asked, WgradPath path, const void* x, const void* txa, const void* dy, const void* txb,
                      const WgradOut& o, hipStream_t s) {
    WgradProblem p = asked;
    if (path != WGRAD_MFMA3X3_F32 && path != WGRAD_GEMM_F32 && path != WGRAD_CONVT_F32) p.flags &= ~UMI_CONV_F32_OPT_IN;      // refused there: the call runs without the flags
    if (!x || !dy || !o.dW || !o.ws || p.N <= 0 || p.H <= 0 || p.W <= 0 || p.Ci <= 0 || p.Co <= 0 || p.ldx < p.Ci || p.lddy < p.Co)
        return UMI_ERR_BADARG;
    switch (path) {
    case WGRAD_MFMA3X3_F32: return umi_wgrad3x3_f32_mfma(p, x, txa, dy, o, s);
    case WGRAD_GEMM_F32: return umi_wgrad_gemm_f32_mfma(p, x, txa, dy, o, s);
    case WGRAD_CONVT_F32:
        if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)txa | (uintptr_t)txb) & 15) {      // not 16-byte aligned: the flag is ignored
            p.flags &= ~UMI_CONV_F32_OPT_IN;
            return conv_wgrad(p, umi_conv_wgrad_path(p), x, txa, dy, txb, o, s);
        }
        return umi_wgrad_convt_f32_mfma(p, x, txa, dy, txb, o, s);
    case WGRAD_MFMA3X3: return umi_wgrad3x3_mfma(p, x, txa, dy, o, s);
    case WGRAD_MFMA1X1: return umi_wgrad1x1_mfma(p, x, txa, dy, o, s);
    case WGRAD_T: return umi_wgradT_mfma(p, x, dy, txb, o, s);
    case WGRAD_GATHER: return umi_wgrad_gather_mfma(p, x, txa, dy, o, s);
    case WGRAD_STEM: return umi_stem_wgrad(p, x, txa, dy, o, s);
    case WGRAD_HEAD: return umi_head_wgrad(p, x, txa, dy, o, s);
    case WGRAD_ROOT: return umi_root_wgrad(p, x, dy, o, s);
    case WGRAD_HEAD3: return umi_head3_wgrad(p, x, txa, dy, o, s);
    case WGRAD_GENERIC: break;
    }
    if (trace_generic())
        fprintf(stderr, "[umi generic wgrad] N=%d H=%d W=%d Ci=%d Co=%d R=%d stride=%d pad=%d flags=%d\n", p.N, p.H, p.W, p.Ci, p.Co,
                p.R, p.stride, p.pad, p.flags);
    return umi_conv_wgrad_generic(p, x, txa, dy, txb, o, s);
}

extern "C" int umi_conv_wgrad(const void* x, int ldx, const void* txa, const void* dy, int lddy, const void* txb,
                              float* dW, long s_co, long s_ci, long s_t, float out_scale, int N, int H, int W, int Ci,
                              int Co, int R, int S, int stride, int pad, int Ho, int Wo, int dtype, int flags, void* ws,
                              size_t ws_bytes, umi_stream_t stream) {
    const WgradProblem p = wgrad_problem(N, H, W, Ci, Co, R, S, stride, pad, Ho, Wo, ldx, lddy, dtype, flags, txa != nullptr, txb != nullptr);
    const WgradOut o{dW, s_co, s_ci, s_t, out_scale, ws, ws_bytes, nullptr, nullptr};
    return conv_wgrad(p, umi_conv_wgrad_path(p), x, txa, dy, txb, o, (hipStream_t)stream);
}

// umi_conv_wgrad whose final split-K reduction is RECORDED in *out instead of launched (umi_wgrad_reduce_group runs many of
// them at once).  `ws` must then stay untouched until that launch; out->part == NULL when the path taken had no separate
// reduction (the gradient is already in dW) or the call failed.
extern "C" int umi_conv_wgrad_deferred(const void* x, int ldx, const void* txa, const void* dy, int lddy, const void* txb,
                                       float* dW, long s_co, long s_ci, long s_t, float out_scale, int N, int H, int W, int Ci,
                                       int Co, int R, int S, int stride, int pad, int Ho, int Wo, int dtype, int flags, void* ws,
                                       size_t ws_bytes, umi_wgrad_pending* out, umi_stream_t stream) {
    if (!out) return UMI_ERR_BADARG;
    out->part = nullptr;
    const WgradProblem p = wgrad_problem(N, H, W, Ci, Co, R, S, stride, pad, Ho, Wo, ldx, lddy, dtype, flags, txa != nullptr, txb != nullptr);
    const WgradOut o{dW, s_co, s_ci, s_t, out_scale, ws, ws_bytes, out, nullptr};
    return conv_wgrad(p, umi_conv_wgrad_path(p), x, txa, dy, txb, o, (hipStream_t)stream);
}

// ConvTranspose2d(2,2) weight gradient (called like umi_conv_wgrad_deferred for it: x = d(up), dy = the ConvT's input) that also
// produces the BIAS gradient d bias[c] = out_scale * sum over pixels of x[.][c] from the operand tiles it stages (reference
// Model.py:56-57 under autograd; replaces umi_colsum's pass over x).  UMI_ERR_UNSUPPORTED (nothing launched) where the 2x2 / stride-2
// matrix-core kernel does not take the problem: run umi_colsum + umi_conv_wgrad instead.  `out` may be NULL (reduce at once).
extern "C" int umi_conv_wgrad_bias(const void* x, int ldx, const void* dy, int lddy, const void* txb, float* dW, long s_co,
                                   long s_ci, long s_t, float* dbias, float out_scale, int N, int H, int W, int Ci, int Co, int Ho,
                                   int Wo, int dtype, int flags, void* ws, size_t ws_bytes, umi_wgrad_pending* out,
                                   umi_stream_t stream) {
    if (!dbias) return UMI_ERR_BADARG;
    const WgradProblem p = wgrad_problem(N, H, W, Ci, Co, 2, 2, 2, 0, Ho, Wo, ldx, lddy, dtype, flags, false, txb != nullptr);
    if (umi_conv_wgrad_path(p) != WGRAD_T) return UMI_ERR_UNSUPPORTED;
    if (out) out->part = nullptr;
    const WgradOut o{dW, s_co, s_ci, s_t, out_scale, ws, ws_bytes, out, dbias};
    return conv_wgrad(p, WGRAD_T, x, nullptr, dy, txb, o, (hipStream_t)stream);
}

// umi_conv_wgrad for `n` pointwise convs / nn.Linear layers of ONE shape (M rows, Ci -> Co, same row strides) in one launch:
// dW[i][co*s_co + ci*s_ci] = out_scale * sum_p x[i][p][ci] * dy[i][p][co].  No workspace: each output tile is owned by one
// workgroup (fixed summation order).  UMI_ERR_UNSUPPORTED where the pointwise matrix-core kernel does not apply.
extern "C" int umi_conv_wgrad_group(int n, const void* const* x, int ldx, const void* const* dy, int lddy, float* const* dW,
                                    long s_co, long s_ci, float out_scale, long M, int Ci, int Co, int dtype,
                                    umi_stream_t stream) {
    if (n <= 0 || !x || !dy || !dW || M <= 0 || Ci <= 0 || Co <= 0 || ldx < Ci || lddy < Co) return UMI_ERR_BADARG;
    for (int i = 0; i < n; ++i)
        if (!x[i] || !dy[i] || !dW[i]) return UMI_ERR_BADARG;
    // (M rows as one image row; the predicate's own offset test refuses any M near 2^31 first)
    if (M >= (1L << 31) ||
        umi_conv_wgrad_path(wgrad_problem(1, 1, (int)M, Ci, Co, 1, 1, 1, 0, 1, (int)M, ldx, lddy, dtype, 0, false, false)) != WGRAD_MFMA1X1)
        return UMI_ERR_UNSUPPORTED;
    return umi_wgrad1x1_mfma_group(n, x, ldx, dy, lddy, dW, s_co, s_ci, out_scale, M, Ci, Co, (hipStream_t)stream);
}

// Weight gradient of a 3x3 conv whose output feeds BatchNorm(+ReLU), fused with stage 3 of that BatchNorm's backward: the
// gradient of the raw conv output, dz = gamma*rstd*(relu'(z)*dA - mean(dz) - xhat*mean(dz*xhat)) (umi_bn_bwd_apply's
// expression, bit for bit), is formed while dA is staged for the matrix cores and written to `dz` once for the
// data-gradient kernel.  `da` is left untouched.  UMI_ERR_UNSUPPORTED where the warp-specialised 3x3 kernel does not apply:
// the caller then runs umi_bn_bwd_apply + umi_conv_wgrad.
extern "C" int umi_conv_wgrad_bnapply_count(const void* x, int ldx, const void* txa, const void* da, int ldda, const void* y, int ldy,
                                      const void* tx_bn, const float* rstd, const float* sum_dz, const float* sum_dzx,
                                      void* dz, int lddz, float* dW, long s_co, long s_ci, long s_t, float out_scale, int N,
                                      int H, int W, int Ci, int Co, int R, int S, int stride, int pad, int dtype, int flags,
                                      long count, void* ws, size_t ws_bytes, umi_stream_t stream) {
    if (!x || !da || !y || !tx_bn || !rstd || !sum_dz || !sum_dzx || !dW || !ws || N <= 0 || H <= 0 || W <= 0 || Ci <= 0 ||
        Co <= 0 || count <= 0 || ldx < Ci || ldda < Co || ldy < Co || (dz && (lddz < Co || dz == da || dz == y)))
        return UMI_ERR_BADARG;
    const WgradProblem p = wgrad_problem(N, H, W, Ci, Co, R, S, stride, pad, H, W, ldx, ldda, dtype, flags, txa != nullptr, false);
    const WgradPath path = umi_conv_wgrad_path(p);
    const WgradOut o{dW, s_co, s_ci, s_t, out_scale, ws, ws_bytes, nullptr, nullptr};
    const WgradBnApply bna{y, ldy, tx_bn, rstd, sum_dz, sum_dzx, dz, lddz, count};
    if (!dz) {
        // dz == NULL: nothing else needs dz (the layer's input takes no gradient: the network's first conv) -- the narrow-input
        // weight-gradient kernel forms it on the fly and never stores it
        if (path != WGRAD_STEM || ldy % 8) return UMI_ERR_UNSUPPORTED;
        return umi_stem_wgrad(p, x, txa, da, o, (hipStream_t)stream, &bna);
    }
    if (path != WGRAD_MFMA3X3 || ldy % 8 || lddz % 8 || (long)H * W * (ldy > lddz ? ldy : lddz) * 2 >= 0x7FFFFFF0L)
        return UMI_ERR_UNSUPPORTED;
    return umi_wgrad3x3_mfma(p, x, txa, da, o, (hipStream_t)stream, &bna);
}

extern "C" int umi_conv_wgrad_bnapply(const void* x, int ldx, const void* txa, const void* da, int ldda, const void* y, int ldy,
                                      const void* tx_bn, const float* rstd, const float* sum_dz, const float* sum_dzx,
                                      void* dz, int lddz, float* dW, long s_co, long s_ci, long s_t, float out_scale, int N,
                                      int H, int W, int Ci, int Co, int R, int S, int stride, int pad, int dtype, int flags,
                                      void* ws, size_t ws_bytes, umi_stream_t stream) {
    if (N <= 0 || H <= 0 || W <= 0) return UMI_ERR_BADARG;
    return umi_conv_wgrad_bnapply_count(x, ldx, txa, da, ldda, y, ldy, tx_bn, rstd, sum_dz, sum_dzx, dz, lddz, dW, s_co, s_ci, s_t,
                                        out_scale, N, H, W, Ci, Co, R, S, stride, pad, dtype, flags, (long)N * H * W, ws, ws_bytes,
                                        stream);
}
