// Internal interface between the .hip files of libunetmi: every host function that is called across files is declared here,
// once, and so are the two problem records and the two selectors that decide which kernel serves a convolution.
#pragma once
#include "common.h"

// ---- convolution forward (also every data gradient: they are forward convolutions over dy) -------------------------------
struct ConvFwdProblem {
    int N, H, W, Ci, Co, R, S, stride, pad, Ho, Wo, ldx, ldy, in_dtype, out_dtype, flags;
    bool has_tx, has_bias, has_stats;      // an input transform / a bias / BatchNorm statistics of the output are asked for
};
// in cascade order: umi_conv_fwd_path returns the first whose predicate accepts the problem
enum ConvFwdPath { FWD_MFMA3X3_F32, FWD_GEMM_F32, FWD_CONVT_F32, FWD_MFMA3X3, FWD_MFMA1X1, FWD_STEM, FWD_HEAD, FWD_SMALLK, FWD_ROOT, FWD_HEAD3, FWD_GENERIC };

// A predicate carries every refusal that depends on the problem alone.  The launcher it guards may then fail only on pointer
// alignment (UMI_ERR_BADARG), a workspace below its own bound (UMI_ERR_WORKSPACE), a HIP error or an env switch.
bool umi_conv3x3_f32_mfma_ok(const ConvFwdProblem& p);  // conv_mfma_f32.hip: only under UMI_CONV_F32_MFMA
bool umi_gemm_f32_mfma_ok(const ConvFwdProblem& p);     // gemm_mfma_f32.hip: only under UMI_CONV_F32_MFMA_1X1
bool umi_convt_f32_mfma_ok(const ConvFwdProblem& p);    // convt_mfma_f32.hip: only under UMI_CONV_F32_MFMA_2X2
bool umi_conv3x3_mfma_ok(const ConvFwdProblem& p);      // conv_mfma.hip
bool umi_conv1x1_mfma_ok(const ConvFwdProblem& p);      // conv1x1_mfma.hip
bool umi_stem_fwd_ok(const ConvFwdProblem& p);          // stem_head.hip
bool umi_head_fwd_ok(const ConvFwdProblem& p);
bool umi_smallk_fwd_ok(const ConvFwdProblem& p);
bool umi_root_fwd_ok(const ConvFwdProblem& p);          // narrow_convs.hip
bool umi_head3_fwd_ok(const ConvFwdProblem& p);

// The ONE place where the order of the forward cascade exists.  The matrix-core paths are chosen on the problem's shape alone
// (the host packs the weights for them before it knows the pointers); the pointwise one writes no statistics, so a caller
// that wants them gets UMI_ERR_UNSUPPORTED from umi_conv_fwd.  The narrow kernels below the head write none either and
// give way to the generic kernel when statistics are asked for.
// UMI_CONV_F32_MFMA (3x3), UMI_CONV_F32_MFMA_1X1 (pointwise) and UMI_CONV_F32_MFMA_2X2 (ConvTranspose2d(2, 2) and its gradients) ask
// for the fp32 matrix-core kernels, each predicate reads its own flag, and a flag is IGNORED where its kernel refuses the problem:
// the rest of the cascade then sees the problem without any of them, so every answer is the flag-less one.  The 2x2 kernels write
// no statistics: like the tap-gather kernel's, their plan stands and a call that asks for them gets UMI_ERR_UNSUPPORTED.
constexpr int UMI_CONV_F32_OPT_IN = UMI_CONV_F32_MFMA | UMI_CONV_F32_MFMA_1X1 | UMI_CONV_F32_MFMA_2X2;
inline ConvFwdPath umi_conv_fwd_path(const ConvFwdProblem& p) {
    if (p.flags & UMI_CONV_F32_OPT_IN) {
        if (umi_conv3x3_f32_mfma_ok(p)) return FWD_MFMA3X3_F32;
        if (umi_gemm_f32_mfma_ok(p)) return FWD_GEMM_F32;
        if (umi_convt_f32_mfma_ok(p)) return FWD_CONVT_F32;
        ConvFwdProblem q = p;
        q.flags &= ~UMI_CONV_F32_OPT_IN;
        return umi_conv_fwd_path(q);
    }
    if (p.flags & UMI_CONV_DGRAD_STRIDED)                  // only the tap-gather matrix-core kernel and the generic one take these
        return umi_conv1x1_mfma_ok(p) ? FWD_MFMA1X1 : FWD_GENERIC;
    if (umi_conv3x3_mfma_ok(p)) return FWD_MFMA3X3;
    if (umi_conv1x1_mfma_ok(p)) return FWD_MFMA1X1;
    if (umi_stem_fwd_ok(p)) return FWD_STEM;
    if ((!p.has_stats || p.out_dtype == UMI_F16) && umi_head_fwd_ok(p)) return FWD_HEAD;
    if (p.has_stats) return FWD_GENERIC;
    if (umi_smallk_fwd_ok(p)) return FWD_SMALLK;
    if (umi_root_fwd_ok(p)) return FWD_ROOT;
    if (umi_head3_fwd_ok(p)) return FWD_HEAD3;
    return FWD_GENERIC;
}

// epilogue of the pointwise matrix-core kernel: 1 / 2 = the ViT linears' elementwise tails (umi_linear_fused), 3 = stage 1 of a
// BatchNorm backward (umi_conv_gather_bnred)
struct UmiLinearEpi {
    int mode; float p; unsigned seed; const unsigned* seed_dev; void* mask; const void* aux; int ldaux; void* y2; int ldy2;
    const void* bn_tx; const float* bn_rstd; float* bn_part;
};

// launchers: (problem, x, tx, weights, bias, y, stat_part, ...) -- arguments a kernel has no use for are left out
int umi_conv_fwd_generic(const ConvFwdProblem& p, const void* x, const void* tx, const void* wp, const float* bias, void* y,
                         float* stat_part, int off_h, int off_w, int out_H, int out_W, hipStream_t s);       // generic_kernels.hip
int umi_conv3x3_f32_mfma_stat_rows(int N, int H, int W);                                                     // conv_mfma_f32.hip
int umi_conv3x3_f32_mfma(const ConvFwdProblem& p, const void* x, const void* tx, const void* wp, void* y, float* stat_part,
                         hipStream_t s);
int umi_gemm_f32_mfma_stat_rows(long M);                                                                      // gemm_mfma_f32.hip
int umi_gemm_f32_mfma(const ConvFwdProblem& p, const void* x, const void* tx, const void* wp, const float* bias, void* y,
                      float* stat_part, hipStream_t s);
// UMI_CONV_UPSAMPLE2 in p.flags: the ConvT forward (scatter at off_h / off_w of the out_H x out_W image); else its data gradient
int umi_convt_f32_mfma(const ConvFwdProblem& p, const void* x, const void* tx, const void* wp, const float* bias, void* y,
                       int off_h, int off_w, int out_H, int out_W, hipStream_t s);                          // convt_mfma_f32.hip
int umi_conv3x3_mfma_stat_rows(int N, int H, int W, int Co);                                                  // conv_mfma.hip
int umi_conv3x3_mfma(const ConvFwdProblem& p, const void* x, const void* tx, const void* wp8, void* y, float* stat_part,
                     hipStream_t s);
int umi_conv3x3_mfma_bnred(const ConvFwdProblem& p, const void* dy, const void* wp8, void* da, const void* ybn, int ldybn,
                           const void* txbn, const float* rstd, float* part, hipStream_t s);
int umi_conv3x3_mfma_act(const ConvFwdProblem& p, const void* x, const void* tx, const void* wp8, const void* out_tx, void* y,
                         hipStream_t s);
int umi_conv1x1_bnred_rows(long M, int Ntot);                                                                 // conv1x1_mfma.hip
int umi_conv1x1_mfma(const ConvFwdProblem& p, const void* x, const void* tx, const void* wp8, const float* bias, void* y,
                     int off_h, int off_w, int out_H, int out_W, hipStream_t s, const UmiLinearEpi* epi = nullptr);
int umi_stem_stat_rows(int N, int H, int W);                                                                  // stem_head.hip
int umi_stem_fwd(const ConvFwdProblem& p, const void* x, const void* tx, const void* wp, void* y, float* part, hipStream_t s);
int umi_head_stat_rows(long P, int Ci);
int umi_head_fwd(const ConvFwdProblem& p, const void* x, const void* tx, const void* wp, const float* bias, void* y, float* part,
                 hipStream_t s);
int umi_smallk_fwd(const ConvFwdProblem& p, const void* x, const void* wp, void* y, hipStream_t s);
int umi_smallk_bnred_rows(long P, int Co);
// P pixels of Ci (<= 8) channels -> Co; dW != NULL: also the head's weight gradient, ws >= umi_smallk_bnred_rows * Co * Ci floats
int umi_smallk_fwd_bnred(const void* x, int ldx, const void* wp, void* y, int ldy, const void* ybn, int ldybn, const void* txbn,
                         const float* rstd, float* part, long P, int Ci, int Co, hipStream_t s, float* dW = nullptr, long s_co = 0,
                         long s_ci = 0, float out_scale = 1.f, void* ws = nullptr, size_t ws_bytes = 0);
int umi_root_fwd(const ConvFwdProblem& p, const void* x, const void* wp, void* y, hipStream_t s);              // narrow_convs.hip
int umi_head3_fwd(const ConvFwdProblem& p, const void* x, const void* tx, const void* wp, const float* bias, void* y,
                  hipStream_t s);

// ---- convolution weight gradient -------------------------------------------------------------------------------------------
struct WgradProblem {
    int N, H, W, Ci, Co, R, S, stride, pad, Ho, Wo, ldx, lddy, dtype, flags;
    bool has_txa, has_txb;                 // transforms of x / of dy
};
// where a weight gradient goes: the parameter (strides in elements), the split-K workspace, and the two optional sinks
struct WgradOut {
    float* dW; long s_co, s_ci, s_t; float out_scale;
    void* ws; size_t ws_bytes;
    umi_wgrad_pending* defer;              // non-NULL: the final split-K reduction is recorded here instead of launched
    float* convT_bias;                     // non-NULL (WGRAD_T only): also out_scale * column sums of x
};
// stage 3 of the BatchNorm(+ReLU) backward formed while the gradient operand is staged (umi_conv_wgrad_bnapply): `dy` is then
// the gradient of the ACTIVATED output
struct WgradBnApply { const void* y; int ldy; const void* tx_bn; const float *rstd, *sum_dz, *sum_dzx; void* dz; int lddz;
                      long count; };   // count: the divisor of the two sums (N * H * W, or the rows of the whole data-parallel batch)
enum WgradPath { WGRAD_MFMA3X3_F32, WGRAD_GEMM_F32, WGRAD_CONVT_F32, WGRAD_MFMA3X3, WGRAD_MFMA1X1, WGRAD_T, WGRAD_GATHER, WGRAD_STEM, WGRAD_HEAD, WGRAD_ROOT, WGRAD_HEAD3, WGRAD_GENERIC };

bool umi_wgrad3x3_f32_mfma_ok(const WgradProblem& p);   // conv_mfma_f32.hip: only under UMI_CONV_F32_MFMA
bool umi_wgrad_gemm_f32_mfma_ok(const WgradProblem& p); // gemm_mfma_f32.hip: only under UMI_CONV_F32_MFMA_1X1
bool umi_wgrad_convt_f32_mfma_ok(const WgradProblem& p); // convt_mfma_f32.hip: only under UMI_CONV_F32_MFMA_2X2
bool umi_wgrad3x3_mfma_ok(const WgradProblem& p);       // wgrad_mfma.hip
bool umi_wgrad1x1_mfma_ok(const WgradProblem& p);
bool umi_wgradT_mfma_ok(const WgradProblem& p);
bool umi_wgrad_gather_mfma_ok(const WgradProblem& p);
bool umi_stem_wgrad_ok(const WgradProblem& p);          // stem_head.hip
bool umi_head_wgrad_ok(const WgradProblem& p);
bool umi_root_wgrad_ok(const WgradProblem& p);          // narrow_convs.hip
bool umi_head3_wgrad_ok(const WgradProblem& p);

// the ONE place where the order of the weight-gradient cascade exists
inline WgradPath umi_conv_wgrad_path(const WgradProblem& p) {
    if (p.flags & UMI_CONV_F32_OPT_IN) {                    // ignored where refused, as in umi_conv_fwd_path
        if (umi_wgrad3x3_f32_mfma_ok(p)) return WGRAD_MFMA3X3_F32;
        if (umi_wgrad_gemm_f32_mfma_ok(p)) return WGRAD_GEMM_F32;
        if (umi_wgrad_convt_f32_mfma_ok(p)) return WGRAD_CONVT_F32;
        WgradProblem q = p;
        q.flags &= ~UMI_CONV_F32_OPT_IN;
        return umi_conv_wgrad_path(q);
    }
    if (umi_wgrad3x3_mfma_ok(p)) return WGRAD_MFMA3X3;
    if (umi_wgrad1x1_mfma_ok(p)) return WGRAD_MFMA1X1;
    if (umi_wgradT_mfma_ok(p)) return WGRAD_T;
    if (umi_wgrad_gather_mfma_ok(p)) return WGRAD_GATHER;
    if (umi_stem_wgrad_ok(p)) return WGRAD_STEM;
    if (umi_head_wgrad_ok(p)) return WGRAD_HEAD;
    if (umi_root_wgrad_ok(p)) return WGRAD_ROOT;
    if (umi_head3_wgrad_ok(p)) return WGRAD_HEAD3;
    return WGRAD_GENERIC;
}

// Workspace bounds for umi_conv_wgrad_ws_bytes, which knows only N, Ho, Wo, Ci, Co, R, S, dtype and flags of `p` (every other
// field is unset): the most workspace the path could ask for over the problems it takes with those facts, 0 if it takes none.
size_t umi_wgrad3x3_f32_mfma_ws_bound(const WgradProblem& p);      // 0 without UMI_CONV_F32_MFMA
size_t umi_wgrad_gemm_f32_mfma_ws_bound(const WgradProblem& p);     // 0 without UMI_CONV_F32_MFMA_1X1
size_t umi_wgrad_convt_f32_mfma_ws_bound(const WgradProblem& p);    // 0 without UMI_CONV_F32_MFMA_2X2
size_t umi_wgrad3x3_mfma_ws_bound(const WgradProblem& p);
size_t umi_wgrad1x1_mfma_ws_bound(const WgradProblem& p);
size_t umi_wgradT_mfma_ws_bound(const WgradProblem& p);
size_t umi_wgrad_gather_mfma_ws_bound(const WgradProblem& p);
size_t umi_stem_wgrad_ws_bound(const WgradProblem& p);
size_t umi_head_wgrad_ws_bound(const WgradProblem& p);
size_t umi_root_wgrad_ws_bound(const WgradProblem& p);
size_t umi_head3_wgrad_ws_bound(const WgradProblem& p);
size_t umi_conv_wgrad_generic_ws_bound(const WgradProblem& p);      // generic_kernels.hip

// launchers: partial slabs into o.ws, then umi_launch_wgrad_reduce
int umi_wgrad3x3_f32_mfma(const WgradProblem& p, const void* x, const void* txa, const void* dy, const WgradOut& o, hipStream_t s);
int umi_wgrad_gemm_f32_mfma(const WgradProblem& p, const void* x, const void* txa, const void* dy, const WgradOut& o, hipStream_t s);
int umi_wgrad_convt_f32_mfma(const WgradProblem& p, const void* x, const void* txa, const void* dy, const void* txb,
                             const WgradOut& o, hipStream_t s);
int umi_wgrad3x3_mfma(const WgradProblem& p, const void* x, const void* txa, const void* dy, const WgradOut& o, hipStream_t s,
                      const WgradBnApply* bna = nullptr);
int umi_wgrad1x1_mfma(const WgradProblem& p, const void* x, const void* txa, const void* dy, const WgradOut& o, hipStream_t s);
int umi_wgradT_mfma(const WgradProblem& p, const void* x, const void* dy, const void* txb, const WgradOut& o, hipStream_t s);
int umi_wgrad_gather_mfma(const WgradProblem& p, const void* x, const void* txa, const void* dy, const WgradOut& o, hipStream_t s);
int umi_stem_wgrad(const WgradProblem& p, const void* x, const void* txa, const void* dy, const WgradOut& o, hipStream_t s,
                   const WgradBnApply* bna = nullptr);
int umi_head_wgrad(const WgradProblem& p, const void* x, const void* txa, const void* dy, const WgradOut& o, hipStream_t s);
int umi_root_wgrad(const WgradProblem& p, const void* x, const void* dy, const WgradOut& o, hipStream_t s);
int umi_head3_wgrad(const WgradProblem& p, const void* x, const void* txa, const void* dy, const WgradOut& o, hipStream_t s);
int umi_conv_wgrad_generic(const WgradProblem& p, const void* x, const void* txa, const void* dy, const void* txb,
                           const WgradOut& o, hipStream_t s);
int umi_wgrad1x1_mfma_group(int n, const void* const* x, int ldx, const void* const* dy, int lddy, float* const* dW, long s_co,
                            long s_ci, float out_scale, long M, int Ci, int Co, hipStream_t s);

// The final reduction of `splits` slabs [RS][Ci][Co] at o.ws into o.dW: recorded in *o.defer when that is set, launched otherwise.
void umi_launch_wgrad_reduce(int splits, int RS, int Ci, int Co, const WgradOut& o, hipStream_t s);               // generic_kernels.hip
void umi_launch_reduce_rows2(const float* ws, int rows, int C, float* out0, float* out1, float scale, hipStream_t s);

// ---- elementwise_f16.hip: 16-B vectorised fp16 fast paths (false: the shape does not qualify) ------------------------------
int umi_bn_bwd_rpb_f16v(long M);
int umi_colsum_rows_f16v(long M, int C);
bool umi_colsum_f16v(const void* x, int ldx, float* ws, long M, int C, hipStream_t s);
bool umi_colsum_group_f16v(int n, const void* const* xs, int ldx, float* const* outs, float scale, float* ws, long M, int C,
                           hipStream_t s);
bool umi_bn_stats_f16v(const void* x, int ldx, float* part, long M, int C, hipStream_t s);
bool umi_bn_bwd_reduce1_f16v(const void* da, int ldda, const void* y, int ldy, const void* tx, const float* rstd, float* ws,
                             long M, int C, hipStream_t s);
bool umi_bn_bwd_apply_f16v(void* da, int ldda, const void* y, int ldy, const void* tx, const float* rstd,
                           const float* sum_dz, const float* sum_dzx, long M, long count, int C, hipStream_t s);
bool umi_pool2_fwd_f16v(const void* x, int ldx, const void* tx, void* y, int ldy, int N, int H, int W, int C,
                        hipStream_t s);
bool umi_pool2_bwd_f16v(const void* dp, int lddp, const void* x, int ldx, const void* tx, void* da, int ldda,
                        int accumulate, int N, int H, int W, int C, hipStream_t s);
int umi_pool2_bwd_bnred_rows(int N, int H, int W, int C);
bool umi_pool2_bwd_bnred_f16v(const void* dp, int lddp, const void* x, int ldx, const void* tx, const float* rstd, void* da,
                              int ldda, int accumulate, float* part, int N, int H, int W, int C, hipStream_t s);

// ---- groupnorm_f16.hip ----------------------------------------------------------------------------------------------------------
int umi_gn_splits(int N, long HW);
bool umi_gn_fwd_f16v(const void* x, int ldx, const float* gamma, const float* beta, const void* res, int ldr, void* y, int ldy,
                     float* mean, float* rstd, int relu, int N, long HW, int C, int G, float eps, float* ws, hipStream_t s);
bool umi_gn_bwd_f16v(const void* dy, int lddy, const void* y, int ldy, const void* x, int ldx, const float* mean,
                     const float* rstd, const float* gamma, int relu, void* dx, int lddx, void* dres, int lddr, int N, long HW,
                     int C, int G, float* part, float* ws, hipStream_t s);
void umi_gn_param_grads_launch(int n, const float* const* parts, const int* Cs, int N, float* const* dgammas, float* const* dbetas,
                               float scale, hipStream_t s);

// ---- elementwise_tu_f16.hip -----------------------------------------------------------------------------------------------------
bool umi_ew_f16v(int mode, const void* x, int ldx, const void* g, int ldg, void* y, int ldy, long M, int C, long bcast_rows,
                 hipStream_t s);
bool umi_pool3s2_fwd_f16v(const void* x, int ldx, void* y, int ldy, void* idx, int N, int H, int W, int C, hipStream_t s);
bool umi_pool3s2_bwd_f16v(const void* dy, int lddy, const void* idx, void* dx, int lddx, int N, int H, int W, int C, hipStream_t s);
bool umi_dropout_f16v(const void* x, int ldx, void* y, int ldy, void* mask, int backward, float p, unsigned seed, long M, int C,
                      const void* tx, const unsigned* seed_dev, hipStream_t s);
bool umi_dropout_fused_f16v(const void* x, int ldx, void* y, int ldy, void* mask, int backward, float p, unsigned seed, long M,
                            int C, const unsigned* seed_dev, const void* aux, int ldaux, int gelu, hipStream_t s);
int umi_ln_bwd_rows_f16v();
bool umi_ln_bwd_f16v(const void* dy, int lddy, const void* x, int ldx, const float* gamma, const float* mean, const float* rstd,
                     void* dx, int lddx, float* part, long M, int C, hipStream_t s);
bool umi_bilinear2x_f16v(const void* x, int ldx, const void* tx, void* y, int ldy, int backward, int N, int H, int W, int C,
                         hipStream_t s);

// (both matrix-core families: `drop` null = the kernels without dropout, else their DROP instantiations, common.h UmiAttnDrop)
// ---- attention_mfma.hip ---------------------------------------------------------------------------------------------------------
bool umi_attn_mfma_ok(int D, int ld, int ldo, int dtype, const void* a, const void* b, const void* c);
int umi_attn_fwd_mfma(const void* q, const void* k, const void* v, int ld, void* o, int ldo, float* lse, int B, int N, int Hh,
                      const UmiAttnDrop* drop, hipStream_t s);
int umi_attn_bwd_mfma(const void* q, const void* k, const void* v, int ld, const void* o, const void* dO, int ldo,
                      const float* lse, void* dq, void* dk, void* dv, int ldd, float* delta, int B, int N, int Hh,
                      const UmiAttnDrop* drop, hipStream_t s);

// ---- attention_mfma_f32.hip: only under UMI_ATTN_F32_MFMA -----------------------------------------------------------------------
// ptrs: the OR of every tensor address of the call (16-byte alignment); ldd = 0 in a forward call
bool umi_attn_f32_mfma_ok(int D, int ld, int ldo, int ldd, int dtype, int flags, uintptr_t ptrs);
int umi_attn_fwd_f32_mfma(const void* q, const void* k, const void* v, int ld, void* o, int ldo, float* lse, int B, int N, int Hh,
                          const UmiAttnDrop* drop, hipStream_t s);
int umi_attn_bwd_f32_mfma(const void* q, const void* k, const void* v, int ld, const void* o, const void* dO, int ldo,
                          const float* lse, void* dq, void* dk, void* dv, int ldd, float* delta, int B, int N, int Hh,
                          const UmiAttnDrop* drop, hipStream_t s);
