/* unetmi.h -- C ABI of libunetmi.so: the MI355X (gfx950) U-Net / TransUNet hot path.
 *
 * The reference (caki35/UNet-Torch) is pure Python and has no FFI of its own: every
 * arithmetic op on its hot path is a torch.nn call.  The drop-in boundary
 * is therefore the reference's Python module API (`Model.UNet`, `Trainer.Trainer`, ...,
 * mirrored under unet-torch_amd/), and THIS header is the C ABI that mirror binds with
 * ctypes.  Each entry point cites the reference call site whose arithmetic it replaces.
 *
 * Conventions
 *  - Plain pointers and sizes only; device pointers are borrowed from the caller
 *    (torch tensor .data_ptr()); nothing is allocated, freed or synchronised inside.
 *  - Every function enqueues on the caller's `stream` and returns an int:
 *    0 = ok, <0 = UMI_ERR_*, >0 = hipError_t of the failed launch.  Nothing throws.
 *  - Activations are NHWC with an explicit pixel stride `ld` (elements), so a tensor may
 *    be a channel slice of a wider concat buffer.  dtype: UMI_F32 / UMI_F16 storage,
 *    accumulation is always fp32.
 *  - Input transform `tx` (nullable): one float4 per input channel {mean, scale, shift, lo};
 *    a conv/pool/etc. consumes  max(fma(x, scale, shift), lo)  of the stored value (`mean` is only
 *    read by the BatchNorm backward kernels),
 *    i.e. BatchNorm-apply + ReLU of the producer is fused into the consumer's load
 *    (lo = 0 for ReLU channels, -inf for pass-through channels of a concat buffer).
 *    Zero padding is applied AFTER the transform, as in the reference
 *    (Conv2d(padding=1) sees zeros of the activated tensor).
 *  - Workspaces: `*_ws_bytes()` returns the bytes the matching call needs.
 */
#ifndef UNETMI_H
#define UNETMI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* umi_stream_t;          /* hipStream_t */

enum { UMI_F32 = 0, UMI_F16 = 1 };
enum { UMI_OK = 0, UMI_ERR_BADARG = -1, UMI_ERR_UNSUPPORTED = -2, UMI_ERR_WORKSPACE = -3 };
/* umi_conv_fwd flags */
enum { UMI_CONV_UPSAMPLE2 = 1,   /* ConvTranspose2d(k=2,s=2): tap t=(dy,dx) scatters to (2h+dy+off_h, 2w+dx+off_w) */
       UMI_CONV_FORCE_GENERIC = 2, /* never take the MFMA fast path (used by tests to cross-check it) */
       UMI_CONV_DGRAD_STRIDED = 4, /* data gradient of a stride>1 conv: x = dy [N,H,W,Ci:=Co_fwd], y = dx [N,Ho,Wo,Co:=Ci_fwd]
                                      with (R,S,stride,pad) of the FORWARD conv; weights packed [R*S][Co_fwd][Ci_fwd] unflipped */
       UMI_CONV_ACCUMULATE = 8,    /* y += conv(...) instead of y = conv(...): the second gradient contribution of a tensor with two
                                      consumers (attention gate, reference Model.py:268-289: g and x each feed two branches).  Only
                                      the pointwise / tap-gather MFMA kernel implements it: umi_conv_fwd_plan and umi_conv_fwd return
                                      UMI_ERR_UNSUPPORTED for any other problem, nothing is written */
       UMI_CONV_F32_MFMA = 16,     /* opt-in: an fp32 3x3 / stride 1 / pad 1 conv (forward, data gradient, weight gradient) runs on the
                                      fp32-input matrix-core instruction (v_mfma_f32_32x32x2_f32: one fp32 rounding per product, an
                                      fmaf chain like the generic kernel's in another order).  Taken when in and out are UMI_F32, no
                                      bias, none of the flags above, Ci % 8 == Co % 8 == 0 and ldx % 4 == ldy % 4 == 0 (weight
                                      gradient: no transform on dy either); IGNORED otherwise: the call, umi_conv_fwd_plan and
                                      umi_conv_wgrad_ws_bytes then answer exactly as without it */
       UMI_CONV_F32_MFMA_1X1 = 32, /* opt-in, independent of the flag above: an fp32 pointwise conv / nn.Linear (R = S = 1, stride 1,
                                      pad 0: Y[M, Co] = X[M, Ci] . W[Ci, Co], M = N * H * W; forward, data gradient, weight gradient)
                                      runs on the same instruction (csrc/gemm_mfma_f32.hip).  Taken when in and out are UMI_F32, none
                                      of the flags 1, 2, 4, 8 is set, Ci % 8 == Co % 8 == 0 and ldx % 4 == ldy % 4 == 0 (weight
                                      gradient: lddy % 4 == 0 and no transform on dy); a bias, an input transform and statistics are
                                      all allowed.  IGNORED otherwise, like the flag above: UMI_CONV_F32_MFMA on a 1x1 call and this
                                      flag on a 3x3 call are ignored, both together name the kernel that fits the geometry */
       UMI_CONV_F32_MFMA_2X2 = 64  /* opt-in, independent of the two flags above: an fp32 nn.ConvTranspose2d(k=2, s=2) runs on the same
                                      instruction (csrc/convt_mfma_f32.hip) in its three calls: umi_conv_fwd with UMI_CONV_UPSAMPLE2
                                      (the forward: input transform, bias, off_h / off_w inside a larger out_H x out_W image and
                                      ldy > Co all allowed), umi_conv_fwd without it on R = S = 2, stride 2, pad 0 with H == 2 Ho and
                                      W == 2 Wo (the data gradient), and umi_conv_wgrad(_deferred) of that geometry (a transform on
                                      either side allowed).  Taken when in and out are UMI_F32, R = S = 2, stride 2, pad 0, none of the
                                      flags 2, 4, 8 is set, Ci % 8 == Co % 8 == 0, ldx % 4 == ldy % 4 == 0 (weight gradient:
                                      lddy % 4 == 0) and x, y, the weights and the transforms (weight gradient: x, dy and the
                                      transforms) are 16-byte aligned.  IGNORED otherwise, like the two flags above (a call with a
                                      misaligned pointer runs as without the flag, whatever the plan said: both read one packing).  These kernels write no BatchNorm statistics (see umi_conv_fwd_plan) */ };

int umi_version(void);
const char* umi_arch(void);          /* "gfx950" */

/* Knob (process-wide) for same-process A/B timing of the conv3x3 matrix-core kernel's forms (csrc/conv_mfma.hip, tools/ab_conv.py):
 *   1 (default)  v_mfma_f32_16x16x32_f16 form where Co % 128 == 0 and Ci % 32 == 0, the 32x32x16 form elsewhere;
 *   2            the 32x32x16 form everywhere (the arithmetic order of rounds 1-2);
 *   3            the 16x16x32 form on the 64-output-channel tiles too (Ci % 32 == 0).
 * The forms differ by fp32 summation order only (<= 1 fp16 ulp on ~0.2 % of the outputs).  Returns the previous value; values
 * outside 1..8 only query.  Initial value: 1 or env UMI_CONV3X3_IMPL. */
int umi_tune_conv3x3_impl(int impl);

/* Re-layout of a weight tensor into the kernels' [T][K][N] packing (dtype storage):
 *   dst[(t*Kpad + k)*Npad + n] = src[t'*st + k*sk + n*sn],  t' = flip_t ? T-1-t : t,
 * zero for k >= K or n >= N.  Used for Conv2d OIHW weights (reference Model.py:15-20),
 * their 180-degree-rotated transpose (dgrad) and ConvTranspose2d [Cin,Cout,2,2]
 * (reference Model.py:56-57). */
int umi_pack_kn(const float* src, void* dst, int T, int K, int N, long st, long sk, long sn,
                int flip_t, int Kpad, int Npad, int dtype, umi_stream_t stream);

/* Same packing for the MFMA kernels: dst[t][k/8][n][k%8] (8 consecutive k contiguous). */
int umi_pack_kn8(const float* src, void* dst, int T, int K, int N, long st, long sk, long sn,
                 int flip_t, int Kpad, int Npad, int dtype, umi_stream_t stream);

/* Convolution forward, NHWC: replaces nn.Conv2d / F.conv2d on the hot path
 * (reference Model.py:15-16,19-20,89; vit_seg_modeling.py:145-148,265-272,321;
 *  vit_seg_modeling_resnet_skip.py:22-25) and, with UMI_CONV_UPSAMPLE2,
 * nn.ConvTranspose2d(k=2,s=2) (reference Model.py:56-57,67).
 *   y[n,ho,wo,co] = bias[co] + sum_{r,s,ci} tx(x[n,ho*stride-pad+r,wo*stride-pad+s,ci]) * wp[r*S+s][ci][co]
 * `stat_part` (nullable) receives per-pixel-tile partial sums for BatchNorm statistics,
 * layout [rows][2][Co] (sum, sum of squares of the *stored* y), rows = umi_conv_stat_rows().
 * Also used for dgrad (weights packed with flip_t, pad' = R-1-pad, stride 1). */
int umi_conv_fwd(const void* x, int ldx, const void* tx, const void* wp, const float* bias,
                 void* y, int ldy, float* stat_part,
                 int N, int H, int W, int Ci, int Co, int R, int S, int stride, int pad,
                 int Ho, int Wo, int off_h, int off_w, int out_H, int out_W,
                 int in_dtype, int out_dtype, int flags, umi_stream_t stream);
/* A ViT-block linear with its elementwise tail in the GEMM epilogue (reference TransUnet/vit_seg_modeling.py:113-119 Mlp.forward,
 * :177-187 Block.forward), fp16 storage:
 *   epi 1: y = x W + b, y2 = dropout(GELU(y)), mask        (fc1: y is kept for the GELU backward)
 *   epi 2: y = dropout(x W + b) + aux, mask                (fc2 / attention output projection, aux = the block's residual)
 * x [M, Ci], y / y2 / aux [M, Co] (ld in elements), wp8 = umi_pack_kn8 of the [Co, Ci] weight, mask: M*Co bytes (as umi_dropout).
 * Same values, random stream and roundings as umi_conv_fwd followed by umi_dropout_fused.  UMI_ERR_UNSUPPORTED where the
 * pointwise matrix-core kernel does not apply (run the two calls). */
int umi_linear_fused(const void* x, int ldx, const void* wp8, const float* bias, void* y, int ldy, long M, int Ci, int Co,
                     int epi, float p, unsigned seed, const unsigned* seed_dev, void* mask, const void* aux, int ldaux,
                     void* y2, int ldy2, int dtype, umi_stream_t stream);

/* Which kernel umi_conv_fwd will take for this problem (the same selector answers both): *layout = 0 -> weights packed with
 * umi_pack_kn, 1 -> umi_pack_kn8, for the two matrix-core kernels.  Both need fp16 in and out, ldx % 8 == ldy % 8 == 0 and no
 * UMI_CONV_FORCE_GENERIC:
 *   3x3:  R = S = 3, stride 1, pad 1, Ci % 16 == 0, Co % 8 == 0, no bias, no UMI_CONV_UPSAMPLE2 / UMI_CONV_DGRAD_STRIDED;
 *   pointwise / tap-gather:  R = S = 1, stride 1, pad 0 with Ci, Co multiples of 8 and >= 16; or, with Ci % 64 == Co % 64 == 0
 *         and R * S <= 49: stride >= 2, UMI_CONV_DGRAD_STRIDED, or UMI_CONV_UPSAMPLE2 with R = S = 2 -- as long as two source
 *         images stay within 31-bit byte offsets (2 * H * W * ldx * 2 < 0x7FFFFFF0).  (It writes no statistics: umi_conv_fwd
 *         with `stat_part` is UMI_ERR_UNSUPPORTED there.)
 * With UMI_CONV_F32_MFMA, where that flag's conditions hold, the fp32 matrix-core 3x3 kernel is named instead: *layout = 0 (it
 * reads umi_pack_kn's [tap][k][n], the flipped / transposed pack for a data gradient) and *stat_rows = one row per 8 x 32 pixel
 * tile, N * ceil(H / 8) * ceil(W / 32); a plan that names it is never followed by UMI_ERR_UNSUPPORTED from umi_conv_fwd.
 * With UMI_CONV_F32_MFMA_1X1, where that flag's conditions hold, the fp32 matrix-core pointwise kernel is named: *layout = 0
 * (umi_pack_kn's [1][Ci][Co]; the transposed pack for a data gradient) and *stat_rows = one row per 128 consecutive output rows,
 * ceil(N * H * W / 128); a plan that names it is never followed by UMI_ERR_UNSUPPORTED from umi_conv_fwd either.
 * With UMI_CONV_F32_MFMA_2X2, where that flag's conditions hold, the fp32 matrix-core ConvTranspose2d kernels are named: *layout = 0
 * (umi_pack_kn's [4][Cin][Cout] for the forward, [4][Cout][Cin] for the data gradient) and *stat_rows = 0.  They write no statistics
 * (no BatchNorm follows a ConvTranspose2d and the fp32 data gradient fuses no reduction), so here the sentence above does NOT hold:
 * like the fp16 tap-gather kernel, umi_conv_fwd with `stat_part` returns UMI_ERR_UNSUPPORTED on this path and writes nothing.
 * *stat_rows = rows of `stat_part` the call will write.  UMI_ERR_UNSUPPORTED: UMI_CONV_ACCUMULATE off the pointwise kernel. */
int umi_conv_fwd_plan(int N, int H, int W, int Ci, int Co, int R, int S, int stride, int pad,
                      int ldx, int ldy, int in_dtype, int out_dtype, int flags, int has_bias,
                      int* layout, int* stat_rows);

/* BatchNorm2d training statistics -> consumer transform (reference Model.py:17,21 =
 * nn.BatchNorm2d: biased batch variance for normalisation, unbiased into running_var,
 * momentum 0.1).  tx_out[c] = {mean, gamma*rstd, beta - mean*gamma*rstd, lo}, lo = 0 -- or NaN where scale or shift is not
 * finite (a NaN / Inf in the channel): max(NaN, NaN) keeps such a channel NaN in every consumer.  Running stats updated in
 * place when non-null. */
int umi_bn_finalize(const float* stat_part, int rows, int C, double count,
                    const float* gamma, const float* beta, float eps, float momentum,
                    float* running_mean, float* running_var,
                    void* tx_out, float* rstd_out, umi_stream_t stream);
/* umi_bn_finalize in two steps, for a data-parallel group that normalises with the statistics of its WHOLE batch: the ranks add
 * their sums (and pixel counts) between the two.
 *   umi_bn_stat_sums      sums[2][C] (float64) = per-channel sum and sum of squares of stat_part[rows][2][C], added in the order
 *                         umi_bn_finalize adds them (both of its reduction forms, chosen by the same rule);
 *   umi_bn_finalize_sums  everything umi_bn_finalize does after its reduction, from such sums and a count.
 * With count = this rank's pixels and its own sums the pair leaves the bits umi_bn_finalize leaves. */
int umi_bn_stat_sums(const float* stat_part, int rows, int C, double* sums, umi_stream_t stream);
int umi_bn_finalize_sums(const double* sums, int C, double count,
                         const float* gamma, const float* beta, float eps, float momentum,
                         float* running_mean, float* running_var,
                         void* tx_out, float* rstd_out, umi_stream_t stream);

/* MaxPool2d(2) of the transformed tensor (reference Model.py:36,42). Floor mode. */
int umi_pool2_fwd(const void* x, int ldx, const void* tx, void* y, int ldy,
                  int N, int H, int W, int C, int dtype, umi_stream_t stream);
/* Its backward: routes dpool to the first arg-max of tx(x) in each 2x2 window (PyTorch
 * tie rule); accumulate != 0 adds into `da` (skip-connection gradient already there). */
int umi_pool2_bwd(const void* dpool, int lddp, const void* x, int ldx, const void* tx,
                  void* da, int ldda, int accumulate,
                  int N, int H, int W, int C, int dtype, umi_stream_t stream);

/* BatchNorm+ReLU backward (autograd of reference Model.py:17-18,21-22).
 *   z = tx(y) before the clamp, dz = da * [z > 0],  xhat = (y - mean) * rstd
 *   reduce: sum_dz[c] = sum dz, sum_dzx[c] = sum dz*xhat      (d beta, d gamma)
 *   apply : dy = gamma*rstd * (dz - sum_dz/M - xhat*sum_dzx/M)   written over `da`. */
size_t umi_bn_bwd_ws_bytes(long M, int C);
int umi_bn_bwd_reduce(const void* da, int ldda, const void* y, int ldy, const void* tx,
                      const float* rstd, float* sum_dz, float* sum_dzx,
                      long M, int C, int dtype, void* ws, size_t ws_bytes, umi_stream_t stream);
int umi_bn_bwd_apply(void* da, int ldda, const void* y, int ldy, const void* tx,
                     const float* rstd, const float* sum_dz, const float* sum_dzx,
                     long M, int C, int dtype, umi_stream_t stream);
/* umi_bn_bwd_apply over M local rows whose two sums are those of `count` rows (a data-parallel group's whole batch: the sums added
 * over the ranks, count = all their rows): dy = gamma*rstd * (dz - sum_dz/count - xhat*sum_dzx/count).  The quotient is formed on
 * the device as in umi_bn_bwd_apply, which is this call with count = M. */
int umi_bn_bwd_apply_count(void* da, int ldda, const void* y, int ldy, const void* tx,
                           const float* rstd, const float* sum_dz, const float* sum_dzx,
                           long M, long count, int C, int dtype, umi_stream_t stream);

/* Fusion of the two previous steps for a DoubleConv's inner layer (reference Model.py:15-22): the 3x3 data gradient that
 * produces `da` = d(activated output) of a BatchNorm+ReLU layer also emits stage 1 of that layer's reduction
 * (`ybn`/`txbn`/`rstd` = that layer's raw output, transform and 1/std): part[rows][2][Co] per-tile sums of dz and
 * dz*xhat, rows = umi_conv_fwd_plan(...)'s stat_rows.  umi_bn_bwd_from_partials finishes the reduction; umi_bn_bwd_apply
 * follows as usual.  Returns UMI_ERR_UNSUPPORTED off the MFMA path (caller falls back to the separate calls). */
int umi_conv_dgrad_bnred(const void* dy, int lddy, const void* wp8, void* da, int ldda, const void* ybn, int ldybn,
                         const void* txbn, const float* rstd, float* part, int N, int H, int W, int Ci, int Co,
                         int dtype, umi_stream_t stream);

/* The same fusion for the data gradients that run on the pointwise / tap-gather matrix-core kernel -- ConvTranspose2d(2,2)'s
 * (a stride-2 2x2 conv over d(up), reference Model.py:56-57 under autograd), 1x1 convs', strided convs' (UMI_CONV_DGRAD_STRIDED):
 * y = conv(x, wp8) as umi_conv_fwd computes it, plus part[rows][2][Co] of the BatchNorm(+ReLU) layer whose activated output y is
 * the gradient of.  rows = umi_conv_gather_bnred_rows(...); 0 = the problem is not on that kernel (use the separate calls). */
int umi_conv_gather_bnred_rows(int N, int H, int W, int Ci, int Co, int R, int S, int stride, int pad, int Ho, int Wo,
                               int ldx, int ldy, int dtype, int flags);
int umi_conv_gather_bnred(const void* x, int ldx, const void* wp8, void* y, int ldy, const void* ybn, int ldybn,
                          const void* txbn, const float* rstd, float* part, int N, int H, int W, int Ci, int Co, int R, int S,
                          int stride, int pad, int Ho, int Wo, int dtype, int flags, umi_stream_t stream);

/* The same fusion for the data gradient of the narrow pointwise head (`OutConv`, reference Model.py:89-93; Ci <= 8 logit channels):
 * da[p][c] = sum_k dl[p][k] * w[k][c] plus part[rows][2][Co], rows = umi_head_dgrad_bnred_rows(...) (0 = shape not taken, call
 * umi_conv_fwd and umi_bn_bwd_reduce).  wp: the generic [1][Ci][Co] fp16 packing (umi_pack_kn). */
int umi_head_dgrad_bnred_rows(long P, int Ci, int Co, int ldda, int dtype);
int umi_head_dgrad_bnred(const void* dl, int lddl, const void* wp, void* da, int ldda, const void* ybn, int ldybn,
                         const void* txbn, const float* rstd, float* part, long P, int Ci, int Co, int dtype,
                         umi_stream_t stream);
/* ... and the head's weight gradient from the same pass (its input is the activated ybn): dW[k * s_co + c * s_ci] <- out_scale *
 * sum_p tx(ybn[p][c]) * dl[p][k] (k < Ci logit channels, c < Co feature channels).  ws: umi_head_bwd_fused_ws_bytes.
 * Co <= 256; UMI_ERR_UNSUPPORTED (nothing launched) above that or where umi_head_dgrad_bnred_rows is 0. */
size_t umi_head_bwd_fused_ws_bytes(long P, int Ci, int Co);
int umi_head_bwd_fused(const void* dl, int lddl, const void* wp, void* da, int ldda, const void* ybn, int ldybn,
                       const void* txbn, const float* rstd, float* part, float* dW, long s_co, long s_ci, float out_scale,
                       void* ws, size_t ws_bytes, long P, int Ci, int Co, int dtype, umi_stream_t stream);

/* Inference form of Conv2d(3, pad 1, bias=False) -> BatchNorm2d (running statistics) -> ReLU (reference Model.py:15-22 under
 * model.eval(), the evaluation loop test_mc3serousv5.py:877-887): the layer's own transform out_tx[Co] = {mean, scale, shift,
 * lo} is applied to the fp32 accumulators in the epilogue, y = max(scale * conv(tx(x), w) + shift, lo) is stored ACTIVATED
 * and consumed without a transform; no statistics are produced.  fp16, matrix-core shapes only (UMI_ERR_UNSUPPORTED
 * otherwise: use umi_conv_fwd + the consumer-side transform). */
int umi_conv3x3_fwd_act(const void* x, int ldx, const void* tx, const void* wp8, const void* out_tx, void* y, int ldy,
                        int N, int H, int W, int Ci, int Co, int dtype, umi_stream_t stream);
/* The same fusion on the other producer of such a gradient: MaxPool2d(2) backward (reference Model.py:36) routes `dpool` into
 * `da` (accumulate != 0: adds to the skip-connection gradient already there) and, being the LAST contribution to `da`, also
 * emits stage 1 of the BatchNorm backward of the pooled layer (x = its raw output, tx / rstd its transform and 1/std):
 * part[rows][2][C], rows = umi_pool2_bwd_bnred_stat_rows().  fp16, even H and W, C % 8 == 0; else UMI_ERR_UNSUPPORTED
 * (caller uses umi_pool2_bwd + umi_bn_bwd_reduce). */
/* BatchNorm batch statistics of a stored fp16 tensor (for a producer without a statistics epilogue: the pointwise MFMA conv
 * of the attention gates, reference Model.py:268-289): part[rows][2][C] = per-block sums / sums of squares, the layout
 * umi_bn_finalize consumes; rows = umi_bn_stats_rows(M, C) (0 = unsupported: C % 8 != 0). */
int umi_bn_stats_rows(long M, int C);
int umi_bn_stats(const void* x, int ldx, float* part, long M, int C, int dtype, umi_stream_t stream);
int umi_pool2_bwd_bnred_stat_rows(int N, int H, int W, int C);
int umi_pool2_bwd_bnred(const void* dpool, int lddp, const void* x, int ldx, const void* tx, const float* rstd, void* da,
                        int ldda, int accumulate, float* part, int N, int H, int W, int C, int dtype, umi_stream_t stream);
int umi_bn_bwd_from_partials(const float* part, int rows, int C, float* sum_dz, float* sum_dzx, umi_stream_t stream);

/* Weight gradient of umi_conv_fwd (autograd of the reference convs):
 *   dW[co*s_co + ci*s_ci + t*s_t] = out_scale * sum_{n,ho,wo} txa(x[...,ci]) * txb(dy[n,ho,wo,co])
 * fp32 output in the parameter's own layout (OIHW: s_co=Ci*R*S, s_ci=R*S, s_t=1).
 * Deterministic: split-K partial slabs in `ws`, reduced in fixed order.  `flags`: UMI_CONV_FORCE_GENERIC, UMI_CONV_F32_MFMA
 * and UMI_CONV_F32_MFMA_1X1 (pass the same flags to umi_conv_wgrad_ws_bytes: the fp32 matrix-core kernels split the pixels their
 * own way).  The split rule of the pointwise fp32 matrix-core kernel: the M = N * Ho * Wo rows are cut into chunks of 32; with
 * tiles = ceil(Ci / TI) * ceil(Co / TJ), TI = 64 if Ci <= 64 else 128 and TJ likewise from Co, it wants ceil(512 / tiles) splits
 * but at most ceil(chunks / 4), at least 1; a split is ceil(chunks / wanted) consecutive chunks, splits = ceil(chunks / that), and
 * the workspace is splits slabs of Ci * Co fp32 values, [split][1][Ci][Co].  UMI_CONV_F32_MFMA_2X2 is a flag of this call too (the
 * ConvTranspose2d weight gradient: x = d(up) [N, 2 Ho, 2 Wo, Ci], dy = the ConvT's input [N, Ho, Wo, Co], txb its transform).  Its
 * split rule is the same with the four taps counted as tiles: the M = N * Ho * Wo pixels are cut into chunks of 32; with tiles =
 * 4 * ceil(Ci / TI) * ceil(Co / TJ), TI and TJ as above, it wants ceil(512 / tiles) splits but at most ceil(chunks / 4), at least 1;
 * a split is ceil(chunks / wanted) consecutive chunks, splits = ceil(chunks / that), and the workspace is splits slabs of
 * 4 * Ci * Co fp32 values, [split][4][Ci][Co]; umi_conv_wgrad_ws_bytes gives the larger of that and the flag-less answer.
 * Summation orders of the three 2x2 kernels (every output ONE fmaf chain, no atomics, identical inputs give identical bits):
 *   forward        k ascending over 0 .. Cin - 1, the bias added once after the chain;
 *   data gradient  taps ascending (t = 2 r + s), channels ascending inside a tap, one accumulator across the four taps;
 *   weight grad.   pixels ascending in (n, ho, wo) order inside a split, one accumulator per (tap, ci, co) and split, then the
 *                  splits' slabs summed by the shared reduction in its fixed order. */
size_t umi_conv_wgrad_ws_bytes(int N, int Ho, int Wo, int Ci, int Co, int R, int S, int dtype, int flags);
int umi_conv_wgrad(const void* x, int ldx, const void* txa, const void* dy, int lddy, const void* txb,
                   float* dW, long s_co, long s_ci, long s_t, float out_scale,
                   int N, int H, int W, int Ci, int Co, int R, int S, int stride, int pad,
                   int Ho, int Wo, int dtype, int flags, void* ws, size_t ws_bytes, umi_stream_t stream);
/* umi_conv_wgrad with its final split-K reduction recorded instead of launched: a reduction is a ~8-us launch over a few
 * hundred KB, a U-Net step has 22 and a TransUNet step 62; umi_wgrad_reduce_group runs 16 per launch (same arithmetic and
 * order, identical results).  `ws` must be the call's own and stay untouched until then.  out->part == NULL: the path taken
 * reduces inside its kernel, dW is already final. */
typedef struct umi_wgrad_pending {
    const float* part;
    float* dW;
    long s_co, s_ci, s_t;
    float scale;
    int splits, RS, Ci, Co;
} umi_wgrad_pending;
int umi_conv_wgrad_deferred(const void* x, int ldx, const void* txa, const void* dy, int lddy, const void* txb,
                            float* dW, long s_co, long s_ci, long s_t, float out_scale, int N, int H, int W, int Ci, int Co,
                            int R, int S, int stride, int pad, int Ho, int Wo, int dtype, int flags, void* ws, size_t ws_bytes,
                            umi_wgrad_pending* out, umi_stream_t stream);
/* UMI_ERR_BADARG (nothing launched, no dW written) if ANY of the n entries has a null part / dW or splits, RS, Ci or Co <= 0. */
int umi_wgrad_reduce_group(int n, const void* items /* umi_wgrad_pending[n], host */, umi_stream_t stream);
/* Weight AND bias gradient of ConvTranspose2d(2,2) (reference Model.py:56-57 under autograd) in one pass over d(up): the arguments of
 * umi_conv_wgrad_deferred for that layer (x = d(up) [N,H,W,Ci], dy = the ConvT's input [N,Ho,Wo,Co] with its transform txb) plus
 * dbias[Ci] <- out_scale * column sums of x.  `out` NULL: the split-K reduction runs at once.  UMI_ERR_UNSUPPORTED (nothing
 * launched) where the 2x2 / stride-2 matrix-core kernel does not apply: umi_colsum + umi_conv_wgrad. */
int umi_conv_wgrad_bias(const void* x, int ldx, const void* dy, int lddy, const void* txb, float* dW, long s_co, long s_ci,
                        long s_t, float* dbias, float out_scale, int N, int H, int W, int Ci, int Co, int Ho, int Wo, int dtype,
                        int flags, void* ws, size_t ws_bytes, umi_wgrad_pending* out, umi_stream_t stream);
/* umi_conv_wgrad (R = S = 1, no transforms) for `n` layers of one shape in one launch: the per-layer weight gradients of a
 * ViT encoder (reference vit_seg_modeling.py:58-62,100-101, twelve Blocks), whose pixel dimension (tokens) is too short to
 * fill the chip one layer at a time without a deep split-K.  x / dy / dW: HOST arrays of n device pointers.  No workspace,
 * deterministic.  UMI_ERR_UNSUPPORTED where the pointwise matrix-core kernel does not apply (call umi_conv_wgrad per layer). */
int umi_conv_wgrad_group(int n, const void* const* x, int ldx, const void* const* dy, int lddy, float* const* dW, long s_co,
                         long s_ci, float out_scale, long M, int Ci, int Co, int dtype, umi_stream_t stream);
/* umi_conv_wgrad of a 3x3/stride-1/pad-1 conv fused with umi_bn_bwd_apply of the BatchNorm(+ReLU) that follows the conv
 * (reference Model.py:14-21 DoubleConv backward: autograd runs cudnn_batch_norm_backward, then convolution_backward):
 * `da` = gradient of the activated output (read only), `y`/`tx_bn`/`rstd`/`sum_dz`/`sum_dzx` as umi_bn_bwd_apply takes them;
 * `dz` (a separate tensor) receives exactly what umi_bn_bwd_apply would have left in `da` (dz == NULL: the layer's input takes no
 * gradient, nothing else reads dz -- accepted for the network's first conv, Ci <= 4, whose kernel then never stores it), dW what umi_conv_wgrad would
 * have produced from it.  UMI_ERR_UNSUPPORTED where the fused kernel does not apply (run the two calls instead). */
int umi_conv_wgrad_bnapply(const void* x, int ldx, const void* txa, const void* da, int ldda, const void* y, int ldy,
                           const void* tx_bn, const float* rstd, const float* sum_dz, const float* sum_dzx, void* dz,
                           int lddz, float* dW, long s_co, long s_ci, long s_t, float out_scale, int N, int H, int W,
                           int Ci, int Co, int R, int S, int stride, int pad, int dtype, int flags, void* ws,
                           size_t ws_bytes, umi_stream_t stream);
/* The same with the divisor of the two sums given separately, as umi_bn_bwd_apply_count takes it (umi_conv_wgrad_bnapply is this
 * call with count = N * H * W). */
int umi_conv_wgrad_bnapply_count(const void* x, int ldx, const void* txa, const void* da, int ldda, const void* y, int ldy,
                                 const void* tx_bn, const float* rstd, const float* sum_dz, const float* sum_dzx, void* dz,
                                 int lddz, float* dW, long s_co, long s_ci, long s_t, float out_scale, int N, int H, int W,
                                 int Ci, int Co, int R, int S, int stride, int pad, int dtype, int flags, long count, void* ws,
                                 size_t ws_bytes, umi_stream_t stream);

/* Per-channel sum over pixels (bias gradients): out[c] = out_scale * sum_p x[p, c]. */
size_t umi_colsum_ws_bytes(long M, int C);
int umi_colsum(const void* x, int ldx, float* out, float out_scale, long M, int C, int dtype,
               void* ws, size_t ws_bytes, umi_stream_t stream);
/* umi_colsum for n fp16 tensors of one shape (C % 8 == 0) in two launches per 16: the bias gradients of a ViT's twelve
 * encoder layers.  xs / outs: HOST arrays of device pointers; ws >= min(n,16) * umi_colsum_ws_bytes(M, C).
 * UMI_ERR_UNSUPPORTED where the vectorised kernel does not apply (call umi_colsum per tensor). */
int umi_colsum_group(int n, const void* const* xs, int ldx, float* const* outs, float out_scale, long M, int C, int dtype,
                     void* ws, size_t ws_bytes, umi_stream_t stream);

/* Materialise an activation (storage + consumer transform) as NCHW fp32: the tensor a
 * reference block returns (e.g. DoubleConv.forward, reference Model.py:25-26). */
int umi_materialize_nchw(const void* x, int ldx, const void* tx, float* y_nchw,
                         int N, int H, int W, int C, int dtype, umi_stream_t stream);

/* ---- TransUNet path (reference TransUnet/vit_seg_modeling.py, vit_seg_modeling_resnet_skip.py) -------------------- */

/* StdConv2d weight standardisation and its backward (resnet_skip.py:20-23): per output channel over K = Ci*R*S,
 * biased variance, w_std = (w - mean) / sqrt(var + eps). fp32 parameters. */
int umi_wstd_fwd(const float* w, float* wstd, float* rstd, int Co, int K, float eps, umi_stream_t stream);
int umi_wstd_bwd(const float* wstd, const float* rstd, const float* g, float* dw, int Co, int K, umi_stream_t stream);
/* The same for ALL StdConv2d layers of a model in one launch each way (a R50 hybrid has 52).  `descs`: DEVICE array sorted
 * by blk0; an entry owns Co workgroups.  Backward: the gradient w.r.t. the standardised weights of entry i is read at
 * g_base + off, the parameter gradient written at dw_base + off (flat per-step buffers, so the table never changes) or,
 * where the entry's `dw` is not NULL, there (e.g. the parameter's slot in a data-parallel gradient bucket). */
typedef struct umi_wstd_desc {
    const float* w;
    float* ws;
    float* rstd;
    long off;
    int Co, K;
    float eps;
    int blk0;
    float* dw;
} umi_wstd_desc;
int umi_wstd_fwd_multi(const void* descs, int n_desc, int total_rows, umi_stream_t stream);
int umi_wstd_bwd_multi(const void* descs, int n_desc, int total_rows, const float* g_base, float* dw_base, umi_stream_t stream);

/* GroupNorm (+ optional residual add, + optional ReLU) on NHWC, y = [relu](gn(x) [+ res]) (resnet_skip.py:47-58,68-73).
 * mean/rstd: [N*G] saved for backward.  Backward: dx (and dres = masked dy when dres != NULL), dgamma/dbeta scaled by
 * out_scale; `y` is the forward OUTPUT (ReLU mask).
 * part_out (backward): NULL, or [N][2][C] floats that receive the per-sample sums (dz*xhat, dz) per channel; dgamma / dbeta
 * may then be NULL and are formed later for many layers at once by umi_gn_param_grads_group (parts / dgammas / dbetas: HOST
 * arrays of n device pointers, Cs: n channel counts; out[c] = out_scale * sum over the N samples). */
size_t umi_gn_fwd_ws_bytes(int N, long HW, int C);
int umi_gn_fwd(const void* x, int ldx, const float* gamma, const float* beta, const void* res, int ldr, void* y, int ldy,
               float* mean, float* rstd, int relu, int N, long HW, int C, int G, float eps, int dtype,
               void* ws, size_t ws_bytes, umi_stream_t stream);
size_t umi_gn_bwd_ws_bytes(int N, long HW, int C, int G);
int umi_gn_bwd(const void* dy, int lddy, const void* y, int ldy, const void* x, int ldx, const float* mean,
               const float* rstd, const float* gamma, int relu, void* dx, int lddx, void* dres, int lddr,
               float* dgamma, float* dbeta, float out_scale, int N, long HW, int C, int G, int dtype,
               void* ws, size_t ws_bytes, float* part_out, umi_stream_t stream);
int umi_gn_param_grads_group(int n, const float* const* parts, const int* Cs, int N, float* const* dgammas,
                             float* const* dbetas, float out_scale, umi_stream_t stream);

/* MaxPool2d(kernel 3, stride 2, pad 0) (resnet_skip.py:147) and its backward (first-max tie rule).
 * idx: NULL, or N*Ho*Wo*C bytes (8-byte aligned, fp16 with C % 8 == 0 only: UMI_ERR_UNSUPPORTED otherwise) in which the forward
 * records the winning tap 0..8 of every output element; a backward given the same buffer reads it instead of re-deriving
 * every window's maximum from the input. */
int umi_pool3s2_fwd(const void* x, int ldx, void* y, int ldy, void* idx, int N, int H, int W, int C, int dtype,
                    umi_stream_t stream);
int umi_pool3s2_bwd(const void* dy, int lddy, const void* x, int ldx, const void* idx, void* dx, int lddx, int N, int H, int W,
                    int C, int dtype, umi_stream_t stream);

/* LayerNorm over the last dim (vit_seg_modeling.py:172-173,232; eps 1e-6) and backward.  * umi_ln_bwd with dgamma == dbeta == NULL leaves its partial rows [*rows_out][2][C] in `ws` (then a buffer of the caller's
 * that stays alive) for umi_gn_param_grads_group (N = *rows_out) to sum for many layers in one launch. */
int umi_ln_fwd(const void* x, int ldx, const float* gamma, const float* beta, void* y, int ldy, float* mean, float* rstd,
               long M, int C, float eps, int dtype, umi_stream_t stream);
size_t umi_ln_bwd_ws_bytes(long M, int C);
int umi_ln_bwd(const void* dy, int lddy, const void* x, int ldx, const float* gamma, const float* mean,
               const float* rstd, void* dx, int lddx, float* dgamma, float* dbeta, float out_scale, long M, int C,
               int dtype, void* ws, size_t ws_bytes, int* rows_out, umi_stream_t stream);

/* Elementwise: mode 0 y = gelu(x) (exact erf form, vit_seg_modeling.py:115); 1 y = g * gelu'(x); 2 y = x + g;
 * 3 y = x + g[row % bcast_rows] (position embedding, vit_seg_modeling.py:163). */
int umi_elementwise(int mode, const void* x, int ldx, const void* g, int ldg, void* y, int ldy, long M, int C,
                    long bcast_rows, int dtype, umi_stream_t stream);

/* Dropout (vit_seg_modeling.py:103,151; U-Net Down / Up, Model.py:37,80-81): forward writes a byte mask (own counter-based
 * RNG stream) and y = keep ? tx(x) / (1-p) : 0 (tx: nullable consumer transform of x, forward only); backward (x = dy)
 * reuses the mask.  0 <= p <= 1 (UMI_ERR_BADARG otherwise, NaN included), here and in umi_dropout_fused / umi_linear_fused;
 * p == 1 keeps nothing, as nn.Dropout(1.0): y = 0 (the residual alone in the fused forms), a zero gradient, nothing non-finite.
 * Stream: keep = u >= p with u = (hash32(e, seed') >> 8) * 2^-24, e = row * C + col (dense index: no ld enters; its high word
 * is xor-ed into seed'), seed' = seed + seed_dev[0] * 0x9E3779B9; tests/dropout_stream.py states it in full.
 * seed_dev (nullable): device counter added into the stream seed inside the kernel, so a step replayed
 * from a captured HIP graph still draws a fresh mask every replay. */
int umi_dropout(const void* x, int ldx, void* y, int ldy, void* mask, int backward, float p, unsigned seed, long M, int C,
                int dtype, const void* tx, const unsigned* seed_dev, umi_stream_t stream);
/* umi_dropout fused with the GELU before it and / or the residual add after it (the MLP and the two residual joins of a
 * transformer Block, reference vit_seg_modeling.py:113-119,177-187); fp16 with C % 8 == 0 only (UMI_ERR_UNSUPPORTED otherwise):
 *   forward : y = dropout(gelu ? GELU(x) : x) + (aux ? aux : 0)
 *   backward: y = dropout'(x) * (gelu ? GELU'(aux) : 1), aux = the forward's x.  Same mask bytes / random stream as umi_dropout. */
int umi_dropout_fused(const void* x, int ldx, void* y, int ldy, void* mask, int backward, float p, unsigned seed, long M, int C,
                      int dtype, const unsigned* seed_dev, const void* aux, int ldaux, int gelu, umi_stream_t stream);

/* Multi-head softmax attention (vit_seg_modeling.py:73-91): q,k,v,o are [B, N, heads*D] token tensors (row stride ld),
 * head h = channels [h*D, (h+1)*D); softmax(q k^T / sqrt(D)) v.  lse/delta: [B*heads*N] fp32 scratch kept for backward.
 * Three kernel families serve these calls (umi_attn_plan names the one a call takes): the VALU kernels (D = 16, 32, 64; fp32 and
 * fp16), the fp16 matrix-core kernels (D = 64) and, opt-in, the fp32 matrix-core kernels (D = 64).  Dropout on the probabilities:
 * umi_attn_fwd_dropout / umi_attn_bwd_dropout below, in all three. */
int umi_attn_fwd(const void* q, const void* k, const void* v, int ld, void* o, int ldo, float* lse, int B, int N, int heads,
                 int D, int dtype, umi_stream_t stream);
int umi_attn_bwd(const void* q, const void* k, const void* v, int ld, const void* o, const void* dO, int ldo,
                 const float* lse, void* dq, void* dk, void* dv, int ldd, float* delta, int B, int N, int heads, int D,
                 int dtype, umi_stream_t stream);
/* umi_attn_fwd_flags / umi_attn_bwd_flags flags */
enum { UMI_ATTN_F32_MFMA = 1 /* opt-in: fp32 attention runs on the fp32-input matrix-core instruction (v_mfma_f32_32x32x2_f32,
                                csrc/attention_mfma_f32.hip: the fp16 kernels' forward / dQ / dKV decomposition, fp32 operands, the
                                same log-sum-exp definition as the VALU kernels, so a forward of either feeds a backward of the
                                other; no atomics, nothing allocated at launch).  Taken when dtype is UMI_F32, D = 64, ld, ldo and
                                (backward) ldd are multiples of 4 and every tensor address is 16-byte aligned; any B, N, heads.
                                IGNORED otherwise, like the two convolution flags: the call then runs exactly as without it */ };
/* The two calls above with `flags` before the stream; flags = 0 is the call above, bit for bit. */
int umi_attn_fwd_flags(const void* q, const void* k, const void* v, int ld, void* o, int ldo, float* lse, int B, int N, int heads,
                       int D, int dtype, int flags, umi_stream_t stream);
int umi_attn_bwd_flags(const void* q, const void* k, const void* v, int ld, const void* o, const void* dO, int ldo,
                       const float* lse, void* dq, void* dk, void* dv, int ldd, float* delta, int B, int N, int heads, int D,
                       int dtype, int flags, umi_stream_t stream);
/* Host only, launches nothing: the selector of the calls above.  *kernel = 0 the VALU kernels, 1 the fp16 matrix-core kernels
 * (UMI_F16, D = 64, strides % 8 == 0, 16-byte aligned addresses; no flag needed), 2 the fp32 matrix-core kernels.  ldd = 0 (a
 * forward call) and null pointers mean "not given, assume fine"; a backward call also looks at dO, dq, dk and dv, which share
 * o's and the gradients' strides.  A call whose plan names 2 never falls back.  UMI_ERR_BADARG for N <= 0, heads <= 0, an
 * unknown dtype or a null `kernel`; UMI_ERR_UNSUPPORTED where no kernel serves D (the VALU kernels know 16, 32 and 64). */
int umi_attn_plan(int N, int heads, int D, int ld, int ldo, int ldd, int dtype, int flags, const void* q, const void* k,
                  const void* v, const void* o, int* kernel);
/* Attention-probability dropout (reference vit_seg_modeling.py:78,86-88: nn.Dropout on the softmax probabilities), in every
 * kernel family.  With P = softmax(q k^T / sqrt(D)), M the keep mask and Z = M / (1 - p):
 *   forward : o = (P o Z) v.  lse is the undropped softmax's, bit for bit what the call without dropout stores: only the operand
 *             of the P.v product is masked, and the final scale is 1 / (rowsum * (1 - p)).
 *   backward: delta = rowsum(dO o o) (o already carries Z); dS = P o (Z o (dO v^T) - delta); dq = scale dS k; dk = scale dS^T q;
 *             dv = (P o Z)^T dO.
 * The mask is never stored: each of the three kernels of a family regenerates its bits, in registers, from umi_dropout's stream
 * on the dense [B * heads * N, N] tensor of probabilities -- element e = ((b * heads + h) * N + i) * N + j in 64 bits (the high
 * word enters as umi_dropout states), seed' = seed + seed_dev[0] * 0x9E3779B9, keep iff u >= p.  So a forward and its backward
 * must be given the same (p, seed, *seed_dev); seed_dev (nullable) is read inside the kernels, a replayed graph draws fresh masks.
 * The kernel is umi_attn_plan's: dropout never changes the selection (a call whose plan names 2 still never falls back), and
 * D must be one the selected family knows (UMI_ERR_UNSUPPORTED otherwise).  0 <= p <= 1, UMI_ERR_BADARG otherwise (NaN
 * included) before anything else is looked at; p == 0 IS umi_attn_fwd_flags / umi_attn_bwd_flags, bit for bit; p == 1 keeps
 * nothing: o = 0, dq = dk = dv = 0, nothing non-finite.  No atomics, nothing allocated at launch, no static device state. */
int umi_attn_fwd_dropout(const void* q, const void* k, const void* v, int ld, void* o, int ldo, float* lse, int B, int N, int heads,
                         int D, int dtype, int flags, float p, unsigned seed, const unsigned* seed_dev, umi_stream_t stream);
int umi_attn_bwd_dropout(const void* q, const void* k, const void* v, int ld, const void* o, const void* dO, int ldo,
                         const float* lse, void* dq, void* dk, void* dv, int ldd, float* delta, int B, int N, int heads, int D,
                         int dtype, int flags, float p, unsigned seed, const unsigned* seed_dev, umi_stream_t stream);

/* UpsamplingBilinear2d(scale_factor=2), align_corners=True (vit_seg_modeling.py:307): forward x[N,H,W,C] -> y[N,2H,2W,C];
 * backward (x = dy [N,2H,2W,C]) -> y = dx [N,H,W,C] (deterministic gather form). */
int umi_bilinear2x(const void* x, int ldx, const void* tx, void* y, int ldy, int backward, int N, int H, int W, int C,
                   int dtype, umi_stream_t stream);   /* tx: consumer transform of x, forward only (nullable) */

/* Patch gather of the pure-ViT variants (vit_seg_modeling.py:137-140: Conv2d(C, hidden, kernel_size=P, stride=P) on the image): the
 * non-overlapping patches of a contiguous NCHW tensor x[B][C][H][W] as the token-major rows of that convolution's GEMM,
 *   rows[(b*gh + ty)*gw + tx][(c*P + ky)*P + kx] = x[b][c][ty*P + ky][tx*P + kx],  gh = H / P, gw = W / P (integer division),
 * M = B*gh*gw rows of K = C*P*P elements, row stride ld >= K (elements).  The column order is PyTorch's flattening of a
 * [hidden][C][P][P] weight.  in_dtype -> out_dtype: any of UMI_F32 / UMI_F16 each; fp32 -> fp16 rounds to nearest even, equal
 * types copy.  Image rows from gh*P and columns from gw*P on are never read; nothing outside rows[0:M][0:K] is written.  Any
 * P >= 1, C >= 1; 64-bit addressing.  16-byte accesses when P, W and ld are multiples of 16 / sizeof(in) elements and both
 * addresses are aligned to their access, element-wise otherwise with the same result.  No LDS, no atomics.
 * UMI_ERR_BADARG (nothing launched): a null pointer, B, C, H, W or P <= 0, P > H or P > W (no patch), ld < K, an unknown dtype.
 * UMI_ERR_UNSUPPORTED: C*P*P or H*W >= 2^31. */
int umi_patch_rows(const void* x, int in_dtype, void* rows, long ld, int out_dtype, int B, int C, int H, int W, int P,
                   umi_stream_t stream);

/* Fused training loss 'dice_bce_mc' (reference loss.py:488-500, DiceLoss loss.py:215-251) on NCHW fp32 logits [N,C,HW],
 * C <= 8: 0.5 * CrossEntropy + 0.5 * mean_c(1 - (2*sum(p*t)+1e-5)/(sum(p*p)+sum(t*t)+1e-5)), p = softmax(logits).
 * target [N,HW] class indices; target_dtype 0 = int64, 1 = float32, 2 = uint8, 3 = int32.
 * fwd fills stats[3*C + 2] = {sum p*t | sum p*p | sum t | CE sum | loss}; bwd writes dlogits = gout[0] * d loss / d logits
 * (gout: device pointer to the upstream scalar gradient, or NULL for 1). */
size_t umi_dice_ce_ws_bytes(int N, int C, long HW);
int umi_dice_ce_fwd(const float* logits, const void* target, int target_dtype, int N, int C, long HW, float* stats, void* ws,
                    size_t ws_bytes, umi_stream_t stream);
int umi_dice_ce_bwd(const float* logits, const void* target, int target_dtype, const float* stats, const float* gout, int N,
                    int C, long HW, float* dlogits, umi_stream_t stream);
/* The forward of `items` independent losses in one pass (a validation group: per-item figures from one batched forward).
 * logits [items*n, C, HW] and target [items*n, HW] hold `items` consecutive groups of n images; stats is [items][3*C + 2], and row i
 * holds the bits umi_dice_ce_fwd leaves for N = n on the i-th slice: the same block decomposition per item (grid = items x that
 * call's grid), the same float64 fixed-order sums (one finalize block per item), no atomics.  Forward only.
 * ws: umi_dice_ce_items_ws_bytes(items, n, C, HW) bytes = items x umi_dice_ce_ws_bytes(n, C, HW); nothing else is written.
 * UMI_ERR_BADARG (nothing launched): a null pointer, items, n or HW <= 0, items > 65535, an unknown target_dtype;
 * UMI_ERR_UNSUPPORTED: C outside 1..8; UMI_ERR_WORKSPACE: ws_bytes too small. */
size_t umi_dice_ce_items_ws_bytes(int items, int n, int C, long HW);
int umi_dice_ce_fwd_items(const float* logits, const void* target, int target_dtype, int items, int n, int C, long HW,
                          float* stats, void* ws, size_t ws_bytes, umi_stream_t stream);
/* The same loss of a data-parallel group's WHOLE batch, every rank holding N of its images:
 *   umi_dice_ce_sums        sums[3*C + 1] (float64) = {sum p*t | sum p*p | sum t | CE sum} of this rank's pixels, added in
 *                           umi_dice_ce_fwd's order; the ranks then add their sums and their pixel counts;
 *   umi_dice_ce_finalize    stats[3*C + 2] as umi_dice_ce_fwd leaves them, from such sums and the pixel count they cover (with this
 *                           rank's own sums and N * HW: the bits of umi_dice_ce_fwd);
 *   umi_dice_ce_bwd_global  dlogits = gout[0] * scale * d(loss of the stats) / d(this rank's logits): the Dice coefficients from
 *                           `stats`, the cross-entropy weight 0.5 / count.  scale = the group's size makes the AVERAGE of the ranks'
 *                           parameter gradients the gradient of the group's loss.  umi_dice_ce_bwd is this call with scale = 1 and
 *                           count = N * HW. */
int umi_dice_ce_sums(const float* logits, const void* target, int target_dtype, int N, int C, long HW, double* sums, void* ws,
                     size_t ws_bytes, umi_stream_t stream);
int umi_dice_ce_finalize(const double* sums, int C, double count, float* stats, umi_stream_t stream);
int umi_dice_ce_bwd_global(const float* logits, const void* target, int target_dtype, const float* stats, const float* gout,
                           float scale, double count, int N, int C, long HW, float* dlogits, umi_stream_t stream);

/* HausdorffDTLoss (reference loss.py:146-212) on fp32 logits `pred` and targets [B,C,H,W], C == 1, 1 <= H, W <= 4096,
 * B <= 65535:
 * s = sigmoid(pred); field(x)[b] = exact Euclidean distance of each pixel to the nearest pixel of the other class of
 * x[b] > 0.5 (0 if x[b] has no foreground, sqrt(1 + h^2 + w^2) if it has no background, as scipy's edt of the (1,H,W) slice);
 * D = field(s)^alpha + field(target)^alpha; loss = mean((s - target)^2 * D), summed in a fixed order (deterministic).
 * fwd writes D[B*H*W], loss[1] and, if `fields` is not NULL, fields[2*B*H*W] = {field(s) | field(target)};
 * bwd writes dpred = gout[0] * 2 (s - t) s (1 - s) D / (B*H*W) (gout: device pointer, or NULL for 1). */
size_t umi_hdt_ws_bytes(int B, int H, int W);
int umi_hdt_fwd(const float* pred, const float* target, int B, int C, int H, int W, float alpha, float* D, float* fields,
                float* loss, void* ws, size_t ws_bytes, umi_stream_t stream);
int umi_hdt_bwd(const float* pred, const float* target, const float* D, const float* gout, int B, int C, int H, int W,
                float* dpred, umi_stream_t stream);

/* Binary-segmentation losses of the reference calc_loss (loss.py:442-516) on NCHW fp32 logits `pred`, s = sigmoid(pred),
 * bce = (1 - t) * pred - log_sigmoid(pred) per pixel.  Every sum is fixed-order with fp64 across threads (deterministic); the
 * workspace holds only per-call scratch, what the backward needs is in the caller's `stats` / `mask`.  gout: device pointer
 * to the upstream scalar gradient, or NULL for 1.  Limits: B <= 65535, B*C*HW < 2^31, C <= 8 (else UMI_ERR_UNSUPPORTED).
 *
 * 'dice_bce' (loss.py:484-487, BinaryDiceLoss :254-307): pred [B,1,HW], target fp32 [B,HW];
 *   loss = 0.5 * mean(bce) + 0.5 * mean_b(1 - (2*sum_b s*t + 1) / (sum_b |s| + sum_b |t| + 1)).
 *   fwd writes stats[5*B] (fp64, per image {sum s*t, sum s, sum |t|, sum t, sum bce}) and loss[1];
 *   bwd writes dpred = gout[0] * d loss / d pred from those stats.
 * 'Tversky' (loss.py:514-515, FocalTverskyLoss :380-420 with gamma 1): tv(TP, P, T) = (TP + 1) / (TP + alpha*(P - TP) +
 *   beta*(T - TP) + 1).  C == 1: target fp32 [B,HW] (target_dtype 1 only), TP = sum s*t, P = sum s, T = sum t over the batch,
 *   loss = 1 - tv, stats[5*B] as for dice_bce.  2 <= C <= 8: p = softmax(pred) over C, target [B,HW] labels (target_dtype
 *   0 = int64, 1 = float32, 2 = uint8, 3 = int32; a value that is not an integer in [0, C) matches no class),
 *   TP_c = sum p_c*[t==c], P_c = sum p_c, T_c = sum [t==c], loss = mean_c(1 - tv_c), stats[3*C] = {TP | P | T}.
 * umi_binloss_ws_bytes(B, C, HW) sizes the workspace of both forwards. */
size_t umi_binloss_ws_bytes(int B, int C, long HW);
int umi_dice_bce_fwd(const float* pred, const float* target, int B, long HW, double* stats, float* loss, void* ws,
                     size_t ws_bytes, umi_stream_t stream);
int umi_dice_bce_bwd(const float* pred, const float* target, const double* stats, const float* gout, int B, long HW,
                     float* dpred, umi_stream_t stream);
int umi_tversky_fwd(const float* pred, const void* target, int target_dtype, int B, int C, long HW, float alpha, float beta,
                    double* stats, float* loss, void* ws, size_t ws_bytes, umi_stream_t stream);
int umi_tversky_bwd(const float* pred, const void* target, int target_dtype, const double* stats, const float* gout, int B,
                    int C, long HW, float alpha, float beta, float* dpred, umi_stream_t stream);

/* Hard-pixel losses on fp32 logits `pred` and fp32 targets of N = B*H*W elements (C == 1, flat NCHW order), 1 <= k <= N < 2^31:
 * loss = sum of bce over the selected set / k.  mode 0 'TopK' (loss.py:445-446, TopKLoss :354-378): the k pixels of LOWEST
 * true-class probability sigmoid(pred) where trunc(t) == 1, 1 - sigmoid(pred) otherwise (the reference's gather index
 * t.long(); other values are an error there and count as 0 here), k = N // 2.  mode 1 'BCE_HEM' (loss.py:447-467): the k
 * pixels of LARGEST bce, k = 500.  The set is exact: a radix select on the fp32 key finds the threshold T and how many keys
 * equal to T are taken; among those, the lowest flat indices are.  Nothing is read back to the host.
 * fwd writes mask[N] (1 = selected, else 0) and loss[1]; bwd writes dpred = mask * gout[0] * (s - t) / k.
 * mask: 4-byte aligned for the vector path (any alignment works). */
size_t umi_topk_loss_ws_bytes(long N);
int umi_topk_loss_fwd(const float* pred, const float* target, long N, long k, int mode, unsigned char* mask, float* loss,
                      void* ws, size_t ws_bytes, umi_stream_t stream);
int umi_topk_loss_bwd(const float* pred, const float* target, const unsigned char* mask, const float* gout, long N, long k,
                      float* dpred, umi_stream_t stream);

/* Count-ratio-weighted two-task loss of the reference's multi_task_trainRatio (Trainer.py:1225-1249) on fp32 head outputs
 * o1, o2 [B,1,HW] and label maps l1, l2 [B,HW] (B <= 65535, B*HW < 2^31, else UMI_ERR_UNSUPPORTED):
 *   R_k = relu(o_k), L_k = mean((R_k - l_k)^2), rG_b = G1_b / (G2_b + G1_b), rP_b = P1_b / (P2_b + P1_b) with G_k,b = sum of
 *   l_k over image b and P_k,b = sum of R_k; r = mean_b |rG_b - rP_b|; loss = (L1 + L2) * (1 + 10 r) if `gate`, else L1 + L2.
 * gate_dev (device, nullable): if given, gate = (gate_dev[0] != 0), read by the kernel, so a captured graph follows it.
 * A zero denominator makes r NaN, as in torch.  Sums are fp32 per thread, then fp64 in a fixed order (deterministic).
 * fwd writes loss, loss1, loss2, ratio (fp32 scalars) and stats[umi_mt_ratio_stats_len(B)] (fp64: per image the six sums
 * {S1, S2, P1, P2, G1, G2} at [6b..6b+5], s_b = sgn(rG_b - rP_b) at [6B + b] with sgn(NaN) = 0, {L1, L2, r, gate} at [7B..]).
 * bwd writes, with {gL, g1, g2, gr} = gout[0..3] (device; NULL for {1, 0, 0, 0}) the upstream gradients of the four scalars,
 * N = B*HW, wL = gL (1 + 10 r gate), cr = gL 10 gate (L1 + L2) + gr:
 *   d1 = [o1 > 0] ((wL + g1) 2 (R1 - l1) / N - cr s_b P2_b / (B (P1_b + P2_b)^2)),
 *   d2 = [o2 > 0] ((wL + g2) 2 (R2 - l2) / N + cr s_b P1_b / (B (P1_b + P2_b)^2)). */
size_t umi_mt_ratio_ws_bytes(int B, long HW);
size_t umi_mt_ratio_stats_len(int B);
int umi_mt_ratio_fwd(const float* o1, const float* o2, const float* l1, const float* l2, int B, long HW, int gate,
                     const float* gate_dev, double* stats, float* loss, float* loss1, float* loss2, float* ratio, void* ws, size_t ws_bytes,
                     umi_stream_t stream);
int umi_mt_ratio_bwd(const float* o1, const float* o2, const float* l1, const float* l2, const double* stats,
                     const float* gout, int B, long HW, float* d1, float* d2, umi_stream_t stream);

/* Multi-tensor optimizer step: torch.optim.SGD / torch.optim.Adam arithmetic (reference train.py:341-347) on every parameter
 * tensor of a model in ONE launch.  `descs` is a DEVICE array of n_desc umi_optim_desc sorted by blk0; a tensor of n elements
 * occupies ceil(n / umi_optim_block_elems()) consecutive blocks starting at blk0; total_blocks = the sum.
 *   SGD:  g += wd*p; m = first_step ? g : momentum*m + (1-dampening)*g; g = nesterov ? g + momentum*m : m; p -= lr*g
 *         (s0 = momentum buffer, NULL when momentum == 0; s1 unused)
 *   Adam: g += wd*p; m += (1-beta1)*(g-m); v = beta2*v + (1-beta2)*g*g; p -= step_size * m / (sqrt(v)/bc2_sqrt + eps)
 *         (s0 = exp_avg, s1 = exp_avg_sq; step_size = lr / (1-beta1^t), bc2_sqrt = sqrt(1-beta2^t), computed by the host)
 *   AdamW (umi_optim_adamw_multi*, below): p *= (float)(1 - lr*wd), then Adam with wd = 0 */
typedef struct umi_optim_desc {
    float* p;            /* parameter (fp32 master), updated in place */
    const float* g;      /* gradient */
    float* s0;
    float* s1;
    long n;              /* elements */
    int blk0;
    int pad_;
} umi_optim_desc;
int umi_optim_block_elems(void);
/* Copies a descriptor table from PINNED (device-mapped) host memory to device memory with a kernel, so that the upload is a
 * plain kernel node inside a HIP-graph capture; nbytes and both pointers are multiples of 16. */
int umi_table_upload(const void* host_pinned, void* dev, size_t nbytes, umi_stream_t stream);
/* hyper-parameters are doubles (Python floats) and are rounded to fp32 where torch rounds them */
int umi_optim_sgd_multi(const void* descs, int n_desc, int total_blocks, double lr, double momentum, double dampening,
                        double weight_decay, int nesterov, int first_step, umi_stream_t stream);
int umi_optim_adam_multi(const void* descs, int n_desc, int total_blocks, double step_size, double beta1, double beta2,
                         double bc2_sqrt, double eps, double weight_decay, umi_stream_t stream);

/* Graph-safe hyper-parameters (reference Trainer.py:719-726: the poly learning-rate rule rewrites the LR after every step,
 * torch.optim.Adam advances `step` on the host).  A captured HIP graph freezes kernel ARGUMENTS, so the values that change
 * from step to step live in a device-resident umi_optim_hyper block per param group instead:
 *   umi_optim_hyper_pre   before the update: Adam t += 1, step_size_f = lr / (1 - beta1^t), bc2_sqrt_f = sqrt(1 - beta2^t)
 *                         (formed in double, rounded to fp32 as torch rounds its Python floats); lr_f = (float)lr
 *   umi_optim_*_multi_dev the same arithmetic as umi_optim_*_multi with lr / step_size / bc2_sqrt read from the block
 *   umi_optim_hyper_poly  after the update: lr = base_lr * (1 - iter / max_iter)^power; iter += 1  (pre-increment iter, as the
 *                         reference does)
 * The host fills the block once (umi_table_upload) and reads it back when it wants param_group['lr'] / state['step']. */
typedef struct umi_optim_hyper {
    double lr, base_lr, iter, max_iter, power, adam_t, beta1, beta2;
    float lr_f, step_size_f, bc2_sqrt_f;
    int kind;                              /* UMI_SCHED_*; read by umi_optim_hyper_schedule only */
    double warmup, final_ratio;            /* (kind, warmup, final_ratio all zero: a block as it was before the schedule rule) */
} umi_optim_hyper;                         /* 96 bytes */
size_t umi_optim_hyper_bytes(void);
int umi_optim_hyper_pre(void* hyper, int adam, umi_stream_t stream);
int umi_optim_hyper_poly(void* hyper, umi_stream_t stream);
/* Warm-up + decay schedule, run after the update of a group where umi_optim_hyper_poly would run (one thread, all in double):
 *     iter += 1;  lr = base_lr * factor(iter)
 *     factor(k) = w(k) * (final_ratio + (1 - final_ratio) * s(k))
 *     w(k) = warmup > 0 ? min(1, (k + 1) / warmup) : 1
 *     x    = min(k, max_iter) / max_iter
 *     s(k) = UMI_SCHED_POLY: (1 - x)^power   UMI_SCHED_COSINE: 0.5 * (1 + cos(pi * x))   UMI_SCHED_CONSTANT (and NONE): 1
 * Step k, counted from 0, uses base_lr * factor(k): unlike the poly rule above this one has no lag, so whoever fills the block
 * writes lr = base_lr * factor(iter) into it.  `iter` counts attempted steps: a step the guard skips advances it too. */
enum { UMI_SCHED_NONE = 0, UMI_SCHED_POLY = 1, UMI_SCHED_COSINE = 2, UMI_SCHED_CONSTANT = 3 };
int umi_optim_hyper_schedule(void* hyper, umi_stream_t stream);
int umi_optim_sgd_multi_dev(const void* descs, int n_desc, int total_blocks, const void* hyper, double momentum,
                            double dampening, double weight_decay, int nesterov, int first_step, umi_stream_t stream);
int umi_optim_adam_multi_dev(const void* descs, int n_desc, int total_blocks, const void* hyper, double beta1, double beta2,
                             double eps, double weight_decay, umi_stream_t stream);
/* AdamW (torch.optim.AdamW = Adam with decoupled_weight_decay): the Adam entry points with the weight decay taken out of the
 * gradient.  Per element, in torch's order:
 *     weight_decay != 0:  p = p * (float)(1 - lr * weight_decay)     (param.mul_(1 - lr * wd): lr and wd doubles, the factor
 *                                                                     formed in double, ONE rounding to fp32, one fp32 multiply)
 *     then the Adam update above with wd = 0.
 * `lr` is the learning rate of THIS step: the block's double `lr` when `hyper` is given (_dev; _guarded with hyper != NULL), the
 * `lr` argument otherwise (step_size = lr / (1 - beta1^t) does not determine it).  Descriptor table, blocks, 16-byte path and
 * status codes as for umi_optim_adam_multi*; the guarded form stores nothing on a skipped step, so it applies no decay either. */
int umi_optim_adamw_multi(const void* descs, int n_desc, int total_blocks, double lr, double step_size, double beta1,
                          double beta2, double bc2_sqrt, double eps, double weight_decay, umi_stream_t stream);
int umi_optim_adamw_multi_dev(const void* descs, int n_desc, int total_blocks, const void* hyper, double beta1, double beta2,
                              double eps, double weight_decay, umi_stream_t stream);

/* Guarded optimizer step: non-finite check, global gradient-norm clipping and a dynamic loss scale, all on the device so that a
 * captured HIP graph keeps deciding per step.  The state is a DEVICE array of UMI_GUARD_LEN doubles (8-byte aligned; the
 * partials workspace `ws` is 16-byte aligned):
 *   last step   NORM (global L2 norm of the gradients with the loss scale divided out; inf / NaN as computed), NONFINITE
 *               (count of inf / NaN gradient elements), COEF (factor the update multiplies every gradient by: clip / SCALE,
 *               0 on a skipped step), SKIP (1: the update kernels store nothing)
 *   state       SCALE (the dynamic loss-scale factor d the NEXT backward pass multiplies its seed by), STREAK (clean steps
 *               since the scale last changed)
 *   totals      STEPS, SKIPPED, CLIPPED
 *   settings    MAX_NORM (<= 0: no clipping), GROWTH_INTERVAL (<= 0: static scale), GROWTH, BACKOFF, MIN_SCALE, MAX_SCALE
 * One step:  umi_grad_norm_partials over every descriptor table (rows of `ws` are disjoint: block_offset), then ONE
 * umi_grad_guard_finalize, then umi_optim_hyper_pre_guarded / umi_optim_*_multi_guarded per table.
 *   partials  row block_offset + blk of `ws` <- { sum of g^2 over the block (squares and sums in double, fixed order, no atomics),
 *             number of non-finite g }; reads g only.  ws_bytes >= umi_grad_guard_ws_bytes(block_offset + total_blocks), else
 *             UMI_ERR_WORKSPACE.
 *   finalize  S, K <- fixed-order sums of the first total_blocks rows; with d = SCALE:
 *               NORM = sqrt(S) / d; NONFINITE = K; SKIP = K > 0
 *               clean:   clip = MAX_NORM > 0 ? min(1, MAX_NORM / (NORM + 1e-6)) : 1; COEF = clip / d; CLIPPED += clip < 1
 *               skipped: COEF = 0; SKIPPED += 1
 *               STEPS += 1
 *               then, if GROWTH_INTERVAL > 0 (torch.amp.GradScaler's rule):
 *                 skipped: d = max(d * BACKOFF, MIN_SCALE), STREAK = 0
 *                 clean:   STREAK += 1; at GROWTH_INTERVAL: d = min(d * GROWTH, MAX_SCALE), STREAK = 0
 *             (COEF is formed with the d the backward pass used; only then does d change.)
 *   update    SKIP set: returns before any store, except that a first SGD step zero-fills its (uninitialised) momentum
 *             buffers.  Otherwise g' = (float)COEF == 1 ? g : g * (float)COEF (one fp32 rounding), then the arithmetic of
 *             umi_optim_*_multi on g'.  `hyper` NULL: lr / step_size / bc2_sqrt are the host values given.  dampening != 0 is
 *             UMI_ERR_BADARG (a skipped first step could not reproduce buf = clone(grad)).
 *   hyper_pre_guarded  umi_optim_hyper_pre, but Adam's t and bias corrections advance only when SKIP is clear. */
enum { UMI_GUARD_NORM = 0, UMI_GUARD_NONFINITE = 1, UMI_GUARD_COEF = 2, UMI_GUARD_SKIP = 3, UMI_GUARD_SCALE = 4,
       UMI_GUARD_STREAK = 5, UMI_GUARD_STEPS = 6, UMI_GUARD_SKIPPED = 7, UMI_GUARD_CLIPPED = 8, UMI_GUARD_MAX_NORM = 9,
       UMI_GUARD_GROWTH_INTERVAL = 10, UMI_GUARD_GROWTH = 11, UMI_GUARD_BACKOFF = 12, UMI_GUARD_MIN_SCALE = 13,
       UMI_GUARD_MAX_SCALE = 14, UMI_GUARD_SPARE = 15, UMI_GUARD_LEN = 16 };
size_t umi_grad_guard_ws_bytes(int total_blocks);
int umi_grad_norm_partials(const void* descs, int n_desc, int total_blocks, int block_offset, void* ws, size_t ws_bytes,
                           umi_stream_t stream);
int umi_grad_guard_finalize(const void* ws, int total_blocks, double* state, umi_stream_t stream);
int umi_optim_hyper_pre_guarded(void* hyper, int adam, const double* guard, umi_stream_t stream);
int umi_optim_sgd_multi_guarded(const void* descs, int n_desc, int total_blocks, const void* hyper, double lr, double momentum,
                                double dampening, double weight_decay, int nesterov, int first_step, const double* guard,
                                umi_stream_t stream);
int umi_optim_adam_multi_guarded(const void* descs, int n_desc, int total_blocks, const void* hyper, double step_size,
                                 double beta1, double beta2, double bc2_sqrt, double eps, double weight_decay,
                                 const double* guard, umi_stream_t stream);
int umi_optim_adamw_multi_guarded(const void* descs, int n_desc, int total_blocks, const void* hyper, double lr, double step_size,
                                  double beta1, double beta2, double bc2_sqrt, double eps, double weight_decay,
                                  const double* guard, umi_stream_t stream);

/* Replica fingerprint (data parallel: every rank must hold bit-identical parameters).  One 64-bit word over the tensors of a
 * umi_optim_desc table; only `p`, `n` and `blk0` are read (blocks of umi_optim_block_elems() words, as for the optimizer), the
 * tensors are viewed as 32-bit words and are only read.  All arithmetic mod 2^64, G = 0x9E3779B97F4A7C15:
 *   mix(z):  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *   H_t = sum_i mix(w_i + G (i + 1))  over the words w_0 .. w_{n-1} of tensor t (in table order);  F = sum_t mix(H_t + G (t + 1))
 * so a changed bit, two words swapped within a tensor and two tensors swapped all change F, and the order of summation does
 * not (wrapping addition): the result is the same bits on every device and in NumPy (umi.ddp.fingerprint_numpy).
 * `ws`: 8-byte aligned device scratch of umi_fingerprint_ws_bytes(total_blocks) bytes (one partial word per block), else
 * UMI_ERR_WORKSPACE; `out`: one 8-byte aligned device word.  n_desc == 0 writes 0; total_blocks == 0 (only empty tensors) needs
 * no `ws`.  No atomics; every store is a vector store of a partial or of the result. */
size_t umi_fingerprint_ws_bytes(int total_blocks);
int umi_fingerprint_multi(const void* descs, int n_desc, int total_blocks, void* ws, size_t ws_bytes, unsigned long long* out,
                          umi_stream_t stream);

/* State snapshot (checkpoints, best-model copies, in-place roll-back): every tensor of a umi_optim_desc table copied into one
 * contiguous device arena in one pass, and back.  The fields mean: `p` the tensor (any alignment of 4 bytes), `s0` its slot in
 * the arena (16-byte aligned), `n` its length in 32-bit words, `blk0` as for the optimizer; `g` and `s1` are not read.
 *   umi_snapshot_multi  copies words p -> s0 and writes zeros into the words between n and 4 * ceil(n / 4), the length of a
 *                       slot, so the arena's bytes are a function of the tensors alone; leaves in *out the word F that
 *                       umi_fingerprint_multi gives on the same table, formed from the words as they are copied (the state is
 *                       read once).  `ws`, `out` and their statuses as for umi_fingerprint_multi
 *                       (umi_snapshot_ws_bytes(total_blocks) bytes).  Two launches: the copy with its block partials, the
 *                       finalize pass.  No atomics.
 *   umi_restore_multi   copies words s0 -> p, exactly n per tensor and nothing past them.  One launch; none when
 *                       total_blocks == 0. */
size_t umi_snapshot_ws_bytes(int total_blocks);
int umi_snapshot_multi(const void* descs, int n_desc, int total_blocks, void* ws, size_t ws_bytes, unsigned long long* out,
                       umi_stream_t stream);
int umi_restore_multi(const void* descs, int n_desc, int total_blocks, umi_stream_t stream);

/* Exponential moving average of the weights (mean teacher, timm.ModelEmaV2, torch.optim.swa_utils.AveragedModel), updated on
 * the device right after the optimizer step so that a captured HIP graph keeps averaging.  The state is a DEVICE array of
 * UMI_EMA_LEN doubles (8-byte aligned), as the guard block is:
 *   settings   DECAY (d, the ceiling), WARMUP (!= 0: d_t = min(d, (1 + t) / (10 + t)), else d_t = d)
 *   state      UPDATES (t: updates applied so far)
 *   last pass  LAST (the d_t of the last update), WEIGHT ((double)w_f, w_f = (float)(1.0 - d_t): the fp32 factor the multi pass
 *              uses), ACTIVE (1: the multi pass stores; 0: it returns before any store)
 * One update:  umi_ema_pre, then umi_ema_multi per descriptor table.
 *   pre    `guard` (nullable) is a guard block (above).  guard != NULL and guard[UMI_GUARD_SKIP] != 0: ACTIVE = 0 and nothing
 *          else changes (a skipped optimizer step does not move the average).  Otherwise, all in double with t = UPDATES:
 *          d_t as above; LAST = d_t; WEIGHT = (double)(float)(1.0 - d_t); ACTIVE = 1; UPDATES = t + 1.  One small launch.
 *   multi  over a umi_optim_desc table: `p` the live fp32 parameter (only read), `s0` its fp32 shadow, `n` and `blk0` as for
 *          the optimizer; `g` and `s1` are not read.  ACTIVE set: every element e of s0 becomes
 *              e + w_f * (p - e)      three separate fp32 roundings (subtract, multiply, add; never a fused multiply-add),
 *          so the NumPy float32 statement e + w * (p - e) gives the same bits.  ACTIVE clear: returns before any store.
 *          Any pointer alignment of 4 bytes: 16-byte accesses where p and s0 share their offset into a 16-byte line (at most
 *          three leading and three trailing elements of a block go one by one), one element per lane where they do not.
 *          Exactly n elements of s0 are written.  No atomics; every store is a vector store.
 *   swap   exchanges the 32-bit words of p and s0, exactly n per row (validation on the averaged weights, in place); the same
 *          alignment rule.  One launch; none when total_blocks == 0.  It does not read the state block.
 * Null pointers (descs with n_desc > 0, state) and negative counts are UMI_ERR_BADARG before any launch; n_desc == 0
 * succeeds and launches nothing. */
enum { UMI_EMA_DECAY = 0, UMI_EMA_WARMUP = 1, UMI_EMA_UPDATES = 2, UMI_EMA_LAST = 3, UMI_EMA_WEIGHT = 4, UMI_EMA_ACTIVE = 5,
       UMI_EMA_SPARE0 = 6, UMI_EMA_SPARE1 = 7, UMI_EMA_LEN = 8 };
int umi_ema_pre(double* state, const double* guard, umi_stream_t stream);
int umi_ema_multi(const void* descs, int n_desc, int total_blocks, const double* state, umi_stream_t stream);
int umi_ema_swap_multi(const void* descs, int n_desc, int total_blocks, umi_stream_t stream);

/* Gradient accumulation: one optimizer step over the mean gradient of a WINDOW of micro-batches, summed on the device in one
 * launch per micro-batch, so that a captured HIP graph keeps accumulating.  The state is a DEVICE array of UMI_ACCUM_LEN doubles
 * (8-byte aligned), as the guard and EMA blocks are:
 *   state      COUNT (micro-batches in the open window; 0: closed)
 *   this call  FIRST, LAST, SCALE (written by pre, read by multi)
 *   totals     WINDOWS (windows closed so far), MICRO (calls so far)
 * One call per micro-batch, after its backward pass:  umi_grad_accum_pre, then umi_grad_accum_multi per descriptor table.
 *   pre    one thread, all in double, with J = COUNT:  FIRST = (J == 0); LAST = (last != 0);
 *          SCALE = (double)(float)(1.0 / (J + 1)); COUNT = last ? 0 : J + 1; MICRO += 1; WINDOWS += (last != 0).
 *          "First" lives in the block and not in an argument: one captured micro-step serves every non-final position.
 *   multi  over a umi_optim_desc table: `g` the fp32 gradient, `s0` its fp32 accumulator, `n` and `blk0` as for the optimizer;
 *          `p` and `s1` are not read.  With s = (float)SCALE, per element:
 *              LAST 0, FIRST 1   s0 = g              words are moved; s0 is NOT read: nobody ever zeroes the accumulator
 *              LAST 0, FIRST 0   s0 = s0 + g         one fp32 rounding; g is not written
 *              LAST 1, FIRST 1   (a window of one)   returns before any access: g keeps its bits, NaN payloads included
 *              LAST 1, FIRST 0   g = (s0 + g) * s    two fp32 roundings (never a fused multiply-add); s0 is not written
 *          so the gradient of a window of r micro-batches is float32(1 / r) * (((g1 + g2) + g3) + ... + gr) in fp32, in arrival
 *          order, and it lands in the gradient itself.  NOTE: the desc declares `g` as `const float*`; the LAST-and-not-FIRST
 *          pass WRITES through it (the table is the optimizer's, its gradients are the destination here).
 *          Any pointer alignment of 4 bytes: 16-byte accesses where g and s0 share their offset into a 16-byte line (at most
 *          three leading and three trailing elements of a block go one by one), one element per lane where they do not.
 *          Exactly n elements are written per tensor.  No atomics; every store is a vector store.
 * A null or misaligned state, null descs with n_desc > 0 and negative counts are UMI_ERR_BADARG before any launch; n_desc == 0
 * succeeds and launches nothing; UMI_ERR_UNSUPPORTED if umi_optim_block_elems() is not this file's block. */
enum { UMI_ACCUM_COUNT = 0, UMI_ACCUM_FIRST = 1, UMI_ACCUM_LAST = 2, UMI_ACCUM_SCALE = 3, UMI_ACCUM_WINDOWS = 4,
       UMI_ACCUM_MICRO = 5, UMI_ACCUM_SPARE0 = 6, UMI_ACCUM_SPARE1 = 7, UMI_ACCUM_LEN = 8 };
int umi_grad_accum_pre(double* state, int last, umi_stream_t stream);
int umi_grad_accum_multi(const void* descs, int n_desc, int total_blocks, const double* state, umi_stream_t stream);

/* umi_pack_kn / umi_pack_kn8 of many weight tensors in one launch (all the convolution weights of a model after an
 * optimizer step).  `descs`: DEVICE array sorted by blk0; an entry owns ceil(T*Kpad*Npad / umi_pack_block_elems()) blocks. */
typedef struct umi_pack_desc {
    const float* src;
    void* dst;
    long st, sk, sn;
    int T, K, N, flip_t, Kpad, Npad, k8, blk0;
    int ldn, pad_;   /* ldn > Npad: the entry fills columns [0, Npad) of rows of length ldn (dst already offset to its first
                        column): several source matrices packed side by side into one operand (Q/K/V projections); 0 = Npad */
} umi_pack_desc;
int umi_pack_block_elems(void);
int umi_pack_kn_multi(const void* descs, int n_desc, int total_blocks, int dtype, umi_stream_t stream);

/* Inference pre-/post-processing, the steps either side of the network in the reference's test scripts.
 * umi_znorm_hwc (test_mc3serousv5.py:115-127 `preprocess`): one HWC image, src_dtype 0 = uint8 (cv2.imread) or
 *   1 = float32, C <= 4 -> out_chw[c'][p] = (img[p][c] - mean_c) / std_c as fp32, c' = reverse_channels ? C-1-c : c
 *   (BGR -> RGB); mean and population std per channel in fp64 (numpy semantics), two-pass variance.
 * umi_argmax_mask (test_mc3serousv5.py:883-885 softmax -> argmax -> uint8): mask[n][p] = argmax_c logits[n][c][p], first
 *   maximum wins; softmax is monotone and therefore skipped. */
/* Additive attention gate of UNet_attention (reference Model.py:265-305, Attention_block.forward :297-305); the 1x1
 * convolutions and BatchNorms of the block go through umi_conv_fwd / umi_bn_finalize, these are the fused elementwise steps:
 *   add2_relu: y = max(txa(a) + txb(b), 0)   (E = relu(Q1 + X1), Model.py:302);  bwd: da = db = dy * [y > 0]
 *   gate:      y[m][c] = txx(x[m][c]) * sigmoid(txp(p[m]))   (x * A, Model.py:303-304; p has ONE channel, txp one row)
 *              bwd: dx = dy * A,  dp[m] = A (1 - A) * sum_c dy[m][c] * txx(x[m][c])   (gradient w.r.t. txp(p), i.e. the
 *              BatchNorm output before the sigmoid). */
int umi_add2_relu_fwd(const void* a, int lda, const void* txa, const void* b, int ldb, const void* txb, void* y, int ldy,
                      long M, int C, int dtype, umi_stream_t stream);
int umi_add2_relu_bwd(const void* dy, int lddy, const void* y, int ldy, void* da, int ldda, void* db, int lddb, long M, int C,
                      int dtype, umi_stream_t stream);
int umi_gate_fwd(const void* x, int ldx, const void* txx, const void* p, const void* txp, void* y, int ldy, long M, int C,
                 int dtype, umi_stream_t stream);
int umi_gate_bwd(const void* dy, int lddy, const void* x, int ldx, const void* txx, const void* p, const void* txp, void* dx,
                 int lddx, void* dp, long M, int C, int dtype, umi_stream_t stream);

size_t umi_znorm_ws_bytes(void);
int umi_znorm_hwc(const void* img, int src_dtype, float* out_chw, long HW, int C, int reverse_channels, void* ws,
                  size_t ws_bytes, umi_stream_t stream);
int umi_argmax_mask(const float* logits, unsigned char* mask, int N, int C, long HW, umi_stream_t stream);
/* umi_zoom_cubic_hwc (test_mc3serousv5.py:100-113, the resize of `preprocess`): scipy.ndimage.zoom(img, (out_h / H, out_w / W[, 1]),
 *   order=3) of one HWC image, C <= 4, src_dtype as umi_znorm_hwc; `out` has the input's type and [out_h][out_w][C] elements.
 *   B-spline prefilter (float64, mirror boundaries), corner-aligned sampling, uint8 results rounded and clipped: SciPy's algorithm,
 *   restated and pinned against SciPy by oracle/ref_resize.py.  ws: umi_zoom_cubic_ws_bytes(H, W, C). */
size_t umi_zoom_cubic_ws_bytes(int H, int W, int C);
int umi_zoom_cubic_hwc(const void* img, int src_dtype, void* out, int H, int W, int C, int out_h, int out_w, void* ws,
                       size_t ws_bytes, umi_stream_t stream);

/* Binary-model (one-logit) post-processing, the reference's test.py:393-404 and loss.py:422-440 (MRAccuracy).
 * umi_binary_mask: mask[i] = 1 where fp32 sigmoid(logits[i]) >= 0.5 as torch evaluates it, i.e. logits[i] >= -0x1.7ffffcp-23
 *   (bit pattern 0xB43FFFFE; 1 / (1 + exp(-x)) rounds to exactly 0.5 from there on), else 0; NaN gives 0.  n elements; logits
 *   4-byte aligned (16-byte accesses when it is 16-byte aligned), mask 16-byte aligned.
 * umi_zoom_nearest: scipy.ndimage.zoom(img, (out_h / H, out_w / W), order=0) of N [H][W] images, dtype 0 = uint8, 1 = float32, same
 *   type out: sample coordinate i * ((in - 1) / (out - 1)) in float64, source index floor(x + 0.5), 0 where the coordinate exceeds
 *   in - 1 on either axis (mode 'constant', as umi_zoom_cubic_hwc).
 * umi_sum_trunc: out[n] = (int)(float64 sum of the HW floats of image n), fixed summation order, truncated toward zero, clamped to
 *   int32, NaN -> 0: int(np.sum(dot_map)), exact for 0/1 maps.  ws: umi_sum_trunc_ws_bytes(N) bytes of partial sums. */
int umi_binary_mask(const float* logits, unsigned char* mask, long n, umi_stream_t stream);
int umi_zoom_nearest(const void* in, int dtype, void* out, int N, int H, int W, int out_h, int out_w, umi_stream_t stream);
size_t umi_sum_trunc_ws_bytes(int N);
int umi_sum_trunc(const float* x, int* out, int N, long HW, void* ws, size_t ws_bytes, umi_stream_t stream);

/* 8-connected component labelling of N uint8 [H][W] masks (foreground = non-zero), cv2.connectedComponents(connectivity=8) /
 * scipy.ndimage.label(structure=ones((3,3))): labels 1..counts[n] in the raster order of each component's first pixel, 0 =
 * background.  A union-find by minimum flat index in separate launches (csrc/components.hip); integer atomics and fixed-order
 * scans only, so two runs give identical bits.
 *   umi_components_cap(H, W) = ceil(H/2) * ceil(W/2): a 2x2 block is mutually 8-adjacent, so it meets at most one component;
 *     the row length of area / sum_y / sum_x.  Entries beyond counts[n] are 0.
 *   umi_count_components: counts only.   umi_label_components: labels[N][H][W], counts[N], area[N][cap] (pixels),
 *     sum_y / sum_x[N][cap] (integer coordinate sums; centroid = sum / area).
 *   ws: umi_components_ws_bytes(N, H, W) bytes (0 for unsupported sizes), re-initialised by every call.  Its first int32 is a
 *     fault word: 0, or a non-zero code when a find / union loop hit its iteration cap or met a corrupted chain (the results
 *     are then invalid; the loops are bounded by the pixel count, so the kernels always terminate).
 *   N * H * W < 2^31 and N <= 65535, else UMI_ERR_UNSUPPORTED. */
size_t umi_components_ws_bytes(int N, int H, int W);
int umi_components_cap(int H, int W);
int umi_count_components(const unsigned char* mask, int* counts, int N, int H, int W, void* ws, size_t ws_bytes,
                         umi_stream_t stream);
int umi_label_components(const unsigned char* mask, int* labels, int* counts, int* area, long long* sum_y, long long* sum_x,
                         int N, int H, int W, void* ws, size_t ws_bytes, umi_stream_t stream);

/* The same for class-valued masks (values 0 .. n_classes - 1, 2 <= n_classes <= 8): two pixels are in one component iff they
 * are 8-connected through pixels of the same non-zero value, i.e. the partition of scipy.ndimage.label(mask == c, ones((3,3)))
 * for every c, all classes in the same launches.  Labels 1..counts[n] run over ALL classes in the raster order of each
 * component's first pixel.
 *   umi_count_class_components: class_counts[N][n_classes] only (column 0 is 0).
 *   umi_label_class_components: labels[N][H][W], counts[N], class_counts[N][n_classes], label_class[N][cap] (uint8, the class
 *     of label i + 1), area[N][cap], sum_y / sum_x[N][cap]; rows beyond counts[n] are 0.  cap (1 .. H * W) is the caller's:
 *     with four classes every pixel can be its own component.  An image with more components than cap keeps counts,
 *     class_counts and labels exact, gets the first cap labels' rows, has nothing written beyond them and sets the fault word
 *     to UMI_CC_FAULT_CAP (6).
 *   A mask value >= n_classes is background and sets the fault word to UMI_CC_FAULT_CLASS (5); it is never used as an index.
 *   ws: umi_class_components_ws_bytes(N, H, W, n_classes) bytes (0: unsupported), first int32 = the fault word as above. */
size_t umi_class_components_ws_bytes(int N, int H, int W, int n_classes);
int umi_count_class_components(const unsigned char* mask, int* class_counts, int N, int H, int W, int n_classes, void* ws,
                               size_t ws_bytes, umi_stream_t stream);
int umi_label_class_components(const unsigned char* mask, int* labels, int* counts, int* class_counts, unsigned char* label_class,
                               int* area, long long* sum_y, long long* sum_x, int N, int H, int W, int n_classes, int cap, void* ws,
                               size_t ws_bytes, umi_stream_t stream);

/* Localisation scoring of a predicted mask's components against a ground-truth dot map (csrc/matching.hip): the reference's
 * CrowdMatchingTest (Gaussian matching), three-argument CrowdMatchingTest2 (distance matching) and GMAE (grid count errors)
 * restated on coordinate lists.  All results are integers; the float64 tables and the distance limit come from the host, so
 * the device evaluates no exp and no square root.  Coordinate pairs are (x, y).  Nothing synchronises with the host.
 *   umi_dot_lists: N [H][W] maps (dtype 0 = uint8, 1 = float32; a dot = a non-zero pixel) -> dots[N][max_dots][2] in raster
 *     order and g_count[N].  max_dots <= umi_match_max_dots() (8192); H, W <= 65536, N * H * W < 2^31, N <= 65535.  An image
 *     with more dots sets the fault word (the first int32 of ws, cleared by every call), keeps its first max_dots dots, stores
 *     g_count = max_dots and writes nothing beyond its row.  ws: umi_dot_lists_ws_bytes(N, H, W) bytes (0: unsupported size).
 *   umi_component_centers: umi_label_components' counts / area / sum_y / sum_x (rows of cap entries) -> centers[N][cap][2] =
 *     (round(sum_x / area), round(sum_y / area)), ties to even, in integers; entries beyond counts[n] are (0, 0).
 *   umi_crowd_match: out[N][S][T][2] = (tp, fp).  Per image the centres 0 .. c_count[n] - 1 (read on the device, clamped to
 *     [0, cap]) are taken in order; each looks for the largest tables[s][dy + r][dx + r] over the still-unmatched dots with
 *     |dx|, |dy| <= r = radii[s] (the lowest dot index on ties; 0 without such a dot); a value < thresh[t] is a false positive,
 *     otherwise a true positive that removes the dot.  tables: the S tables of (2 r + 1)^2 float64 one after the other on
 *     the device, table_len doubles in all; radii: S ints on the HOST, read before the call returns; S <= 8; thresh: T float64
 *     on the device.  Dot coordinates must lie in [0, 65535]; centres may be any int32 (no address is formed from them).
 *   umi_distance_match: out[N][3] = (tp, centres, dots).  Per image the dots in order; each takes the nearest centre not taken
 *     yet (squared integer distance, the lowest centre index on ties) when its d2 <= d2_max.  |coordinates| < 2^29.
 *     ws: umi_distance_match_ws_bytes(N, cap) bytes.
 *   umi_grid_sums: out[N][8][8] = sums over the 8 x 8 grid of (size / 8)-pixel cells, clipped to the image: int64 for uint8 maps,
 *     float64 in a fixed order for float32 maps.  size % 8 == 0.
 *   umi_scatter_centers: map[N][H][W] (uint8) = 0, then 1 at every centre c < c_count[n] that lies inside the image.
 *   umi_split_classes: a class-valued uint8 map[N][H][W] -> planes[N][n_classes - 1][H][W] (uint8 0/1), plane c - 1 = (map == c);
 *     the functions above take the planes as N * (n_classes - 1) images.
 *   umi_class_center_lists: umi_label_class_components' counts / label_class / area / sum_y / sum_x (rows of cap entries) ->
 *     centers[N * (n_classes - 1)][cap][2] and c_count[N * (n_classes - 1)]: per (image, class 1 .. n_classes - 1) the centres
 *     (as umi_component_centers forms them) of that class's labels in label order, (0, 0) beyond the count.  Labels beyond
 *     cap (UMI_CC_FAULT_CAP) are not listed. */
int umi_match_max_dots(void);
size_t umi_dot_lists_ws_bytes(int N, int H, int W);
int umi_dot_lists(const void* map, int dtype, int* dots, int* g_count, int N, int H, int W, int max_dots, void* ws, size_t ws_bytes,
                  umi_stream_t stream);
int umi_component_centers(const int* counts, const int* area, const long long* sum_y, const long long* sum_x, int* centers, int N,
                          int cap, umi_stream_t stream);
int umi_crowd_match(const int* dots, const int* g_count, int max_dots, const int* centers, const int* c_count, int cap,
                    const double* tables, size_t table_len, const int* radii, int S, const double* thresh, int T, int* out, int N,
                    umi_stream_t stream);
size_t umi_distance_match_ws_bytes(int N, int cap);
int umi_distance_match(const int* dots, const int* g_count, int max_dots, const int* centers, const int* c_count, int cap,
                       long long d2_max, int* out, int N, void* ws, size_t ws_bytes, umi_stream_t stream);
int umi_grid_sums(const void* map, int dtype, void* out, int N, int H, int W, int size, umi_stream_t stream);
int umi_scatter_centers(const int* centers, const int* c_count, int cap, unsigned char* map, int N, int H, int W,
                        umi_stream_t stream);
int umi_split_classes(const unsigned char* map, unsigned char* planes, int N, int H, int W, int n_classes, umi_stream_t stream);
int umi_class_center_lists(const int* counts, const unsigned char* label_class, const int* area, const long long* sum_y,
                           const long long* sum_x, int* centers, int* c_count, int N, int cap, int n_classes, umi_stream_t stream);

/* Density-map (regression) evaluation (csrc/peaks.hip; statement and rule: umi/peaks.py): what the reference's test_single_reg /
 * test_multiple_reg do with a head's output before CrowdMatchingTest(..., inputType='Regression').
 *   umi_density_maps: x[N][H][W] fp32 -> pred = max(x, 0) / scale with an IEEE-rounded division (NaN stays NaN); counts[N]
 *     (float64) = the sum of pred per image in a fixed order (per 4096-pixel block: 256 strided partial sums and a fixed tree;
 *     then the blocks the same way), vmin[N] (fp32, nullable) = the minimum of pred per image with a NaN counted as 0 (what
 *     umi_peak_lists needs of the image minimum).  scale > 0.  With pred null nothing is rectified, divided or stored: counts and
 *     vmin are those of x itself (the sums of a map that exists already).  ws: umi_density_maps_ws_bytes(N, H, W) bytes, 8-byte
 *     aligned.  No atomics.
 *   umi_peak_lists: the local maxima of N fp32 maps [H][W] by the project's restatement of
 *     skimage.feature.peak_local_max(map, min_distance=d) after map[map < floor] = 0, d = min_distance in 1..8, floor >= 0:
 *       a = x >= floor ? x : 0 (NaN -> 0);  m = max of a over the (2d+1)^2 window clipped to the image;
 *       candidate: a == m, a > min(a) over the image, d <= y < H - d, d <= x < W - d;
 *       spacing: the candidates in raster order, each kept unless an already kept one lies at Chebyshev distance <= d - 1;
 *       order: value descending, raster ascending among equal values.
 *     peaks[N][max_peaks][2] (x, y) and p_count[N]; every entry beyond p_count[n] is written (0, 0).  max_peaks <=
 *     umi_peaks_max() (8192).  vmin: umi_density_maps' vmin of the same maps, or null (the minimum is then taken here).
 *     The fault word (the first int32 of ws, cleared by every call) is an OR of UMI_PEAKS_FAULT_OVERFLOW (1): an image has more
 *     than max_peaks peaks, its first max_peaks in output order are listed and p_count = max_peaks, and
 *     UMI_PEAKS_FAULT_CONTESTED (2): an image has more candidates with another candidate within d - 1 than the contested list
 *     holds (min(H * W, 131072)); those beyond it are dropped and the image's list is invalid.  The spacing loop runs at most as
 *     many rounds as the list holds entries, so the call always terminates.
 *     H, W <= 4096, N <= 65535, N * H * W < 2^31, else UMI_ERR_UNSUPPORTED; ws: umi_peak_lists_ws_bytes(N, H, W) bytes (0:
 *     unsupported size).  Nothing synchronises with the host; integer atomics only, and the lists do not depend on the order in
 *     which they complete; no value of a map forms an address. */
enum { UMI_PEAKS_FAULT_OVERFLOW = 1, UMI_PEAKS_FAULT_CONTESTED = 2 };
int umi_peaks_max(void);
size_t umi_density_maps_ws_bytes(int N, int H, int W);
int umi_density_maps(const float* x, float* pred, double* counts, float* vmin, int N, int H, int W, float scale, void* ws,
                     size_t ws_bytes, umi_stream_t stream);
size_t umi_peak_lists_ws_bytes(int N, int H, int W);
int umi_peak_lists(const float* maps, const float* vmin, int* peaks, int* p_count, int N, int H, int W, int min_distance,
                   float floor, int max_peaks, void* ws, size_t ws_bytes, umi_stream_t stream);

/* Training-batch transform (csrc/augment.hip; statement and rule: umi/augment.py): the reference's Dataset.transform for a batch.
 * Per sample params[n] = {mode, k, axis, angle} (int32) and geom[n] = {M00, M01, M10, M11, off0, off1} (float64, formed on the
 * host as scipy.ndimage.rotate forms them), both on the device and read there: mode 1 = np.flip(np.rot90(x, k), axis) (an odd k
 * needs H == W, else the sample comes out 0), mode 2 = SciPy's order-0 rotation (y = (off0 + r * M00) + q * M01 and
 * x = (off1 + r * M10) + q * M11 in float64 without contraction; 0 unless 0 <= y <= H - 1 and 0 <= x <= W - 1, else
 * src[floor(y + 0.5)][floor(x + 0.5)]), any other mode = identity.  dtype 0 = uint8, 1 = float32.  C <= 4, N <= 65535,
 * H * W < 2^30.  Nothing synchronises with the host, and no value of params / geom can form an address outside its sample.
 *   umi_augment_geometry: src[N][H][W][C] -> dst, same shape and type.
 *   umi_augment_labels: src[N][H][W] -> dst[N][out_h][out_w] (dst_dtype 0 = float32, 1 = int64) = the order-0 zoom
 *     (umi_zoom_nearest's rule) of the augmented map as one gather; value = (float)v * scale, truncated for int64.
 *   umi_augment_znorm: src[N][H][W][C] -> out[N][C][H][W] float32 = (augmented - mean) / std per (sample, channel), float64
 *     statistics in a fixed summation order (exact integer sums for uint8, which limits H * W to 2^23; two passes for float32),
 *     channels reversed when reverse_channels.  The augmented image is not written.  ws: umi_augment_znorm_ws_bytes(N) bytes. */
int umi_augment_geometry(const void* src, int dtype, void* dst, const int* params, const double* geom, int N, int H, int W, int C,
                         umi_stream_t stream);
int umi_augment_labels(const void* src, int src_dtype, void* dst, int dst_dtype, float scale, const int* params, const double* geom,
                       int N, int H, int W, int out_h, int out_w, umi_stream_t stream);
size_t umi_augment_znorm_ws_bytes(int N);
int umi_augment_znorm(const void* src, int dtype, float* out_nchw, const int* params, const double* geom, int N, int H, int W, int C,
                      int reverse_channels, void* ws, size_t ws_bytes, umi_stream_t stream);

/* Random-crop training batches and padded tile grids (csrc/crops.hip; statement: umi/augment.py crop_transform_numpy and
 * grid_transform_numpy): the reference's DataRandomCrop, train and validation, cut out of images that stay on the device.
 * A POOL is one device buffer of images of different sizes but one channel count and type (dtype 0 = uint8, 1 = float32, C <= 4):
 * offsets[n_images] (int64) = the element offset of each image, sizes[n_images][2] (int32) = {H, W}, pool_elems = the buffer's
 * length in elements.  Label and dot maps are pools of their own (C = 1).  All tables are on the device and read there; nothing
 * synchronises with the host; no atomics: two runs give the same bits.
 *   umi_crop_znorm: crops[N][3] = {index, r0, c0} (int32), params[N][4] and geom[N][6] as for umi_augment_* with H = W = crop
 *     -> out[N][C][crop][crop] float32 = (augmented crop - mean) / std per (crop, channel) as umi_augment_znorm forms them.  The
 *     geometry acts on the crop window: a rotation brings in 0, not the neighbouring image pixels.  N <= 65535.
 *     ws: umi_crop_znorm_ws_bytes(N) bytes.
 *   umi_crop_labels: the same gather for a map pool -> dst[N][crop][crop]; dst_dtype 0 = float32 ((float)v * scale), 1 = int64
 *     (that product truncated), 2 = uint8 (the value as it is; uint8 pools only).
 *   A crop row whose index is outside [0, n_images), whose window leaves its image, or whose image leaves the buffer, comes out
 *   all 0 and reads nothing: no value of any table can form an address outside its image.
 *   umi_grid_znorm: ONE image src[H][W][C], thought padded with the constant pad_value (0 .. 255) to [Hp][Wp] with the source at
 *     (pad_top, pad_left); Hp % th == 0, Wp % tw == 0 -> out[T][C][th][tw] float32, the row-major th x tw tiles of
 *     (padded - mean) / std, with the statistics of the WHOLE padded image: the source's sums plus the closed-form pad terms
 *     (uint8: exact integers; float32: two float64 passes, the pad term added last).  The padded image is never written.
 *     th = Hp, tw = Wp gives the padded image itself.  T <= 65535, Hp * Wp < 2^31.  ws: umi_grid_znorm_ws_bytes() bytes.
 *   umi_grid_labels: the same tiles of a map src[H][W], padded with 0; dst_dtype as umi_crop_labels.
 * Exactness bound of the uint8 statistics: std = sqrt(n * S2 - S1 * S1) / n in unsigned 64-bit integers is exact while
 * (255 * n)^2 < 2^64, i.e. for n <= 16,843,009 pixels (n = crop * crop, or Hp * Wp; 4096 x 4096 fits).  Beyond it the uint8 forms
 * return UMI_ERR_UNSUPPORTED and launch nothing. */
size_t umi_crop_znorm_ws_bytes(int N);
int umi_crop_znorm(const void* pool, int dtype, const long long* offsets, const int* sizes, int n_images, long long pool_elems, int C,
                   const int* crops, const int* params, const double* geom, int N, int crop, float* out_nchw, int reverse_channels,
                   void* ws, size_t ws_bytes, umi_stream_t stream);
int umi_crop_labels(const void* pool, int src_dtype, const long long* offsets, const int* sizes, int n_images, long long pool_elems,
                    const int* crops, const int* params, const double* geom, int N, int crop, void* dst, int dst_dtype, float scale,
                    umi_stream_t stream);
size_t umi_grid_znorm_ws_bytes(void);
int umi_grid_znorm(const void* src, int dtype, int H, int W, int C, int pad_top, int pad_left, int pad_value, int Hp, int Wp, int th,
                   int tw, float* out, int reverse_channels, void* ws, size_t ws_bytes, umi_stream_t stream);
int umi_grid_labels(const void* src, int src_dtype, int H, int W, int pad_top, int pad_left, int Hp, int Wp, int th, int tw, void* dst,
                    int dst_dtype, float scale, umi_stream_t stream);

/* Hard-mask segmentation metrics (csrc/seg_metrics.hip; statement: umi/metrics.py): an exact integer confusion matrix per item
 * and Dice / IoU / pixel error from it.  `items` consecutive groups of n images; target [items*n][HW] with target_dtype as
 * umi_dice_ce_fwd (0 = int64, 1 = float32, 2 = uint8, 3 = int32).
 *   umi_confusion_logits: fp32 logits [items*n][C][HW], 1 <= C <= 8.  C >= 2: K = C classes, prediction = umi_argmax_mask's rule
 *     (the first strict maximum wins; a NaN never wins, so a NaN in channel 0 stays).  C == 1: K = 2, prediction =
 *     umi_binary_mask's rule (1 where x >= -0x1.7ffffcp-23; NaN gives 0).
 *   umi_confusion_masks: a uint8 prediction mask [items*n][HW] in place of the logits, 2 <= K <= 8 given; values >= K fall in
 *     column K.
 *   counts[items][K+1][K+1] (int64, 8-byte aligned): row = target class, column = predicted class.  Row K = "not a class": an
 *     integer label outside 0..K-1, or a float32 label that is not exactly one of 0.0 .. K-1 (the reference's one-hot encoder
 *     matches such a pixel to no class, loss.py:220-226, while its prediction still counts).  Column K is 0 from logits.
 *     EVERY entry is written; neither counts nor ws needs presetting.  ws: umi_confusion_ws_bytes(items, n, K, HW) bytes of
 *     uint32 partial rows, 4-byte aligned (0 for sizes out of range).  16-byte loads when HW % 4 == 0 and logits / target are
 *     16-byte aligned (uint8: 4-byte), scalar loads otherwise.  No global atomics: integer sums, exact in any order.
 *   umi_confusion_scores: out[item] (fp32) from counts, with I_c = counts[c][c], Z_c = column sum and Y_c = row sum over all
 *     K+1 entries; float64 in this order without contraction, one rounding to fp32:
 *       kind 0 (Dice error)   1 - (sum_{c = c0..K-1} (2 I_c + 1e-5) / (Z_c + Y_c + 1e-5)) / (K - c0), classes in class order; with
 *                             c0 = 0 the reference's DiceLoss(K)(one_hot(argmax), target, softmax=False) (loss.py:228-251)
 *       kind 1 (IoU error)    the same with (I_c + 1e-5) / (Z_c + Y_c - I_c + 1e-5)
 *       kind 2 (pixel error)  1 - (sum_c I_c + 1e-5) / (sum_{rows < K} Y_c + 1e-5)
 * UMI_ERR_BADARG: null pointers, items / n / HW <= 0, items > 65535, unknown target_dtype / kind, c0 outside 0..K-1, misaligned
 * pointers.  UMI_ERR_UNSUPPORTED: C or K out of range, n * HW >= 2^31.  UMI_ERR_WORKSPACE: ws_bytes too small.  Nothing is
 * launched then.  No allocation, no host synchronisation, one stream: all three calls can be captured. */
size_t umi_confusion_ws_bytes(int items, int n, int K, long HW);
int umi_confusion_logits(const float* logits, const void* target, int target_dtype, int items, int n, int C, long HW,
                         long long* counts, void* ws, size_t ws_bytes, umi_stream_t stream);
int umi_confusion_masks(const unsigned char* mask, const void* target, int target_dtype, int items, int n, int K, long HW,
                        long long* counts, void* ws, size_t ws_bytes, umi_stream_t stream);
int umi_confusion_scores(const long long* counts, int items, int K, int kind, int c0, float* out, umi_stream_t stream);

/* Surface-distance metrics of hard masks (csrc/surface_metrics.hip; statement: umi/surface.py), unit pixel spacing, 2-D.
 * Per image b and class c in c0..K-1: A = (pred_mask == c), G = (target is class c; target_dtype and the label rule as
 * umi_confusion_masks).  Surface of a mask = its pixels on the image edge or with a 4-neighbour outside the mask.  Every surface
 * pixel of one side gets the exact integer squared distance to the nearest surface pixel of the other side; S = the roots
 * (float64) of both directions, n of them.
 *   umi_surface_distances: pred_mask uint8 [B][H][W], target [B][H][W].  stats[B][K][4] (float64) = hd = max(S); hd95 =
 *     np.percentile(S, 95) (v = (n-1) * 0.95, lo = floor(v), t = v - lo, a = S[lo], b = S[min(lo+1, n-1)], a + (b-a) t if t < 0.5 else
 *     b - (b-a)(1-t), no contraction); assd = (mean of A->G + mean of G->A) / 2, each sum in a fixed order; state = 0 both sides
 *     non-empty, 1 both empty, 2 prediction empty only, 3 label empty only (hd, hd95, assd are 0 unless state is 0).
 *     counts[B][K][2] (int64) = surface pixels of A, of G.  Classes below c0 get zeros.  EVERY entry is written; neither the
 *     outputs nor ws needs presetting, and two runs agree bit for bit.  ws: umi_surface_ws_bytes(B, K, c0, H, W) bytes, 8-byte aligned
 *     (0 for sizes out of range): 12 bytes per pixel and 64 KiB per (image, class) for the B * (K - c0) scored pairs.
 *   umi_surface_scores: out[item] (fp32) = the float64 mean over the item's n images and the classes c0..K-1, in (image, class)
 *     order, of stats[..][kind] (kind 0 hd, 1 hd95, 2 assd) in state 0, of 0.0 in state 1, and in states 2 and 3 of
 *     sqrt((H-1)^2 + (W-1)^2) (empty_rule 0), 0.0 (1) or NaN (2); one rounding to fp32.  stats [items*n][K][4].
 * UMI_ERR_BADARG: null or misaligned pointers, B / items / n / H / W <= 0, unknown target_dtype / kind / empty_rule, c0 outside
 * 0..K-1.  UMI_ERR_UNSUPPORTED: H or W > 4096, K outside 2..8, B * K * H * W >= 2^31, B * K > 65535.  UMI_ERR_WORKSPACE: ws_bytes
 * too small.  Nothing is launched then.  Four launches and one, no allocation, no host synchronisation, one stream, integer
 * atomics only: both calls can be captured. */
size_t umi_surface_ws_bytes(int B, int K, int c0, int H, int W);
int umi_surface_distances(const unsigned char* pred_mask, const void* target, int target_dtype, int B, int K, int c0, int H, int W,
                          double* stats, long long* counts, void* ws, size_t ws_bytes, umi_stream_t stream);
int umi_surface_scores(const double* stats, int items, int n, int K, int c0, int kind, int empty_rule, int H, int W, float* out,
                       umi_stream_t stream);

/* Overlap-tile / sliding-window inference over an image larger than the network input (csrc/tiles.hip; statement and the host
 * plan: umi/tiles.py).  A plan is a grid of ny x nx equal th x tw tiles, tile id = iy * nx + ix, with origins oy[ny], ox[nx] in
 * image coordinates (negative, or past H - th: the tile hangs over the edge), fp32 windows wy[th], wx[tw] (finite, >= 0) and their
 * sums over the tiles sy[H], sx[W] (> 0).  A chunk is n slots of tile ids; a slot with id < 0 (or >= ny * nx) is empty.  oy, ox, wy,
 * wx, sy, sx and ids are DEVICE arrays, read by the kernels: a captured call replays with other ids copied into the same buffer.
 *   umi_tile_gather: x fp32 [C][H][W] -> tiles fp32 [n][C][th][tw], tile pixel (i, j) = x[c][r(oy + i)][r(ox + j)].  pad_mode 0
 *     (reflect): r(i) over an axis of m: 0 for m == 1, else p = 2 (m - 1), q = i mod p (non-negative), q if q < m else p - q
 *     (numpy.pad mode='reflect' for every pad width).  pad_mode 1: pad_value where the sample lies outside the image.  An empty slot
 *     is written as zeros: every element of `tiles` is written.
 *   umi_tile_blend: logits fp32 [n][K][th][tw]; for every canvas pixel p and the chunk's slots in order, for a tile that contains p
 *     at (i, j) with w = fp32(wy[i] * wx[j]) > 0: acc[k][p] = fp32(acc[k][p] + fp32(w * logit)), two roundings, no fused
 *     multiply-add.  A tile with w == 0 at p is skipped, so a non-finite logit there does not reach the canvas.  No atomics: one
 *     thread owns a pixel per launch; calls on one stream with the ids ascending give every pixel its tiles in ascending order
 *     whatever the chunk size.  acc fp32 [K][H][W], zeroed by the caller before the first chunk.
 *   umi_tile_finish: acc[k][y][x] = fp32(acc[k][y][x] / fp32(sy[y] * sx[x])) in place; mask (uint8 [H][W], or NULL) = for K == 1
 *     umi_binary_mask's rule on the quotient (1 where >= -0x1.7ffffcp-23, NaN gives 0), for K >= 2 umi_argmax_mask's (first
 *     maximum wins).
 * UMI_ERR_BADARG: null pointers (but `mask`), non-positive sizes, unknown pad_mode, pointers not 4-byte aligned.
 * UMI_ERR_UNSUPPORTED: th or tw > 4096, ny or nx > 1024, n > 64, K * H * W or n * max(C, K) * th * tw >= 2^31 (each call checks
 * its own tensors), n * C or n * K > 65535, K > 256 in umi_tile_finish.  Nothing is launched then.  One launch each, no allocation,
 * no host synchronisation: all three can be captured. */
int umi_tile_gather(const float* x, int C, int H, int W, float* tiles, int th, int tw, const int* oy, const int* ox, int ny, int nx,
                    const int* ids, int n, int pad_mode, float pad_value, umi_stream_t stream);
int umi_tile_blend(const float* logits, int K, int th, int tw, float* acc, int H, int W, const int* oy, const int* ox, int ny, int nx,
                   const float* wy, const float* wx, const int* ids, int n, umi_stream_t stream);
int umi_tile_finish(float* acc, int K, int H, int W, const float* sy, const float* sx, unsigned char* mask, umi_stream_t stream);

/* Test-time augmentation over the rot90 / flip symmetries of the square, and model ensembles (csrc/tta.hip; statement:
 * umi/tta.py).  Element e in 0..7: k = e & 3 quarter turns as np.rot90(x, k, axes=(-2, -1)), then np.flip(axis=-1) if e >> 2; odd k
 * turns [H][W] into [W][H].  `elems` holds the V <= 16 elements of a call BY VALUE, 4 bits each, the first in the lowest bits; they
 * must share one output shape [H'][W'] (any mix for H == W, otherwise all even or all odd k).  mode: 0 = logit, 1 = relu, 2 = prob.
 *   umi_tta_views: x fp32 [N][C][H][W] -> out fp32 [V*N][C][H'][W'], view-major: out[s*N + n] = view_e(s)(x[n]).  Every element of
 *     `out` is written.
 *   umi_tta_accumulate: y fp32 [V*N][K][H'][W'], the network's outputs for those views; for every image pixel p and the views in
 *     order, acc[n][k][p] = fp32(acc[n][k][p] + t(y[s*N + n][.][q])[k]) with q the view pixel that shows p and t by mode: the value;
 *     0 where the value < 0 (a NaN and -0.0 pass through); the fp32 softmax over the K channels, exp(v - max) / sum, for K == 1
 *     1 / (1 + exp(-v)).  One thread owns a pixel and holds its K sums in registers: one read and one write of acc per call, no
 *     atomics.  acc fp32 [N][K][H][W], zeroed by the caller before the first call.
 *   umi_tta_finish: acc = fp32(acc / float(count)) in place.  mask (uint8 [N][H][W], or NULL): K >= 2 umi_argmax_mask's rule on the
 *     quotient (the first strict maximum wins, a NaN never wins); K == 1 umi_binary_mask's (>= -0x1.7ffffcp-23) in modes 0 and 1,
 *     >= 0.5 in mode 2; NaN gives 0.  entropy (fp32 [N][H][W], or NULL; mode 2 only): -sum_k p log p over the quotients with p > 0,
 *     for K == 1 over p and fp32(1 - p).
 * UMI_ERR_BADARG: null pointers (but `mask`, `entropy`), pointers not 4-byte aligned, non-positive sizes or count, V outside 1..16,
 * an element above 7 or bits above the V-th element, two output shapes in one call, an unknown mode, `entropy` outside mode 2.
 * UMI_ERR_UNSUPPORTED: K > 32, V * N * C * H * W (views), V * N * K * H * W (accumulate) or N * K * H * W (finish) >= 2^31, N * C
 * (views) or N (accumulate, finish) > 65535.  Nothing is launched then.  One launch each, no allocation, no host
 * synchronisation, no host memory read at launch time: all three can be captured. */
int umi_tta_views(const float* x, int N, int C, int H, int W, float* out, long long elems, int V, umi_stream_t stream);
int umi_tta_accumulate(float* acc, int N, int K, int H, int W, const float* y, long long elems, int V, int mode, umi_stream_t stream);
int umi_tta_finish(float* acc, int N, int K, int H, int W, int count, int mode, unsigned char* mask, float* entropy,
                   umi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* UNETMI_H */
