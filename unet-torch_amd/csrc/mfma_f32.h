// What the fp32 matrix-core kernels (conv_mfma_f32.hip, gemm_mfma_f32.hip, attention_mfma_f32.hip, convt_mfma_f32.hip) share:
// the v_mfma_f32_32x32x2_f32 primitives, the two GEMM tiles of the pointwise and the 2x2-transposed convolutions, and the
// host rules that size their grids.  Nothing here branches on its caller.
#pragma once
#include "common.h"

// Operand maps of the 32x32x2 form (lane l): A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31], one VGPR each;
// D[row = (reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5)][col = l & 31], 16 VGPRs.
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int d_row(int reg, int kh) { return (reg & 3) + 8 * (reg >> 2) + 4 * kh; }
__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}

// ---- the 128-row forward tile --------------------------------------------------------------------------------------------------
// D[m][co] += X[m][k] * W[k][co]: the A operand's lanes run along the rows of x, the B operand's and D's along co.  A workgroup
// (4 waves, WM x WN) owns 128 rows and TN = WN * NT * 32 = 128 or 64 output channels; a wave owns MT x NT tiles of 32 x 32 = 4
// (TN = 128) or 2 (TN = 64) independent accumulators.  Per chunk of 32 input channels the x tile ([row][k], 33 dwords per row:
// the A operand's 32 lanes stride by one row and so fall on 32 distinct banks) and the weights ([k][co] as packed) are staged
// in LDS; a kernel keeps the next chunk's global loads in flight while the current one is multiplied.
constexpr int P_TM = 128, P_KC = 32, P_XS = P_KC + 1;

// one staged chunk; pa = xl + (wm * MT * 32 + col) * P_XS + kh, pb = wl + kh * TN + wn * NT * 32 + col
template <int TN, int MT, int NT>
__device__ __forceinline__ void fwd_tile_multiply(f32x16 (&acc)[MT][NT], const float* pa, const float* pb) {
#pragma unroll
    for (int kk = 0; kk < P_KC / 2; ++kk) {
        float av[MT], bv[NT];
#pragma unroll
        for (int a = 0; a < MT; ++a) av[a] = pa[a * 32 * P_XS + 2 * kk];
#pragma unroll
        for (int b = 0; b < NT; ++b) bv[b] = pb[2 * kk * TN + b * 32];
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int b = 0; b < NT; ++b) acc[a][b] = mfma32(av[a], bv[b], acc[a][b]);
    }
}

// ---- the channel-lane weight-gradient tile -------------------------------------------------------------------------------------
// dW[ci][co] = sum over rows of A[m][ci] * B[m][co]: M = ci, N = co, K = rows.  Lanes run along the channels for both operands, so
// both are read straight from [row][channel] LDS tiles.  A workgroup (2 x 2 waves) owns TI x TJ = 64 or 128 input and output
// channels (TI = 2 * MT * 32, TJ = 2 * NT * 32) over the rows of one split, in chunks of 32 rows; a wave carries MT x NT
// accumulators.
constexpr int Q_KC = 32;

// one staged chunk; pa = xl + kh * TI + wi * MT * 32 + col, pb = dl + kh * TJ + wj * NT * 32 + col
template <int MT, int NT>
__device__ __forceinline__ void wgrad_tile_multiply(f32x16 (&acc)[MT][NT], const float* pa, const float* pb) {
    constexpr int TI = 2 * MT * 32, TJ = 2 * NT * 32;
#pragma unroll
    for (int kk = 0; kk < Q_KC / 2; ++kk) {
        float av[MT], bv[NT];
#pragma unroll
        for (int a = 0; a < MT; ++a) av[a] = pa[2 * kk * TI + a * 32];
#pragma unroll
        for (int b = 0; b < NT; ++b) bv[b] = pb[2 * kk * TJ + b * 32];
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int b = 0; b < NT; ++b) acc[a][b] = mfma32(av[a], bv[b], acc[a][b]);
    }
}

// ---- host rules (taps = 1: pointwise, 4: the 2x2 transposed convolution) -------------------------------------------------------
// 64-wide tiles where the channel count fits one, or where 128-wide ones would leave most compute units without a workgroup
static inline bool fwd_narrow(long M, int Co, int taps) {
    return Co <= 64 || (long)umi_cdiv(M, P_TM) * umi_cdiv(Co, 128) * taps < 512;
}

// the split of the rows: a function of the shape alone (umi_conv_wgrad_ws_bytes must give the same answer)
static inline void wgrad_plan(long M, int Ci, int Co, int taps, int* ti, int* tj, int* splits, long* rps) {
    *ti = Ci <= 64 ? 64 : 128;
    *tj = Co <= 64 ? 64 : 128;
    const long tiles = (long)taps * umi_cdiv(Ci, *ti) * umi_cdiv(Co, *tj);
    long want = (512 + tiles - 1) / tiles;               // aim for >= 512 workgroups ...
    const long chunks = (M + Q_KC - 1) / Q_KC;
    const long most = (chunks + 3) / 4;                  // ... of at least 4 chunks of 32 rows each
    if (want > most) want = most;
    if (want < 1) want = 1;
    const long cps = (chunks + want - 1) / want;
    *rps = cps * Q_KC;
    *splits = (int)((chunks + cps - 1) / cps);
}
