// Count-ratio-weighted two-task regression loss of the reference's multi_task_trainRatio (Trainer.py:1225-1249) on fp32
// head outputs o1, o2 [B,1,HW] and label maps l1, l2 [B,HW]:
//   R_k = relu(o_k), L_k = mean((R_k - l_k)^2)
//   rG_b = G1_b / (G2_b + G1_b), rP_b = P1_b / (P2_b + P1_b), G_k,b = sum_b l_k, P_k,b = sum_b R_k
//   r = mean_b |rG_b - rP_b|;  loss = (L1 + L2) * (1 + 10 r) with the gate on (epoch > 5), L1 + L2 with it off
// Per-thread sums are fp32, every sum across threads and blocks is fp64 in a fixed order, so results are deterministic run to
// run; all state crosses between phases at kernel boundaries, none stays in static device memory.
//
//   mtr_stats_kernel : grid (nb, B), block (j, b) streams a contiguous slice of image b; fp64 part row b*nb + j =
//                      {sum (R1-l1)^2, sum (R2-l2)^2, sum R1, sum R2, sum l1, sum l2}
//   mtr_finish_kernel: one block; per-image column sums in row order -> stats, then s_b = sgn(rG_b - rP_b) (torch's sgn:
//                      0 at 0 and for NaN), L1, L2, r and the loss; the gate is an argument or a device flag (graph replay)
//   mtr_bwd_kernel   : same grid as the stats pass; per-image coefficients in fp64 from the stats, then one streaming pass
//                      dO1 = [o1 > 0] * (a * (R1 - l1) + c1_b), dO2 likewise (see the header for a and c_b)
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MTR_COLS = 6;                   // {S1, S2, P1, P2, G1, G2}
constexpr long MTR_PIX_PER_BLOCK = 16L * THREADS;

// torch.relu: NaN stays NaN, negatives become 0
__device__ __forceinline__ float mtr_relu(float x) { return x < 0.f ? 0.f : x; }

// fixed-order fp64 block sum of K values per thread (wave shuffles, then the 4 waves in order) -> out[0..K-1]
template <int K>
__device__ __forceinline__ void mtr_block_sum(double (&v)[K], double* __restrict__ out) {
    __shared__ double red[THREADS / 64][K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < K; ++c)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[c] += __shfl_xor(v[c], o);
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < K; ++c) red[wave][c] = v[c];
    __syncthreads();
    if ((int)threadIdx.x < K) out[threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// the contiguous slice [lo, hi) of an image of HW elements that block j of nb owns; a multiple of 4 except at the end
__device__ __forceinline__ void mtr_slice(long HW, int j, int nb, long* lo, long* hi) {
    const long per = ((HW + nb - 1) / nb + 3) & ~3L;
    *lo = (long)j * per;
    *hi = *lo + per < HW ? *lo + per : HW;
}

__global__ __launch_bounds__(THREADS) void mtr_stats_kernel(const float* __restrict__ o1, const float* __restrict__ o2,
                                                            const float* __restrict__ l1, const float* __restrict__ l2,
                                                            long HW, bool vec, double* __restrict__ part) {
    const int b = blockIdx.y;
    const long off = (long)b * HW;
    long lo, hi;
    mtr_slice(HW, blockIdx.x, gridDim.x, &lo, &hi);
    float a[MTR_COLS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto acc = [&](float x1, float x2, float t1, float t2) {
        const float r1 = mtr_relu(x1), r2 = mtr_relu(x2);
        const float d1 = r1 - t1, d2 = r2 - t2;
        a[0] = fmaf(d1, d1, a[0]);
        a[1] = fmaf(d2, d2, a[1]);
        a[2] += r1;
        a[3] += r2;
        a[4] += t1;
        a[5] += t2;
    };
    long i = lo + 4L * threadIdx.x;
    if (vec) {                                 // every image and every slice starts 16-byte aligned
        for (; i + 3 < hi; i += 4L * THREADS) {
            const float4 x1 = *reinterpret_cast<const float4*>(o1 + off + i);
            const float4 x2 = *reinterpret_cast<const float4*>(o2 + off + i);
            const float4 t1 = *reinterpret_cast<const float4*>(l1 + off + i);
            const float4 t2 = *reinterpret_cast<const float4*>(l2 + off + i);
            acc(x1.x, x2.x, t1.x, t2.x); acc(x1.y, x2.y, t1.y, t2.y);
            acc(x1.z, x2.z, t1.z, t2.z); acc(x1.w, x2.w, t1.w, t2.w);
        }
    }
    for (; i < hi; i += 4L * THREADS)          // scalar path: misaligned pointers, or the last < 4 elements of an image
        for (int q = 0; q < 4 && i + q < hi; ++q) {
            const long e = off + i + q;
            acc(o1[e], o2[e], l1[e], l2[e]);
        }
    double v[MTR_COLS];
#pragma unroll
    for (int c = 0; c < MTR_COLS; ++c) v[c] = (double)a[c];
    mtr_block_sum<MTR_COLS>(v, part + ((long)b * gridDim.x + blockIdx.x) * MTR_COLS);
}

// torch.sgn on a real value: 0 at 0 and for NaN
__device__ __forceinline__ double mtr_sgn(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0); }

// stats layout (fp64): [b*6 + c] per-image column sums | [6B + b] s_b | [7B + 0..3] {L1, L2, r, gate}
__global__ __launch_bounds__(THREADS) void mtr_finish_kernel(const double* __restrict__ part, int B, int nb, long HW,
                                                             int gate_arg, const float* __restrict__ gate_dev,
                                                             double* __restrict__ stats, float* __restrict__ loss,
                                                             float* __restrict__ loss1, float* __restrict__ loss2,
                                                             float* __restrict__ ratio) {
    for (int gc = threadIdx.x; gc < B * MTR_COLS; gc += THREADS) {
        const int b = gc / MTR_COLS, c = gc - b * MTR_COLS;
        double s = 0.0;
        for (int r = 0; r < nb; ++r) s += part[((long)b * nb + r) * MTR_COLS + c];
        stats[gc] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const bool gate = gate_dev ? gate_dev[0] != 0.f : gate_arg != 0;
    double s1 = 0.0, s2 = 0.0, r = 0.0;
    for (int b = 0; b < B; ++b) {
        const double* st = stats + b * MTR_COLS;
        s1 += st[0];
        s2 += st[1];
        const double d = st[4] / (st[5] + st[4]) - st[2] / (st[3] + st[2]);
        r += fabs(d);
        stats[MTR_COLS * B + b] = mtr_sgn(d);
    }
    const double N = (double)B * (double)HW;
    const double L1 = s1 / N, L2 = s2 / N;
    r /= B;
    double* sc = stats + 7 * B;
    sc[0] = L1; sc[1] = L2; sc[2] = r; sc[3] = gate ? 1.0 : 0.0;
    loss[0] = (float)(gate ? (L1 + L2) * (1.0 + 10.0 * r) : L1 + L2);
    loss1[0] = (float)L1;
    loss2[0] = (float)L2;
    ratio[0] = (float)r;
}

__device__ __forceinline__ float mtr_grad(float x, float t, float a, float c) {
    return x > 0.f ? fmaf(a, x - t, c) : 0.f;    // relu backward: 0 where the output is <= 0 (and for NaN)
}

// gout: {gL, g1, g2, gr} (device), NULL = {1, 0, 0, 0}
__global__ __launch_bounds__(THREADS) void mtr_bwd_kernel(const float* __restrict__ o1, const float* __restrict__ o2,
                                                          const float* __restrict__ l1, const float* __restrict__ l2,
                                                          const double* __restrict__ stats, const float* __restrict__ gout,
                                                          long HW, bool vec, float* __restrict__ d1, float* __restrict__ d2) {
    const int b = blockIdx.y, B = gridDim.y;
    const double* sc = stats + 7 * B;
    const double L1 = sc[0], L2 = sc[1], r = sc[2];
    const bool gate = sc[3] != 0.0;
    const double gL = gout ? gout[0] : 1.0, g1 = gout ? gout[1] : 0.0, g2 = gout ? gout[2] : 0.0, gr = gout ? gout[3] : 0.0;
    const double N = (double)B * (double)HW;
    // d/dL_k = gL * (1 + 10 r gate) + g_k; d/dr = gL * 10 gate (L1 + L2) + gr; nothing of r enters with the gate off
    const double wL = gate ? gL * (1.0 + 10.0 * r) : gL;
    const double cr = (gate ? gL * 10.0 * (L1 + L2) : 0.0) + gr;
    const double P1 = stats[b * MTR_COLS + 2], P2 = stats[b * MTR_COLS + 3], sb = stats[MTR_COLS * B + b];
    const double den = P1 + P2;
    // dr/dP1_b = -s_b P2 / (B den^2), dr/dP2_b = +s_b P1 / (B den^2).  den == 0 gives NaN here, as in torch, but then every
    // output of the image is <= 0 and the ReLU mask discards it
    const float a1 = (float)((wL + g1) * 2.0 / N), a2 = (float)((wL + g2) * 2.0 / N);
    const float c1 = (float)(-cr * sb * P2 / (B * den * den)), c2 = (float)(cr * sb * P1 / (B * den * den));
    const long off = (long)b * HW;
    long lo, hi;
    mtr_slice(HW, blockIdx.x, gridDim.x, &lo, &hi);
    long i = lo + 4L * threadIdx.x;
    if (vec) {
        for (; i + 3 < hi; i += 4L * THREADS) {
            const float4 x1 = *reinterpret_cast<const float4*>(o1 + off + i);
            const float4 x2 = *reinterpret_cast<const float4*>(o2 + off + i);
            const float4 t1 = *reinterpret_cast<const float4*>(l1 + off + i);
            const float4 t2 = *reinterpret_cast<const float4*>(l2 + off + i);
            *reinterpret_cast<float4*>(d1 + off + i) = make_float4(mtr_grad(x1.x, t1.x, a1, c1), mtr_grad(x1.y, t1.y, a1, c1),
                                                                   mtr_grad(x1.z, t1.z, a1, c1), mtr_grad(x1.w, t1.w, a1, c1));
            *reinterpret_cast<float4*>(d2 + off + i) = make_float4(mtr_grad(x2.x, t2.x, a2, c2), mtr_grad(x2.y, t2.y, a2, c2),
                                                                   mtr_grad(x2.z, t2.z, a2, c2), mtr_grad(x2.w, t2.w, a2, c2));
        }
    }
    for (; i < hi; i += 4L * THREADS)
        for (int q = 0; q < 4 && i + q < hi; ++q) {
            const long e = off + i + q;
            d1[e] = mtr_grad(o1[e], l1[e], a1, c1);
            d2[e] = mtr_grad(o2[e], l2[e], a2, c2);
        }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

bool mtr_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int mtr_blocks(long HW) {                              // per image: ~16 pixels per thread
    const long nb = (HW + MTR_PIX_PER_BLOCK - 1) / MTR_PIX_PER_BLOCK;
    return (int)(nb < 1 ? 1 : (nb > 1024 ? 1024 : nb));
}

bool mtr_bad_shape(int B, long HW) { return (long)B * HW >= (1L << 31) || B > 65535; }

}  // namespace

extern "C" size_t umi_mt_ratio_ws_bytes(int B, long HW) {
    if (B <= 0 || HW <= 0) return 0;
    return (size_t)B * mtr_blocks(HW) * MTR_COLS * sizeof(double);
}

extern "C" size_t umi_mt_ratio_stats_len(int B) { return B <= 0 ? 0 : (size_t)7 * B + 4; }

extern "C" int umi_mt_ratio_fwd(const float* o1, const float* o2, const float* l1, const float* l2, int B, long HW, int gate,
                                const float* gate_dev, double* stats, float* loss, float* loss1, float* loss2, float* ratio, void* ws,
                                size_t ws_bytes, umi_stream_t st) {
    if (!o1 || !o2 || !l1 || !l2 || !stats || !loss || !loss1 || !loss2 || !ratio || !ws || B <= 0 || HW <= 0)
        return UMI_ERR_BADARG;
    if (mtr_bad_shape(B, HW)) return UMI_ERR_UNSUPPORTED;
    if (ws_bytes < umi_mt_ratio_ws_bytes(B, HW)) return UMI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)st;
    const int nb = mtr_blocks(HW);
    const bool vec = HW % 4 == 0 && mtr_aligned16(o1) && mtr_aligned16(o2) && mtr_aligned16(l1) && mtr_aligned16(l2);
    hipLaunchKernelGGL(mtr_stats_kernel, dim3(nb, B), dim3(THREADS), 0, s, o1, o2, l1, l2, HW, vec, (double*)ws);
    UMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(mtr_finish_kernel, dim3(1), dim3(THREADS), 0, s, (const double*)ws, B, nb, HW, gate ? 1 : 0, gate_dev, stats, loss,
                       loss1, loss2, ratio);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_mt_ratio_bwd(const float* o1, const float* o2, const float* l1, const float* l2, const double* stats,
                                const float* gout, int B, long HW, float* d1, float* d2, umi_stream_t st) {
    if (!o1 || !o2 || !l1 || !l2 || !stats || !d1 || !d2 || B <= 0 || HW <= 0) return UMI_ERR_BADARG;
    if (mtr_bad_shape(B, HW)) return UMI_ERR_UNSUPPORTED;
    const bool vec = HW % 4 == 0 && mtr_aligned16(o1) && mtr_aligned16(o2) && mtr_aligned16(l1) && mtr_aligned16(l2) &&
                     mtr_aligned16(d1) && mtr_aligned16(d2);
    hipLaunchKernelGGL(mtr_bwd_kernel, dim3(mtr_blocks(HW), B), dim3(THREADS), 0, (hipStream_t)st, o1, o2, l1, l2, stats, gout,
                       HW, vec, d1, d2);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
