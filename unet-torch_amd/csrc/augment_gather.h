// Device helpers shared by the gathers of augment.hip (whole samples) and crops.hip (crop windows of pooled images): the
// per-sample parameters, the source pixel of an output pixel under the sample's geometry, the fixed-order block sum and the
// finish kernel of the per-(sample, channel) statistics.
// The rotation coordinates are float64 with every product and sum rounded on its own, so contraction is off for every
// translation unit that includes this header, from here on.
#pragma once
#include <type_traits>
#include "common.h"

#pragma clang fp contract(off)
namespace {

constexpr int AG_MAXC = 4;
constexpr int AG_TX = 64, AG_TY = 4;                     // workgroup = 64 x 4 output pixels
constexpr int AG_STAT_BLOCKS = 64;                       // partial sums per sample

struct AgSample {
    int mode, k, axis;
    double m00, m01, m10, m11, o0, o1;
};

__device__ inline AgSample ag_load(const int* __restrict__ params, const double* __restrict__ geom, int n) {
    AgSample s;
    s.mode = params[n * 4 + 0];
    s.k = params[n * 4 + 1] & 3;
    s.axis = params[n * 4 + 2] & 1;
    const double* g = geom + (long)n * 6;
    s.m00 = g[0]; s.m01 = g[1]; s.m10 = g[2]; s.m11 = g[3]; s.o0 = g[4]; s.o1 = g[5];
    return s;
}

// source pixel (y, x) of output pixel (r, q), 0 <= r < H, 0 <= q < W; false where the output is 0.  Every (y, x) returned
// lies in [0, H) x [0, W): nothing read from `params` or `geom` can form an address outside the sample.
__device__ inline bool ag_src_yx(const AgSample& s, int r, int q, int H, int W, int& y, int& x) {
    if (s.mode == 1) {
        if ((s.k & 1) && H != W) return false;
        const int i = s.axis == 0 ? H - 1 - r : r;       // undo the flip: (i, j) indexes rot90(x, k)
        const int j = s.axis == 1 ? W - 1 - q : q;
        switch (s.k) {                                   // rot90(x, 1)[i][j] = x[j][W - 1 - i], counter-clockwise
            case 0: y = i; x = j; break;
            case 1: y = j; x = W - 1 - i; break;
            case 2: y = H - 1 - i; x = W - 1 - j; break;
            default: y = H - 1 - j; x = i; break;
        }
        return true;
    }
    if (s.mode == 2) {
        const double fy = (s.o0 + (double)r * s.m00) + (double)q * s.m01;
        const double fx = (s.o1 + (double)r * s.m10) + (double)q * s.m11;
        if (!(fy >= 0.0 && fy <= (double)(H - 1) && fx >= 0.0 && fx <= (double)(W - 1))) return false;     // NaN: outside
        y = (int)floor(fy + 0.5);
        x = (int)floor(fx + 0.5);
        return true;
    }
    y = r;
    x = q;
    return true;
}

// the same as the pixel index y * W + x in [0, H * W); -1 where the output is 0
__device__ inline int ag_src(const AgSample& s, int r, int q, int H, int W) {
    int y, x;
    return ag_src_yx(s, r, q, H, W, y, x) ? y * W + x : -1;
}

// Sum over the workgroup (blockDim.x threads, a multiple of 64, at most 1024): wave shuffle, then LDS in wave order.
template <typename V>
__device__ inline V ag_block_sum(V v, V* sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    V r = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += sh[i];
    return r;                                            // valid in thread 0
}

// Finish of the per-(sample, channel) statistics: part[N][AG_STAT_BLOCKS][2][AG_MAXC] partial sums (unsigned 64-bit S1, S2 for
// uint8; float64 sums for float32) -> stats[N][2][AG_MAXC] (mean, std).  PASS 0: uint8 mean and std, float32 mean; PASS 1: float32
// std from the sum of squared deviations.  One thread per (sample, channel), the slices in index order.
template <typename T, int PASS>
__global__ __launch_bounds__(64) void ag_stats_finish_kernel(const void* __restrict__ part_, int N, int HW, int C,
                                                             double* __restrict__ stats) {
    constexpr bool U8 = sizeof(T) == 1;
    typedef typename std::conditional<U8, unsigned long long, double>::type V;
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= N * C) return;
    const int n = t / C, c = t - n * C;
    const V* part = (const V*)part_ + (long)n * AG_STAT_BLOCKS * 2 * AG_MAXC;
    V s1 = 0, s2 = 0;
    for (int b = 0; b < AG_STAT_BLOCKS; ++b) {
        s1 += part[(long)b * 2 * AG_MAXC + c];
        if (U8) s2 += part[(long)b * 2 * AG_MAXC + AG_MAXC + c];
    }
    double* st = stats + (long)n * 2 * AG_MAXC;
    if (U8) {
        const unsigned long long cnt = (unsigned long long)HW;
        st[c] = (double)s1 / (double)HW;
        st[AG_MAXC + c] = sqrt((double)(cnt * (unsigned long long)s2 - (unsigned long long)s1 * (unsigned long long)s1)) / (double)HW;
    } else if (PASS == 0) st[c] = (double)s1 / (double)HW;
    else st[AG_MAXC + c] = sqrt((double)s1 / (double)HW);
}

}  // namespace
