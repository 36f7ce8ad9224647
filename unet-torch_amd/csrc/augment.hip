// Training-batch transform (reference DataLoader.py `transform` of Data_Binary :636-680, Data_Reg :275-373, Data_Reg_Binary
// :132-174; statement: umi/augment.py): random rot90 + flip or scipy.ndimage.rotate(order=0, reshape=False), the order-0 zoom of
// the label maps, the float64 z-normalisation and the HWC -> CHW copy with reversed channels, for a whole batch per launch.
//
//   umi_augment_geometry   src[N][H][W][C] -> dst of the same shape and type: the augmented samples (used when a cubic resize follows)
//   umi_augment_labels     label maps [N][H][W] -> [N][oh][ow] float32 / int64: order-0 zoom and geometry as ONE gather (two
//                          nearest gathers compose exactly), scale and cast on the store
//   umi_augment_znorm      images -> [N][C][H][W] float32, z-normalised with the float64 statistics of the AUGMENTED image, which
//                          is never written out: statistics pass(es) that gather, then one pass that gathers, normalises, stores
//
// Every sample carries its own parameters, read on the device: params[n] = {mode, k, axis, angle}, geom[n] = {M00, M01, M10,
// M11, off0, off1} (float64, formed on the host the way SciPy forms them; `angle` is not read here).
//   mode 1: out = np.flip(np.rot90(x, k), axis), an integer index map; an odd k needs H == W (otherwise the sample comes out 0);
//   mode 2: output pixel (r, q) samples y = (off0 + r * M00) + q * M01, x = (off1 + r * M10) + q * M11 in float64, each product
//           and sum rounded on its own (no contraction: hipcc fuses by default, and SciPy's C does not); 0 unless
//           0 <= y <= H - 1 and 0 <= x <= W - 1, else src[floor(y + 0.5)][floor(x + 0.5)], one source pixel for all channels;
//   any other mode: the identity.
// All three are gathers: one thread per output pixel, 64 x 4 pixel tiles so that a wave stores one contiguous row segment and
// the source pixels of a tile (a slanted strip for a rotation, a column strip for an odd k) stay close in L2.
#include <type_traits>
#include "augment_gather.h"             // AgSample, ag_load, ag_src, ag_block_sum, the tile constants
#include "zoom_nearest_rule.h"

#pragma clang fp contract(off)
namespace {

template <typename T>
__global__ __launch_bounds__(AG_TX * AG_TY) void ag_geometry_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                                    const int* __restrict__ params, const double* __restrict__ geom,
                                                                    int H, int W, int C) {
    const int q = blockIdx.x * AG_TX + threadIdx.x, r = blockIdx.y * AG_TY + threadIdx.y, n = blockIdx.z;
    if (q >= W || r >= H) return;
    const AgSample s = ag_load(params, geom, n);
    const int sp = ag_src(s, r, q, H, W);
    const long base = (long)n * H * W;
    const T* in = src + (base + (sp < 0 ? 0 : sp)) * C;
    T* out = dst + (base + (long)r * W + q) * C;
    for (int c = 0; c < C; ++c) out[c] = sp < 0 ? (T)0 : in[c];
}

// TO = float: (float)v * scale; TO = long long: that product converted like torch's .long() (truncation)
template <typename T, typename TO>
__global__ __launch_bounds__(AG_TX * AG_TY) void ag_labels_kernel(const T* __restrict__ src, TO* __restrict__ dst, float scale,
                                                                  const int* __restrict__ params, const double* __restrict__ geom,
                                                                  int H, int W, int oh, int ow) {
    const int q = blockIdx.x * AG_TX + threadIdx.x, r = blockIdx.y * AG_TY + threadIdx.y, n = blockIdx.z;
    if (q >= ow || r >= oh) return;
    int sp = -1;
    const int zr = oh == H ? r : zn_src(r, H, oh), zq = ow == W ? q : zn_src(q, W, ow);    // pixel of the augmented map
    if (zr >= 0 && zq >= 0) sp = ag_src(ag_load(params, geom, n), zr, zq, H, W);
    const float v = sp < 0 ? 0.f : (float)src[(long)n * H * W + sp] * scale;
    dst[((long)n * oh + r) * ow + q] = (TO)v;
}

// ---- statistics of the augmented image, per (sample, channel), in a fixed order -----------------------------------------------
// uint8: S1 = sum v and S2 = sum v * v as exact 64-bit integers in one pass; mean = S1 / n, std = sqrt(n * S2 - S1 * S1) / n
//        (n * S2 and S1 * S1 stay below 2^63 for n <= 2^23 pixels).
// float32: float64 sum -> mean, then the float64 sum of (v - mean)^2 (two passes, as numpy.std: survives |mean| >> std).
// Partial sums: AG_STAT_BLOCKS slices per sample, threads striding a slice, wave shuffle then LDS in wave order; the finish
// kernel (ag_stats_finish_kernel, augment_gather.h) adds the slices in index order.
// ws: stats[N][2][AG_MAXC] float64 (mean, std), then part[N][AG_STAT_BLOCKS][2][AG_MAXC].
// PASS 0: uint8 -> S1, S2; float -> sum.  PASS 1 (float only): sum of squared deviations from stats' mean.
template <typename T, int PASS>
__global__ __launch_bounds__(256) void ag_stats_kernel(const T* __restrict__ src, const int* __restrict__ params,
                                                       const double* __restrict__ geom, int H, int W, int C,
                                                       const double* __restrict__ stats, void* __restrict__ part_) {
    constexpr bool U8 = sizeof(T) == 1;
    typedef typename std::conditional<U8, unsigned long long, double>::type V;
    __shared__ V sh[4];
    const int n = blockIdx.y, HW = H * W;
    const AgSample s = ag_load(params, geom, n);
    const T* img = src + (long)n * HW * C;
    V a1[AG_MAXC] = {0, 0, 0, 0}, a2[AG_MAXC] = {0, 0, 0, 0};
    double mean[AG_MAXC] = {0.0, 0.0, 0.0, 0.0};
    if (PASS == 1)
        for (int c = 0; c < C; ++c) mean[c] = stats[(long)n * 2 * AG_MAXC + c];
    const int per = (HW + AG_STAT_BLOCKS - 1) / AG_STAT_BLOCKS;
    const int lo = blockIdx.x * per, hi = lo + per < HW ? lo + per : HW;
    for (int p = lo + threadIdx.x; p < hi; p += 256) {
        const int r = p / W, q = p - r * W;
        const int sp = ag_src(s, r, q, H, W);
        for (int c = 0; c < C; ++c) {
            if (U8) {
                const V v = sp < 0 ? 0 : (V)img[(long)sp * C + c];
                a1[c] += v;
                a2[c] += v * v;
            } else {
                const double d = (sp < 0 ? 0.0 : (double)img[(long)sp * C + c]) - mean[c];
                a1[c] += PASS == 0 ? d : d * d;
            }
        }
    }
    V* part = (V*)part_ + ((long)n * AG_STAT_BLOCKS + blockIdx.x) * 2 * AG_MAXC;
    for (int c = 0; c < C; ++c) {
        const V t1 = ag_block_sum(a1[c], sh);
        if (threadIdx.x == 0) part[c] = t1;
        if (U8) {
            const V t2 = ag_block_sum(a2[c], sh);
            if (threadIdx.x == 0) part[AG_MAXC + c] = t2;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(AG_TX * AG_TY) void ag_znorm_kernel(const T* __restrict__ src, float* __restrict__ out,
                                                                 const int* __restrict__ params, const double* __restrict__ geom,
                                                                 int H, int W, int C, int reverse, const double* __restrict__ stats) {
    const int q = blockIdx.x * AG_TX + threadIdx.x, r = blockIdx.y * AG_TY + threadIdx.y, n = blockIdx.z;
    if (q >= W || r >= H) return;
    const AgSample s = ag_load(params, geom, n);
    const int sp = ag_src(s, r, q, H, W);
    const long HW = (long)H * W;
    const T* in = src + ((long)n * HW + (sp < 0 ? 0 : sp)) * C;
    const double* st = stats + (long)n * 2 * AG_MAXC;
    float* o = out + (long)n * C * HW + (long)r * W + q;
    for (int c = 0; c < C; ++c) {
        const double v = ((sp < 0 ? 0.0 : (double)in[c]) - st[c]) / st[AG_MAXC + c];      // fp64, then one rounding to fp32
        o[(long)(reverse ? C - 1 - c : c) * HW] = (float)v;
    }
}

// shared argument checks: 0 when the gather grids can be formed
int ag_check(const void* src, const void* dst, const int* params, const double* geom, int dtype, int N, int H, int W, int C) {
    if (!src || !dst || !params || !geom || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C > AG_MAXC) return UMI_ERR_BADARG;
    if (dtype != 0 && dtype != 1) return UMI_ERR_BADARG;
    if (N > 65535 || (long)H * W >= (1L << 30) || (long)N * H * W * C >= (1L << 40)) return UMI_ERR_UNSUPPORTED;
    return UMI_OK;
}

dim3 ag_grid(int N, int H, int W) { return dim3((unsigned)((W + AG_TX - 1) / AG_TX), (unsigned)((H + AG_TY - 1) / AG_TY), (unsigned)N); }

}  // namespace

extern "C" int umi_augment_geometry(const void* src, int dtype, void* dst, const int* params, const double* geom, int N, int H,
                                    int W, int C, umi_stream_t stream) {
    const int bad = ag_check(src, dst, params, geom, dtype, N, H, W, C);
    if (bad) return bad;
    if ((H + AG_TY - 1) / AG_TY > 65535) return UMI_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == 0)
        hipLaunchKernelGGL((ag_geometry_kernel<unsigned char>), ag_grid(N, H, W), dim3(AG_TX, AG_TY), 0, s, (const unsigned char*)src,
                           (unsigned char*)dst, params, geom, H, W, C);
    else
        hipLaunchKernelGGL((ag_geometry_kernel<float>), ag_grid(N, H, W), dim3(AG_TX, AG_TY), 0, s, (const float*)src, (float*)dst,
                           params, geom, H, W, C);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_augment_labels(const void* src, int src_dtype, void* dst, int dst_dtype, float scale, const int* params,
                                  const double* geom, int N, int H, int W, int out_h, int out_w, umi_stream_t stream) {
    const int bad = ag_check(src, dst, params, geom, src_dtype, N, H, W, 1);
    if (bad) return bad;
    if (out_h <= 0 || out_w <= 0 || (dst_dtype != 0 && dst_dtype != 1)) return UMI_ERR_BADARG;
    if ((out_h + AG_TY - 1) / AG_TY > 65535 || (long)out_h * out_w >= (1L << 31)) return UMI_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid = ag_grid(N, out_h, out_w), block(AG_TX, AG_TY);
#define AG_LABELS(T, TO) \
    hipLaunchKernelGGL((ag_labels_kernel<T, TO>), grid, block, 0, s, (const T*)src, (TO*)dst, scale, params, geom, H, W, out_h, out_w)
    if (src_dtype == 0 && dst_dtype == 0) AG_LABELS(unsigned char, float);
    else if (src_dtype == 0) AG_LABELS(unsigned char, long long);
    else if (dst_dtype == 0) AG_LABELS(float, float);
    else AG_LABELS(float, long long);
#undef AG_LABELS
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" size_t umi_augment_znorm_ws_bytes(int N) {
    return N > 0 ? (size_t)N * (2 + 2 * AG_STAT_BLOCKS) * AG_MAXC * sizeof(double) : 0;
}

extern "C" int umi_augment_znorm(const void* src, int dtype, float* out_nchw, const int* params, const double* geom, int N, int H,
                                 int W, int C, int reverse_channels, void* ws, size_t ws_bytes, umi_stream_t stream) {
    const int bad = ag_check(src, out_nchw, params, geom, dtype, N, H, W, C);
    if (bad) return bad;
    if (!ws || ws_bytes < umi_augment_znorm_ws_bytes(N)) return UMI_ERR_WORKSPACE;
    if ((H + AG_TY - 1) / AG_TY > 65535) return UMI_ERR_UNSUPPORTED;
    if (dtype == 0 && (long)H * W > (1L << 23)) return UMI_ERR_UNSUPPORTED;      // the exact integer variance needs n * S2 < 2^63
    hipStream_t s = (hipStream_t)stream;
    double* stats = (double*)ws;
    void* part = stats + (size_t)N * 2 * AG_MAXC;
    const dim3 sgrid(AG_STAT_BLOCKS, N), fgrid((N * C + 63) / 64);
    const int HW = H * W;
    if (dtype == 0) {
        typedef unsigned char T;
        hipLaunchKernelGGL((ag_stats_kernel<T, 0>), sgrid, dim3(256), 0, s, (const T*)src, params, geom, H, W, C, stats, part);
        hipLaunchKernelGGL((ag_stats_finish_kernel<T, 0>), fgrid, dim3(64), 0, s, part, N, HW, C, stats);
        hipLaunchKernelGGL((ag_znorm_kernel<T>), ag_grid(N, H, W), dim3(AG_TX, AG_TY), 0, s, (const T*)src, out_nchw, params, geom, H,
                           W, C, reverse_channels, stats);
    } else {
        typedef float T;
        hipLaunchKernelGGL((ag_stats_kernel<T, 0>), sgrid, dim3(256), 0, s, (const T*)src, params, geom, H, W, C, stats, part);
        hipLaunchKernelGGL((ag_stats_finish_kernel<T, 0>), fgrid, dim3(64), 0, s, part, N, HW, C, stats);
        hipLaunchKernelGGL((ag_stats_kernel<T, 1>), sgrid, dim3(256), 0, s, (const T*)src, params, geom, H, W, C, stats, part);
        hipLaunchKernelGGL((ag_stats_finish_kernel<T, 1>), fgrid, dim3(64), 0, s, part, N, HW, C, stats);
        hipLaunchKernelGGL((ag_znorm_kernel<T>), ag_grid(N, H, W), dim3(AG_TX, AG_TY), 0, s, (const T*)src, out_nchw, params, geom, H,
                           W, C, reverse_channels, stats);
    }
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
