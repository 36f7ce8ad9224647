// The steps either side of the network at inference time (reference test_mc3serousv5.py:100-127 `preprocess`,
// :877-887 softmax -> argmax -> uint8 mask).  Both are one-pass HBM-bound byte/float streams.
//
//   umi_znorm_hwc     HWC image (uint8 as cv2.imread returns it, or float32) -> per-channel z-normalised CHW fp32,
//                     optional channel reversal (BGR -> RGB); mean / population std in fp64 like numpy.
//   umi_argmax_mask   NCHW fp32 logits -> uint8 class mask; the first maximum wins (torch.argmax).  softmax is monotone,
//                     so the reference's softmax before the argmax is skipped.
#include "common.h"
#include "zoom_nearest_rule.h"

namespace {

constexpr int ZN_BLOCKS = 512;
constexpr int ZN_MAXC = 4;

template <typename T>
__device__ inline double zn_load(const T* p, long i) { return (double)p[i]; }

__device__ inline double block_sum(double v, double* sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += sh[i];
    return r;                                    // valid in thread 0
}

// pass 0: partial sums of x; pass 1: partial sums of (x - mean)^2 (two-pass variance, as numpy.std)
template <typename T, int PASS>
__global__ __launch_bounds__(256) void znorm_reduce_kernel(const T* __restrict__ img, long HW, int C,
                                                            const double* __restrict__ stats, double* __restrict__ part) {
    __shared__ double sh[4];
    double acc[ZN_MAXC] = {0.0, 0.0, 0.0, 0.0};
    double mean[ZN_MAXC] = {0.0, 0.0, 0.0, 0.0};
    if (PASS == 1)
        for (int c = 0; c < C; ++c) mean[c] = stats[c];
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long)gridDim.x * 256)
        for (int c = 0; c < C; ++c) {
            const double v = zn_load(img, p * C + c) - mean[c];
            acc[c] += PASS == 0 ? v : v * v;
        }
    for (int c = 0; c < C; ++c) {
        const double s = block_sum(acc[c], sh);
        if (threadIdx.x == 0) part[(long)blockIdx.x * ZN_MAXC + c] = s;
    }
}

// stats[c] = mean (PASS 0) / stats[ZN_MAXC + c] = population std (PASS 1): fixed-order sum of the block partials
template <int PASS>
__global__ __launch_bounds__(64) void znorm_finalize_kernel(const double* __restrict__ part, int nblk, long HW, int C,
                                                            double* __restrict__ stats) {
    const int c = threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(long)b * ZN_MAXC + c];
    if (PASS == 0) stats[c] = s / (double)HW;
    else stats[ZN_MAXC + c] = sqrt(s / (double)HW);
}

template <typename T>
__global__ __launch_bounds__(256) void znorm_apply_kernel(const T* __restrict__ img, float* __restrict__ out, long HW, int C,
                                                          int reverse, const double* __restrict__ stats) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    for (int c = 0; c < C; ++c) {
        const double v = (zn_load(img, p * C + c) - stats[c]) / stats[ZN_MAXC + c];     // fp64, then one rounding to fp32
        out[(long)(reverse ? C - 1 - c : c) * HW + p] = (float)v;
    }
}

template <int C>
__global__ __launch_bounds__(256) void argmax_mask_kernel(const float* __restrict__ logits, unsigned char* __restrict__ mask,
                                                          long HW, int Cdyn) {
    const int n = blockIdx.y;
    const long p4 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p4 >= HW) return;
    const float* base = logits + (long)n * (C ? C : Cdyn) * HW;
    const int nc = C ? C : Cdyn;
    if (p4 + 4 <= HW && (HW & 3) == 0) {
        float4 best = *reinterpret_cast<const float4*>(base + p4);
        uchar4 bi = make_uchar4(0, 0, 0, 0);
        for (int c = 1; c < nc; ++c) {
            const float4 v = *reinterpret_cast<const float4*>(base + (long)c * HW + p4);
            if (v.x > best.x) { best.x = v.x; bi.x = (unsigned char)c; }
            if (v.y > best.y) { best.y = v.y; bi.y = (unsigned char)c; }
            if (v.z > best.z) { best.z = v.z; bi.z = (unsigned char)c; }
            if (v.w > best.w) { best.w = v.w; bi.w = (unsigned char)c; }
        }
        *reinterpret_cast<uchar4*>(mask + (long)n * HW + p4) = bi;
    } else {
        for (long p = p4; p < HW && p < p4 + 4; ++p) {
            float best = base[p];
            unsigned char bi = 0;
            for (int c = 1; c < nc; ++c) {
                const float v = base[(long)c * HW + p];
                if (v > best) { best = v; bi = (unsigned char)c; }
            }
            mask[(long)n * HW + p] = bi;
        }
    }
}


// ---- cubic resize: scipy.ndimage.zoom(img, (oh / H, ow / W[, 1]), order=3) as `preprocess` calls it (test_mc3serousv5.py:100-113)
// SciPy's algorithm (ndimage/_interpolation.py zoom; ni_splines.c, ni_interpolation.c NI_ZoomShift), restated by
// oracle/ref_resize.py and pinned against SciPy itself there:
//   1. cubic B-spline prefilter in float64 along H, then W: gain 6, pole sqrt(3) - 2, MIRROR initialisation (mode 'constant'
//      filters as 'mirror');
//   2. corner-aligned sampling x = i * ((in - 1) / (out - 1)), 4 x 4 coefficients around floor(x) - 1, mirrored indices;
//   3. mode 'constant' (cval 0): an output whose x is < 0 or > in - 1 on either axis is 0 (ni_interpolation.c map_coordinate).
//      x is the same float64 product as SciPy's, and the last one rounds just above in - 1 for some sizes (e.g. 32, 512, 1000,
//      2048 -> 224): SciPy's whole last output row / column is then 0, and so is ours;
//   4. uint8 images: floor(v + 0.5) clipped to [0, 255] (the output has the input's type).
// All arithmetic in float64 without contraction, the oracle's sequence of operations.  SciPy's spline coefficients differ from
// those in the last float64 bits, so uint8 results are SciPy's except at exact half-way values k + 0.5 (2- and 3-pixel axes), and
// float32 ones are within one float32 ulp of SciPy's.
#pragma clang fp contract(off)
constexpr double ZC_POLE = -0.26794919243112270647;       // sqrt(3) - 2

// one thread = one line (a column of one channel for AXIS 0, a row of one channel for AXIS 1) of the float64 coefficient image
// c[H][W][C]; AXIS 0 also converts the source image into it
template <typename T, int AXIS>
__global__ __launch_bounds__(256) void zoom_prefilter_kernel(const T* __restrict__ img, double* __restrict__ c, int H, int W, int C) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long lines = AXIS == 0 ? (long)W * C : (long)H * C;
    if (t >= lines) return;
    const int n = AXIS == 0 ? H : W;
    const long stride = AXIS == 0 ? (long)W * C : C;
    const long base = AXIS == 0 ? t : (t / C) * (long)W * C + (t % C);
    double* p = c + base;
    const double z = ZC_POLE;
    const double gain = (1.0 - z) * (1.0 - 1.0 / z);
    if (AXIS == 0)
        for (int i = 0; i < n; ++i) p[i * stride] = (double)img[base + i * stride];
    if (n < 2) return;
    for (int i = 0; i < n; ++i) p[i * stride] *= gain;
    const double z_n_1 = pow(z, (double)(n - 1));
    double c0 = p[0] + z_n_1 * p[(n - 1) * stride];
    double z_i = z;
    for (int i = 1; i < n - 1; ++i) {
        c0 = c0 + z_i * (p[i * stride] + z_n_1 * p[(n - 1 - i) * stride]);
        z_i *= z;
    }
    p[0] = c0 / (1.0 - z_n_1 * z_n_1);
    for (int i = 1; i < n; ++i) p[i * stride] += z * p[(i - 1) * stride];
    p[(n - 1) * stride] = (z * p[(n - 2) * stride] + p[(n - 1) * stride]) * z / (z * z - 1.0);
    for (int i = n - 2; i >= 0; --i) p[i * stride] = z * (p[(i + 1) * stride] - p[i * stride]);
}

__device__ inline int zc_mirror(int idx, int n) {
    if (n <= 1) return 0;
    const int s2 = 2 * n - 2;
    idx = (idx < 0 ? -idx : idx) % s2;
    return idx >= n ? s2 - idx : idx;
}
// returns false when x lies outside [0, n_in - 1] (step 3: the output is cval = 0)
__device__ inline bool zc_plan(int i, int n_in, int n_out, int idx[4], double w[4]) {
    const double x = (double)i * (n_out > 1 ? (double)(n_in - 1) / (double)(n_out - 1) : 0.0);
    if (x < 0.0 || x > (double)(n_in - 1)) return false;
    const double f = floor(x), t = x - f, z = 1.0 - t;
    w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
    w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
    w[0] = z * z * z / 6.0;
    w[3] = 1.0 - w[0] - w[1] - w[2];
    for (int k = 0; k < 4; ++k) idx[k] = zc_mirror((int)f - 1 + k, n_in);
    return true;
}

template <typename T>
__global__ __launch_bounds__(256) void zoom_sample_kernel(const double* __restrict__ c, T* __restrict__ out, int H, int W, int C,
                                                          int oh, int ow) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)oh * ow * C) return;
    const int ch = (int)(t % C), ox = (int)((t / C) % ow), oy = (int)(t / ((long)C * ow));
    int iy[4], ix[4];
    double wy[4], wx[4];
    const bool inside_y = zc_plan(oy, H, oh, iy, wy);
    const bool inside_x = zc_plan(ox, W, ow, ix, wx);
    if (!inside_y || !inside_x) {
        out[t] = (T)0;
        return;
    }
    double v = 0.0;
    for (int ky = 0; ky < 4; ++ky) {
        double acc = 0.0;
        for (int kx = 0; kx < 4; ++kx) acc += wx[kx] * c[((long)iy[ky] * W + ix[kx]) * C + ch];
        v += wy[ky] * acc;
    }
    if (sizeof(T) == 1) {
        v = floor(v + 0.5);
        v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
        out[t] = (T)(int)v;
    } else out[t] = (T)v;
}
}  // namespace

extern "C" size_t umi_znorm_ws_bytes(void) { return (size_t)(ZN_BLOCKS + 2) * ZN_MAXC * sizeof(double); }

extern "C" int umi_znorm_hwc(const void* img, int src_dtype, float* out_chw, long HW, int C, int reverse_channels, void* ws,
                             size_t ws_bytes, umi_stream_t stream) {
    if (!img || !out_chw || HW <= 0 || C < 1 || C > ZN_MAXC || (src_dtype != 0 && src_dtype != 1)) return UMI_ERR_BADARG;
    if (!ws || ws_bytes < umi_znorm_ws_bytes()) return UMI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double* stats = (double*)ws;                          // [2][ZN_MAXC]: mean, std
    double* part = stats + 2 * ZN_MAXC;                   // [ZN_BLOCKS][ZN_MAXC]
    long want = (HW + 255) / 256;
    const int nblk = (int)(want < ZN_BLOCKS ? want : ZN_BLOCKS);
    const int ablk = (int)((HW + 255) / 256);
#define ZN_RUN(T)                                                                                                      \
    do {                                                                                                               \
        hipLaunchKernelGGL((znorm_reduce_kernel<T, 0>), dim3(nblk), dim3(256), 0, s, (const T*)img, HW, C, stats, part); \
        hipLaunchKernelGGL((znorm_finalize_kernel<0>), dim3(1), dim3(64), 0, s, part, nblk, HW, C, stats);             \
        hipLaunchKernelGGL((znorm_reduce_kernel<T, 1>), dim3(nblk), dim3(256), 0, s, (const T*)img, HW, C, stats, part); \
        hipLaunchKernelGGL((znorm_finalize_kernel<1>), dim3(1), dim3(64), 0, s, part, nblk, HW, C, stats);             \
        hipLaunchKernelGGL((znorm_apply_kernel<T>), dim3(ablk), dim3(256), 0, s, (const T*)img, out_chw, HW, C,        \
                           reverse_channels, stats);                                                                   \
    } while (0)
    if (src_dtype == 0) ZN_RUN(unsigned char); else ZN_RUN(float);
#undef ZN_RUN
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_argmax_mask(const float* logits, unsigned char* mask, int N, int C, long HW, umi_stream_t stream) {
    if (!logits || !mask || N <= 0 || C < 1 || C > 256 || HW <= 0) return UMI_ERR_BADARG;
    if (((unsigned long)logits & 15) || ((unsigned long)mask & 3)) return UMI_ERR_BADARG;
    dim3 grid((unsigned)((HW + 1023) / 1024), N);
    hipStream_t s = (hipStream_t)stream;
    if (C == 2) hipLaunchKernelGGL((argmax_mask_kernel<2>), grid, dim3(256), 0, s, logits, mask, HW, C);
    else if (C == 4) hipLaunchKernelGGL((argmax_mask_kernel<4>), grid, dim3(256), 0, s, logits, mask, HW, C);
    else hipLaunchKernelGGL((argmax_mask_kernel<0>), grid, dim3(256), 0, s, logits, mask, HW, C);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

// scipy.ndimage.zoom(order=3) of one HWC image (C <= 4; src_dtype 0 = uint8, 1 = float32; the result has the same type), see the
// kernels above.  ws: umi_zoom_cubic_ws_bytes(H, W, C) bytes (the float64 coefficient image).
extern "C" size_t umi_zoom_cubic_ws_bytes(int H, int W, int C) { return (size_t)H * W * C * sizeof(double); }

extern "C" int umi_zoom_cubic_hwc(const void* img, int src_dtype, void* out, int H, int W, int C, int out_h, int out_w, void* ws,
                                  size_t ws_bytes, umi_stream_t stream) {
    if (!img || !out || !ws || H <= 0 || W <= 0 || C <= 0 || C > ZN_MAXC || out_h <= 0 || out_w <= 0) return UMI_ERR_BADARG;
    if (src_dtype != 0 && src_dtype != 1) return UMI_ERR_BADARG;
    if (ws_bytes < umi_zoom_cubic_ws_bytes(H, W, C)) return UMI_ERR_WORKSPACE;
    if ((long)H * W * C >= (1L << 31) || (long)out_h * out_w * C >= (1L << 31)) return UMI_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    double* c = (double*)ws;
    const unsigned g0 = (unsigned)(((long)W * C + 255) / 256), g1 = (unsigned)(((long)H * C + 255) / 256);
    const unsigned gs = (unsigned)(((long)out_h * out_w * C + 255) / 256);
    if (src_dtype == 0) {
        hipLaunchKernelGGL((zoom_prefilter_kernel<unsigned char, 0>), dim3(g0), dim3(256), 0, s, (const unsigned char*)img, c, H, W, C);
        hipLaunchKernelGGL((zoom_prefilter_kernel<unsigned char, 1>), dim3(g1), dim3(256), 0, s, (const unsigned char*)img, c, H, W, C);
        hipLaunchKernelGGL((zoom_sample_kernel<unsigned char>), dim3(gs), dim3(256), 0, s, c, (unsigned char*)out, H, W, C, out_h, out_w);
    } else {
        hipLaunchKernelGGL((zoom_prefilter_kernel<float, 0>), dim3(g0), dim3(256), 0, s, (const float*)img, c, H, W, C);
        hipLaunchKernelGGL((zoom_prefilter_kernel<float, 1>), dim3(g1), dim3(256), 0, s, (const float*)img, c, H, W, C);
        hipLaunchKernelGGL((zoom_sample_kernel<float>), dim3(gs), dim3(256), 0, s, c, (float*)out, H, W, C, out_h, out_w);
    }
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

// ---- binary-model post-processing (reference test.py:393-404 sigmoid -> >= 0.5 -> 0/1 mask -> scipy.ndimage.zoom(order=0);
// loss.py:425-431 the same threshold and the dot count of MRAccuracy)
//   umi_binary_mask    fp32 logits -> uint8, 1 where fp32 sigmoid(x) >= 0.5.  torch's 1 / (1 + exp(-x)) rounds to exactly 0.5 for
//                      every x >= -0x1.7ffffcp-23 (bits 0xB43FFFFE), found by bisection over bit patterns against torch.sigmoid
//                      (tests/test_binary_infer.py repeats it), so the kernel compares with that constant and evaluates no exp.
//                      NaN compares false: 0.
//   umi_zoom_nearest   SciPy's order-0 zoom of N uint8 / float32 images: sample coordinate x = i * ((in - 1) / (out - 1)) in
//                      float64 (0 for out == 1), source index floor(x + 0.5), and 0 where x exceeds in - 1 on either axis
//                      (mode 'constant', step 3 of the cubic resize above).
//   umi_sum_trunc      out[n] = (int) sum of image n in float64, fixed order (64 slice sums per image, then those in index order),
//                      truncated toward zero and clamped to int32 (int(np.sum(dot_map)); exact for 0/1 maps).
namespace {

constexpr unsigned BM_CUTOFF_BITS = 0xB43FFFFEu;          // -0x1.7ffffcp-23 = -1.7881390590446244e-07

__device__ inline unsigned bm_bit(float x, float cut) { return x >= cut ? 1u : 0u; }

// one thread = 16 consecutive logits -> one 16-byte store; `in_al` says the logits are 16-byte aligned as well (a view that
// starts inside its storage is not: scalar loads then)
__global__ __launch_bounds__(256) void binary_mask_kernel(const float* __restrict__ x, unsigned char* __restrict__ m, long n, int in_al) {
    const float cut = __builtin_bit_cast(float, BM_CUTOFF_BITS);
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 16;
    if (i0 >= n) return;
    if (i0 + 16 <= n) {
        unsigned w[4];
        for (int j = 0; j < 4; ++j) {
            float4 v;
            if (in_al) v = *reinterpret_cast<const float4*>(x + i0 + 4 * j);
            else v = make_float4(x[i0 + 4 * j], x[i0 + 4 * j + 1], x[i0 + 4 * j + 2], x[i0 + 4 * j + 3]);
            w[j] = bm_bit(v.x, cut) | bm_bit(v.y, cut) << 8 | bm_bit(v.z, cut) << 16 | bm_bit(v.w, cut) << 24;
        }
        *reinterpret_cast<uint4*>(m + i0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (long i = i0; i < n; ++i) m[i] = (unsigned char)bm_bit(x[i], cut);
    }
}


// one thread = 16 bytes of one output row (blockIdx.y = row, blockIdx.z = image); `al`: every row of `out` starts 16-byte aligned
template <typename T>
__global__ __launch_bounds__(256) void zoom_nearest_kernel(const T* __restrict__ in, T* __restrict__ out, int H, int W, int oh, int ow,
                                                           int al) {
    constexpr int V = 16 / sizeof(T);
    const int j0 = (blockIdx.x * 256 + threadIdx.x) * V;
    if (j0 >= ow) return;
    const int oy = blockIdx.y;
    const int sy = zn_src(oy, H, oh);
    const T* src = in + ((long)blockIdx.z * H + (sy < 0 ? 0 : sy)) * W;
    T* dst = out + ((long)blockIdx.z * oh + oy) * ow;
    alignas(16) T v[V];
    for (int k = 0; k < V; ++k) {
        const int sx = j0 + k < ow ? zn_src(j0 + k, W, ow) : -1;
        v[k] = (sy < 0 || sx < 0) ? (T)0 : src[sx];
    }
    if (al && j0 + V <= ow) *reinterpret_cast<uint4*>(dst + j0) = *reinterpret_cast<const uint4*>(v);
    else
        for (int k = 0; k < V && j0 + k < ow; ++k) dst[j0 + k] = v[k];
}

constexpr int ST_BLOCKS = 64;                             // partial sums per image

// blockIdx.x = slice of image blockIdx.y: part[n][b] = float64 sum of the slice, threads striding it, fixed-order tree
__global__ __launch_bounds__(256) void sum_trunc_partial_kernel(const float* __restrict__ x, double* __restrict__ part, long HW) {
    __shared__ double sh[256];
    const float* p = x + (long)blockIdx.y * HW;
    const long per = (HW + ST_BLOCKS - 1) / ST_BLOCKS, lo = (long)blockIdx.x * per, hi = lo + per < HW ? lo + per : HW;
    double acc = 0.0;
    for (long i = lo + threadIdx.x; i < hi; i += 256) acc += (double)p[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(long)blockIdx.y * ST_BLOCKS + blockIdx.x] = sh[0];
}

// one thread per image: the partials in index order, then the truncation
__global__ __launch_bounds__(64) void sum_trunc_finish_kernel(const double* __restrict__ part, int* __restrict__ out, int N) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    double s = 0.0;
    for (int b = 0; b < ST_BLOCKS; ++b) s += part[(long)n * ST_BLOCKS + b];
    out[n] = s != s ? 0 : (s >= 2147483647.0 ? 2147483647 : (s <= -2147483648.0 ? -2147483647 - 1 : (int)s));
}
}  // namespace

extern "C" int umi_binary_mask(const float* logits, unsigned char* mask, long n, umi_stream_t stream) {
    if (!logits || !mask || n <= 0) return UMI_ERR_BADARG;
    if (((unsigned long)logits & 3) || ((unsigned long)mask & 15)) return UMI_ERR_BADARG;
    if ((n + 4095) / 4096 >= (1L << 31)) return UMI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(binary_mask_kernel, dim3((unsigned)((n + 4095) / 4096)), dim3(256), 0, (hipStream_t)stream, logits, mask, n,
                       ((unsigned long)logits & 15) == 0 ? 1 : 0);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_zoom_nearest(const void* in, int dtype, void* out, int N, int H, int W, int out_h, int out_w, umi_stream_t stream) {
    if (!in || !out || N <= 0 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0) return UMI_ERR_BADARG;
    if (dtype != 0 && dtype != 1) return UMI_ERR_BADARG;
    if (N > 65535 || out_h > 65535 || (long)N * H * W >= (1L << 31) || (long)N * out_h * out_w >= (1L << 31)) return UMI_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int esz = dtype == 0 ? 1 : 4, V = 16 / esz;
    const int al = (((unsigned long)out & 15) == 0 && ((long)out_w * esz) % 16 == 0) ? 1 : 0;
    const dim3 grid((unsigned)((out_w + 256 * V - 1) / (256 * V)), out_h, N);
    if (dtype == 0)
        hipLaunchKernelGGL((zoom_nearest_kernel<unsigned char>), grid, dim3(256), 0, s, (const unsigned char*)in, (unsigned char*)out, H, W,
                           out_h, out_w, al);
    else
        hipLaunchKernelGGL((zoom_nearest_kernel<float>), grid, dim3(256), 0, s, (const float*)in, (float*)out, H, W, out_h, out_w, al);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" size_t umi_sum_trunc_ws_bytes(int N) { return N > 0 ? (size_t)N * ST_BLOCKS * sizeof(double) : 0; }

extern "C" int umi_sum_trunc(const float* x, int* out, int N, long HW, void* ws, size_t ws_bytes, umi_stream_t stream) {
    if (!x || !out || N <= 0 || HW <= 0) return UMI_ERR_BADARG;
    if (N > 65535) return UMI_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < umi_sum_trunc_ws_bytes(N)) return UMI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sum_trunc_partial_kernel, dim3(ST_BLOCKS, N), dim3(256), 0, s, x, (double*)ws, HW);
    hipLaunchKernelGGL(sum_trunc_finish_kernel, dim3((N + 63) / 64), dim3(64), 0, s, (const double*)ws, out, N);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
