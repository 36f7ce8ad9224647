// Random-crop training batches and padded tile grids cut out of images that stay on the device (reference DataLoader.py
// `DataRandomCrop` :928-1069 with `pad_image` :27-47, and test.py `preprocessCrop` :91-128; statement: umi/augment.py
// crop_transform_numpy / grid_transform_numpy).
//
// The sources of the crop kernels live in a POOL: one buffer holding images of different sizes but one channel count and type,
// offsets[i] = the element offset of image i, sizes[i] = {H, W}.  Label and dot maps have pools of their own with the same sizes.
//
//   umi_crop_znorm    N crops -> [N][C][crop][crop] float32: per crop {index, r0, c0}, the geometry of augment.hip applied to the
//                     crop window (a rotation samples the crop, so what lay outside it comes out 0), float64 statistics of the
//                     augmented crop, then one pass that gathers, normalises and stores.  The augmented crop is never written.
//   umi_crop_labels   the same gather for a map pool -> [N][crop][crop] float32 / int64 / uint8
//   umi_grid_znorm    one image, constant-padded to [Hp][Wp] -> its row-major [T][C][th][tw] tiles, z-normalised with the
//                     statistics of the whole padded image = the source's sums plus the closed-form pad terms.  The padded image
//                     is never materialised; th = Hp, tw = Wp is the whole padded image (preprocessCrop).
//   umi_grid_labels   the same tile walk for a map, pad value 0
//
// All are gathers of the shape of augment.hip: one thread per output pixel in 64 x 4 tiles, so a wave stores one contiguous row
// segment and reads source rows strided by the image width.  The sums run in a fixed order without atomics: two runs give the same
// bits.  Every table is read on the device and nothing synchronises with the host, so each call can be captured in a graph; the
// number of launches does not depend on N.
//
// Safety: a crop row is used only when 0 <= index < n_images, the window [r0, r0 + crop) x [c0, c0 + crop) lies inside that image
// and the image lies inside the pool buffer; otherwise the whole sample comes out 0 and nothing of the pool is read.  Inside a
// valid window every source pixel is (r0 + y, c0 + x) with (y, x) in [0, crop)^2 (ag_src_yx), addressed in 64 bits.
#include <type_traits>
#include "augment_gather.h"

#pragma clang fp contract(off)
namespace {

constexpr int GR_BLOCKS = 256;                           // partial sums of the one image of a grid call
// uint8 variance from exact integers: n * S2 - S1 * S1 in unsigned 64 bits is exact while (255 * n)^2 < 2^64
constexpr long CR_MAX_U8_PIXELS = 16843009;

struct CrWindow {
    long base;                                           // element offset of the image in the pool
    int W, r0, c0;
    bool ok;
};

__device__ inline CrWindow cr_window(const long long* __restrict__ offsets, const int* __restrict__ sizes, int n_images,
                                     long long pool_elems, int C, const int* __restrict__ crops, int n, int crop) {
    CrWindow w = {0, 0, 0, 0, false};
    const int idx = crops[n * 3 + 0], r0 = crops[n * 3 + 1], c0 = crops[n * 3 + 2];
    if (idx < 0 || idx >= n_images) return w;
    const int H = sizes[idx * 2 + 0], W = sizes[idx * 2 + 1];
    const long long off = offsets[idx];
    if (H < crop || W < crop || r0 < 0 || c0 < 0 || r0 > H - crop || c0 > W - crop) return w;
    if ((long long)H * W > pool_elems / C) return w;     // the pool's own tables: the image has to lie inside the buffer
    if (off < 0 || off > pool_elems - (long long)H * W * C) return w;
    w.base = (long)off;
    w.W = W;
    w.r0 = r0;
    w.c0 = c0;
    w.ok = true;
    return w;
}

// element index of channel 0 of the source pixel of output pixel (r, q) of the crop; -1 where the output is 0
__device__ inline long cr_src(const CrWindow& w, const AgSample& s, int r, int q, int crop, int C) {
    int y, x;
    if (!ag_src_yx(s, r, q, crop, crop, y, x)) return -1;
    return w.base + ((long)(w.r0 + y) * w.W + (w.c0 + x)) * C;
}

// ---- crops: statistics of the augmented crop per (sample, channel), the scheme of augment.hip --------------------------------
// ws: stats[N][2][AG_MAXC] float64 (mean, std), then part[N][AG_STAT_BLOCKS][2][AG_MAXC].
template <typename T, int PASS>
__global__ __launch_bounds__(256) void cr_stats_kernel(const T* __restrict__ pool, const long long* __restrict__ offsets,
                                                       const int* __restrict__ sizes, int n_images, long long pool_elems,
                                                       const int* __restrict__ crops, const int* __restrict__ params,
                                                       const double* __restrict__ geom, int crop, int C,
                                                       const double* __restrict__ stats, void* __restrict__ part_) {
    constexpr bool U8 = sizeof(T) == 1;
    typedef typename std::conditional<U8, unsigned long long, double>::type V;
    __shared__ V sh[4];
    const int n = blockIdx.y, HW = crop * crop;
    const CrWindow w = cr_window(offsets, sizes, n_images, pool_elems, C, crops, n, crop);
    const AgSample s = ag_load(params, geom, n);
    V a1[AG_MAXC] = {0, 0, 0, 0}, a2[AG_MAXC] = {0, 0, 0, 0};
    double mean[AG_MAXC] = {0.0, 0.0, 0.0, 0.0};
    if (PASS == 1)
        for (int c = 0; c < C; ++c) mean[c] = stats[(long)n * 2 * AG_MAXC + c];
    const int per = (HW + AG_STAT_BLOCKS - 1) / AG_STAT_BLOCKS;
    const int lo = blockIdx.x * per, hi = lo + per < HW ? lo + per : HW;
    if (w.ok)                                            // wave-uniform: an invalid sample reads nothing
        for (int p = lo + threadIdx.x; p < hi; p += 256) {
            const int r = p / crop, q = p - r * crop;
            const long sp = cr_src(w, s, r, q, crop, C);
            for (int c = 0; c < C; ++c) {
                if (U8) {
                    const V v = sp < 0 ? 0 : (V)pool[sp + c];
                    a1[c] += v;
                    a2[c] += v * v;
                } else {
                    const double d = (sp < 0 ? 0.0 : (double)pool[sp + c]) - mean[c];
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
__global__ __launch_bounds__(AG_TX * AG_TY) void cr_znorm_kernel(const T* __restrict__ pool, const long long* __restrict__ offsets,
                                                                 const int* __restrict__ sizes, int n_images, long long pool_elems,
                                                                 const int* __restrict__ crops, const int* __restrict__ params,
                                                                 const double* __restrict__ geom, int crop, int C, int reverse,
                                                                 const double* __restrict__ stats, float* __restrict__ out) {
    const int q = blockIdx.x * AG_TX + threadIdx.x, r = blockIdx.y * AG_TY + threadIdx.y, n = blockIdx.z;
    if (q >= crop || r >= crop) return;
    const long HW = (long)crop * crop;
    float* o = out + (long)n * C * HW + (long)r * crop + q;
    const CrWindow w = cr_window(offsets, sizes, n_images, pool_elems, C, crops, n, crop);
    if (!w.ok) {
        for (int c = 0; c < C; ++c) o[(long)c * HW] = 0.f;
        return;
    }
    const long sp = cr_src(w, ag_load(params, geom, n), r, q, crop, C);
    const double* st = stats + (long)n * 2 * AG_MAXC;
    for (int c = 0; c < C; ++c) {
        const double v = ((sp < 0 ? 0.0 : (double)pool[sp + c]) - st[c]) / st[AG_MAXC + c];      // fp64, then one rounding to fp32
        o[(long)(reverse ? C - 1 - c : c) * HW] = (float)v;
    }
}

// TO = float: (float)v * scale; TO = long long: that product converted like torch's .long() (truncation); TO = unsigned char:
// the uint8 source value as it is (dot maps)
template <typename T, typename TO>
__device__ inline TO cr_label_value(T v, float scale) {
    if constexpr (sizeof(TO) == 1) return (TO)v;
    else return (TO)((float)v * scale);
}

template <typename T, typename TO>
__global__ __launch_bounds__(AG_TX * AG_TY) void cr_labels_kernel(const T* __restrict__ pool, const long long* __restrict__ offsets,
                                                                  const int* __restrict__ sizes, int n_images, long long pool_elems,
                                                                  const int* __restrict__ crops, const int* __restrict__ params,
                                                                  const double* __restrict__ geom, int crop, float scale,
                                                                  TO* __restrict__ dst) {
    const int q = blockIdx.x * AG_TX + threadIdx.x, r = blockIdx.y * AG_TY + threadIdx.y, n = blockIdx.z;
    if (q >= crop || r >= crop) return;
    const CrWindow w = cr_window(offsets, sizes, n_images, pool_elems, 1, crops, n, crop);
    const long sp = w.ok ? cr_src(w, ag_load(params, geom, n), r, q, crop, 1) : -1;
    dst[((long)n * crop + r) * crop + q] = sp < 0 ? (TO)0 : cr_label_value<T, TO>(pool[sp], scale);
}

// ---- grid: statistics of the padded image = sums over the source + the pad terms ---------------------------------------------
// ws: stats[2][AG_MAXC] float64 (mean, std), then part[GR_BLOCKS][2][AG_MAXC].
template <typename T, int PASS>
__global__ __launch_bounds__(256) void gr_stats_kernel(const T* __restrict__ src, long HW, int C, const double* __restrict__ stats,
                                                       void* __restrict__ part_) {
    constexpr bool U8 = sizeof(T) == 1;
    typedef typename std::conditional<U8, unsigned long long, double>::type V;
    __shared__ V sh[4];
    V a1[AG_MAXC] = {0, 0, 0, 0}, a2[AG_MAXC] = {0, 0, 0, 0};
    double mean[AG_MAXC] = {0.0, 0.0, 0.0, 0.0};
    if (PASS == 1)
        for (int c = 0; c < C; ++c) mean[c] = stats[c];
    const long per = (HW + GR_BLOCKS - 1) / GR_BLOCKS;
    const long lo = blockIdx.x * per, hi = lo + per < HW ? lo + per : HW;
    for (long p = lo + threadIdx.x; p < hi; p += 256)
        for (int c = 0; c < C; ++c) {
            if (U8) {
                const V v = (V)src[p * C + c];
                a1[c] += v;
                a2[c] += v * v;
            } else {
                const double d = (double)src[p * C + c] - mean[c];
                a1[c] += PASS == 0 ? d : d * d;
            }
        }
    V* part = (V*)part_ + (long)blockIdx.x * 2 * AG_MAXC;
    for (int c = 0; c < C; ++c) {
        const V t1 = ag_block_sum(a1[c], sh);
        if (threadIdx.x == 0) part[c] = t1;
        if (U8) {
            const V t2 = ag_block_sum(a2[c], sh);
            if (threadIdx.x == 0) part[AG_MAXC + c] = t2;
        }
    }
}

// one thread per channel: the slices in index order, then the pad term, added last
template <typename T, int PASS>
__global__ __launch_bounds__(64) void gr_stats_finish_kernel(const void* __restrict__ part_, int C, long n, long npad, int pad_value,
                                                             double* __restrict__ stats) {
    constexpr bool U8 = sizeof(T) == 1;
    typedef typename std::conditional<U8, unsigned long long, double>::type V;
    const int c = threadIdx.x;
    if (c >= C) return;
    const V* part = (const V*)part_;
    V s1 = 0, s2 = 0;
    for (int b = 0; b < GR_BLOCKS; ++b) {
        s1 += part[(long)b * 2 * AG_MAXC + c];
        if (U8) s2 += part[(long)b * 2 * AG_MAXC + AG_MAXC + c];
    }
    if (U8) {
        const unsigned long long cnt = (unsigned long long)n, v = (unsigned long long)pad_value;
        const unsigned long long t1 = (unsigned long long)s1 + (unsigned long long)npad * v;
        const unsigned long long t2 = (unsigned long long)s2 + (unsigned long long)npad * v * v;
        stats[c] = (double)t1 / (double)n;
        stats[AG_MAXC + c] = sqrt((double)(cnt * t2 - t1 * t1)) / (double)n;
    } else if (PASS == 0) {
        stats[c] = ((double)s1 + (double)npad * (double)pad_value) / (double)n;
    } else {
        const double d = (double)pad_value - stats[c];
        stats[AG_MAXC + c] = sqrt(((double)s1 + (double)npad * (d * d)) / (double)n);
    }
}

// tile pixel (r, q) of tile t -> element index of the source pixel, -1 in the padding
__device__ inline long gr_src(int t, int r, int q, int H, int W, int pad_top, int pad_left, int tiles_x, int th, int tw) {
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const long sy = (long)ty * th + r - pad_top, sx = (long)tx * tw + q - pad_left;
    return sy >= 0 && sy < H && sx >= 0 && sx < W ? sy * W + sx : -1;
}

template <typename T>
__global__ __launch_bounds__(AG_TX * AG_TY) void gr_znorm_kernel(const T* __restrict__ src, int H, int W, int C, int pad_top,
                                                                 int pad_left, int pad_value, int tiles_x, int th, int tw,
                                                                 int reverse, const double* __restrict__ stats,
                                                                 float* __restrict__ out) {
    const int q = blockIdx.x * AG_TX + threadIdx.x, r = blockIdx.y * AG_TY + threadIdx.y, t = blockIdx.z;
    if (q >= tw || r >= th) return;
    const long sp = gr_src(t, r, q, H, W, pad_top, pad_left, tiles_x, th, tw);
    const long HW = (long)th * tw;
    float* o = out + (long)t * C * HW + (long)r * tw + q;
    for (int c = 0; c < C; ++c) {
        const double v = ((sp < 0 ? (double)pad_value : (double)src[sp * C + c]) - stats[c]) / stats[AG_MAXC + c];
        o[(long)(reverse ? C - 1 - c : c) * HW] = (float)v;
    }
}

template <typename T, typename TO>
__global__ __launch_bounds__(AG_TX * AG_TY) void gr_labels_kernel(const T* __restrict__ src, int H, int W, int pad_top, int pad_left,
                                                                  int tiles_x, int th, int tw, float scale, TO* __restrict__ dst) {
    const int q = blockIdx.x * AG_TX + threadIdx.x, r = blockIdx.y * AG_TY + threadIdx.y, t = blockIdx.z;
    if (q >= tw || r >= th) return;
    const long sp = gr_src(t, r, q, H, W, pad_top, pad_left, tiles_x, th, tw);
    dst[((long)t * th + r) * tw + q] = sp < 0 ? (TO)0 : cr_label_value<T, TO>(src[sp], scale);
}

// shared argument checks of the crop calls: 0 when the gather grids can be formed
int cr_check(const void* pool, const long long* offsets, const int* sizes, const int* crops, const int* params, const double* geom,
             const void* dst, int dtype, int n_images, long long pool_elems, int C, int N, int crop) {
    if (!pool || !offsets || !sizes || !crops || !params || !geom || !dst) return UMI_ERR_BADARG;
    if (n_images <= 0 || pool_elems <= 0 || N <= 0 || crop <= 0 || C <= 0 || C > AG_MAXC || (dtype != 0 && dtype != 1))
        return UMI_ERR_BADARG;
    if (N > 65535 || (crop + AG_TY - 1) / AG_TY > 65535 || (long)crop * crop >= (1L << 30)) return UMI_ERR_UNSUPPORTED;
    return UMI_OK;
}

// 0 when the padded image [Hp][Wp] holds the source at (pad_top, pad_left) and splits into whole th x tw tiles
int gr_check(const void* src, const void* dst, int dtype, int H, int W, int C, int pad_top, int pad_left, int Hp, int Wp, int th,
             int tw) {
    if (!src || !dst || H <= 0 || W <= 0 || C <= 0 || C > AG_MAXC || (dtype != 0 && dtype != 1)) return UMI_ERR_BADARG;
    if (pad_top < 0 || pad_left < 0 || th <= 0 || tw <= 0 || Hp < H || Wp < W || pad_top > Hp - H || pad_left > Wp - W)
        return UMI_ERR_BADARG;
    if (Hp % th || Wp % tw) return UMI_ERR_BADARG;
    if ((long)(Hp / th) * (Wp / tw) > 65535 || (th + AG_TY - 1) / AG_TY > 65535 || (long)Hp * Wp >= (1L << 31))
        return UMI_ERR_UNSUPPORTED;
    return UMI_OK;
}

dim3 cr_grid(int N, int h, int w) { return dim3((unsigned)((w + AG_TX - 1) / AG_TX), (unsigned)((h + AG_TY - 1) / AG_TY), (unsigned)N); }

}  // namespace

extern "C" size_t umi_crop_znorm_ws_bytes(int N) {
    return N > 0 ? (size_t)N * (2 + 2 * AG_STAT_BLOCKS) * AG_MAXC * sizeof(double) : 0;
}

extern "C" int umi_crop_znorm(const void* pool, int dtype, const long long* offsets, const int* sizes, int n_images,
                              long long pool_elems, int C, const int* crops, const int* params, const double* geom, int N, int crop,
                              float* out_nchw, int reverse_channels, void* ws, size_t ws_bytes, umi_stream_t stream) {
    const int bad = cr_check(pool, offsets, sizes, crops, params, geom, out_nchw, dtype, n_images, pool_elems, C, N, crop);
    if (bad) return bad;
    if (!ws || ws_bytes < umi_crop_znorm_ws_bytes(N)) return UMI_ERR_WORKSPACE;
    if (dtype == 0 && (long)crop * crop > CR_MAX_U8_PIXELS) return UMI_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    double* stats = (double*)ws;
    void* part = stats + (size_t)N * 2 * AG_MAXC;
    const dim3 sgrid(AG_STAT_BLOCKS, N), fgrid((N * C + 63) / 64);
    const int HW = crop * crop;
#define CR_STATS(T, PASS)                                                                                                          \
    do {                                                                                                                           \
        hipLaunchKernelGGL((cr_stats_kernel<T, PASS>), sgrid, dim3(256), 0, s, (const T*)pool, offsets, sizes, n_images, pool_elems, \
                           crops, params, geom, crop, C, stats, part);                                                             \
        hipLaunchKernelGGL((ag_stats_finish_kernel<T, PASS>), fgrid, dim3(64), 0, s, part, N, HW, C, stats);                       \
    } while (0)
#define CR_ZNORM(T)                                                                                                                \
    hipLaunchKernelGGL((cr_znorm_kernel<T>), cr_grid(N, crop, crop), dim3(AG_TX, AG_TY), 0, s, (const T*)pool, offsets, sizes,     \
                       n_images, pool_elems, crops, params, geom, crop, C, reverse_channels, stats, out_nchw)
    if (dtype == 0) {
        CR_STATS(unsigned char, 0);
        CR_ZNORM(unsigned char);
    } else {
        CR_STATS(float, 0);
        CR_STATS(float, 1);
        CR_ZNORM(float);
    }
#undef CR_STATS
#undef CR_ZNORM
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_crop_labels(const void* pool, int src_dtype, const long long* offsets, const int* sizes, int n_images,
                               long long pool_elems, const int* crops, const int* params, const double* geom, int N, int crop,
                               void* dst, int dst_dtype, float scale, umi_stream_t stream) {
    const int bad = cr_check(pool, offsets, sizes, crops, params, geom, dst, src_dtype, n_images, pool_elems, 1, N, crop);
    if (bad) return bad;
    if (dst_dtype < 0 || dst_dtype > 2 || (dst_dtype == 2 && src_dtype != 0)) return UMI_ERR_BADARG;
    hipStream_t s = (hipStream_t)stream;
#define CR_LABELS(T, TO)                                                                                                           \
    hipLaunchKernelGGL((cr_labels_kernel<T, TO>), cr_grid(N, crop, crop), dim3(AG_TX, AG_TY), 0, s, (const T*)pool, offsets, sizes, \
                       n_images, pool_elems, crops, params, geom, crop, scale, (TO*)dst)
    if (dst_dtype == 2) CR_LABELS(unsigned char, unsigned char);
    else if (src_dtype == 0 && dst_dtype == 0) CR_LABELS(unsigned char, float);
    else if (src_dtype == 0) CR_LABELS(unsigned char, long long);
    else if (dst_dtype == 0) CR_LABELS(float, float);
    else CR_LABELS(float, long long);
#undef CR_LABELS
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" size_t umi_grid_znorm_ws_bytes(void) { return (size_t)(2 + 2 * GR_BLOCKS) * AG_MAXC * sizeof(double); }

extern "C" int umi_grid_znorm(const void* src, int dtype, int H, int W, int C, int pad_top, int pad_left, int pad_value, int Hp,
                              int Wp, int th, int tw, float* out, int reverse_channels, void* ws, size_t ws_bytes,
                              umi_stream_t stream) {
    const int bad = gr_check(src, out, dtype, H, W, C, pad_top, pad_left, Hp, Wp, th, tw);
    if (bad) return bad;
    if (pad_value < 0 || pad_value > 255) return UMI_ERR_BADARG;
    if (!ws || ws_bytes < umi_grid_znorm_ws_bytes()) return UMI_ERR_WORKSPACE;
    const long n = (long)Hp * Wp, HW = (long)H * W, npad = n - HW;
    if (dtype == 0 && n > CR_MAX_U8_PIXELS) return UMI_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    double* stats = (double*)ws;
    void* part = stats + 2 * AG_MAXC;
    const int tiles_x = Wp / tw, T = (Hp / th) * tiles_x;
#define GR_STATS(T_, PASS)                                                                                                         \
    do {                                                                                                                           \
        hipLaunchKernelGGL((gr_stats_kernel<T_, PASS>), dim3(GR_BLOCKS), dim3(256), 0, s, (const T_*)src, HW, C, stats, part);     \
        hipLaunchKernelGGL((gr_stats_finish_kernel<T_, PASS>), dim3(1), dim3(64), 0, s, part, C, n, npad, pad_value, stats);       \
    } while (0)
#define GR_ZNORM(T_)                                                                                                               \
    hipLaunchKernelGGL((gr_znorm_kernel<T_>), cr_grid(T, th, tw), dim3(AG_TX, AG_TY), 0, s, (const T_*)src, H, W, C, pad_top,      \
                       pad_left, pad_value, tiles_x, th, tw, reverse_channels, stats, out)
    if (dtype == 0) {
        GR_STATS(unsigned char, 0);
        GR_ZNORM(unsigned char);
    } else {
        GR_STATS(float, 0);
        GR_STATS(float, 1);
        GR_ZNORM(float);
    }
#undef GR_STATS
#undef GR_ZNORM
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_grid_labels(const void* src, int src_dtype, int H, int W, int pad_top, int pad_left, int Hp, int Wp, int th,
                               int tw, void* dst, int dst_dtype, float scale, umi_stream_t stream) {
    const int bad = gr_check(src, dst, src_dtype, H, W, 1, pad_top, pad_left, Hp, Wp, th, tw);
    if (bad) return bad;
    if (dst_dtype < 0 || dst_dtype > 2 || (dst_dtype == 2 && src_dtype != 0)) return UMI_ERR_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const int tiles_x = Wp / tw, T = (Hp / th) * tiles_x;
#define GR_LABELS(T_, TO)                                                                                                          \
    hipLaunchKernelGGL((gr_labels_kernel<T_, TO>), cr_grid(T, th, tw), dim3(AG_TX, AG_TY), 0, s, (const T_*)src, H, W, pad_top,    \
                       pad_left, tiles_x, th, tw, scale, (TO*)dst)
    if (dst_dtype == 2) GR_LABELS(unsigned char, unsigned char);
    else if (src_dtype == 0 && dst_dtype == 0) GR_LABELS(unsigned char, float);
    else if (src_dtype == 0) GR_LABELS(unsigned char, long long);
    else if (dst_dtype == 0) GR_LABELS(float, float);
    else GR_LABELS(float, long long);
#undef GR_LABELS
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
