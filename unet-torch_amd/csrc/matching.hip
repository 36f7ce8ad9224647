// Localisation scoring on the device: what the reference's evaluation scripts do with the components of a predicted mask
// (reference CrowdMatching.py: CrowdMatchingTest :108-189, the three-argument CrowdMatchingTest2 :270-296, GMAE :309-331).
// Everything here is integer work or a look-up in a float64 table that the HOST computed with the reference's expression, so
// the device evaluates no exp and no square root and every result is exact.
//
//   dot lists    (N,H,W) dot map -> per image the coordinates (x, y) of its non-zero pixels in RASTER order and their number.
//                Three launches: non-zeros per 1024-pixel block, a fixed-order scan per image, ranks by ballot.  Raster order is
//                the tie rule of both matchings.  An image with more than max_dots dots sets the fault word (first int32 of the
//                workspace), keeps the first max_dots of them and writes nothing beyond its row.
//   centres      label statistics -> (x, y) = (round(sum_x / area), round(sum_y / area)), half to even, in integers.
//   crowd match  one workgroup per (image, sigma, threshold).  The centres are taken one after the other (each match removes
//                a dot, so the loop over centres is a true dependency chain); for one centre the 256 lanes scan the image's
//                dots in LDS, look table[dy + r][dx + r] up for the remaining dots inside the (2r+1)^2 window and reduce to
//                (largest value, lowest dot index) in two LDS steps: atomicMax of the value's bit pattern (non-negative
//                doubles order like their bits), a barrier, then atomicMin of the index among the lanes that hold that value.
//                Only lanes with a dot inside the window issue an atomic, a centre whose best value is below the threshold
//                skips the second step, and the slots rotate through three copies so that clearing the next one never meets
//                a late reader of the last one.  (A shuffle tree over (float64, index) pairs -- 18 ds_bpermute in a row per
//                centre -- measured 1.4 us per centre at 400 dots against 1.16 us for this; DESIGN.md.)  Thread t owns the dots t, t + 256, ...: their
//                `remaining` bits are ONE REGISTER of that thread (max_dots <= 8192 = 32 * 256), which only the owner reads
//                and clears.
//                The tables stay in global memory: one centre reads a handful of entries (the dots inside its window), the
//                sigma-20 table (161 x 161 float64 = 207 KB) does not fit LDS next to the dots, and it is L2-resident anyway.
//                No address is ever formed from a centre's coordinates, so an out-of-range centre cannot fault.
//   distance     one workgroup per image: the dots in raster order, for each the nearest still-free centre by squared integer
//                distance (lowest centre index on ties), matched when d2 <= d2_max: the same two LDS steps, atomicMin of d2
//                among the lanes whose nearest free centre is within reach, then atomicMin of the index.  Thread t owns the
//                centres t, t + 256, ...: `taken` is a register for the first 8192 centres and a byte of the workspace,
//                touched by the owner only, beyond; the first 4096 centres are staged in LDS.
//   grid sums    one workgroup per cell of the 8 x 8 grid of size/8-pixel cells: int64 for uint8 maps, float64 in a fixed order
//                (strided per thread, then a fixed tree) for float32 maps.
//   scatter      map[n][y][x] = 1 per centre inside the image (a store, not an add: coinciding centres count once).
//   class split  a class-valued map (N,H,W) -> (N,K-1,H,W) 0/1 planes, plane c - 1 = (map == c); the passes above then run
//                unchanged on the (N * (K - 1), H, W) view.
//   class lists  umi_label_class_components' statistics -> per (image, class) the centres of that class's labels in label order
//                (the raster order of first pixels) and their number: one workgroup per (image, class) walks the labels 256 at a
//                time, positions by ballot rank plus a running total, so the order is fixed and no atomic is involved.
#include "common.h"

namespace {

constexpr int MT_BLK = 1024;            // pixels per block of the compaction passes
constexpr int MT_HEAD = 256;            // bytes in front of the workspace; the first int32 is the fault word
constexpr int MT_MAX_DOTS = 8192;       // 32 register bits x 256 threads
constexpr int MT_MAX_SIGMAS = 8;
constexpr int MT_LDS_CENTERS = 4096;    // centres of the distance matching kept in LDS; the rest is read from global memory
constexpr int MT_REG_CENTERS = 8192;    // centres whose `taken` flag is a register bit
constexpr int MT_NONE = 0x7fffffff;     // "no candidate" index

template <typename T>
__global__ __launch_bounds__(256) void mt_dot_count_kernel(const T* __restrict__ map, int HW, int nblk, int* __restrict__ blockcnt) {
    __shared__ int wsum[4];
    const T* img = map + (long)blockIdx.y * HW;
    int mine = 0;
    for (int k = 0; k < MT_BLK / 256; ++k) {
        const int i = blockIdx.x * MT_BLK + k * 256 + threadIdx.x;
        mine += __popcll(__ballot(i < HW && img[i] != (T)0));
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) blockcnt[(long)blockIdx.y * nblk + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup per image: blockcnt -> exclusive prefix in raster order (in place); g_count[n] = min(total, max_dots)
__global__ __launch_bounds__(256) void mt_dot_scan_kernel(int* __restrict__ blockcnt, int nblk, int max_dots, int* __restrict__ g_count,
                                                          int* __restrict__ err) {
    __shared__ int part[256];
    int* c = blockcnt + (long)blockIdx.x * nblk;
    const int seg = (nblk + 255) / 256, b0 = min((int)threadIdx.x * seg, nblk), b1 = min(b0 + seg, nblk);
    int s = 0;
    for (int b = b0; b < b1; ++b) s += c[b];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) {
            const int v = part[t];
            part[t] = run;
            run += v;
        }
        g_count[blockIdx.x] = min(run, max_dots);
        if (run > max_dots) *err = 1;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int b = b0; b < b1; ++b) {
        const int v = c[b];
        c[b] = run;
        run += v;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void mt_dot_write_kernel(const T* __restrict__ map, int HW, int W, int nblk,
                                                           const int* __restrict__ blockoff, int max_dots, int* __restrict__ dots) {
    __shared__ int wcnt[MT_BLK / 64];
    const T* img = map + (long)blockIdx.y * HW;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bool flag[MT_BLK / 256];
    int before[MT_BLK / 256];
    for (int k = 0; k < MT_BLK / 256; ++k) {
        const int i = blockIdx.x * MT_BLK + k * 256 + threadIdx.x;
        flag[k] = i < HW && img[i] != (T)0;
        const unsigned long long b = __ballot(flag[k]);
        before[k] = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[k * 4 + wv] = __popcll(b);
    }
    __syncthreads();
    const int off = blockoff[(long)blockIdx.y * nblk + blockIdx.x];
    int* row = dots + (long)blockIdx.y * max_dots * 2;
    for (int k = 0; k < MT_BLK / 256; ++k) {
        if (!flag[k]) continue;
        int pre = 0;
        for (int j = 0; j < k * 4 + wv; ++j) pre += wcnt[j];
        const int pos = off + pre + before[k];
        if (pos < 0 || pos >= max_dots) continue;               // the scan pass reports the overflow
        const int i = blockIdx.x * MT_BLK + k * 256 + threadIdx.x, y = i / W;
        row[2 * pos] = i - y * W;
        row[2 * pos + 1] = y;
    }
}

// round(s / a) with ties to even, s >= 0, a > 0
__device__ __forceinline__ int mt_round_div(long long s, long long a) {
    const long long q = s / a, r2 = 2 * (s - q * a);
    return (int)(r2 > a || (r2 == a && (q & 1)) ? q + 1 : q);
}

__global__ __launch_bounds__(256) void mt_centers_kernel(const int* __restrict__ counts, const int* __restrict__ area,
                                                         const long long* __restrict__ sum_y, const long long* __restrict__ sum_x,
                                                         int* __restrict__ centers, int N, int cap) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)N * cap) return;
    const int n = (int)(t / cap), c = (int)(t - (long)n * cap);
    int x = 0, y = 0;
    const int a = area[t];
    if (c < counts[n] && a > 0 && sum_x[t] >= 0 && sum_y[t] >= 0) {
        x = mt_round_div(sum_x[t], a);
        y = mt_round_div(sum_y[t], a);
    }
    centers[2 * t] = x;
    centers[2 * t + 1] = y;
}

struct MtSigmas {
    int r[MT_MAX_SIGMAS];
    int off[MT_MAX_SIGMAS];              // first entry of the sigma's (2r+1)^2 table, in doubles
};

// grid (T, S, N); out[n][s][t] = (tp, fp)
__global__ __launch_bounds__(256) void mt_crowd_match_kernel(const int* __restrict__ dots, const int* __restrict__ g_count, int max_dots,
                                                             const int* __restrict__ centers, const int* __restrict__ c_count,
                                                             int cap, const double* __restrict__ tables, MtSigmas sg,
                                                             const double* __restrict__ thresh, int* __restrict__ out) {
    __shared__ int sdot[MT_MAX_DOTS];                           // y << 16 | x
    __shared__ unsigned long long vmax[3];                      // three slots in rotation (file header)
    __shared__ int imin[3];
    const int n = blockIdx.z, s = blockIdx.y, t = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int ng = min(max(g_count[n], 0), max_dots), nc = min(max(c_count[n], 0), cap);
    const int* drow = dots + (long)n * max_dots * 2;
    unsigned remaining = 0;                                     // bit j: dot j * 256 + tid is still unmatched
    for (int i = tid, j = 0; i < ng; i += 256, ++j) {
        sdot[i] = (drow[2 * i + 1] & 0xffff) << 16 | (drow[2 * i] & 0xffff);
        remaining |= 1u << j;
    }
    if (tid < 3) {
        vmax[tid] = 0ull;
        imin[tid] = MT_NONE;
    }
    __syncthreads();
    const int r = sg.r[s], K = 2 * r + 1;
    const double* tab = tables + sg.off[s];
    const double th = thresh[t];
    const int* crow = centers + (long)n * cap * 2;
    int tp = 0, fp = 0, p = 0;
    int lx = 0, ly = 0;                                         // centre (c & ~63) + lane: one coalesced load per 64 centres
    for (int c = 0; c < nc; ++c) {
        if ((c & 63) == 0 && c + lane < nc) {
            lx = crow[2 * (c + lane)];
            ly = crow[2 * (c + lane) + 1];
        }
        const long long cx = __shfl(lx, c & 63, 64), cy = __shfl(ly, c & 63, 64);
        double best = 0.0;
        int bi = MT_NONE;
        unsigned m = remaining;
        while (m) {
            const int j = __builtin_ctz(m);
            m &= m - 1;
            const int i = j * 256 + tid, d = sdot[i];
            const long long dx = (long long)(d & 0xffff) - cx, dy = (long long)((unsigned)d >> 16) - cy;
            if (dx < -r || dx > r || dy < -r || dy > r) continue;
            const double v = tab[(int)(dy + r) * K + (int)(dx + r)];
            if (v > best || (v == best && i < bi)) {
                best = v;
                bi = i;
            }
        }
        const int q = p == 2 ? 0 : p + 1;
        if (tid == 0) {                                         // the next centre's slot: last read two centres ago
            vmax[q] = 0ull;
            imin[q] = MT_NONE;
        }
        // non-negative doubles order like their bit patterns
        const unsigned long long bits = (unsigned long long)__double_as_longlong(best);
        if (bi != MT_NONE && bits) atomicMax(&vmax[p], bits);
        __syncthreads();
        const unsigned long long top = vmax[p];
        if (__longlong_as_double((long long)top) < th) {        // workgroup-uniform
            ++fp;
            p = q;
            continue;
        }
        if (bi != MT_NONE && bits == top) atomicMin(&imin[p], bi);
        __syncthreads();
        const int hit = imin[p];
        ++tp;
        if (hit < ng && (hit & 255) == tid) remaining &= ~(1u << (hit >> 8));
        p = q;
    }
    if (tid == 0) {
        int* o = out + (((long)n * gridDim.y + s) * gridDim.x + t) * 2;
        o[0] = tp;
        o[1] = fp;
    }
}

// grid (N); out[n] = (tp, centres, dots)
__global__ __launch_bounds__(256) void mt_distance_match_kernel(const int* __restrict__ dots, const int* __restrict__ g_count,
                                                                int max_dots, const int* __restrict__ centers,
                                                                const int* __restrict__ c_count, int cap, long long d2_max,
                                                                unsigned char* __restrict__ taken_far, int far_stride,
                                                                int* __restrict__ out) {
    __shared__ int scx[MT_LDS_CENTERS], scy[MT_LDS_CENTERS];
    __shared__ unsigned long long vmin[3];
    __shared__ int imin[3];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int ng = min(max(g_count[n], 0), max_dots), nc = min(max(c_count[n], 0), cap);
    const int* drow = dots + (long)n * max_dots * 2;
    const int* crow = centers + (long)n * cap * 2;
    unsigned char* far = taken_far + (long)n * far_stride;     // flags of the centres MT_REG_CENTERS, ... (owner thread only)
    for (int c = tid; c < nc; c += 256) {
        if (c < MT_LDS_CENTERS) {
            scx[c] = crow[2 * c];
            scy[c] = crow[2 * c + 1];
        }
        if (c >= MT_REG_CENTERS) far[c - MT_REG_CENTERS] = 0;
    }
    if (tid < 3) {
        vmin[tid] = ~0ull;
        imin[tid] = MT_NONE;
    }
    __syncthreads();
    unsigned taken = 0;                                         // bit j: centre j * 256 + tid is matched
    const long long none = 0x7fffffffffffffffll;
    int tp = 0, p = 0;
    int lx = 0, ly = 0;                                         // dot (g & ~63) + lane
    for (int g = 0; g < ng; ++g) {
        if ((g & 63) == 0 && g + lane < ng) {
            lx = drow[2 * (g + lane)];
            ly = drow[2 * (g + lane) + 1];
        }
        const long long gx = __shfl(lx, g & 63, 64), gy = __shfl(ly, g & 63, 64);
        long long best = none;
        int bi = MT_NONE;
        for (int c = tid, j = 0; c < nc; c += 256, ++j) {
            if (c < MT_REG_CENTERS ? (taken >> j) & 1u : far[c - MT_REG_CENTERS] != 0) continue;
            const long long dx = (c < MT_LDS_CENTERS ? scx[c] : crow[2 * c]) - gx;
            const long long dy = (c < MT_LDS_CENTERS ? scy[c] : crow[2 * c + 1]) - gy;
            const long long d2 = dx * dx + dy * dy;             // |coordinates| < 2^29: no overflow
            if (d2 < best) {                                    // c ascends: the first of equal distances stays
                best = d2;
                bi = c;
            }
        }
        const int q = p == 2 ? 0 : p + 1;
        if (tid == 0) {                                         // the next dot's slot: last read two dots ago
            vmin[q] = ~0ull;
            imin[q] = MT_NONE;
        }
        if (bi != MT_NONE && best <= d2_max) atomicMin(&vmin[p], (unsigned long long)best);
        __syncthreads();
        const unsigned long long top = vmin[p];
        if (top == ~0ull) {                                     // no free centre within reach (workgroup-uniform)
            p = q;
            continue;
        }
        if (bi != MT_NONE && (unsigned long long)best == top) atomicMin(&imin[p], bi);
        __syncthreads();
        const int hit = imin[p];
        ++tp;
        if (hit < nc && (hit & 255) == tid) {
            if (hit < MT_REG_CENTERS) taken |= 1u << (hit >> 8);
            else far[hit - MT_REG_CENTERS] = 1;
        }
        p = q;
    }
    if (tid == 0) {
        out[3 * n] = tp;
        out[3 * n + 1] = nc;
        out[3 * n + 2] = ng;
    }
}

// grid (64, N): cell (blockIdx.x / 8, blockIdx.x % 8) of image blockIdx.y, cs = size / 8 pixels on a side, clipped to the image
template <typename T, typename ACC>
__global__ __launch_bounds__(256) void mt_grid_sums_kernel(const T* __restrict__ map, int H, int W, int cs, ACC* __restrict__ out) {
    __shared__ ACC part[256];
    const T* img = map + (long)blockIdx.y * H * W;
    const long y0 = (long)(blockIdx.x >> 3) * cs, x0 = (long)(blockIdx.x & 7) * cs;
    const int h = y0 >= H ? 0 : (int)(y0 + cs <= H ? cs : H - y0), w = x0 >= W ? 0 : (int)(x0 + cs <= W ? cs : W - x0);
    ACC s = 0;
    for (long i = threadIdx.x; i < (long)h * w; i += 256) {
        const long y = i / w, x = i - y * w;
        s += (ACC)img[(y0 + y) * W + x0 + x];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(long)blockIdx.y * 64 + blockIdx.x] = part[0];
}

__global__ __launch_bounds__(256) void mt_scatter_kernel(const int* __restrict__ centers, const int* __restrict__ c_count, int cap,
                                                         unsigned char* __restrict__ map, int N, int H, int W) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)N * cap) return;
    const int n = (int)(t / cap), c = (int)(t - (long)n * cap);
    if (c >= c_count[n]) return;
    const int x = centers[2 * t], y = centers[2 * t + 1];
    if (x < 0 || x >= W || y < 0 || y >= H) return;
    map[((long)n * H + y) * W + x] = 1;
}

// grid (cdiv(HW, 256), K - 1, N)
__global__ __launch_bounds__(256) void mt_split_classes_kernel(const unsigned char* __restrict__ map, unsigned char* __restrict__ planes,
                                                               int HW) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const int c = blockIdx.y + 1;
    planes[((long)blockIdx.z * gridDim.y + blockIdx.y) * HW + i] = map[(long)blockIdx.z * HW + i] == c;
}

// grid (K - 1, N): class blockIdx.x + 1 of image blockIdx.y.  centers was zeroed by the launch function.
__global__ __launch_bounds__(256) void mt_class_centers_kernel(const int* __restrict__ counts, const unsigned char* __restrict__ label_class,
                                                               const int* __restrict__ area, const long long* __restrict__ sum_y,
                                                               const long long* __restrict__ sum_x, int* __restrict__ centers,
                                                               int* __restrict__ c_count, int cap) {
    __shared__ int wcnt[4];
    const int n = blockIdx.y, c = blockIdx.x + 1, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nl = min(max(counts[n], 0), cap);
    const long row = (long)n * cap;
    int* out = centers + ((long)n * gridDim.x + blockIdx.x) * cap * 2;
    int run = 0;                                                 // workgroup-uniform
    for (int i0 = 0; i0 < nl; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const bool f = i < nl && label_class[row + i] == c;
        const unsigned long long b = __ballot(f);
        if (lane == 0) wcnt[wv] = __popcll(b);
        __syncthreads();
        int pre = 0;
        for (int j = 0; j < wv; ++j) pre += wcnt[j];
        const int tot = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (f) {
            const int pos = run + pre + __popcll(b & ((1ull << lane) - 1ull));      // < nl <= cap
            const int a = area[row + i];
            int x = 0, y = 0;
            if (a > 0 && sum_x[row + i] >= 0 && sum_y[row + i] >= 0) {
                x = mt_round_div(sum_x[row + i], a);
                y = mt_round_div(sum_y[row + i], a);
            }
            out[2 * pos] = x;
            out[2 * pos + 1] = y;
        }
        run += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) c_count[(long)n * gridDim.x + blockIdx.x] = run;
}

struct DotPlan {
    int hw, nblk;
    size_t total;
};
int dot_plan(int N, int H, int W, DotPlan* pl) {
    if (N <= 0 || H <= 0 || W <= 0) return UMI_ERR_BADARG;
    if (H > 65536 || W > 65536 || (long)N * H * W >= (1L << 31) || N > 65535) return UMI_ERR_UNSUPPORTED;
    pl->hw = H * W;
    pl->nblk = (pl->hw + MT_BLK - 1) / MT_BLK;
    pl->total = MT_HEAD + (((size_t)N * pl->nblk * sizeof(int) + 255) & ~(size_t)255);
    return UMI_OK;
}

size_t far_stride(int cap) { return cap > MT_REG_CENTERS ? (((size_t)(cap - MT_REG_CENTERS) + 255) & ~(size_t)255) : 0; }

}  // namespace

extern "C" int umi_match_max_dots(void) { return MT_MAX_DOTS; }

extern "C" size_t umi_dot_lists_ws_bytes(int N, int H, int W) {
    DotPlan pl;
    return dot_plan(N, H, W, &pl) == UMI_OK ? pl.total : 0;
}

extern "C" int umi_dot_lists(const void* map, int dtype, int* dots, int* g_count, int N, int H, int W, int max_dots, void* ws,
                             size_t ws_bytes, umi_stream_t stream) {
    if (!map || !dots || !g_count || (dtype != 0 && dtype != 1) || max_dots <= 0) return UMI_ERR_BADARG;
    DotPlan pl;
    const int st = dot_plan(N, H, W, &pl);
    if (st != UMI_OK) return st;
    if (max_dots > MT_MAX_DOTS) return UMI_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < pl.total) return UMI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int* err = (int*)ws;
    int* blk = (int*)((char*)ws + MT_HEAD);
    const hipError_t e = hipMemsetAsync(err, 0, MT_HEAD, s);
    if (e != hipSuccess) return (int)e;
    const dim3 grid(pl.nblk, N);
    if (dtype == 0) hipLaunchKernelGGL(mt_dot_count_kernel<unsigned char>, grid, dim3(256), 0, s, (const unsigned char*)map, pl.hw, pl.nblk, blk);
    else hipLaunchKernelGGL(mt_dot_count_kernel<float>, grid, dim3(256), 0, s, (const float*)map, pl.hw, pl.nblk, blk);
    hipLaunchKernelGGL(mt_dot_scan_kernel, dim3(N), dim3(256), 0, s, blk, pl.nblk, max_dots, g_count, err);
    if (dtype == 0)
        hipLaunchKernelGGL(mt_dot_write_kernel<unsigned char>, grid, dim3(256), 0, s, (const unsigned char*)map, pl.hw, W, pl.nblk, blk,
                           max_dots, dots);
    else hipLaunchKernelGGL(mt_dot_write_kernel<float>, grid, dim3(256), 0, s, (const float*)map, pl.hw, W, pl.nblk, blk, max_dots, dots);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_component_centers(const int* counts, const int* area, const long long* sum_y, const long long* sum_x, int* centers,
                                     int N, int cap, umi_stream_t stream) {
    if (!counts || !area || !sum_y || !sum_x || !centers || N <= 0 || cap <= 0) return UMI_ERR_BADARG;
    if ((long)N * cap >= (1L << 30)) return UMI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mt_centers_kernel, dim3(umi_cdiv((long)N * cap, 256)), dim3(256), 0, (hipStream_t)stream, counts, area, sum_y,
                       sum_x, centers, N, cap);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_crowd_match(const int* dots, const int* g_count, int max_dots, const int* centers, const int* c_count, int cap,
                               const double* tables, size_t table_len, const int* radii, int S, const double* thresh, int T, int* out,
                               int N, umi_stream_t stream) {
    if (!dots || !g_count || !centers || !c_count || !tables || !radii || !thresh || !out || N <= 0 || S <= 0 || T <= 0 ||
        max_dots <= 0 || cap <= 0)
        return UMI_ERR_BADARG;
    if (max_dots > MT_MAX_DOTS || S > MT_MAX_SIGMAS || N > 65535 || T > 65535) return UMI_ERR_UNSUPPORTED;
    MtSigmas sg = {};
    size_t off = 0;
    for (int s = 0; s < S; ++s) {
        if (radii[s] < 0 || radii[s] > 16383) return UMI_ERR_BADARG;
        sg.r[s] = radii[s];
        sg.off[s] = (int)off;
        off += (size_t)(2 * radii[s] + 1) * (2 * radii[s] + 1);
        if (off >= (1u << 30)) return UMI_ERR_UNSUPPORTED;
    }
    if (table_len < off) return UMI_ERR_BADARG;
    hipLaunchKernelGGL(mt_crowd_match_kernel, dim3(T, S, N), dim3(256), 0, (hipStream_t)stream, dots, g_count, max_dots, centers, c_count,
                       cap, tables, sg, thresh, out);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" size_t umi_distance_match_ws_bytes(int N, int cap) {
    if (N <= 0 || cap <= 0) return 0;
    return MT_HEAD + (size_t)N * far_stride(cap);
}

extern "C" int umi_distance_match(const int* dots, const int* g_count, int max_dots, const int* centers, const int* c_count, int cap,
                                  long long d2_max, int* out, int N, void* ws, size_t ws_bytes, umi_stream_t stream) {
    if (!dots || !g_count || !centers || !c_count || !out || N <= 0 || max_dots <= 0 || cap <= 0) return UMI_ERR_BADARG;
    if (!ws || ws_bytes < umi_distance_match_ws_bytes(N, cap)) return UMI_ERR_WORKSPACE;
    hipLaunchKernelGGL(mt_distance_match_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, dots, g_count, max_dots, centers, c_count,
                       cap, d2_max, (unsigned char*)ws + MT_HEAD, (int)far_stride(cap), out);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_grid_sums(const void* map, int dtype, void* out, int N, int H, int W, int size, umi_stream_t stream) {
    if (!map || !out || (dtype != 0 && dtype != 1) || N <= 0 || H <= 0 || W <= 0 || size <= 0 || size % 8) return UMI_ERR_BADARG;
    if ((long)N * H * W >= (1L << 31) || N > 65535) return UMI_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == 0)
        hipLaunchKernelGGL((mt_grid_sums_kernel<unsigned char, long long>), dim3(64, N), dim3(256), 0, s, (const unsigned char*)map, H, W,
                           size / 8, (long long*)out);
    else
        hipLaunchKernelGGL((mt_grid_sums_kernel<float, double>), dim3(64, N), dim3(256), 0, s, (const float*)map, H, W, size / 8,
                           (double*)out);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_scatter_centers(const int* centers, const int* c_count, int cap, unsigned char* map, int N, int H, int W,
                                   umi_stream_t stream) {
    if (!centers || !c_count || !map || N <= 0 || H <= 0 || W <= 0 || cap <= 0) return UMI_ERR_BADARG;
    if ((long)N * H * W >= (1L << 31) || (long)N * cap >= (1L << 30)) return UMI_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(map, 0, (size_t)N * H * W, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mt_scatter_kernel, dim3(umi_cdiv((long)N * cap, 256)), dim3(256), 0, s, centers, c_count, cap, map, N, H, W);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_split_classes(const unsigned char* map, unsigned char* planes, int N, int H, int W, int n_classes, umi_stream_t stream) {
    if (!map || !planes || N <= 0 || H <= 0 || W <= 0 || n_classes < 2) return UMI_ERR_BADARG;
    if (n_classes > 256 || (long)N * (n_classes - 1) * H * W >= (1L << 31) || N > 65535) return UMI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mt_split_classes_kernel, dim3(umi_cdiv((long)H * W, 256), n_classes - 1, N), dim3(256), 0, (hipStream_t)stream, map,
                       planes, H * W);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_class_center_lists(const int* counts, const unsigned char* label_class, const int* area, const long long* sum_y,
                                      const long long* sum_x, int* centers, int* c_count, int N, int cap, int n_classes,
                                      umi_stream_t stream) {
    if (!counts || !label_class || !area || !sum_y || !sum_x || !centers || !c_count || N <= 0 || cap <= 0 || n_classes < 2)
        return UMI_ERR_BADARG;
    if (n_classes > 256 || (long)N * (n_classes - 1) * cap >= (1L << 30) || N > 65535) return UMI_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(centers, 0, (size_t)N * (n_classes - 1) * cap * 2 * sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mt_class_centers_kernel, dim3(n_classes - 1, N), dim3(256), 0, s, counts, label_class, area, sum_y, sum_x, centers,
                       c_count, cap);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
