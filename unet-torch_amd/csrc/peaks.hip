// Density-map evaluation on the device: the head output -> count map (umi_density_maps) and the local maxima of a count map
// (umi_peak_lists), the project's restatement of skimage.feature.peak_local_max(map, min_distance=d) after map[map < floor] = 0
// (reference test_mc3serousv5.py test_single_reg, CrowdMatching.py inputType='Regression').  Rule and NumPy statement:
// umi/peaks.py; the C contract: include/unetmi.h.
//
//   density      pred = max(x, 0) / scale, a true division (the build passes no fast-math flag, so `/` is the correctly rounded
//                v_div sequence, not a multiplication by a reciprocal).  Per 4096-pixel block 256 strided float64 partial sums and
//                a fixed tree, then one workgroup per image over the block sums the same way: a fixed order, no atomics.  The
//                minimum (a NaN counted as 0) rides along.  Without an output map the same two launches sum a map as it is.
//   peak lists   four launches, one status byte per pixel in the workspace (0 no candidate, 1 kept, 2 candidate not decided yet,
//                3 rejected):
//     minimum    a = x >= floor ? x : 0 is >= 0, so its bit pattern orders like its value: one integer atomicMin per block.
//                Skipped when the caller passes umi_density_maps' minimum.
//     candidates PK_TW x PK_TH = 64 x 16 pixel tiles with a d-pixel halo in LDS (outside the image: -1, below every a); the row
//                maximum over 2d+1 columns, then the column maximum over 2d+1 rows; candidate = (a == m, a > min, inside the border).
//     contested  the candidate bytes of a tile with a (d-1)-pixel halo; a candidate with another candidate in its (2d-1)^2
//                neighbourhood becomes 2 (in place: a neighbouring tile that reads the byte meanwhile sees 1 or 2, a candidate
//                either way).  Not launched for d = 1.
//     lists      one workgroup of 1024 threads per image.  It scans the status bytes sixteen at a time, lists the contested
//                pixels, and runs the spacing rule on them as a fixed point: a contested candidate is REJECTED once an earlier
//                (raster order) candidate within Chebyshev distance d - 1 is kept, and KEPT once all of them are rejected.  Both
//                decisions are final when taken, so reading a neighbour's byte before or after its owner rewrote it in the same
//                round gives the same fixed point.  TERMINATION: in every round the earliest undecided entry of the list has only
//                decided earlier neighbours and decides, so after at most `entries` rounds nothing is undecided; the loop is
//                `for (round < entries)` and cannot run longer whatever the bytes hold.  (With more contested pixels than the
//                list holds, PK_CCAP, the loop is skipped, they all stay 2 and are never listed, and the call sets
//                UMI_PEAKS_FAULT_CONTESTED.)  On a full plateau the depth is about W + d * H rounds, two barriers each.
//                Then the kept pixels become 64-bit keys (~value bits << 32 | raster index: ascending key = descending value,
//                raster order among equal values; a kept value is > 0, so its bits order like its value), are collected in LDS
//                with an LDS atomic counter and sorted there (bitonic, 8192 keys of 8 bytes), so the list does not depend on the
//                order of collection.  With more than max_peaks kept pixels the max_peaks-th smallest key is found first, bit by
//                bit from the top with one counting scan per bit (56 scans: the fault path), and only keys up to it are collected.
//                No address is formed from a map value: indices come from the scan position and are < H * W.
#include "common.h"

namespace {

constexpr int PK_TW = 64, PK_TH = 16;   // pixel tile of the candidate and contested passes
constexpr int PK_DMAX = 8;              // largest min_distance
constexpr int PK_HEAD = 256;            // bytes in front of the workspace; the first int32 is the fault word
constexpr int PK_MAX_PEAKS = 8192;
constexpr int PK_CCAP = 131072;         // contested entries per image
constexpr int PK_BLK = 4096;            // pixels per block of the streaming passes
constexpr int PK_LT = 1024;             // threads of the list kernel

// ---- density ---------------------------------------------------------------------------------------------------------------
template <bool MAP>
__global__ __launch_bounds__(256) void pk_density_kernel(const float* __restrict__ x, float* __restrict__ pred, int HW, int nblk, float scale,
                                                         double* __restrict__ psum, float* __restrict__ pmin) {
    __shared__ double ssum[256];
    __shared__ float smin[256];
    const long base = (long)blockIdx.y * HW;
    double s = 0.0;
    float mn = __builtin_inff();
    for (int k = 0; k < PK_BLK / 256; ++k) {
        const int i = blockIdx.x * PK_BLK + k * 256 + threadIdx.x;
        if (i < HW) {
            const float v = x[base + i];
            float p = v;
            if (MAP) {
                p = (v != v ? v : fmaxf(v, 0.f)) / scale;               // NaN stays NaN, as torch.relu leaves it
                pred[base + i] = p;
            }
            s += (double)p;
            mn = fminf(mn, p != p ? 0.f : p);
        }
    }
    ssum[threadIdx.x] = s;
    smin[threadIdx.x] = mn;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            ssum[threadIdx.x] += ssum[threadIdx.x + o];
            smin[threadIdx.x] = fminf(smin[threadIdx.x], smin[threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        psum[(long)blockIdx.y * nblk + blockIdx.x] = ssum[0];
        pmin[(long)blockIdx.y * nblk + blockIdx.x] = smin[0];
    }
}

__global__ __launch_bounds__(256) void pk_density_final_kernel(const double* __restrict__ psum, const float* __restrict__ pmin, int nblk,
                                                               double* __restrict__ counts, float* __restrict__ vmin) {
    __shared__ double ssum[256];
    __shared__ float smin[256];
    const double* ps = psum + (long)blockIdx.x * nblk;
    const float* pm = pmin + (long)blockIdx.x * nblk;
    double s = 0.0;
    float mn = __builtin_inff();
    for (int b = threadIdx.x; b < nblk; b += 256) {
        s += ps[b];
        mn = fminf(mn, pm[b]);
    }
    ssum[threadIdx.x] = s;
    smin[threadIdx.x] = mn;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            ssum[threadIdx.x] += ssum[threadIdx.x + o];
            smin[threadIdx.x] = fminf(smin[threadIdx.x], smin[threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = ssum[0];
        if (vmin) vmin[blockIdx.x] = smin[0];
    }
}

// ---- peak lists ------------------------------------------------------------------------------------------------------------
// the floored value: >= 0 (+0 for everything below the floor, NaN included), possibly +inf
__device__ __forceinline__ float pk_floor(float v, float fl) {
    const float a = v >= fl ? v : 0.f;
    return a == 0.f ? 0.f : a;                                  // -0 (floor = 0) -> +0: the bit pattern must order like the value
}

// grid (cdiv(HW, PK_BLK), N); amin[n] was preset to 0xFFFFFFFF
__global__ __launch_bounds__(256) void pk_min_kernel(const float* __restrict__ maps, int HW, float fl, unsigned* __restrict__ amin) {
    __shared__ unsigned smin[256];
    const float* img = maps + (long)blockIdx.y * HW;
    unsigned mn = 0xFFFFFFFFu;
    for (int k = 0; k < PK_BLK / 256; ++k) {
        const int i = blockIdx.x * PK_BLK + k * 256 + threadIdx.x;
        if (i < HW) mn = min(mn, __float_as_uint(pk_floor(img[i], fl)));
    }
    smin[threadIdx.x] = mn;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) smin[threadIdx.x] = min(smin[threadIdx.x], smin[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMin(&amin[blockIdx.y], smin[0]);
}

// grid (cdiv(W, PK_TW), cdiv(H, PK_TH), N)
__global__ __launch_bounds__(256) void pk_cand_kernel(const float* __restrict__ maps, const float* __restrict__ vmin,
                                                      const unsigned* __restrict__ amin_bits, unsigned char* __restrict__ status,
                                                      long stride, int H, int W, int d, float fl) {
    __shared__ float sa[PK_TH + 2 * PK_DMAX][PK_TW + 2 * PK_DMAX + 1];
    __shared__ float sr[PK_TH + 2 * PK_DMAX][PK_TW];
    const int n = blockIdx.z, x0 = blockIdx.x * PK_TW, y0 = blockIdx.y * PK_TH, tid = threadIdx.x;
    const float* img = maps + (long)n * H * W;
    const int rows = PK_TH + 2 * d, cols = PK_TW + 2 * d;     // d <= PK_DMAX: inside sa
    for (int i = tid; i < rows * cols; i += 256) {
        const int r = i / cols, c = i - r * cols, y = y0 - d + r, x = x0 - d + c;
        float a = -1.f;                                         // outside the image: below every floored value
        if (y >= 0 && y < H && x >= 0 && x < W) a = pk_floor(img[(long)y * W + x], fl);
        sa[r][c] = a;
    }
    __syncthreads();
    for (int i = tid; i < rows * PK_TW; i += 256) {
        const int r = i / PK_TW, c = i - r * PK_TW;
        float m = sa[r][c];
        for (int k = 1; k <= 2 * d; ++k) m = fmaxf(m, sa[r][c + k]);
        sr[r][c] = m;
    }
    __syncthreads();
    float amin;
    if (vmin) {
        const float v = vmin[n];
        amin = v >= fl ? v : 0.f;                               // floor >= 0: one pixel below it makes the minimum 0
    } else {
        amin = __uint_as_float(amin_bits[n]);
    }
    unsigned char* st = status + (long)n * stride;
    for (int i = tid; i < PK_TH * PK_TW; i += 256) {
        const int r = i / PK_TW, c = i - r * PK_TW, y = y0 + r, x = x0 + c;
        if (y >= H || x >= W) continue;
        float m = sr[r][c];
        for (int k = 1; k <= 2 * d; ++k) m = fmaxf(m, sr[r + k][c]);
        const float a = sa[r + d][c + d];
        st[(long)y * W + x] = a == m && a > amin && y >= d && y < H - d && x >= d && x < W - d;
    }
}

// grid as above; d >= 2
__global__ __launch_bounds__(256) void pk_contest_kernel(unsigned char* __restrict__ status, long stride, int H, int W, int d) {
    __shared__ unsigned char sc[PK_TH + 2 * (PK_DMAX - 1)][PK_TW + 2 * (PK_DMAX - 1) + 2];
    const int n = blockIdx.z, x0 = blockIdx.x * PK_TW, y0 = blockIdx.y * PK_TH, tid = threadIdx.x, h = d - 1;
    unsigned char* st = status + (long)n * stride;
    const int rows = PK_TH + 2 * h, cols = PK_TW + 2 * h;
    for (int i = tid; i < rows * cols; i += 256) {
        const int r = i / cols, c = i - r * cols, y = y0 - h + r, x = x0 - h + c;
        sc[r][c] = y >= 0 && y < H && x >= 0 && x < W && st[(long)y * W + x] != 0;
    }
    __syncthreads();
    for (int i = tid; i < PK_TH * PK_TW; i += 256) {
        const int r = i / PK_TW, c = i - r * PK_TW, y = y0 + r, x = x0 + c;
        if (y >= H || x >= W || !sc[r + h][c + h]) continue;
        int cnt = 0;
        for (int dy = 0; dy <= 2 * h; ++dy)
            for (int dx = 0; dx <= 2 * h; ++dx) cnt += sc[r + dy][c + dx];
        if (cnt > 1) st[(long)y * W + x] = 2;
    }
}

// f(raster index, status) for every non-zero status byte of the image, sixteen bytes per load (the row of bytes is 16-byte aligned
// and padded to a multiple of 16; the padding is never interpreted)
template <typename F>
__device__ __forceinline__ void pk_scan(const unsigned char* st, int HW, F f) {
    const uint4* w = (const uint4*)st;
    const int nw = (HW + 15) >> 4;
    for (int i = threadIdx.x; i < nw; i += PK_LT) {
        const uint4 v = w[i];
        const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!u[j]) continue;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned s = (u[j] >> (8 * b)) & 255u;
                const int idx = i * 16 + j * 4 + b;
                if (s && idx < HW) f(idx, s);
            }
        }
    }
}

__device__ __forceinline__ unsigned long long pk_key(const float* img, int idx) {
    return (unsigned long long)(~__float_as_uint(img[idx])) << 32 | (unsigned)idx;
}

// 1 keep, 3 reject, 2 not yet: the earlier candidates within Chebyshev distance h of pixel p
__device__ __forceinline__ int pk_decide(const volatile unsigned char* st, int p, int H, int W, int h) {
    const int py = p / W, px = p - py * W;
    bool pending = false;
    for (int y = max(py - h, 0); y <= py; ++y) {
        const int xe = y == py ? px - 1 : min(px + h, W - 1);
        for (int x = max(px - h, 0); x <= xe; ++x) {
            const unsigned s = st[y * W + x];
            if (s == 1) return 3;
            pending |= s == 2;
        }
    }
    return pending ? 2 : 1;
}

// grid (N), PK_LT threads
__global__ __launch_bounds__(PK_LT) void pk_list_kernel(const float* __restrict__ maps, unsigned char* status, long stride,
                                                        int* __restrict__ clist, int H, int W, int d, int max_peaks,
                                                        int* __restrict__ peaks, int* __restrict__ p_count, int* err) {
    __shared__ unsigned long long sk[PK_MAX_PEAKS];
    __shared__ int s_kept, s_cont, s_cnt, s_out, s_stamp;
    const int n = blockIdx.x, tid = threadIdx.x, HW = H * W;
    const float* img = maps + (long)n * HW;
    unsigned char* st = status + (long)n * stride;
    int* cl = clist + (long)n * PK_CCAP;
    if (tid == 0) {
        s_kept = 0;
        s_cont = 0;
        s_out = 0;
        s_stamp = 0;
    }
    __syncthreads();
    // 1. the uncontested peaks are counted, the contested candidates listed
    {
        int kept = 0;
        pk_scan(st, HW, [&](int idx, unsigned s) {
            if (s == 1) {
                ++kept;
            } else if (s == 2) {
                const int slot = atomicAdd(&s_cont, 1);
                if (slot < PK_CCAP) cl[slot] = idx;
            }
        });
        if (kept) atomicAdd(&s_kept, kept);
    }
    __syncthreads();
    // a list that overflowed is not walked at all: its entries could wait for ever for one that is not in it
    const int ncont = s_cont, nc = ncont > PK_CCAP ? 0 : ncont;
    int fault = ncont > PK_CCAP ? UMI_PEAKS_FAULT_CONTESTED : 0;
    // 2. the spacing rule as a fixed point; at most nc rounds (file header)
    for (int round = 0; round < nc; ++round) {
        bool pending = false;
        int kept = 0;
        for (int e = tid; e < nc; e += PK_LT) {
            const int p = cl[e];
            if (p < 0 || p >= HW || ((const volatile unsigned char*)st)[p] != 2) continue;
            const int dec = pk_decide(st, p, H, W, d - 1);
            if (dec == 2) {
                pending = true;
            } else {
                ((volatile unsigned char*)st)[p] = (unsigned char)dec;
                kept += dec == 1;
            }
        }
        if (kept) atomicAdd(&s_kept, kept);
        if (pending) s_stamp = round + 1;
        __syncthreads();
        const bool more = s_stamp == round + 1;
        __syncthreads();
        if (!more) break;                                       // workgroup-uniform
    }
    const int total = s_kept;
    // 3. more than max_peaks: the max_peaks-th smallest key, bit by bit
    unsigned long long limit = ~0ull;
    if (total > max_peaks) {
        fault |= UMI_PEAKS_FAULT_OVERFLOW;
        limit = 0ull;
        for (int b = 63; b >= 0; --b) {
            if (b < 32 && b >= 24) continue;                    // raster indices are < 2^24: these bits are 0 in every key
            const unsigned long long trial = limit | ((1ull << b) - 1ull);
            if (tid == 0) s_cnt = 0;
            __syncthreads();
            int c = 0;
            pk_scan(st, HW, [&](int idx, unsigned s) { c += s == 1 && pk_key(img, idx) <= trial; });
            if (c) atomicAdd(&s_cnt, c);
            __syncthreads();
            if (s_cnt < max_peaks) limit |= 1ull << b;          // workgroup-uniform
            __syncthreads();
        }
    }
    // 4. collect, sort, write
    pk_scan(st, HW, [&](int idx, unsigned s) {
        if (s != 1) return;
        const unsigned long long k = pk_key(img, idx);
        if (k > limit) return;
        const int slot = atomicAdd(&s_out, 1);
        if (slot < PK_MAX_PEAKS) sk[slot] = k;
    });
    __syncthreads();
    const int cnt = min(min(s_out, max_peaks), PK_MAX_PEAKS);
    int n2 = 2;
    while (n2 < cnt) n2 <<= 1;                                  // <= PK_MAX_PEAKS
    for (int i = cnt + tid; i < n2; i += PK_LT) sk[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += PK_LT) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = sk[i], b = sk[l];
                    if ((a > b) == ((i & k) == 0)) {
                        sk[i] = b;
                        sk[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    int* row = peaks + (long)n * max_peaks * 2;
    for (int i = tid; i < max_peaks; i += PK_LT) {
        int x = 0, y = 0;
        if (i < cnt) {
            const int idx = (int)(unsigned)(sk[i] & 0xFFFFFFFFull);
            y = idx / W;
            x = idx - y * W;
        }
        row[2 * i] = x;
        row[2 * i + 1] = y;
    }
    if (tid == 0) {
        p_count[n] = cnt;
        if (fault) atomicOr(err, fault);
    }
}

struct PeakPlan {
    int hw, nblk;
    long stride;
    size_t off_min, off_status, off_clist, total;
};
int peak_plan(int N, int H, int W, PeakPlan* pl) {
    if (N <= 0 || H <= 0 || W <= 0) return UMI_ERR_BADARG;
    if (H > 4096 || W > 4096 || N > 65535 || (long)N * H * W >= (1L << 31)) return UMI_ERR_UNSUPPORTED;
    pl->hw = H * W;
    pl->nblk = (pl->hw + PK_BLK - 1) / PK_BLK;
    pl->stride = ((long)pl->hw + 15) & ~15L;
    pl->off_min = PK_HEAD;
    pl->off_status = pl->off_min + (((size_t)N * sizeof(unsigned) + 255) & ~(size_t)255);
    pl->off_clist = pl->off_status + (((size_t)N * pl->stride + 255) & ~(size_t)255);
    pl->total = pl->off_clist + (size_t)N * PK_CCAP * sizeof(int);
    return UMI_OK;
}

}  // namespace

extern "C" int umi_peaks_max(void) { return PK_MAX_PEAKS; }

extern "C" size_t umi_density_maps_ws_bytes(int N, int H, int W) {
    PeakPlan pl;
    if (peak_plan(N, H, W, &pl) != UMI_OK) return 0;
    return (size_t)N * pl.nblk * (sizeof(double) + sizeof(float)) + 256;
}

extern "C" int umi_density_maps(const float* x, float* pred, double* counts, float* vmin, int N, int H, int W, float scale, void* ws,
                                size_t ws_bytes, umi_stream_t stream) {
    if (!x || !counts || !(scale > 0.f) || scale == __builtin_inff()) return UMI_ERR_BADARG;
    PeakPlan pl;
    const int st = peak_plan(N, H, W, &pl);
    if (st != UMI_OK) return st;
    if (!ws || ws_bytes < umi_density_maps_ws_bytes(N, H, W) || ((uintptr_t)ws & 7)) return UMI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double* psum = (double*)ws;
    float* pmin = (float*)(psum + (size_t)N * pl.nblk);
    if (pred) hipLaunchKernelGGL(pk_density_kernel<true>, dim3(pl.nblk, N), dim3(256), 0, s, x, pred, pl.hw, pl.nblk, scale, psum, pmin);
    else hipLaunchKernelGGL(pk_density_kernel<false>, dim3(pl.nblk, N), dim3(256), 0, s, x, pred, pl.hw, pl.nblk, scale, psum, pmin);
    hipLaunchKernelGGL(pk_density_final_kernel, dim3(N), dim3(256), 0, s, psum, pmin, pl.nblk, counts, vmin);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" size_t umi_peak_lists_ws_bytes(int N, int H, int W) {
    PeakPlan pl;
    return peak_plan(N, H, W, &pl) == UMI_OK ? pl.total : 0;
}

extern "C" int umi_peak_lists(const float* maps, const float* vmin, int* peaks, int* p_count, int N, int H, int W, int min_distance,
                              float floor, int max_peaks, void* ws, size_t ws_bytes, umi_stream_t stream) {
    if (!maps || !peaks || !p_count || max_peaks <= 0 || min_distance < 1 || !(floor >= 0.f) || floor == __builtin_inff())
        return UMI_ERR_BADARG;
    PeakPlan pl;
    const int st = peak_plan(N, H, W, &pl);
    if (st != UMI_OK) return st;
    if (min_distance > PK_DMAX || max_peaks > PK_MAX_PEAKS) return UMI_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < pl.total || ((uintptr_t)ws & 15)) return UMI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int* err = (int*)ws;
    unsigned* amin = (unsigned*)((char*)ws + pl.off_min);
    unsigned char* status = (unsigned char*)ws + pl.off_status;
    int* clist = (int*)((char*)ws + pl.off_clist);
    hipError_t e = hipMemsetAsync(err, 0, PK_HEAD, s);
    if (e != hipSuccess) return (int)e;
    if (!vmin) {
        e = hipMemsetAsync(amin, 0xFF, (size_t)N * sizeof(unsigned), s);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(pk_min_kernel, dim3(pl.nblk, N), dim3(256), 0, s, maps, pl.hw, floor, amin);
    }
    const dim3 grid(umi_cdiv(W, PK_TW), umi_cdiv(H, PK_TH), N);
    hipLaunchKernelGGL(pk_cand_kernel, grid, dim3(256), 0, s, maps, vmin, amin, status, pl.stride, H, W, min_distance, floor);
    if (min_distance > 1) hipLaunchKernelGGL(pk_contest_kernel, grid, dim3(256), 0, s, status, pl.stride, H, W, min_distance);
    hipLaunchKernelGGL(pk_list_kernel, dim3(N), dim3(PK_LT), 0, s, maps, status, pl.stride, clist, H, W, min_distance, max_peaks, peaks,
                       p_count, err);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
