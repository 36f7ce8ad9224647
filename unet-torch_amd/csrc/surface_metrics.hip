// Surface-distance metrics of hard masks: Hausdorff distance, its 95th percentile and the average symmetric surface distance
// per (image, class), unit pixel spacing (statement: umi/surface.py surface_numpy, surface_scores_numpy).
//
//   A = (pred_mask == c), G = (label is class c); surface(M) = M & ~erode4(M), pixels outside the image count as 0; d2 of a
//   surface pixel of one side = exact integer squared Euclidean distance to the nearest surface pixel of the other side.
//
//   sd_col_kernel      per (image, class, side): 64-row chunk bitmasks of the class mask per column (62 columns + 2 halo columns
//                      per wave row), the surface bits from the four neighbours' bitmasks, and per pixel the distance to the
//                      nearest surface pixel of ITS OWN column (the separable transform's first pass, as hdt_col_kernel):
//                      tab = g | surface << 15 as 16 bits.  It also zeroes the histograms of its (image, class).
//   sd_row_kernel      one block per (image, class, row): both sides' table rows in LDS; every surface pixel searches the other
//                      side's row outward, stopping once k^2 >= best (exact, int32 for H, W <= 4096).  d2 goes to the row's compact
//                      list (slot order is arbitrary; only order-free integer work reads it) and into the level-1 histogram of
//                      d2 >> 12 (integer atomics; the leading key's count stays in registers and the four
//                      waves' runs are merged, so a row whose distances share a bin adds once).  Per row and side: the surface count, the maximum and the float64 sum of
//                      sqrt(d2) in a fixed order (thread t takes pixels t, t + 256, ...; a xor-shuffle tree; the waves in order).
//                      When either side is empty nothing is searched.
//   sd_select_kernel   ranks lo = floor((n - 1) * 0.95) and min(lo + 1, n - 1) of the union multiset: their level-1 bins from
//                      the histogram, then the level-2 histograms (d2 & 4095) of the keys in those bins.
//   sd_finalize_kernel one block per (image, class): counts, state, the fixed-order float64 sums over the rows (thread t takes
//                      rows t, t + 256, ...; a binary tree), the two order statistics, stats = {hd, hd95, assd, state}.
//                      Classes below c0 get zeros.
//   sd_scores_kernel   one thread per item: the float64 mean over (image, class) in that order, one rounding to fp32.
// Four launches (+ one for the scores), no allocation, nothing read back, no floating-point atomics: integer histograms are exact
// in any order, and every word of ws that is read was written by an earlier launch of the same call.
#include "common.h"

namespace {

constexpr int SD_MAX = 4096;              // H, W limit: column distances fit 15 bits, squared distances stay below 2^25
constexpr int SD_MAXK = 8;
constexpr unsigned SD_NONE = 0x7FFFu;     // "this column has no surface pixel of that side"
constexpr unsigned SD_SURF = 0x8000u;     // this pixel is a surface pixel of its side
constexpr int SD_INF = 0x3fffffff;        // squared-distance infinity; INF + (W-1)^2 stays below 2^31
constexpr int SD_COLS = 62;               // columns per block of the column pass (64 lanes - 2 halo lanes)
constexpr int SD_LOW = 12;                // key = d2 < 2^25: level 1 = d2 >> 12 (8192 bins), level 2 = d2 & 4095 (4096 bins, x 2 ranks)
constexpr int SD_BINS1 = 8192, SD_BINS2 = 4096;
constexpr int SD_HIST = SD_BINS1 + 2 * SD_BINS2;      // words per (image, class)
constexpr int SD_SEL_BLOCKS = 16;

__device__ __forceinline__ bool sd_is_class(const void* t, int tdtype, long i, int c) {
    if (tdtype == 0) return reinterpret_cast<const long long*>(t)[i] == (long long)c;
    if (tdtype == 1) return reinterpret_cast<const float*>(t)[i] == (float)c;          // NaN, 1.5: no class
    if (tdtype == 2) return (int)reinterpret_cast<const unsigned char*>(t)[i] == c;
    return reinterpret_cast<const int*>(t)[i] == c;
}

// distance from row r0 + i to the nearest set row: m = this chunk's bits, above / below = nearest set row outside the chunk (-1 none)
__device__ __forceinline__ unsigned sd_col_dist(unsigned long long m, int i, int r0, int above, int below) {
    const unsigned long long up = m & ((2ull << i) - 1ull);
    const unsigned long long dn = m >> i;
    const int a = up ? r0 + 63 - __clzll((long long)up) : above;
    const int b = dn ? r0 + i + __ffsll((long long)dn) - 1 : below;
    const int r = r0 + i;
    int d = SD_NONE;
    if (a >= 0) d = r - a;
    if (b >= 0) d = min(d, b - r);
    return (unsigned)d;
}

// hist[key] += 1 for every valid lane; call in wave-uniform control flow.  The lanes that share the first valid lane's key are
// counted by a ballot and added once (identical masks put a whole wave into one bin).
__device__ __forceinline__ void sd_hist_add(unsigned* hist, int key, bool valid) {
    const unsigned long long todo = __ballot(valid);
    if (!todo) return;
    const int first = __ffsll((long long)todo) - 1;
    const int k = __builtin_amdgcn_readlane(key, first);
    const unsigned long long same = __ballot(valid && key == k);
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist[k], (unsigned)__popcll(same));
    else if (valid && key != k) atomicAdd(&hist[key], 1u);
}

// The same inside a loop over one histogram: the count of the leading key stays in the wave-uniform pair `run` (scalar registers)
// until another key leads a round, so a row whose distances share a bin costs one atomic per wave, not one per round.
struct SdRun { int k; unsigned n; };
__device__ __forceinline__ void sd_run_add(unsigned* hist, SdRun& run, int key, bool valid) {
    const unsigned long long todo = __ballot(valid);
    if (!todo) return;
    const int first = __ffsll((long long)todo) - 1;
    const int k = __builtin_amdgcn_readlane(key, first);
    const unsigned long long same = __ballot(valid && key == k);
    if (k != run.k) {
        if ((threadIdx.x & 63) == 0 && run.n) atomicAdd(&hist[run.k], run.n);
        run.k = k;
        run.n = 0u;
    }
    run.n += (unsigned)__popcll(same);
    if (valid && key != k) atomicAdd(&hist[key], 1u);
}

// grid (ceil(W / 62), B * (K - c0), 2): blockIdx.z = 0 prediction, 1 label.  block = 64 lanes x nw waves; lane l holds column
// blockIdx.x * 62 + l - 1 (lanes 0 and 63 are halo columns: read, not written); wave v owns the 64-row chunks v, v + nw, ...
__global__ __launch_bounds__(1024) void sd_col_kernel(const unsigned char* __restrict__ pred, const void* __restrict__ target, int tdtype,
                                                      int K, int c0, int H, int W, unsigned short* __restrict__ tab,
                                                      unsigned* __restrict__ hist) {
    __shared__ unsigned long long s_m[64][64];                 // [chunk][lane]
    __shared__ short s_last[64][64], s_first[64][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int Ka = K - c0, bk = blockIdx.y, b = bk / Ka, c = c0 + bk % Ka, side = blockIdx.z;
    const int col = blockIdx.x * SD_COLS + lane - 1;
    {                                                          // the blocks of this (image, class) zero its histograms
        const int nb = 2 * gridDim.x, id = side * gridDim.x + blockIdx.x;
        unsigned* h = hist + (long)bk * SD_HIST;
        for (int i = id * blockDim.x + threadIdx.x; i < SD_HIST; i += nb * blockDim.x) h[i] = 0u;
    }
    const int nchunk = (H + 63) >> 6;
    const bool inimg = col >= 0 && col < W;
    const long img = (long)b * H * W;
    for (int j = 0; j < 4; ++j) {
        const int ch = wave + j * nw, r0 = ch * 64;
        if (ch >= nchunk) break;
        unsigned long long m = 0ull;
        if (inimg) {
            const int n = min(64, H - r0);
            for (int i = 0; i < n; ++i) {
                const long p = img + (long)(r0 + i) * W + col;
                const bool in = side == 0 ? (int)pred[p] == c : sd_is_class(target, tdtype, p, c);
                if (in) m |= 1ull << i;
            }
        }
        s_m[ch][lane] = m;
    }
    __syncthreads();
    unsigned long long sf[4] = {0ull, 0ull, 0ull, 0ull};
    for (int j = 0; j < 4; ++j) {
        const int ch = wave + j * nw, r0 = ch * 64;
        if (ch >= nchunk) break;
        const unsigned long long m = s_m[ch][lane];
        const unsigned long long prev = ch > 0 ? s_m[ch - 1][lane] : 0ull, next = ch + 1 < nchunk ? s_m[ch + 1][lane] : 0ull;
        const unsigned long long left = lane > 0 ? s_m[ch][lane - 1] : 0ull, right = lane < 63 ? s_m[ch][lane + 1] : 0ull;
        const unsigned long long up = (m << 1) | (prev >> 63), down = (m >> 1) | (next << 63);
        const unsigned long long s = m & ~(up & down & left & right);      // rows >= H and columns outside the image are 0 bits
        sf[j] = s;
        s_first[ch][lane] = s ? (short)(r0 + __ffsll((long long)s) - 1) : (short)-1;
        s_last[ch][lane] = s ? (short)(r0 + 63 - __clzll((long long)s)) : (short)-1;
    }
    __syncthreads();
    if (wave == 0) {       // chunk summaries -> "nearest surface row above the chunk" (s_last) and "below the chunk" (s_first)
        int l = -1;
        for (int ch = 0; ch < nchunk; ++ch) {
            const int t = s_last[ch][lane];
            s_last[ch][lane] = (short)l;
            if (t >= 0) l = t;
        }
        int f = -1;
        for (int ch = nchunk - 1; ch >= 0; --ch) {
            const int t = s_first[ch][lane];
            s_first[ch][lane] = (short)f;
            if (t >= 0) f = t;
        }
    }
    __syncthreads();
    if (lane == 0 || lane == 63 || col >= W) return;
    unsigned short* out = tab + ((long)side * gridDim.y + bk) * H * W + col;
    for (int j = 0; j < 4; ++j) {
        const int ch = wave + j * nw, r0 = ch * 64;
        if (ch >= nchunk) break;
        const int n = min(64, H - r0);
        const int above = s_last[ch][lane], below = s_first[ch][lane];
        for (int i = 0; i < n; ++i)
            out[(long)(r0 + i) * W] = (unsigned short)(sd_col_dist(sf[j], i, r0, above, below) | ((sf[j] >> i) & 1ull ? SD_SURF : 0u));
    }
}

// squared distance of column w to the nearest surface pixel of the side whose table row is t (that side is not empty)
__device__ __forceinline__ int sd_row_d2(const unsigned short* __restrict__ t, int w, int W) {
    auto g2 = [&](int x) {
        const int g = (int)(t[x] & SD_NONE);
        return g == (int)SD_NONE ? SD_INF : g * g;
    };
    int best = g2(w);
    for (int k = 1; k * k < best && (w - k >= 0 || w + k < W); ++k) {      // a column k away adds k^2
        if (w - k >= 0) best = min(best, g2(w - k) + k * k);
        if (w + k < W) best = min(best, g2(w + k) + k * k);
    }
    return best;
}

// grid (H, B * (K - c0)), block 256, dynamic LDS 2 * W * 2 bytes.  Per row: list [2][W] int32 (the first rowcnt entries of a side, when
// both sides are non-empty), rowcnt [2], rowsum [2], rowmax.
__global__ __launch_bounds__(256) void sd_row_kernel(const unsigned short* __restrict__ tab, int H, int W, int* __restrict__ list,
                                                     int* __restrict__ rowcnt, double* __restrict__ rowsum, int* __restrict__ rowmax,
                                                     unsigned* __restrict__ hist) {
    extern __shared__ unsigned short s_row[];                  // [2][W]
    __shared__ int s_flags, s_slot[2], s_cnt[2][4], s_max[4], s_runk[4];
    __shared__ unsigned s_runn[4];
    __shared__ double s_sum[2][4];
    const int h = blockIdx.x, bk = blockIdx.y, nbk = gridDim.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)bk * H + h;
    if (threadIdx.x == 0) { s_flags = 0; s_slot[0] = 0; s_slot[1] = 0; }
    __syncthreads();
    int flags = 0;
    for (int w = threadIdx.x; w < W; w += 256) {
        const unsigned short a = tab[row * W + w], g = tab[((long)nbk * H + row) * W + w];
        s_row[w] = a;
        s_row[W + w] = g;
        // a column with a finite distance holds a surface pixel of that side, so any one row reveals whether a side is empty
        flags |= ((a & SD_NONE) != SD_NONE) | ((g & SD_NONE) != SD_NONE) << 1;
    }
    if (flags) atomicOr(&s_flags, flags);
    __syncthreads();
    const bool both = s_flags == 3;
    unsigned* hb = hist + (long)bk * SD_HIST;
    int mx = 0;
    SdRun run = {0, 0u};
    for (int s = 0; s < 2; ++s) {
        const unsigned short* src = s_row + s * W;
        const unsigned short* oth = s_row + (1 - s) * W;
        int* out = list + (row * 2 + s) * W;
        int cnt = 0;
        double sum = 0.0;
        for (int base = 0; base < W; base += 256) {
            const int w = base + threadIdx.x;
            const bool surf = w < W && (src[w] & SD_SURF);
            cnt += surf;
            const bool valid = surf && both;
            int d2 = 0;
            if (valid) {
                d2 = sd_row_d2(oth, w, W);
                sum += sqrt((double)d2);
                mx = max(mx, d2);
                out[atomicAdd(&s_slot[s], 1)] = d2;
            }
            sd_run_add(hb, run, d2 >> SD_LOW, valid);
        }
        for (int o = 32; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o);
            cnt += __shfl_xor(cnt, o);
        }
        if (lane == 0) { s_sum[s][wave] = sum; s_cnt[s][wave] = cnt; }
    }
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
    if (lane == 0) { s_max[wave] = mx; s_runk[wave] = run.k; s_runn[wave] = run.n; }
    __syncthreads();
    if (threadIdx.x == 3) {                                    // the four waves' pending runs: equal keys are added once
        int k = s_runk[0];
        unsigned n = s_runn[0];
        for (int v = 1; v < 4; ++v) {
            if (s_runk[v] == k) { n += s_runn[v]; continue; }
            if (n) atomicAdd(&hb[k], n);
            k = s_runk[v];
            n = s_runn[v];
        }
        if (n) atomicAdd(&hb[k], n);
    }
    if (threadIdx.x < 2) {
        const int s = threadIdx.x;
        rowcnt[row * 2 + s] = s_cnt[s][0] + s_cnt[s][1] + s_cnt[s][2] + s_cnt[s][3];
        rowsum[row * 2 + s] = ((s_sum[s][0] + s_sum[s][1]) + s_sum[s][2]) + s_sum[s][3];
    }
    if (threadIdx.x == 2) rowmax[row] = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
}

// the two ranks of np.percentile(S, 95) on n > 0 values, and the weight t
__device__ __forceinline__ void sd_ranks(long long n, long long& lo, long long& hi, double& t) {
#pragma clang fp contract(off)
    const double v = (double)(n - 1) * 0.95;
    lo = (long long)floor(v);
    t = v - (double)lo;
    hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
}

// The bin that holds rank r (0-based, ascending) of a histogram of nbins = 256 * per bins, and r's rank inside that bin; total in
// *s_total.  Every thread of the 256-thread block calls it; r must be below the total unless the total is 0.
__device__ void sd_find(const unsigned* __restrict__ hist, int nbins, long long r, unsigned long long* s_part, int* s_bin,
                        long long* s_res, long long* s_total) {
    const int per = nbins >> 8, t = threadIdx.x;
    unsigned long long sum = 0;
    for (int i = 0; i < per; ++i) sum += hist[t * per + i];
    __syncthreads();                                           // the previous call's readers are done with s_part / s_bin
    s_part[t] = sum;
    __syncthreads();
    if (t == 0) {
        long long total = 0;
        for (int u = 0; u < 256; ++u) total += (long long)s_part[u];
        long long cum = 0;
        int u = 0;
        while (u < 255 && r >= cum + (long long)s_part[u]) cum += (long long)s_part[u++];
        int bin = u * per;
        for (int i = 0; i < per - 1; ++i) {
            const long long hv = hist[u * per + i];
            if (r < cum + hv) break;
            cum += hv;
            ++bin;
        }
        *s_bin = bin;
        *s_res = r - cum;
        *s_total = total;
    }
    __syncthreads();
}

// grid (SD_SEL_BLOCKS, B * (K - c0)), block 256: block x takes the rows x, x + gridDim.x, ...
__global__ __launch_bounds__(256) void sd_select_kernel(const int* __restrict__ list, const int* __restrict__ rowcnt, int H, int W,
                                                        unsigned* __restrict__ hist) {
    __shared__ unsigned long long s_part[256];
    __shared__ int s_bin;
    __shared__ long long s_res, s_total;
    const int bk = blockIdx.y;
    unsigned* h1 = hist + (long)bk * SD_HIST;
    unsigned* h2 = h1 + SD_BINS1;
    sd_find(h1, SD_BINS1, 0, s_part, &s_bin, &s_res, &s_total);
    const long long n = s_total;
    if (n == 0) return;                                        // a side is empty: nothing to select
    long long lo, hi;
    double t;
    sd_ranks(n, lo, hi, t);
    sd_find(h1, SD_BINS1, lo, s_part, &s_bin, &s_res, &s_total);
    const int p0 = s_bin;
    sd_find(h1, SD_BINS1, hi, s_part, &s_bin, &s_res, &s_total);
    const int p1 = s_bin;
    for (int h = blockIdx.x; h < H; h += gridDim.x) {
        const long row = (long)bk * H + h;
        for (int s = 0; s < 2; ++s) {
            const int cnt = rowcnt[row * 2 + s];
            const int* src = list + (row * 2 + s) * W;
            for (int base = 0; base < cnt; base += 256) {
                const int i = base + threadIdx.x;
                const int key = i < cnt ? src[i] : 0;
                sd_hist_add(h2, key & (SD_BINS2 - 1), i < cnt && (key >> SD_LOW) == p0);
                sd_hist_add(h2 + SD_BINS2, key & (SD_BINS2 - 1), i < cnt && (key >> SD_LOW) == p1);
            }
        }
    }
}

// grid (B * K), block 256
__global__ __launch_bounds__(256) void sd_finalize_kernel(const int* __restrict__ rowcnt, const double* __restrict__ rowsum,
                                                          const int* __restrict__ rowmax, const unsigned* __restrict__ hist, int K,
                                                          int c0, int H, double* __restrict__ stats, long long* __restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_part[256];
    __shared__ int s_bin;
    __shared__ long long s_res, s_total;
    __shared__ double s_sum[2][256];
    __shared__ long long s_cnt[2][256];
    __shared__ int s_mx[256];
    const int b = blockIdx.x / K, c = blockIdx.x % K, t = threadIdx.x;
    double* st = stats + (long)blockIdx.x * 4;
    long long* ct = counts + (long)blockIdx.x * 2;
    if (c < c0) {
        if (t < 4) st[t] = 0.0;
        if (t < 2) ct[t] = 0;
        return;
    }
    const int bk = b * (K - c0) + (c - c0);
    double sum[2] = {0.0, 0.0};
    long long cnt[2] = {0, 0};
    int mx = 0;
    for (int h = t; h < H; h += 256) {
        const long row = (long)bk * H + h;
        sum[0] += rowsum[row * 2];
        sum[1] += rowsum[row * 2 + 1];
        cnt[0] += rowcnt[row * 2];
        cnt[1] += rowcnt[row * 2 + 1];
        mx = max(mx, rowmax[row]);
    }
    s_sum[0][t] = sum[0]; s_sum[1][t] = sum[1]; s_cnt[0][t] = cnt[0]; s_cnt[1][t] = cnt[1]; s_mx[t] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            s_sum[0][t] += s_sum[0][t + o]; s_sum[1][t] += s_sum[1][t + o];
            s_cnt[0][t] += s_cnt[0][t + o]; s_cnt[1][t] += s_cnt[1][t + o];
            s_mx[t] = max(s_mx[t], s_mx[t + o]);
        }
        __syncthreads();
    }
    const long long nA = s_cnt[0][0], nG = s_cnt[1][0];
    const int state = nA > 0 ? (nG > 0 ? 0 : 3) : (nG > 0 ? 2 : 1);
    if (state != 0) {                                          // block-uniform
        if (t == 0) {
            st[0] = 0.0; st[1] = 0.0; st[2] = 0.0; st[3] = (double)state;
            ct[0] = nA; ct[1] = nG;
        }
        return;
    }
    const unsigned* h1 = hist + (long)bk * SD_HIST;
    const unsigned* h2 = h1 + SD_BINS1;
    const long long n = nA + nG;
    long long lo, hi;
    double w;
    sd_ranks(n, lo, hi, w);
    sd_find(h1, SD_BINS1, lo, s_part, &s_bin, &s_res, &s_total);
    const int p0 = s_bin;
    const long long r0 = s_res;
    sd_find(h1, SD_BINS1, hi, s_part, &s_bin, &s_res, &s_total);
    const int p1 = s_bin;
    const long long r1 = s_res;
    sd_find(h2, SD_BINS2, r0, s_part, &s_bin, &s_res, &s_total);
    const int q0 = s_bin;
    sd_find(h2 + SD_BINS2, SD_BINS2, r1, s_part, &s_bin, &s_res, &s_total);
    const int q1 = s_bin;
    if (t == 0) {
        const double a = sqrt((double)((p0 << SD_LOW) | q0)), bb = sqrt((double)((p1 << SD_LOW) | q1));
        const double diff = bb - a;
        st[0] = sqrt((double)s_mx[0]);
        st[1] = w < 0.5 ? a + diff * w : bb - diff * (1.0 - w);
        st[2] = (s_sum[0][0] / (double)nA + s_sum[1][0] / (double)nG) / 2.0;
        st[3] = 0.0;
        ct[0] = nA; ct[1] = nG;
    }
}

// one thread per item of n images: the float64 mean over (image, class c0..K-1) in that order, one rounding to fp32
__global__ __launch_bounds__(64) void sd_scores_kernel(const double* __restrict__ stats, int items, int n, int K, int c0, int kind,
                                                       int empty_rule, int H, int W, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int it = blockIdx.x * 64 + threadIdx.x;
    if (it >= items) return;
    const double diag = sqrt((double)((H - 1) * (H - 1) + (W - 1) * (W - 1)));
    const double empty = empty_rule == 0 ? diag : (empty_rule == 1 ? 0.0 : __builtin_nan(""));
    double total = 0.0;
    for (int i = 0; i < n; ++i)
        for (int c = c0; c < K; ++c) {
            const double* st = stats + (((long)it * n + i) * K + c) * 4;
            const int state = (int)st[3];
            total += state == 0 ? st[kind] : (state == 1 ? 0.0 : empty);
        }
    out[it] = (float)(total / (double)(n * (K - c0)));
}

size_t sd_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct SdLayout { size_t tab, list, rowsum, rowcnt, rowmax, hist, total; };

// bka = B * (K - c0): only the scored (image, class) pairs take workspace
SdLayout sd_layout(int bka, int H, int W) {
    const size_t bk = (size_t)bka, px = bk * H * W, rows = bk * H;
    SdLayout l;
    l.tab = 0;
    l.list = l.tab + sd_align(2 * px * sizeof(unsigned short));
    l.rowsum = l.list + sd_align(2 * px * sizeof(int));
    l.rowcnt = l.rowsum + sd_align(2 * rows * sizeof(double));
    l.rowmax = l.rowcnt + sd_align(2 * rows * sizeof(int));
    l.hist = l.rowmax + sd_align(rows * sizeof(int));
    l.total = l.hist + sd_align(bk * SD_HIST * sizeof(unsigned));
    return l;
}

bool sd_shape_ok(int B, int K, int H, int W) {
    return H <= SD_MAX && W <= SD_MAX && K >= 2 && K <= SD_MAXK && (long)B * K * H * W < (1L << 31) && (long)B * K <= 65535;
}

}  // namespace

extern "C" size_t umi_surface_ws_bytes(int B, int K, int c0, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || !sd_shape_ok(B, K, H, W) || c0 < 0 || c0 >= K) return 0;
    return sd_layout(B * (K - c0), H, W).total;
}

extern "C" int umi_surface_distances(const unsigned char* pred_mask, const void* target, int target_dtype, int B, int K, int c0, int H,
                                     int W, double* stats, long long* counts, void* ws, size_t ws_bytes, umi_stream_t stream) {
    if (!pred_mask || !target || !stats || !counts || !ws || B <= 0 || H <= 0 || W <= 0 || target_dtype < 0 || target_dtype > 3)
        return UMI_ERR_BADARG;
    const unsigned long tal = target_dtype == 0 ? 7 : (target_dtype == 2 ? 0 : 3);
    if (((unsigned long)target & tal) || ((unsigned long)stats & 7) || ((unsigned long)counts & 7) || ((unsigned long)ws & 7))
        return UMI_ERR_BADARG;
    if (!sd_shape_ok(B, K, H, W)) return UMI_ERR_UNSUPPORTED;      // B * K <= 65535: grid.y of the launches
    if (c0 < 0 || c0 >= K) return UMI_ERR_BADARG;
    if (ws_bytes < umi_surface_ws_bytes(B, K, c0, H, W)) return UMI_ERR_WORKSPACE;
    const SdLayout l = sd_layout(B * (K - c0), H, W);
    char* base = (char*)ws;
    unsigned short* tab = (unsigned short*)(base + l.tab);
    int* list = (int*)(base + l.list);
    double* rowsum = (double*)(base + l.rowsum);
    int* rowcnt = (int*)(base + l.rowcnt);
    int* rowmax = (int*)(base + l.rowmax);
    unsigned* hist = (unsigned*)(base + l.hist);
    hipStream_t s = (hipStream_t)stream;
    const int bka = B * (K - c0), nw = min(16, (H + 63) / 64);
    hipLaunchKernelGGL(sd_col_kernel, dim3((W + SD_COLS - 1) / SD_COLS, bka, 2), dim3(64 * nw), 0, s, pred_mask, target, target_dtype,
                       K, c0, H, W, tab, hist);
    UMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(sd_row_kernel, dim3(H, bka), dim3(256), 2 * W * sizeof(unsigned short), s, (const unsigned short*)tab, H, W,
                       list, rowcnt, rowsum, rowmax, hist);
    UMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(sd_select_kernel, dim3(min(SD_SEL_BLOCKS, H), bka), dim3(256), 0, s, (const int*)list, (const int*)rowcnt, H, W,
                       hist);
    UMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(sd_finalize_kernel, dim3(B * K), dim3(256), 0, s, (const int*)rowcnt, (const double*)rowsum,
                       (const int*)rowmax, (const unsigned*)hist, K, c0, H, stats, counts);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_surface_scores(const double* stats, int items, int n, int K, int c0, int kind, int empty_rule, int H, int W,
                                  float* out, umi_stream_t stream) {
    if (!stats || !out || items <= 0 || n <= 0 || H <= 0 || W <= 0 || kind < 0 || kind > 2 || empty_rule < 0 || empty_rule > 2 ||
        ((unsigned long)stats & 7))
        return UMI_ERR_BADARG;
    if (K < 2 || K > SD_MAXK || H > SD_MAX || W > SD_MAX) return UMI_ERR_UNSUPPORTED;
    if (c0 < 0 || c0 >= K) return UMI_ERR_BADARG;
    hipLaunchKernelGGL(sd_scores_kernel, dim3((items + 63) / 64), dim3(64), 0, (hipStream_t)stream, stats, items, n, K, c0, kind,
                       empty_rule, H, W, out);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
