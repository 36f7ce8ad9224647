// HausdorffDTLoss (reference loss.py:146-212) on fp32 logits and targets [B,1,H,W]:
//   s = sigmoid(pred), field(img)[b] = exact Euclidean distance of every pixel to the nearest pixel of the OTHER class of
//   img[b] > 0.5 (0 if the image has no foreground; sqrt(1 + h^2 + w^2) if it has no background -- scipy's edt of an
//   all-ones (1,H,W) slice measures from a virtual zero at index -1 of the size-1 axis),
//   D = field(s)^alpha + field(target)^alpha,   loss = mean((s - target)^2 * D).
// The fields are an integer problem, solved separably (Saito-Toriwaki): squared distance = min over w' of g(w')^2 + (w-w')^2,
// g = 1-D column distance.  Squared distances are exact int32; field = (float)sqrt((double)d2) equals scipy's float64
// sqrt cast to float32 bit for bit (no fast-math root).
//   hdt_col_kernel : threshold + per-column distances to the nearest fg / bg pixel of both images (one 64-row bitmask per
//                    thread, chunk summaries scanned through LDS), packed {g_fg, g_bg} as 2 x 16 bits per pixel
//   hdt_row_kernel : one block per (image, row): both tables' rows in LDS, outward exact search per pixel, the degenerate
//                    rules, D, optional fields, and the row's fp64 partial of sum((s-t)^2 * D) (fixed order)
//   hdt_finalize   : fixed-order fp64 sum of the row partials -> loss (deterministic run to run)
//   hdt_bwd_kernel : one streaming pass, dpred = gout * 2 (s-t) s (1-s) D / numel
#include "common.h"

namespace {

constexpr int HDT_MAX = 4096;           // H, W limit: column distances fit 16 bits, squared distances int32
constexpr unsigned HDT_NONE = 0xFFFFu;  // "this column has no pixel of that class"
constexpr int HDT_INF = 0x3fffffff;     // squared-distance infinity; INF + (W-1)^2 stays below 2^31
constexpr int ROW_THREADS = 256;
constexpr int MAX_WAVES = 16;           // column pass: up to 16 waves x 64 columns, <= 4 chunks of 64 rows per thread

// torch.sigmoid's device arithmetic, one / (one + exp(-x)), so the mask equals `torch.sigmoid(x) > 0.5` on the device
__device__ __forceinline__ float hdt_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ bool hdt_fg(const float* src, long i, bool is_pred) {
    const float v = src[i];
    return (is_pred ? hdt_sigmoid(v) : v) > 0.5f;
}

// distance from row r to the nearest set row: m = this chunk's mask (bit i = row r0 + i), above/below = nearest set row
// outside the chunk (-1 = none)
__device__ __forceinline__ unsigned hdt_col_dist(unsigned long long m, int i, int r0, int above, int below) {
    const unsigned long long up = m & ((2ull << i) - 1ull);      // bits 0..i (i = 63: 2ull << 63 == 0, minus 1 == all)
    const unsigned long long dn = m >> i;
    const int a = up ? r0 + 63 - __clzll((long long)up) : above;
    const int b = dn ? r0 + i + __ffsll((long long)dn) - 1 : below;
    const int r = r0 + i;
    int d = HDT_NONE;
    if (a >= 0) d = r - a;
    if (b >= 0) d = min(d, b - r);
    return (unsigned)d;
}

// grid (ceil(W/64), B, 2): blockIdx.z = 0 pred, 1 target.  block = 64 columns x nw waves, nw = min(16, ceil(H/64));
// wave v owns the 64-row chunks v, v + nw, ...   tab[z][b][h][w] = g_fg | g_bg << 16.
__global__ __launch_bounds__(1024) void hdt_col_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                       int B, int H, int W, unsigned* __restrict__ tab) {
    __shared__ short s_lastF[64][64], s_firstF[64][64], s_lastB[64][64], s_firstB[64][64];   // [chunk][column]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int col = blockIdx.x * 64 + lane, b = blockIdx.y, z = blockIdx.z;
    const bool is_pred = z == 0;
    const float* src = (is_pred ? pred : target) + (long)b * H * W;
    const int nchunk = (H + 63) >> 6;
    unsigned long long mf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = wave + j * nw, r0 = c * 64;
        mf[j] = 0ull;
        if (c < nchunk) {
            const int n = min(64, H - r0);
            if (col < W) {
#pragma unroll 16
                for (int i = 0; i < 64; ++i)
                    if (i < n && hdt_fg(src, (long)(r0 + i) * W + col, is_pred)) mf[j] |= 1ull << i;
            }
            const unsigned long long valid = n == 64 ? ~0ull : (1ull << n) - 1ull;
            const unsigned long long mb = ~mf[j] & valid;
            s_firstF[c][lane] = mf[j] ? (short)(r0 + __ffsll((long long)mf[j]) - 1) : (short)-1;
            s_lastF[c][lane] = mf[j] ? (short)(r0 + 63 - __clzll((long long)mf[j])) : (short)-1;
            s_firstB[c][lane] = mb ? (short)(r0 + __ffsll((long long)mb) - 1) : (short)-1;
            s_lastB[c][lane] = mb ? (short)(r0 + 63 - __clzll((long long)mb)) : (short)-1;
        }
    }
    __syncthreads();
    // wave 0 turns the chunk summaries into "nearest set row above the chunk" (s_last*) and "below the chunk" (s_first*)
    if (wave == 0) {
        int lf = -1, lb = -1;
        for (int c = 0; c < nchunk; ++c) {
            const int tf = s_lastF[c][lane], tb = s_lastB[c][lane];
            s_lastF[c][lane] = (short)lf;
            s_lastB[c][lane] = (short)lb;
            if (tf >= 0) lf = tf;
            if (tb >= 0) lb = tb;
        }
        int ff = -1, fb = -1;
        for (int c = nchunk - 1; c >= 0; --c) {
            const int tf = s_firstF[c][lane], tb = s_firstB[c][lane];
            s_firstF[c][lane] = (short)ff;
            s_firstB[c][lane] = (short)fb;
            if (tf >= 0) ff = tf;
            if (tb >= 0) fb = tb;
        }
    }
    __syncthreads();
    if (col >= W) return;
    unsigned* out = tab + ((long)z * B + b) * H * W + col;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = wave + j * nw, r0 = c * 64;
        if (c >= nchunk) break;
        const int n = min(64, H - r0);
        const unsigned long long valid = n == 64 ? ~0ull : (1ull << n) - 1ull;
        const unsigned long long f = mf[j], bg = ~f & valid;
        const int af = s_lastF[c][lane], bf = s_firstF[c][lane], ab = s_lastB[c][lane], bb = s_firstB[c][lane];
#pragma unroll 8
        for (int i = 0; i < n; ++i)
            out[(long)(r0 + i) * W] = hdt_col_dist(f, i, r0, af, bf) | hdt_col_dist(bg, i, r0, ab, bb) << 16;
    }
}

// squared distance of pixel w of this row to the nearest pixel of the other class, given both classes exist in the image
__device__ __forceinline__ int hdt_row_d2(const unsigned* __restrict__ t, int w, int W) {
    const int sh = (t[w] & 0xFFFFu) == 0 ? 16 : 0;      // a foreground pixel reads the table of distances to background
    auto g2 = [&](int x) {
        const int g = (int)((t[x] >> sh) & 0xFFFFu);
        return g == (int)HDT_NONE ? HDT_INF : g * g;
    };
    int best = g2(w);
    // exact: a column k away adds k^2, so the search stops once k^2 >= best
    for (int k = 1; k * k < best && (w - k >= 0 || w + k < W); ++k) {
        if (w - k >= 0) best = min(best, g2(w - k) + k * k);
        if (w + k < W) best = min(best, g2(w + k) + k * k);
    }
    return best;
}

__device__ __forceinline__ float hdt_field(const unsigned* t, int h, int w, int W, bool any_fg, bool any_bg) {
    if (!any_fg) return 0.f;
    const int d2 = any_bg ? hdt_row_d2(t, w, W) : 1 + h * h + w * w;
    return (float)sqrt((double)d2);                    // correctly rounded: == scipy's float64 sqrt cast to float32
}

// grid (H, B), block 256, dynamic LDS 2 * W * 4 bytes (the row of both tables)
__global__ __launch_bounds__(ROW_THREADS) void hdt_row_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                              const unsigned* __restrict__ tab, int B, int H, int W,
                                                              float alpha, float* __restrict__ D, float* __restrict__ fields,
                                                              double* __restrict__ part) {
    extern __shared__ unsigned s_tab[];
    unsigned* tp = s_tab;
    unsigned* tt = s_tab + W;
    __shared__ int s_flags;
    __shared__ double red[ROW_THREADS / 64];
    const int h = blockIdx.x, b = blockIdx.y;
    const long HW = (long)H * W, N = (long)B * HW;
    const long row = (long)b * HW + (long)h * W;
    if (threadIdx.x == 0) s_flags = 0;
    __syncthreads();
    int flags = 0;
    for (int w = threadIdx.x; w < W; w += ROW_THREADS) {
        const unsigned p = tab[row + w], t = tab[N + row + w];
        tp[w] = p;
        tt[w] = t;
        // a column with a finite distance to a class holds that class, so any one row reveals the whole image's classes
        flags |= ((p & 0xFFFFu) != HDT_NONE) | ((p >> 16) != HDT_NONE) << 1 | ((t & 0xFFFFu) != HDT_NONE) << 2 |
                 ((t >> 16) != HDT_NONE) << 3;
    }
    if (flags) atomicOr(&s_flags, flags);
    __syncthreads();
    const int f = s_flags;
    double acc = 0.0;
    for (int w = threadIdx.x; w < W; w += ROW_THREADS) {
        const float fp = hdt_field(tp, h, w, W, f & 1, f & 2);
        const float ft = hdt_field(tt, h, w, W, f & 4, f & 8);
        const float d = powf(fp, alpha) + powf(ft, alpha);
        const long i = row + w;
        D[i] = d;
        if (fields) {
            fields[i] = fp;
            fields[N + i] = ft;
        }
        {
#pragma clang fp contract(off)
            const float e = hdt_sigmoid(pred[i]) - target[i];
            acc += (double)((e * e) * d);
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int v = 0; v < ROW_THREADS / 64; ++v) s += red[v];
        part[(long)b * H + h] = s;
    }
}

// one block of 1024: thread k sums rows k, k+1024, ... then a fixed-shape tree
__global__ __launch_bounds__(1024) void hdt_finalize_kernel(const double* __restrict__ part, long rows, long numel,
                                                            float* __restrict__ loss) {
    __shared__ double s[1024];
    double acc = 0.0;
    for (long r = threadIdx.x; r < rows; r += 1024) acc += part[r];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(s[0] / (double)numel);
}

// the reference's autograd chain: mean -> * D -> pow(., 2) -> sigmoid
__device__ __forceinline__ float hdt_grad(float x, float t, float d, float gn) {
#pragma clang fp contract(off)
    const float s = hdt_sigmoid(x);
    return ((gn * d) * (2.f * (s - t))) * ((1.f - s) * s);
}

__global__ __launch_bounds__(256) void hdt_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                      const float* __restrict__ D, const float* __restrict__ gout, long N,
                                                      long n4, float* __restrict__ dpred) {
    const float gn = (gout ? gout[0] : 1.f) / (float)N;
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const float4 x = reinterpret_cast<const float4*>(pred)[i];
        const float4 t = reinterpret_cast<const float4*>(target)[i];
        const float4 d = reinterpret_cast<const float4*>(D)[i];
        reinterpret_cast<float4*>(dpred)[i] =
            make_float4(hdt_grad(x.x, t.x, d.x, gn), hdt_grad(x.y, t.y, d.y, gn), hdt_grad(x.z, t.z, d.z, gn),
                        hdt_grad(x.w, t.w, d.w, gn));
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < N; i += stride)
        dpred[i] = hdt_grad(pred[i], target[i], D[i], gn);
}

size_t tab_bytes(int B, int H, int W) { return ((size_t)2 * B * H * W * sizeof(unsigned) + 255) & ~(size_t)255; }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" size_t umi_hdt_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return tab_bytes(B, H, W) + (size_t)B * H * sizeof(double);
}

extern "C" int umi_hdt_fwd(const float* pred, const float* target, int B, int C, int H, int W, float alpha, float* D,
                           float* fields, float* loss, void* ws, size_t ws_bytes, umi_stream_t st) {
    if (!pred || !target || !D || !loss || !ws || B <= 0 || C <= 0 || H <= 0 || W <= 0) return UMI_ERR_BADARG;
    if (C != 1 || H > HDT_MAX || W > HDT_MAX || B > 65535) return UMI_ERR_UNSUPPORTED;    // B: grid.y of the launches
    if (ws_bytes < umi_hdt_ws_bytes(B, H, W)) return UMI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)st;
    unsigned* tab = (unsigned*)ws;
    double* part = (double*)((char*)ws + tab_bytes(B, H, W));
    const int nw = min(MAX_WAVES, (H + 63) / 64);
    hipLaunchKernelGGL(hdt_col_kernel, dim3((W + 63) / 64, B, 2), dim3(64 * nw), 0, s, pred, target, B, H, W, tab);
    UMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(hdt_row_kernel, dim3(H, B), dim3(ROW_THREADS), 2 * W * sizeof(unsigned), s, pred, target, (const unsigned*)tab, B, H, W, alpha,
                       D, fields, part);
    UMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(hdt_finalize_kernel, dim3(1), dim3(1024), 0, s, (const double*)part, (long)B * H, (long)B * H * W,
                       loss);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_hdt_bwd(const float* pred, const float* target, const float* D, const float* gout, int B, int C, int H,
                           int W, float* dpred, umi_stream_t st) {
    if (!pred || !target || !D || !dpred || B <= 0 || C <= 0 || H <= 0 || W <= 0) return UMI_ERR_BADARG;
    if (C != 1 || H > HDT_MAX || W > HDT_MAX || B > 65535) return UMI_ERR_UNSUPPORTED;    // B: grid.y of the launches
    const long N = (long)B * H * W;
    const long n4 = aligned16(pred) && aligned16(target) && aligned16(D) && aligned16(dpred) ? N / 4 : 0;   // float4 body
    long grid = (N / 4 + 255) / 256;
    grid = grid < 1 ? 1 : (grid > 2048 ? 2048 : grid);
    hipLaunchKernelGGL(hdt_bwd_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)st, pred, target, D, gout, N, n4, dpred);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
