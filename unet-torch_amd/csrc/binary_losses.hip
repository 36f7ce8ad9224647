// Binary-segmentation training losses of the reference calc_loss (loss.py:442-516) on NCHW fp32 logits:
//   'dice_bce' (:484-487, BinaryDiceLoss :254-307): 0.5 * BCEWithLogits + 0.5 * mean_b (1 - (2*sum_b s*t + 1) / (sum_b |s| +
//              sum_b |t| + 1)), s = sigmoid(x), sums per image
//   'Tversky'  (:514-515, FocalTverskyLoss :380-420, gamma 1): C == 1: TP/FP/FN of s over the whole batch,
//              loss = 1 - (TP + 1) / (TP + alpha*FP + beta*FN + 1); C > 1: the same per class of softmax(x) against
//              [label == c], mean over classes
//   'TopK'     (:445-446, TopKLoss :354-378): mean BCE over the k = N//2 pixels of LOWEST true-class probability
//              (sigmoid(x) where trunc(t) == 1, 1 - sigmoid(x) otherwise)
//   'BCE_HEM'  (:447-467): mean BCE over the k = 500 pixels of LARGEST BCE
// BCE term = (1 - t) * x - log_sigmoid(x), torch's formula.  Every sum is fixed-order (fp64 across threads), so results are
// deterministic run to run; all state crosses between phases at kernel boundaries, none stays in static device memory.
//
// Streaming statistics (dice_bce, Tversky):
//   bin_stats_kernel  : grid (nb, B), per-block fp64 rows {sum s*t, sum s, sum |t|, sum t, sum bce} of one image
//   mc_stats_kernel<C>: grid-stride over pixels, softmax in registers, per-block fp64 rows {TP_c | P_c | T_c}
//   stats_finalize    : fixed-order fp64 column sums per group -> stats, then the loss
//   bin_bwd / mc_bwd  : one streaming pass each, coefficients from the fp64 stats
// Exact selection (TopK, BCE_HEM): an order-preserving uint32 map of the fp32 key, "smaller = taken first"; block b of the
// streaming passes owns the contiguous flat range [b*chunk, (b+1)*chunk), so block order is flat-index order.
//   sel_hist_kernel x4 : 8-bit digit histograms of the keys that match the prefix found so far (LDS, then integer atomics)
//   sel_pick_kernel  x4: one block picks the digit that holds rank k -> {prefix, remaining rank} in device memory; after the
//                        last digit, prefix = threshold key T, rank = r = how many keys equal to T are taken, and the per-block
//                        counts of keys == T are scanned into per-block tie offsets
//   sel_sum_kernel     : keys < T are taken, keys == T by flat index while the tie count stays below r; writes the mask and
//                        per-block fp64 BCE sums
//   sum_finalize       : fixed-order sum -> loss = sum / k
//   sel_bwd_kernel     : dpred = mask * gout * (s - t) / k
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int BIN_COLS = 5;            // {sum s*t, sum s, sum |t|, sum t, sum bce}
constexpr int SEL_MAX_BLOCKS = 1024;   // blocks of the selection passes: one 1024-thread scan covers their tie counts
constexpr long SEL_TILE = 4L * THREADS;

// torch.sigmoid's device arithmetic
__device__ __forceinline__ float bl_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// BCEWithLogits per element: (1 - t) * x - log_sigmoid(x), log_sigmoid(x) = min(x, 0) - log1p(exp(-|x|))
__device__ __forceinline__ float bl_bce(float x, float t) {
    const float ls = fminf(x, 0.f) - log1pf(expf(-fabsf(x)));
    return (1.f - t) * x - ls;
}

// 4 consecutive elements from e (< end); float4 when the caller proved alignment and all 4 are in range
__device__ __forceinline__ void load4(const float* __restrict__ p, long e, long end, bool vec, float v[4]) {
    if (vec && e + 3 < end) {
        const float4 f = *reinterpret_cast<const float4*>(p + e);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = e + q < end ? p[e + q] : 0.f;
    }
}

// block-wide fixed-order sum of K doubles per thread (wave shuffles, then the 4 waves in order); result valid in thread 0..K-1
template <int K>
__device__ __forceinline__ void block_sum_rows(double (&v)[K], double* __restrict__ out) {
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

// ---------------------------------------------------------------------------------------------------------------------
// dice_bce and binary Tversky

// grid (nb, B): block (j, b) streams image b's pixels j*256 + tid, + nb*256, ...; part row b*nb + j.  vec: HW % 4 == 0 and
// both pointers 16-byte aligned (then every image starts aligned).
__global__ __launch_bounds__(THREADS) void bin_stats_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                            long HW, bool vec, double* __restrict__ part) {
    const int b = blockIdx.y;
    const float* x = pred + (long)b * HW;
    const float* t = target + (long)b * HW;
    float a[BIN_COLS] = {0.f, 0.f, 0.f, 0.f, 0.f};
    auto acc = [&](float xv, float tv) {
        const float s = bl_sigmoid(xv);
        a[0] = fmaf(s, tv, a[0]);
        a[1] += s;
        a[2] += fabsf(tv);
        a[3] += tv;
        a[4] += bl_bce(xv, tv);
    };
    const long stride = (long)gridDim.x * THREADS;
    if (vec) {
        for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < HW / 4; i += stride) {
            const float4 xv = reinterpret_cast<const float4*>(x)[i];
            const float4 tv = reinterpret_cast<const float4*>(t)[i];
            acc(xv.x, tv.x); acc(xv.y, tv.y); acc(xv.z, tv.z); acc(xv.w, tv.w);
        }
    } else {
        for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < HW; i += stride) acc(x[i], t[i]);
    }
    double v[BIN_COLS];
#pragma unroll
    for (int c = 0; c < BIN_COLS; ++c) v[c] = (double)a[c];
    block_sum_rows<BIN_COLS>(v, part + ((long)b * gridDim.x + blockIdx.x) * BIN_COLS);
}

// label of pixel i as a class index in [0, NC), or -1 (matches no class, as `target == c` in the reference)
template <int NC>
__device__ __forceinline__ int load_label(const void* t, int tdtype, long i) {
    long long v;
    if (tdtype == 0) v = reinterpret_cast<const long long*>(t)[i];
    else if (tdtype == 2) v = reinterpret_cast<const unsigned char*>(t)[i];
    else if (tdtype == 3) v = reinterpret_cast<const int*>(t)[i];
    else {
        const float f = reinterpret_cast<const float*>(t)[i];
        return (f >= 0.f && f < (float)NC && f == truncf(f)) ? (int)f : -1;
    }
    return (v >= 0 && v < NC) ? (int)v : -1;
}

// part row layout: [TP_0..TP_{NC-1}, P_0.., T_0..]
template <int NC>
__global__ __launch_bounds__(THREADS) void mc_stats_kernel(const float* __restrict__ logits, const void* __restrict__ target,
                                                           int tdtype, long HW, long total, double* __restrict__ part) {
    float tp[NC], ps[NC], ts[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) tp[c] = ps[c] = ts[c] = 0.f;
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < total; i += (long)gridDim.x * THREADS) {
        const long n = i / HW, hw = i - n * HW;
        const float* x = logits + n * NC * HW + hw;
        float v[NC], m = -INFINITY;
#pragma unroll
        for (int c = 0; c < NC; ++c) { v[c] = x[(long)c * HW]; m = fmaxf(m, v[c]); }
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) { v[c] = expf(v[c] - m); s += v[c]; }
        const float inv = 1.f / s;
        const int t = load_label<NC>(target, tdtype, i);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float p = v[c] * inv;
            ps[c] += p;
            if (c == t) { tp[c] += p; ts[c] += 1.f; }
        }
    }
    double r[3 * NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { r[c] = tp[c]; r[NC + c] = ps[c]; r[2 * NC + c] = ts[c]; }
    block_sum_rows<3 * NC>(r, part + (long)blockIdx.x * 3 * NC);
}

enum { LOSS_DICE_BCE = 0, LOSS_TVERSKY_BIN = 1, LOSS_TVERSKY_MC = 2 };

// 1 - (TP + 1) / (TP + alpha*FP + beta*FN + 1), FP = P - TP, FN = T - TP
__device__ __forceinline__ double tversky(double tp, double p, double t, double alpha, double beta) {
    return 1.0 - (tp + 1.0) / (tp + alpha * (p - tp) + beta * (t - tp) + 1.0);
}

// one block of 1024: stats[g*cols + c] = sum over rows r of group g of part[(g*rows + r)*cols + c], rows in order; then the
// loss from the stats (fp64), cast once to fp32
__global__ __launch_bounds__(1024) void stats_finalize_kernel(const double* __restrict__ part, int groups, int rows, int cols,
                                                              int kind, long numel, float alpha, float beta,
                                                              double* __restrict__ stats, float* __restrict__ loss) {
    for (int gc = threadIdx.x; gc < groups * cols; gc += 1024) {
        const int g = gc / cols, c = gc - g * cols;
        double s = 0.0;
        for (int r = 0; r < rows; ++r) s += part[((long)g * rows + r) * cols + c];
        stats[gc] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double l = 0.0;
    if (kind == LOSS_DICE_BCE) {
        double bce = 0.0, dice = 0.0;
        for (int b = 0; b < groups; ++b) {
            const double* r = stats + b * BIN_COLS;
            bce += r[4];
            dice += 1.0 - (2.0 * r[0] + 1.0) / (r[1] + r[2] + 1.0);
        }
        l = 0.5 * bce / (double)numel + 0.5 * dice / groups;
    } else if (kind == LOSS_TVERSKY_BIN) {
        double tp = 0.0, p = 0.0, t = 0.0;
        for (int b = 0; b < groups; ++b) { tp += stats[b * BIN_COLS]; p += stats[b * BIN_COLS + 1]; t += stats[b * BIN_COLS + 3]; }
        l = tversky(tp, p, t, alpha, beta);
    } else {
        const int nc = cols / 3;
        for (int c = 0; c < nc; ++c) l += tversky(stats[c], stats[nc + c], stats[2 * nc + c], alpha, beta);
        l /= nc;
    }
    loss[0] = (float)l;
}

// d loss / d s_i = c1 * t_i + c2 (the Dice or Tversky part), plus cb * (s_i - t_i) d loss / d x_i from the BCE part
struct BinCoef { float cb, c1, c2; };

__device__ __forceinline__ BinCoef bin_coef(const double* __restrict__ stats, int kind, int b, int B, long numel, float alpha,
                                            float beta) {
    BinCoef k;
    if (kind == LOSS_DICE_BCE) {
        const double* r = stats + b * BIN_COLS;
        const double num = 2.0 * r[0] + 1.0, den = r[1] + r[2] + 1.0;
        k.cb = (float)(0.5 / (double)numel);
        k.c1 = (float)(-0.5 / B * 2.0 / den);
        k.c2 = (float)(0.5 / B * num / (den * den));
    } else {
        double tp = 0.0, p = 0.0, t = 0.0;
        for (int i = 0; i < B; ++i) { tp += stats[i * BIN_COLS]; p += stats[i * BIN_COLS + 1]; t += stats[i * BIN_COLS + 3]; }
        // L = 1 - n/d, n = TP + 1, d = (1 - alpha - beta) TP + alpha P + beta T + 1; dTP/ds = t, dP/ds = 1, dT/ds = 0
        const double n = tp + 1.0, d = tp + alpha * (p - tp) + beta * (t - tp) + 1.0;
        k.cb = 0.f;
        k.c1 = (float)(-1.0 / d + n * (1.0 - alpha - beta) / (d * d));
        k.c2 = (float)(alpha * n / (d * d));
    }
    return k;
}

__device__ __forceinline__ float bin_grad(float x, float t, BinCoef k, float g) {
    const float s = bl_sigmoid(x);
    return g * (k.cb * (s - t) + fmaf(k.c1, t, k.c2) * (s * (1.f - s)));
}

// same grid as bin_stats_kernel
__global__ __launch_bounds__(THREADS) void bin_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                          const double* __restrict__ stats, const float* __restrict__ gout,
                                                          int kind, long HW, bool vec, float alpha, float beta,
                                                          float* __restrict__ dpred) {
    const int b = blockIdx.y;
    const BinCoef k = bin_coef(stats, kind, b, gridDim.y, (long)gridDim.y * HW, alpha, beta);
    const float g = gout ? gout[0] : 1.f;
    const long off = (long)b * HW, stride = (long)gridDim.x * THREADS;
    const float* x = pred + off;
    const float* t = target + off;
    float* o = dpred + off;
    if (vec) {
        for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < HW / 4; i += stride) {
            const float4 xv = reinterpret_cast<const float4*>(x)[i];
            const float4 tv = reinterpret_cast<const float4*>(t)[i];
            reinterpret_cast<float4*>(o)[i] = make_float4(bin_grad(xv.x, tv.x, k, g), bin_grad(xv.y, tv.y, k, g),
                                                          bin_grad(xv.z, tv.z, k, g), bin_grad(xv.w, tv.w, k, g));
        }
    } else {
        for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < HW; i += stride) o[i] = bin_grad(x[i], t[i], k, g);
    }
}

template <int NC>
__global__ __launch_bounds__(THREADS) void mc_bwd_kernel(const float* __restrict__ logits, const void* __restrict__ target,
                                                         int tdtype, const double* __restrict__ stats,
                                                         const float* __restrict__ gout, long HW, long total, float alpha,
                                                         float beta, float* __restrict__ dlogits) {
    const float g = gout ? gout[0] : 1.f;
    float c1[NC], c2[NC];                               // d loss / d p_c = c1_c * [t == c] + c2_c
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double tp = stats[c], p = stats[NC + c], t = stats[2 * NC + c];
        const double n = tp + 1.0, d = tp + alpha * (p - tp) + beta * (t - tp) + 1.0;
        c1[c] = (float)((-1.0 / d + n * (1.0 - alpha - beta) / (d * d)) / NC);
        c2[c] = (float)(alpha * n / (d * d) / NC);
    }
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < total; i += (long)gridDim.x * THREADS) {
        const long n = i / HW, hw = i - n * HW;
        const float* x = logits + n * NC * HW + hw;
        float p[NC], m = -INFINITY;
#pragma unroll
        for (int c = 0; c < NC; ++c) { p[c] = x[(long)c * HW]; m = fmaxf(m, p[c]); }
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) { p[c] = expf(p[c] - m); s += p[c]; }
        const float inv = 1.f / s;
        const int t = load_label<NC>(target, tdtype, i);
        float h[NC], dot = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            p[c] *= inv;
            h[c] = (c == t ? c1[c] : 0.f) + c2[c];
            dot = fmaf(h[c], p[c], dot);
        }
        float* o = dlogits + n * NC * HW + hw;
#pragma unroll
        for (int c = 0; c < NC; ++c) o[(long)c * HW] = g * (p[c] * (h[c] - dot));
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// TopK and BCE_HEM: exact k-th order statistic

enum { SEL_TOPK = 0, SEL_BCE_HEM = 1 };

// rank key: smaller = taken first.  TopK takes the smallest true-class probabilities, BCE_HEM the largest BCE.
__device__ __forceinline__ unsigned sel_key(float x, float t, int mode) {
    float v;
    if (mode == SEL_TOPK) {
        const float p = bl_sigmoid(x);
        v = truncf(t) == 1.f ? p : 1.f - p;            // the gather index t.long(): 1 -> foreground, 0 -> background
    } else {
        v = bl_bce(x, t);
    }
    unsigned u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // order-preserving map of fp32 to uint32
    return mode == SEL_TOPK ? u : ~u;
}

struct SelState { unsigned prefix, rank; };

// histogram of digit `pass` (bits 31-24 first) over the keys whose higher digits equal the prefix found so far.
// rows: NULL, or [nblk][256] per-block counts (the last pass: the tie counts of every candidate threshold).
__global__ __launch_bounds__(THREADS) void sel_hist_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                           long N, long chunk, int mode, int pass, bool vec,
                                                           const SelState* __restrict__ st, unsigned* __restrict__ hist,
                                                           unsigned* __restrict__ rows) {
    __shared__ unsigned h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const unsigned hmask = pass ? ~0u << (shift + 8) : 0u;
    const unsigned prefix = pass ? st->prefix : 0u;
    const long base = (long)blockIdx.x * chunk, end = min(N, base + chunk);
    for (long e = base + 4 * threadIdx.x; e < end; e += SEL_TILE) {
        float x[4], t[4];
        load4(pred, e, end, vec, x);
        load4(target, e, end, vec, t);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned u = sel_key(x[q], t[q], mode);
            if (e + q < end && (u & hmask) == prefix) atomicAdd(&h[(u >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    const unsigned c = h[threadIdx.x];
    if (c) atomicAdd(&hist[threadIdx.x], c);
    if (rows) rows[(long)blockIdx.x * 256 + threadIdx.x] = c;
}

// one block of 1024: inclusive-exclusive scan of the 256 bins, the digit whose range holds the remaining rank.  After the
// last digit also tie_off[b] = sum over blocks b' < b of their count of keys == T.
__global__ __launch_bounds__(1024) void sel_pick_kernel(const unsigned* __restrict__ hist, int pass, unsigned k,
                                                        SelState* __restrict__ st, const unsigned* __restrict__ rows, int nblk,
                                                        unsigned* __restrict__ tie_off) {
    __shared__ unsigned cum[1024];
    __shared__ unsigned s_digit;
    const int tid = threadIdx.x;
    const unsigned rank = pass ? st->rank : k, prefix = pass ? st->prefix : 0u;
    const int shift = 24 - 8 * pass;
    if (tid == 0) s_digit = 0;
    cum[tid] = tid < 256 ? hist[tid] : 0u;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const unsigned v = tid >= o ? cum[tid - o] : 0u;
        __syncthreads();
        cum[tid] += v;
        __syncthreads();
    }
    if (tid < 256) {
        const unsigned incl = cum[tid], excl = tid ? cum[tid - 1] : 0u;
        if (excl < rank && rank <= incl) {
            s_digit = tid;
            st->prefix = prefix | ((unsigned)tid << shift);
            st->rank = rank - excl;
        }
    }
    __syncthreads();
    if (pass != 3) return;
    const unsigned d = s_digit;
    const unsigned mine = tid < nblk ? rows[(long)tid * 256 + d] : 0u;
    __syncthreads();
    cum[tid] = mine;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const unsigned v = tid >= o ? cum[tid - o] : 0u;
        __syncthreads();
        cum[tid] += v;
        __syncthreads();
    }
    if (tid < nblk) tie_off[tid] = cum[tid] - mine;
}

// the selected set: key < T, or key == T and fewer than r keys == T precede it in flat order.  Writes mask[N] (0/1) and
// part[block] = fp64 sum of the selected BCE terms.
__global__ __launch_bounds__(THREADS) void sel_sum_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                          long N, long chunk, int mode, bool vec,
                                                          const SelState* __restrict__ st,
                                                          const unsigned* __restrict__ tie_off,
                                                          unsigned char* __restrict__ mask, double* __restrict__ part) {
    __shared__ unsigned wtot[THREADS / 64];
    const unsigned T = st->prefix, r = st->rank;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned ties = tie_off[blockIdx.x];               // keys == T before this tile, in flat order
    const long base = (long)blockIdx.x * chunk, end = min(N, base + chunk);
    double acc = 0.0;
    for (long e0 = base; e0 < end; e0 += SEL_TILE) {   // block-uniform trip count (the barriers below)
        const long e = e0 + 4 * threadIdx.x;
        float x[4], t[4];
        load4(pred, e, end, vec, x);
        load4(target, e, end, vec, t);
        unsigned u[4];
        int nt = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u[q] = sel_key(x[q], t[q], mode);
            nt += (e + q < end && u[q] == T);
        }
        unsigned before = 0;                            // keys == T of this tile in lanes / waves before this thread
        if (__syncthreads_count(nt)) {
            unsigned incl = (unsigned)nt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned v = __shfl_up(incl, o);
                if (lane >= o) incl += v;
            }
            if (lane == 63) wtot[wave] = incl;
            __syncthreads();
            before = incl - (unsigned)nt;
            unsigned all = 0;
            for (int w = 0; w < THREADS / 64; ++w) {
                if (w < wave) before += wtot[w];
                all += wtot[w];
            }
            before += ties;
            ties += all;
            __syncthreads();                           // wtot is rewritten by the next tile
        }
        unsigned char m[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bool take = false;
            if (e + q < end) {
                if (u[q] < T) take = true;
                else if (u[q] == T) take = before++ < r;
            }
            m[q] = take;
            if (take) acc += (double)bl_bce(x[q], t[q]);
        }
        if (vec && e + 3 < end) {
            *reinterpret_cast<uchar4*>(mask + e) = make_uchar4(m[0], m[1], m[2], m[3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (e + q < end) mask[e + q] = m[q];
        }
    }
    double v[1] = {acc};
    block_sum_rows<1>(v, part + blockIdx.x);
}

// one block of 1024: thread j sums part[j], part[j + 1024], ...; then a fixed-shape tree.  loss = sum / k
__global__ __launch_bounds__(1024) void sum_finalize_kernel(const double* __restrict__ part, long n, double k,
                                                            float* __restrict__ loss) {
    __shared__ double s[1024];
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 1024) acc += part[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(s[0] / k);
}

__device__ __forceinline__ float sel_grad(float x, float t, unsigned char m, float gk) {
    return m ? gk * (bl_sigmoid(x) - t) : 0.f;
}

__global__ __launch_bounds__(THREADS) void sel_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                          const unsigned char* __restrict__ mask,
                                                          const float* __restrict__ gout, long N, long n4, float k,
                                                          float* __restrict__ dpred) {
    const float gk = (gout ? gout[0] : 1.f) / k;
    const long stride = (long)gridDim.x * THREADS;
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < n4; i += stride) {
        const float4 x = reinterpret_cast<const float4*>(pred)[i];
        const float4 t = reinterpret_cast<const float4*>(target)[i];
        const uchar4 m = reinterpret_cast<const uchar4*>(mask)[i];
        reinterpret_cast<float4*>(dpred)[i] = make_float4(sel_grad(x.x, t.x, m.x, gk), sel_grad(x.y, t.y, m.y, gk),
                                                          sel_grad(x.z, t.z, m.z, gk), sel_grad(x.w, t.w, m.w, gk));
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * THREADS + threadIdx.x; i < N; i += stride)
        dpred[i] = sel_grad(pred[i], target[i], mask[i], gk);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

bool host_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int bin_blocks(long HW) {                               // per image: ~16 pixels per thread
    const long nb = (HW + 16L * THREADS - 1) / (16L * THREADS);
    return (int)(nb < 1 ? 1 : (nb > 65535 ? 65535 : nb));
}

int mc_blocks(long total) {                             // ~4 pixels per thread
    const long b = (total + 4L * THREADS - 1) / (4L * THREADS);
    return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

// selection partition: nblk <= SEL_MAX_BLOCKS blocks of `chunk` elements (a multiple of one tile), the last one short
void sel_grid(long N, long* chunk, int* nblk) {
    long per = (N + SEL_MAX_BLOCKS - 1) / SEL_MAX_BLOCKS;
    per = per < 16 * SEL_TILE ? 16 * SEL_TILE : per;   // >= 16 tiles per block
    *chunk = (per + SEL_TILE - 1) / SEL_TILE * SEL_TILE;
    *nblk = (int)((N + *chunk - 1) / *chunk);
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// selection workspace: hist[4][256] + state | rows[nblk][256] | tie_off[nblk] | part[nblk] (fp64)
constexpr size_t SEL_HEAD = 4 * 256 * sizeof(unsigned) + 256;

bool bad_bin_shape(int B, long HW) { return (long)B * HW >= (1L << 31) || B > 65535; }

}  // namespace

extern "C" size_t umi_binloss_ws_bytes(int B, int C, long HW) {
    if (B <= 0 || C <= 0 || HW <= 0) return 0;
    if (C == 1) return (size_t)B * bin_blocks(HW) * BIN_COLS * sizeof(double);
    return (size_t)mc_blocks((long)B * HW) * 3 * C * sizeof(double);
}

extern "C" int umi_dice_bce_fwd(const float* pred, const float* target, int B, long HW, double* stats, float* loss, void* ws,
                                size_t ws_bytes, umi_stream_t st) {
    if (!pred || !target || !stats || !loss || !ws || B <= 0 || HW <= 0) return UMI_ERR_BADARG;
    if (bad_bin_shape(B, HW)) return UMI_ERR_UNSUPPORTED;
    if (ws_bytes < umi_binloss_ws_bytes(B, 1, HW)) return UMI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)st;
    const int nb = bin_blocks(HW);
    const bool vec = HW % 4 == 0 && host_aligned16(pred) && host_aligned16(target);
    hipLaunchKernelGGL(bin_stats_kernel, dim3(nb, B), dim3(THREADS), 0, s, pred, target, HW, vec, (double*)ws);
    UMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(stats_finalize_kernel, dim3(1), dim3(1024), 0, s, (const double*)ws, B, nb, BIN_COLS, (int)LOSS_DICE_BCE,
                       (long)B * HW, 0.f, 0.f, stats, loss);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_dice_bce_bwd(const float* pred, const float* target, const double* stats, const float* gout, int B, long HW,
                                float* dpred, umi_stream_t st) {
    if (!pred || !target || !stats || !dpred || B <= 0 || HW <= 0) return UMI_ERR_BADARG;
    if (bad_bin_shape(B, HW)) return UMI_ERR_UNSUPPORTED;
    const bool vec = HW % 4 == 0 && host_aligned16(pred) && host_aligned16(target) && host_aligned16(dpred);
    hipLaunchKernelGGL(bin_bwd_kernel, dim3(bin_blocks(HW), B), dim3(THREADS), 0, (hipStream_t)st, pred, target, stats, gout,
                       (int)LOSS_DICE_BCE, HW, vec, 0.f, 0.f, dpred);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_tversky_fwd(const float* pred, const void* target, int target_dtype, int B, int C, long HW, float alpha,
                               float beta, double* stats, float* loss, void* ws, size_t ws_bytes, umi_stream_t st) {
    if (!pred || !target || !stats || !loss || !ws || B <= 0 || C <= 0 || HW <= 0 || target_dtype < 0 || target_dtype > 3)
        return UMI_ERR_BADARG;
    if (C > 8 || (long)B * C * HW >= (1L << 31) || B > 65535 || (C == 1 && target_dtype != 1)) return UMI_ERR_UNSUPPORTED;
    if (ws_bytes < umi_binloss_ws_bytes(B, C, HW)) return UMI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)st;
    if (C == 1) {
        const int nb = bin_blocks(HW);
        const bool vec = HW % 4 == 0 && host_aligned16(pred) && host_aligned16(target);
        hipLaunchKernelGGL(bin_stats_kernel, dim3(nb, B), dim3(THREADS), 0, s, pred, (const float*)target, HW, vec, (double*)ws);
        UMI_LAUNCH_CHECK();
        hipLaunchKernelGGL(stats_finalize_kernel, dim3(1), dim3(1024), 0, s, (const double*)ws, B, nb, BIN_COLS,
                           (int)LOSS_TVERSKY_BIN, (long)B * HW, alpha, beta, stats, loss);
        UMI_LAUNCH_CHECK();
        return UMI_OK;
    }
    const long total = (long)B * HW;
    const int rows = mc_blocks(total);
#define GO(NC) hipLaunchKernelGGL(mc_stats_kernel<NC>, dim3(rows), dim3(THREADS), 0, s, pred, target, target_dtype, HW, total, (double*)ws)
    switch (C) { case 2: GO(2); break; case 3: GO(3); break; case 4: GO(4); break; case 5: GO(5); break;
                 case 6: GO(6); break; case 7: GO(7); break; default: GO(8); }
#undef GO
    UMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(stats_finalize_kernel, dim3(1), dim3(1024), 0, s, (const double*)ws, 1, rows, 3 * C,
                       (int)LOSS_TVERSKY_MC, total, alpha, beta, stats, loss);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_tversky_bwd(const float* pred, const void* target, int target_dtype, const double* stats, const float* gout,
                               int B, int C, long HW, float alpha, float beta, float* dpred, umi_stream_t st) {
    if (!pred || !target || !stats || !dpred || B <= 0 || C <= 0 || HW <= 0 || target_dtype < 0 || target_dtype > 3)
        return UMI_ERR_BADARG;
    if (C > 8 || (long)B * C * HW >= (1L << 31) || B > 65535 || (C == 1 && target_dtype != 1)) return UMI_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)st;
    if (C == 1) {
        const bool vec = HW % 4 == 0 && host_aligned16(pred) && host_aligned16(target) && host_aligned16(dpred);
        hipLaunchKernelGGL(bin_bwd_kernel, dim3(bin_blocks(HW), B), dim3(THREADS), 0, s, pred, (const float*)target, stats, gout,
                           (int)LOSS_TVERSKY_BIN, HW, vec, alpha, beta, dpred);
        UMI_LAUNCH_CHECK();
        return UMI_OK;
    }
    const long total = (long)B * HW;
    const int grid = mc_blocks(total);
#define GO(NC) hipLaunchKernelGGL(mc_bwd_kernel<NC>, dim3(grid), dim3(THREADS), 0, s, pred, target, target_dtype, stats, gout, HW, total, alpha, beta, dpred)
    switch (C) { case 2: GO(2); break; case 3: GO(3); break; case 4: GO(4); break; case 5: GO(5); break;
                 case 6: GO(6); break; case 7: GO(7); break; default: GO(8); }
#undef GO
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" size_t umi_topk_loss_ws_bytes(long N) {
    if (N <= 0) return 0;
    long chunk;
    int nblk;
    sel_grid(N, &chunk, &nblk);
    return SEL_HEAD + align256((size_t)nblk * 256 * sizeof(unsigned)) + align256((size_t)nblk * sizeof(unsigned)) +
           (size_t)nblk * sizeof(double);
}

extern "C" int umi_topk_loss_fwd(const float* pred, const float* target, long N, long k, int mode, unsigned char* mask,
                                 float* loss, void* ws, size_t ws_bytes, umi_stream_t st) {
    if (!pred || !target || !mask || !loss || !ws || N <= 0 || k <= 0 || (mode != SEL_TOPK && mode != SEL_BCE_HEM))
        return UMI_ERR_BADARG;
    if (N >= (1L << 31) || k > N) return UMI_ERR_UNSUPPORTED;
    if (ws_bytes < umi_topk_loss_ws_bytes(N)) return UMI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)st;
    long chunk;
    int nblk;
    sel_grid(N, &chunk, &nblk);
    char* w = (char*)ws;
    unsigned* hist = (unsigned*)w;                                      // [4][256], zeroed each call
    SelState* state = (SelState*)(w + 4 * 256 * sizeof(unsigned));
    unsigned* rows = (unsigned*)(w + SEL_HEAD);
    unsigned* tie_off = (unsigned*)((char*)rows + align256((size_t)nblk * 256 * sizeof(unsigned)));
    double* part = (double*)((char*)tie_off + align256((size_t)nblk * sizeof(unsigned)));
    const bool vec = host_aligned16(pred) && host_aligned16(target) && ((uintptr_t)mask & 3) == 0;
    hipError_t e = hipMemsetAsync(hist, 0, 4 * 256 * sizeof(unsigned), s);
    if (e != hipSuccess) return (int)e;
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(sel_hist_kernel, dim3(nblk), dim3(THREADS), 0, s, pred, target, N, chunk, mode, pass, vec,
                           (const SelState*)state, hist + pass * 256, pass == 3 ? rows : (unsigned*)nullptr);
        UMI_LAUNCH_CHECK();
        hipLaunchKernelGGL(sel_pick_kernel, dim3(1), dim3(1024), 0, s, (const unsigned*)(hist + pass * 256), pass, (unsigned)k,
                           state, (const unsigned*)rows, nblk, tie_off);
        UMI_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sel_sum_kernel, dim3(nblk), dim3(THREADS), 0, s, pred, target, N, chunk, mode, vec,
                       (const SelState*)state, (const unsigned*)tie_off, mask, part);
    UMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(sum_finalize_kernel, dim3(1), dim3(1024), 0, s, (const double*)part, (long)nblk, (double)k, loss);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_topk_loss_bwd(const float* pred, const float* target, const unsigned char* mask, const float* gout, long N,
                                 long k, float* dpred, umi_stream_t st) {
    if (!pred || !target || !mask || !dpred || N <= 0 || k <= 0) return UMI_ERR_BADARG;
    if (N >= (1L << 31) || k > N) return UMI_ERR_UNSUPPORTED;
    const bool vec = host_aligned16(pred) && host_aligned16(target) && host_aligned16(dpred) && ((uintptr_t)mask & 3) == 0;
    const long n4 = vec ? N / 4 : 0;
    long grid = (N / 4 + THREADS - 1) / THREADS;
    grid = grid < 1 ? 1 : (grid > 2048 ? 2048 : grid);
    hipLaunchKernelGGL(sel_bwd_kernel, dim3((unsigned)grid), dim3(THREADS), 0, (hipStream_t)st, pred, target, mask, gout, N, n4,
                       (float)k, dpred);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
