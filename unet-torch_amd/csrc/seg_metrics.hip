// Hard-mask segmentation metrics: logits (or a uint8 class mask) and labels -> an exact integer confusion matrix per item ->
// Dice / IoU / pixel error (statement: umi/metrics.py confusion_numpy, scores_numpy).
//
//   counting   one streaming pass, every byte read once: per lane 4 consecutive pixels = one 16-byte load per channel plane (the
//              rule and the loads of argmax_mask_kernel / binary_mask_kernel), scalar loads when HW % 4 != 0 or a pointer is not
//              aligned for the vector form.  The prediction never reaches memory.
//              key = row * (K+1) + col.  Real validation data puts most pixels of a wave in one bin, so same-key contention is the
//              common case and one LDS atomic per lane would serialise.  Per round the wave takes the first lane's key, counts the
//              lanes that share it with a ballot + popcount and keeps that count in scalar registers until another key leads a
//              round (a run of one bin touches no LDS); only the lanes with OTHER keys -- class boundaries, or labels spread over
//              many bins, where contention is low by construction -- add 1 each to the wave's own LDS row with an atomic that
//              returns nothing.
//              The four wave rows are added into the block's int32 row of `ws` (a block sees fewer than 2^31 pixels, so a uint32
//              cannot wrap); EVERY entry of the row is stored, so `ws` needs no presetting.
//   finalize   one workgroup per item sums that item's rows in int64 and stores all (K+1)^2 entries of counts[item].
//   scores     one thread per item, float64 in the stated order without contraction, one rounding to fp32.
// No global atomics (the LDS ones stay inside a wave's row), no allocation, nothing read back: integer sums are exact in any
// order, and the calls can be captured.
#include "common.h"

namespace {

constexpr int CM_MAXK = 8;
constexpr int CM_MAXKEYS = (CM_MAXK + 1) * (CM_MAXK + 1);      // 81
constexpr int CM_MAXROWS = 256;                                // blocks (partial rows) per item
constexpr unsigned CM_CUTOFF_BITS = 0xB43FFFFEu;               // umi_binary_mask's threshold: fp32 sigmoid(x) >= 0.5 from here on
constexpr double CM_EPS = 1e-5;

enum { CM_LOGITS = 0, CM_BINARY = 1, CM_MASK = 2 };

// the row of a label: its class, or K ("not a class") for an integer outside 0..K-1 / a float that is not exactly one of 0.0..K-1
__device__ __forceinline__ int cm_row_ll(long long v, int K) { return (unsigned long long)v < (unsigned long long)K ? (int)v : K; }
__device__ __forceinline__ int cm_row_f(float f, int K) {
    int r = K;
    if (f >= 0.f && f < (float)K) {                            // NaN fails both
        const int i = (int)f;
        if ((float)i == f) r = i;
    }
    return r;
}
__device__ __forceinline__ int cm_row(const void* t, int tdtype, long i, int K) {
    if (tdtype == 0) return cm_row_ll(reinterpret_cast<const long long*>(t)[i], K);
    if (tdtype == 1) return cm_row_f(reinterpret_cast<const float*>(t)[i], K);
    if (tdtype == 2) return cm_row_ll((long long)reinterpret_cast<const unsigned char*>(t)[i], K);
    return cm_row_ll((long long)reinterpret_cast<const int*>(t)[i], K);
}
// the rows of 4 consecutive labels starting at element i (i % 4 == 0 and the base aligned for these loads: the caller's `vec`)
__device__ __forceinline__ void cm_row4(const void* t, int tdtype, long i, int K, int r[4]) {
    if (tdtype == 0) {
        const longlong2 a = reinterpret_cast<const longlong2*>(reinterpret_cast<const long long*>(t) + i)[0];
        const longlong2 b = reinterpret_cast<const longlong2*>(reinterpret_cast<const long long*>(t) + i)[1];
        r[0] = cm_row_ll(a.x, K); r[1] = cm_row_ll(a.y, K); r[2] = cm_row_ll(b.x, K); r[3] = cm_row_ll(b.y, K);
    } else if (tdtype == 1) {
        const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(t) + i);
        r[0] = cm_row_f(a.x, K); r[1] = cm_row_f(a.y, K); r[2] = cm_row_f(a.z, K); r[3] = cm_row_f(a.w, K);
    } else if (tdtype == 2) {
        const uchar4 a = *reinterpret_cast<const uchar4*>(reinterpret_cast<const unsigned char*>(t) + i);
        r[0] = cm_row_ll(a.x, K); r[1] = cm_row_ll(a.y, K); r[2] = cm_row_ll(a.z, K); r[3] = cm_row_ll(a.w, K);
    } else {
        const int4 a = *reinterpret_cast<const int4*>(reinterpret_cast<const int*>(t) + i);
        r[0] = cm_row_ll(a.x, K); r[1] = cm_row_ll(a.y, K); r[2] = cm_row_ll(a.z, K); r[3] = cm_row_ll(a.w, K);
    }
}

// One round of counting: every lane of the wave calls this (in uniform control flow) with its key and whether it holds a pixel.
// `row`: the wave's own LDS counters.  The lanes that share the first pending lane's key are counted by a ballot, and their count
// stays in the wave-uniform pair `acc` (scalar registers) until another key leads a round: a run of one bin -- the common case --
// touches no LDS at all.  The remaining lanes (a class boundary, or labels spread over many bins, where same-address contention
// is low by construction) add 1 each with an LDS atomic that returns nothing, so nothing waits for it.
struct CmAcc { int k; unsigned n; };
__device__ __forceinline__ void cm_flush(unsigned* row, const CmAcc& acc, int lane) {
    if (lane == 0 && acc.n) atomicAdd(&row[acc.k], acc.n);
}
__device__ __forceinline__ void cm_count(unsigned* row, CmAcc& acc, int key, bool valid, int lane) {
    const unsigned long long todo = __ballot(valid);           // wave-uniform
    if (!todo) return;
    const int first = __ffsll((long long)todo) - 1;
    const int k = __builtin_amdgcn_readlane(key, first);
    const unsigned long long same = __ballot(valid && key == k);
    if (k != acc.k) {
        cm_flush(row, acc, lane);
        acc.k = k;
        acc.n = 0u;
    }
    acc.n += (unsigned)__popcll(same);
    if (valid && key != k) atomicAdd(&row[key], 1u);
}

// blockIdx.y = item, blockIdx.x of gridDim.x = the block (partial row) inside the item.  `src`: fp32 logits [items*n][NC][HW]
// (CM_LOGITS: argmax over NC >= 2 planes, first strict maximum wins, a NaN never wins; CM_BINARY: one plane, 1 where
// x >= the cutoff, NaN gives 0) or a uint8 mask [items*n][HW] (CM_MASK: values >= K fall in column K).
// part: [items][gridDim.x][(K+1)^2] uint32.
template <int MODE, int NC>
__global__ __launch_bounds__(256) void confusion_count_kernel(const void* __restrict__ src, const void* __restrict__ target, int tdtype,
                                                              long HW, long total, int K, int vec, unsigned* __restrict__ part) {
    __shared__ unsigned cnt[4][CM_MAXKEYS];
    const int K1 = K + 1, KK = K1 * K1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < 4 * CM_MAXKEYS; i += 256) (&cnt[0][0])[i] = 0u;
    __syncthreads();
    const long item = blockIdx.y;
    const int planes = MODE == CM_MASK ? 1 : NC;
    const float* x = reinterpret_cast<const float*>(src) + item * total * planes;
    const unsigned char* m = reinterpret_cast<const unsigned char*>(src) + item * total;
    const long tb = tdtype == 0 ? 8 : (tdtype == 2 ? 1 : 4);
    const void* t = reinterpret_cast<const char*>(target) + item * total * tb;
    const float cut = __builtin_bit_cast(float, CM_CUTOFF_BITS);
    unsigned* row = cnt[wave];
    CmAcc acc = {0, 0u};

    if (vec) {                                                 // HW % 4 == 0: a group of 4 pixels never leaves its image
        const long units = total >> 2;
        for (long base = (long)blockIdx.x * 256; base < units; base += (long)gridDim.x * 256) {
            const long u = base + threadIdx.x;
            const bool valid = u < units;
            int key[4] = {0, 0, 0, 0};
            if (valid) {
                const long i = u << 2;
                int r[4], c[4] = {0, 0, 0, 0};
                cm_row4(t, tdtype, i, K, r);
                if (MODE == CM_MASK) {
                    const uchar4 v = *reinterpret_cast<const uchar4*>(m + i);
                    c[0] = v.x < K ? v.x : K; c[1] = v.y < K ? v.y : K; c[2] = v.z < K ? v.z : K; c[3] = v.w < K ? v.w : K;
                } else if (MODE == CM_BINARY) {
                    const float4 v = *reinterpret_cast<const float4*>(x + i);
                    c[0] = v.x >= cut; c[1] = v.y >= cut; c[2] = v.z >= cut; c[3] = v.w >= cut;
                } else {
                    const long img = i / HW, hw = i - img * HW;
                    const float* p = x + img * NC * HW + hw;
                    float4 best = *reinterpret_cast<const float4*>(p);
#pragma unroll
                    for (int ch = 1; ch < NC; ++ch) {
                        const float4 v = *reinterpret_cast<const float4*>(p + (long)ch * HW);
                        if (v.x > best.x) { best.x = v.x; c[0] = ch; }
                        if (v.y > best.y) { best.y = v.y; c[1] = ch; }
                        if (v.z > best.z) { best.z = v.z; c[2] = ch; }
                        if (v.w > best.w) { best.w = v.w; c[3] = ch; }
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) key[j] = r[j] * K1 + c[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) cm_count(row, acc, key[j], valid, lane);
        }
    } else {
        for (long base = (long)blockIdx.x * 256; base < total; base += (long)gridDim.x * 256) {
            const long i = base + threadIdx.x;
            const bool valid = i < total;
            int key = 0;
            if (valid) {
                const int r = cm_row(t, tdtype, i, K);
                int c = 0;
                if (MODE == CM_MASK) {
                    c = m[i] < K ? m[i] : K;
                } else if (MODE == CM_BINARY) {
                    c = x[i] >= cut;
                } else {
                    const long img = i / HW, hw = i - img * HW;
                    const float* p = x + img * NC * HW + hw;
                    float best = p[0];
#pragma unroll
                    for (int ch = 1; ch < NC; ++ch) {
                        const float v = p[(long)ch * HW];
                        if (v > best) { best = v; c = ch; }
                    }
                }
                key = r * K1 + c;
            }
            cm_count(row, acc, key, valid, lane);
        }
    }
    cm_flush(row, acc, lane);
    __syncthreads();
    if ((int)threadIdx.x < KK)
        part[(item * gridDim.x + blockIdx.x) * KK + threadIdx.x] =
            cnt[0][threadIdx.x] + cnt[1][threadIdx.x] + cnt[2][threadIdx.x] + cnt[3][threadIdx.x];
}

// one workgroup per item: 8 row lanes x 128 columns; counts[item][key] = the int64 sum of the item's partial rows
__global__ __launch_bounds__(1024) void confusion_finalize_kernel(const unsigned* __restrict__ part, int rows, int KK,
                                                                  long long* __restrict__ counts) {
    __shared__ long long lanes[8][CM_MAXKEYS];
    const int col = threadIdx.x & 127, rl = threadIdx.x >> 7;
    part += (long)blockIdx.x * rows * KK;
    if (col < KK) {
        long long s = 0;
        for (int r = rl; r < rows; r += 8) s += (long long)part[(long)r * KK + col];
        lanes[rl][col] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < KK) {
        long long s = 0;
        for (int l = 0; l < 8; ++l) s += lanes[l][threadIdx.x];
        counts[(long)blockIdx.x * KK + threadIdx.x] = s;
    }
}

// one thread per item; the float64 statement of umi/metrics.py scores_numpy, operation for operation
__global__ __launch_bounds__(64) void confusion_scores_kernel(const long long* __restrict__ counts, int items, int K, int kind, int c0,
                                                              float* __restrict__ out) {
#pragma clang fp contract(off)
    const int it = blockIdx.x * 64 + threadIdx.x;
    if (it >= items) return;
    const int K1 = K + 1;
    const long long* m = counts + (long)it * K1 * K1;
    if (kind == 2) {
        long long inter = 0, labelled = 0;
        for (int c = 0; c < K; ++c) {
            inter += m[c * K1 + c];
            for (int j = 0; j < K1; ++j) labelled += m[c * K1 + j];
        }
        out[it] = (float)(1.0 - ((double)inter + CM_EPS) / ((double)labelled + CM_EPS));
        return;
    }
    double sum = 0.0;
    for (int c = c0; c < K; ++c) {
        long long z = 0, y = 0;
        for (int j = 0; j < K1; ++j) { z += m[j * K1 + c]; y += m[c * K1 + j]; }
        const double I = (double)m[c * K1 + c], Z = (double)z, Y = (double)y;
        if (kind == 0) sum += (2.0 * I + CM_EPS) / (Z + Y + CM_EPS);
        else sum += (I + CM_EPS) / (Z + Y - I + CM_EPS);
    }
    out[it] = (float)(1.0 - sum / (double)(K - c0));
}

int cm_rows(long total) {
    long b = (total + 4095) / 4096;                     // ~16 pixels (4 loads of 4) per thread
    return (int)(b < 1 ? 1 : (b > CM_MAXROWS ? CM_MAXROWS : b));
}

int cm_check(const void* src, const void* target, int tdtype, int items, int n, long HW, const void* counts) {
    if (!src || !target || !counts || items <= 0 || items > 65535 || n <= 0 || HW <= 0 || tdtype < 0 || tdtype > 3) return UMI_ERR_BADARG;
    const unsigned long tal = tdtype == 0 ? 7 : (tdtype == 2 ? 0 : 3);
    if (((unsigned long)target & tal) || ((unsigned long)counts & 7)) return UMI_ERR_BADARG;
    return UMI_OK;
}

// the vector form: whole groups of 4 pixels inside one image, 16-byte plane loads, 4 labels per load
bool cm_vec(const void* src, int src_elem, const void* target, int tdtype, long HW) {
    const unsigned long tal = tdtype == 0 ? 15 : (tdtype == 2 ? 3 : 15);
    return (HW & 3) == 0 && ((unsigned long)src & (src_elem == 4 ? 15 : 3)) == 0 && ((unsigned long)target & tal) == 0;
}

}  // namespace

extern "C" size_t umi_confusion_ws_bytes(int items, int n, int K, long HW) {
    if (items <= 0 || n <= 0 || HW <= 0 || K < 2 || K > CM_MAXK || (long)n * HW >= (1L << 31)) return 0;
    return (size_t)items * cm_rows((long)n * HW) * (K + 1) * (K + 1) * sizeof(unsigned);
}

extern "C" int umi_confusion_logits(const float* logits, const void* target, int target_dtype, int items, int n, int C, long HW,
                                    long long* counts, void* ws, size_t ws_bytes, umi_stream_t stream) {
    const int st = cm_check(logits, target, target_dtype, items, n, HW, counts);
    if (st) return st;
    if (!ws || ((unsigned long)logits & 3) || ((unsigned long)ws & 3)) return UMI_ERR_BADARG;
    if (C < 1 || C > CM_MAXK || (long)n * HW >= (1L << 31)) return UMI_ERR_UNSUPPORTED;
    const int K = C == 1 ? 2 : C;
    if (ws_bytes < umi_confusion_ws_bytes(items, n, K, HW)) return UMI_ERR_WORKSPACE;
    const long total = (long)n * HW;
    const int rows = cm_rows(total), vec = cm_vec(logits, 4, target, target_dtype, HW) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
#define GO(MODE, NC) hipLaunchKernelGGL((confusion_count_kernel<MODE, NC>), dim3(rows, items), dim3(256), 0, s, (const void*)logits, \
                                        target, target_dtype, HW, total, K, vec, (unsigned*)ws)
    switch (C) { case 1: GO(CM_BINARY, 1); break; case 2: GO(CM_LOGITS, 2); break; case 3: GO(CM_LOGITS, 3); break;
                 case 4: GO(CM_LOGITS, 4); break; case 5: GO(CM_LOGITS, 5); break; case 6: GO(CM_LOGITS, 6); break;
                 case 7: GO(CM_LOGITS, 7); break; default: GO(CM_LOGITS, 8); }
#undef GO
    UMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(confusion_finalize_kernel, dim3(items), dim3(1024), 0, s, (const unsigned*)ws, rows, (K + 1) * (K + 1), counts);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_confusion_masks(const unsigned char* mask, const void* target, int target_dtype, int items, int n, int K, long HW,
                                   long long* counts, void* ws, size_t ws_bytes, umi_stream_t stream) {
    const int st = cm_check(mask, target, target_dtype, items, n, HW, counts);
    if (st) return st;
    if (!ws || ((unsigned long)ws & 3)) return UMI_ERR_BADARG;
    if (K < 2 || K > CM_MAXK || (long)n * HW >= (1L << 31)) return UMI_ERR_UNSUPPORTED;
    if (ws_bytes < umi_confusion_ws_bytes(items, n, K, HW)) return UMI_ERR_WORKSPACE;
    const long total = (long)n * HW;
    const int rows = cm_rows(total), vec = cm_vec(mask, 1, target, target_dtype, HW) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((confusion_count_kernel<CM_MASK, 1>), dim3(rows, items), dim3(256), 0, s, (const void*)mask, target, target_dtype,
                       HW, total, K, vec, (unsigned*)ws);
    UMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(confusion_finalize_kernel, dim3(items), dim3(1024), 0, s, (const unsigned*)ws, rows, (K + 1) * (K + 1), counts);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_confusion_scores(const long long* counts, int items, int K, int kind, int c0, float* out, umi_stream_t stream) {
    if (!counts || !out || items <= 0 || kind < 0 || kind > 2) return UMI_ERR_BADARG;
    if (K < 2 || K > CM_MAXK) return UMI_ERR_UNSUPPORTED;
    if (c0 < 0 || c0 >= K) return UMI_ERR_BADARG;
    hipLaunchKernelGGL(confusion_scores_kernel, dim3((items + 63) / 64), dim3(64), 0, (hipStream_t)stream, counts, items, K, kind, c0,
                       out);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
