// Gradient accumulation over the micro-batches of one optimizer step (include/unetmi.h, umi_grad_accum_*): the state machine of
// one call (umi_grad_accum_pre) and the pass over every gradient of a umi_optim_desc table in one launch (umi_grad_accum_multi).
//
// The layout is the optimizer's and the walk is csrc/ema.hip's: a workgroup owns one block of umi_optim_block_elems() elements of
// ONE tensor, found by binary search over blk0.  A block starts a multiple of 4,096 elements into its tensor, so every block of a
// tensor sees the tensor's own offsets into a 16-byte line.  Where `g` and `s0` share that offset the block is walked as
//   head  the (at most three) elements in front of the first 16-byte boundary, one per lane
//   body  16 bytes per lane; a whole block of an aligned tensor issues its four loads of g and of s0 together
//   tail  the (at most three) elements behind the last whole quad, one per lane
// and where they do not, one element per lane.  Exactly n elements of the pass's destination are written.
//
// What a call does is decided by the device block, not by a kernel argument (one captured micro-step graph serves every
// non-final position of a window):
//   FIRST, not LAST   s0 <- g         words are moved; s0 is NOT read, so nobody ever has to zero the accumulator
//   neither           s0 <- s0 + g    one fp32 rounding; g is not written
//   FIRST and LAST    nothing         returns before any access: g keeps its bits, NaN payloads included
//   LAST, not FIRST   g  <- (s0 + g) * s,  s = (float)SCALE: two fp32 roundings (contraction is off in this file, so no
//                     multiply-add is fused); s0 is not written.  This pass writes through the desc's `const float* g`.
//
// Cache policy (UMI_ACCUM_POLICY): 0 = default loads and stores, 1 = every 16-byte access non-temporal, as in ema.hip and
// snapshot.hip (kept: the gradients and the accumulator are each touched once per micro-batch and are not read again before a whole
// forward and backward pass has gone through the caches).
// No atomics, no static device memory; every store is a vector store.
#include "common.h"

#pragma clang fp contract(off)

#ifndef UMI_ACCUM_POLICY
#define UMI_ACCUM_POLICY 1
#endif

namespace {

constexpr int ACC_BLOCK = 4096;      // = umi_optim_block_elems(), checked by the entry point
constexpr int ACC_THREADS = 256;
constexpr int ACC_QUADS = ACC_BLOCK / (4 * ACC_THREADS);
constexpr bool NT = UMI_ACCUM_POLICY == 1;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

enum { MODE_FIRST = 0, MODE_ADD = 1, MODE_LAST = 2 };

__device__ __forceinline__ f32x4 load4(const float* p) {
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return *reinterpret_cast<const f32x4*>(p);
}
__device__ __forceinline__ void store4(float* p, const f32x4 v) {
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
    else *reinterpret_cast<f32x4*>(p) = v;
}
// the same 16 bytes as words: the FIRST pass moves them and computes nothing (a float move may quiet a signalling NaN)
__device__ __forceinline__ u32x4 load4w(const float* p) {
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    return *reinterpret_cast<const u32x4*>(p);
}
__device__ __forceinline__ void store4w(float* p, const u32x4 v) {
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
    else *reinterpret_cast<u32x4*>(p) = v;
}

__device__ inline int find_desc(const umi_optim_desc* d, int n, int blk) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (d[mid].blk0 <= blk) lo = mid; else hi = mid - 1;       // of equal blk0 (empty tensors) the last one owns the block
    }
    return lo;
}

// Plain operators under the file's contract(off): no `contract` flag, so the backend cannot fuse the add into the multiply.
__device__ __forceinline__ float mean1(float a, float g, float s) {
    const float t = a + g;
    return t * s;
}
__device__ __forceinline__ f32x4 add4(const f32x4 a, const f32x4 g) {
    f32x4 r;
    r.x = a.x + g.x; r.y = a.y + g.y; r.z = a.z + g.z; r.w = a.w + g.w;
    return r;
}
__device__ __forceinline__ f32x4 mean4(const f32x4 a, const f32x4 g, float s) {
    f32x4 r;
    r.x = mean1(a.x, g.x, s); r.y = mean1(a.y, g.y, s); r.z = mean1(a.z, g.z, s); r.w = mean1(a.w, g.w, s);
    return r;
}

// The walk of one block: [0, head) and [head + 4 * nq, cnt) one element per lane, nq quads in between
struct Walk {
    int cnt, head, nq;
};
__device__ __forceinline__ Walk walk_of(const float* g, const float* a, long left) {
    Walk w;
    w.cnt = left < ACC_BLOCK ? (int)left : ACC_BLOCK;
    const unsigned ag = (unsigned)((uintptr_t)g & 15), aa = (unsigned)((uintptr_t)a & 15);
    if (ag == aa) {
        const int h = (int)(((16u - ag) & 15u) >> 2);
        w.head = h < w.cnt ? h : w.cnt;
        w.nq = (w.cnt - w.head) >> 2;
    } else {
        w.head = w.cnt;
        w.nq = 0;
    }
    return w;
}

__global__ void accum_pre_kernel(double* __restrict__ st, int last) {
    const double j = st[UMI_ACCUM_COUNT];
    st[UMI_ACCUM_FIRST] = j == 0.0 ? 1.0 : 0.0;
    st[UMI_ACCUM_LAST] = last ? 1.0 : 0.0;
    st[UMI_ACCUM_SCALE] = (double)(float)(1.0 / (j + 1.0));
    st[UMI_ACCUM_COUNT] = last ? 0.0 : j + 1.0;
    st[UMI_ACCUM_MICRO] += 1.0;
    st[UMI_ACCUM_WINDOWS] += last ? 1.0 : 0.0;
}

// one element: `g` and `a` of the block, s the fp32 factor of the LAST pass
template <int MODE> __device__ __forceinline__ void one(float* __restrict__ g, float* __restrict__ a, int i, float s) {
    if (MODE == MODE_FIRST) reinterpret_cast<unsigned*>(a)[i] = reinterpret_cast<const unsigned*>(g)[i];
    else if (MODE == MODE_ADD) a[i] = a[i] + g[i];
    else g[i] = mean1(a[i], g[i], s);
}

template <int MODE> __device__ __forceinline__ void walk_block(float* __restrict__ g, float* __restrict__ a, const Walk w, float s) {
    if (w.head == 0 && w.cnt == ACC_BLOCK) {        // a full block of an aligned tensor: all loads of a lane in flight together
        const int t4 = threadIdx.x * 4;
        if (MODE == MODE_FIRST) {
            u32x4 gv[ACC_QUADS];
#pragma unroll
            for (int j = 0; j < ACC_QUADS; ++j) gv[j] = load4w(g + t4 + 4 * ACC_THREADS * j);
#pragma unroll
            for (int j = 0; j < ACC_QUADS; ++j) store4w(a + t4 + 4 * ACC_THREADS * j, gv[j]);
        } else {
            f32x4 gv[ACC_QUADS], av[ACC_QUADS];
#pragma unroll
            for (int j = 0; j < ACC_QUADS; ++j) {
                gv[j] = load4(g + t4 + 4 * ACC_THREADS * j);
                av[j] = load4(a + t4 + 4 * ACC_THREADS * j);
            }
#pragma unroll
            for (int j = 0; j < ACC_QUADS; ++j) {
                if (MODE == MODE_ADD) store4(a + t4 + 4 * ACC_THREADS * j, add4(av[j], gv[j]));
                else store4(g + t4 + 4 * ACC_THREADS * j, mean4(av[j], gv[j], s));
            }
        }
        return;
    }
    for (int i = threadIdx.x; i < w.head; i += ACC_THREADS) one<MODE>(g, a, i, s);
    for (int q = threadIdx.x; q < w.nq; q += ACC_THREADS) {
        const int i = w.head + 4 * q;
        if (MODE == MODE_FIRST) store4w(a + i, load4w(g + i));
        else if (MODE == MODE_ADD) store4(a + i, add4(load4(a + i), load4(g + i)));
        else store4(g + i, mean4(load4(a + i), load4(g + i), s));
    }
    for (int i = w.head + 4 * w.nq + threadIdx.x; i < w.cnt; i += ACC_THREADS) one<MODE>(g, a, i, s);
}

__global__ __launch_bounds__(ACC_THREADS) void accum_multi_kernel(const umi_optim_desc* __restrict__ descs, int n_desc,
                                                                  const double* __restrict__ state) {
    const bool first = state[UMI_ACCUM_FIRST] != 0.0, last = state[UMI_ACCUM_LAST] != 0.0;
    if (first && last) return;                       // a window of one: the gradient is already the mean
    const float s = (float)state[UMI_ACCUM_SCALE];
    const int blk = blockIdx.x;
    const umi_optim_desc d = descs[find_desc(descs, n_desc, blk)];
    const long base = (long)(blk - d.blk0) * ACC_BLOCK;
    float* g = const_cast<float*>(d.g) + base;       // written by the LAST pass alone
    float* a = d.s0 + base;
    const Walk w = walk_of(g, a, d.n - base);
    if (first) walk_block<MODE_FIRST>(g, a, w, s);
    else if (!last) walk_block<MODE_ADD>(g, a, w, s);
    else walk_block<MODE_LAST>(g, a, w, s);
}

}  // namespace

extern "C" int umi_grad_accum_pre(double* state, int last, umi_stream_t stream) {
    if (!state || ((uintptr_t)state & 7)) return UMI_ERR_BADARG;
    hipLaunchKernelGGL(accum_pre_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, last);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_grad_accum_multi(const void* descs, int n_desc, int total_blocks, const double* state, umi_stream_t stream) {
    if (!state || ((uintptr_t)state & 7)) return UMI_ERR_BADARG;
    if (n_desc < 0 || total_blocks < 0) return UMI_ERR_BADARG;
    if (n_desc > 0 && !descs) return UMI_ERR_BADARG;
    if (total_blocks > 0 && n_desc == 0) return UMI_ERR_BADARG;
    if (umi_optim_block_elems() != ACC_BLOCK) return UMI_ERR_UNSUPPORTED;
    if (n_desc == 0 || total_blocks == 0) return UMI_OK;
    hipLaunchKernelGGL(accum_multi_kernel, dim3(total_blocks), dim3(ACC_THREADS), 0, (hipStream_t)stream,
                       (const umi_optim_desc*)descs, n_desc, state);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
