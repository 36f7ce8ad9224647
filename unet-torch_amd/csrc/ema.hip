// Exponential moving average of the weights (include/unetmi.h, umi_ema_*): the state machine of one update (umi_ema_pre), the
// update of every shadow of a umi_optim_desc table in one launch (umi_ema_multi) and the exchange of parameters and shadows
// (umi_ema_swap_multi).
//
// The layout is the optimizer's: a workgroup owns one block of umi_optim_block_elems() elements of ONE tensor, found by binary
// search over blk0.  A block starts a multiple of 4,096 elements into its tensor, so every block of a tensor sees the tensor's
// own offsets into a 16-byte line.  Where `p` and `s0` share that offset the block is walked as
//   head  the (at most three) elements in front of the first 16-byte boundary, one per lane
//   body  16 bytes per lane; a whole block of an aligned tensor issues its four loads of p and of s0 together
//   tail  the (at most three) elements behind the last whole quad, one per lane
// and where they do not, one element per lane.  Exactly n elements of s0 (swap: and of p) are written.
//
//   e <- e + w_f * (p - e) is three fp32 roundings: contraction is off in this file (#pragma clang fp contract(off) below), so
//   no multiply-add is fused.  The NumPy float32 statement has none, and the shadows are promised to equal it bit for bit.
//
// Cache policy (UMI_EMA_POLICY; tools/bench_ema.py measured all three, DESIGN.md and profiles/ema.json have the figures):
// 0 = default loads and stores, 1 = every 16-byte access non-temporal as in snapshot.hip (kept: fastest on cold buffers, on the
// swap and behind TransUNet's optimizer step; 3 us behind policy 2 behind UNet(1,2,64)'s step), 2 = `p` by default loads (the
// optimizer has just written it), the shadow non-temporal.  The default policy (0) lost everywhere, by 9-64 %.
// No atomics, no static device memory; every store is a vector store.
#include "common.h"

#pragma clang fp contract(off)

#ifndef UMI_EMA_POLICY
#define UMI_EMA_POLICY 1
#endif

namespace {

constexpr int EMA_BLOCK = 4096;      // = umi_optim_block_elems(), checked by the entry points
constexpr int EMA_THREADS = 256;
constexpr int EMA_QUADS = EMA_BLOCK / (4 * EMA_THREADS);

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <bool NT> __device__ __forceinline__ f32x4 load4(const float* p) {
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return *reinterpret_cast<const f32x4*>(p);
}
template <bool NT> __device__ __forceinline__ void store4(float* p, const f32x4 v) {
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
    else *reinterpret_cast<f32x4*>(p) = v;
}
constexpr bool NT_P = UMI_EMA_POLICY == 1;                             // loads of the live parameter
constexpr bool NT_E = UMI_EMA_POLICY != 0;                             // loads and stores of the shadow (swap: and stores of p)

__device__ inline int find_desc(const umi_optim_desc* d, int n, int blk) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (d[mid].blk0 <= blk) lo = mid; else hi = mid - 1;       // of equal blk0 (empty tensors) the last one owns the block
    }
    return lo;
}

// Plain operators under the file's contract(off): the operations carry no `contract` flag, so the backend cannot fuse them.
// (HIP's __fmul_rn / __fadd_rn are inline `x * y` / `x + y` compiled under the HEADER's contraction mode and did fuse here.)
__device__ __forceinline__ float ema1(float e, float p, float w) {
    const float d = p - e;
    const float s = w * d;
    return e + s;
}
__device__ __forceinline__ f32x4 ema4(const f32x4 e, const f32x4 p, float w) {
    f32x4 r;
    r.x = ema1(e.x, p.x, w); r.y = ema1(e.y, p.y, w); r.z = ema1(e.z, p.z, w); r.w = ema1(e.w, p.w, w);
    return r;
}

// The walk of one block: [0, head) and [head + 4 * nq, cnt) one element per lane, nq quads in between
struct Walk {
    int cnt, head, nq;
};
__device__ __forceinline__ Walk walk_of(const float* p, const float* e, long left) {
    Walk w;
    w.cnt = left < EMA_BLOCK ? (int)left : EMA_BLOCK;
    const unsigned ap = (unsigned)((uintptr_t)p & 15), ae = (unsigned)((uintptr_t)e & 15);
    if (ap == ae) {
        const int h = (int)(((16u - ap) & 15u) >> 2);
        w.head = h < w.cnt ? h : w.cnt;
        w.nq = (w.cnt - w.head) >> 2;
    } else {
        w.head = w.cnt;
        w.nq = 0;
    }
    return w;
}

__global__ void ema_pre_kernel(double* __restrict__ st, const double* __restrict__ guard) {
    if (guard && guard[UMI_GUARD_SKIP] != 0.0) {        // a skipped optimizer step: the average does not move, t does not advance
        st[UMI_EMA_ACTIVE] = 0.0;
        return;
    }
    const double t = st[UMI_EMA_UPDATES];
    double d = st[UMI_EMA_DECAY];
    if (st[UMI_EMA_WARMUP] != 0.0) {
        const double w = (1.0 + t) / (10.0 + t);
        if (w < d) d = w;
    }
    st[UMI_EMA_LAST] = d;
    st[UMI_EMA_WEIGHT] = (double)(float)(1.0 - d);
    st[UMI_EMA_ACTIVE] = 1.0;
    st[UMI_EMA_UPDATES] = t + 1.0;
}

__global__ __launch_bounds__(EMA_THREADS) void ema_multi_kernel(const umi_optim_desc* __restrict__ descs, int n_desc,
                                                                const double* __restrict__ state) {
    if (state[UMI_EMA_ACTIVE] == 0.0) return;
    const float wf = (float)state[UMI_EMA_WEIGHT];
    const int blk = blockIdx.x;
    const umi_optim_desc d = descs[find_desc(descs, n_desc, blk)];
    const long base = (long)(blk - d.blk0) * EMA_BLOCK;
    const float* __restrict__ p = d.p + base;
    float* __restrict__ e = d.s0 + base;
    const Walk w = walk_of(p, e, d.n - base);
    if (w.head == 0 && w.cnt == EMA_BLOCK) {        // a full block of an aligned tensor: all eight loads of a lane in flight together
        f32x4 pv[EMA_QUADS], ev[EMA_QUADS];
#pragma unroll
        for (int j = 0; j < EMA_QUADS; ++j) {
            pv[j] = load4<NT_P>(p + threadIdx.x * 4 + 4 * EMA_THREADS * j);
            ev[j] = load4<NT_E>(e + threadIdx.x * 4 + 4 * EMA_THREADS * j);
        }
#pragma unroll
        for (int j = 0; j < EMA_QUADS; ++j) store4<NT_E>(e + threadIdx.x * 4 + 4 * EMA_THREADS * j, ema4(ev[j], pv[j], wf));
        return;
    }
    for (int i = threadIdx.x; i < w.head; i += EMA_THREADS) e[i] = ema1(e[i], p[i], wf);
    for (int q = threadIdx.x; q < w.nq; q += EMA_THREADS) {
        const int i = w.head + 4 * q;
        store4<NT_E>(e + i, ema4(load4<NT_E>(e + i), load4<NT_P>(p + i), wf));
    }
    for (int i = w.head + 4 * w.nq + threadIdx.x; i < w.cnt; i += EMA_THREADS) e[i] = ema1(e[i], p[i], wf);
}

__global__ __launch_bounds__(EMA_THREADS) void ema_swap_kernel(const umi_optim_desc* __restrict__ descs, int n_desc) {
    const int blk = blockIdx.x;
    const umi_optim_desc d = descs[find_desc(descs, n_desc, blk)];
    const long base = (long)(blk - d.blk0) * EMA_BLOCK;
    float* __restrict__ p = d.p + base;              // words are moved, never computed on: NaN payloads and denormals keep their bits
    float* __restrict__ e = d.s0 + base;
    const Walk w = walk_of(p, e, d.n - base);
    if (w.head == 0 && w.cnt == EMA_BLOCK) {
        f32x4 pv[EMA_QUADS], ev[EMA_QUADS];
#pragma unroll
        for (int j = 0; j < EMA_QUADS; ++j) {
            pv[j] = load4<NT_P>(p + threadIdx.x * 4 + 4 * EMA_THREADS * j);
            ev[j] = load4<NT_E>(e + threadIdx.x * 4 + 4 * EMA_THREADS * j);
        }
#pragma unroll
        for (int j = 0; j < EMA_QUADS; ++j) {
            store4<NT_E>(e + threadIdx.x * 4 + 4 * EMA_THREADS * j, pv[j]);
            store4<NT_E>(p + threadIdx.x * 4 + 4 * EMA_THREADS * j, ev[j]);
        }
        return;
    }
    unsigned* __restrict__ pw = reinterpret_cast<unsigned*>(p);
    unsigned* __restrict__ ew = reinterpret_cast<unsigned*>(e);
    for (int i = threadIdx.x; i < w.head; i += EMA_THREADS) { const unsigned a = pw[i], b = ew[i]; pw[i] = b; ew[i] = a; }
    for (int q = threadIdx.x; q < w.nq; q += EMA_THREADS) {
        const int i = w.head + 4 * q;
        const f32x4 a = load4<NT_P>(p + i), b = load4<NT_E>(e + i);
        store4<NT_E>(p + i, b);
        store4<NT_E>(e + i, a);
    }
    for (int i = w.head + 4 * w.nq + threadIdx.x; i < w.cnt; i += EMA_THREADS) { const unsigned a = pw[i], b = ew[i]; pw[i] = b; ew[i] = a; }
}

int table_status(const void* descs, int n_desc, int total_blocks) {
    if (n_desc < 0 || total_blocks < 0) return UMI_ERR_BADARG;
    if (n_desc > 0 && !descs) return UMI_ERR_BADARG;
    if (total_blocks > 0 && n_desc == 0) return UMI_ERR_BADARG;
    if (umi_optim_block_elems() != EMA_BLOCK) return UMI_ERR_UNSUPPORTED;
    return UMI_OK;
}

}  // namespace

extern "C" int umi_ema_pre(double* state, const double* guard, umi_stream_t stream) {
    if (!state || (((uintptr_t)state | (uintptr_t)guard) & 7)) return UMI_ERR_BADARG;
    hipLaunchKernelGGL(ema_pre_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, guard);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_ema_multi(const void* descs, int n_desc, int total_blocks, const double* state, umi_stream_t stream) {
    if (!state || ((uintptr_t)state & 7)) return UMI_ERR_BADARG;
    const int st = table_status(descs, n_desc, total_blocks);
    if (st != UMI_OK) return st;
    if (n_desc == 0 || total_blocks == 0) return UMI_OK;
    hipLaunchKernelGGL(ema_multi_kernel, dim3(total_blocks), dim3(EMA_THREADS), 0, (hipStream_t)stream,
                       (const umi_optim_desc*)descs, n_desc, state);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_ema_swap_multi(const void* descs, int n_desc, int total_blocks, umi_stream_t stream) {
    const int st = table_status(descs, n_desc, total_blocks);
    if (st != UMI_OK) return st;
    if (n_desc == 0 || total_blocks == 0) return UMI_OK;
    hipLaunchKernelGGL(ema_swap_kernel, dim3(total_blocks), dim3(EMA_THREADS), 0, (hipStream_t)stream,
                       (const umi_optim_desc*)descs, n_desc);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
