// State snapshot: every tensor of a umi_optim_desc table copied into one contiguous arena in ONE pass, with the replica
// fingerprint of the table (fingerprint_mix.h) formed from the words as they pass through registers (include/unetmi.h,
// umi_snapshot_multi), and the copy back (umi_restore_multi).
//
// The layout is the optimizer's and the fingerprint's: a workgroup owns one block of umi_optim_block_elems() words of ONE
// tensor, found by binary search over blk0.  Tensor t's slot `s0` is 16-byte aligned and 4 * ceil(n / 4) words long; a block
// starts a multiple of 4,096 words into it, so every arena access is a 16-byte one whatever the alignment of `p`.  The words
// between n and the end of the slot are written as zeros: the arena's bytes are a function of the tensors alone.
//   snapshot  p -> s0, block partial of H_t -> ws;  then fingerprint_finalize_kernel -> *out.  A full block of an aligned
//             tensor issues its four 16-byte loads together before the mixes and the stores.  The 16-byte loads and stores
//             are non-temporal (nothing is touched twice): 12 % faster than the default policy on UNet(1,2,64)'s 124 MB.
//   restore   s0 -> p, exactly n words: a misaligned `p` is written one word per lane, an aligned one 16 bytes per lane with
//             its last n % 4 words one per lane.
// No atomics; every store is a vector store.
#include "fingerprint_mix.h"

namespace {

// the tensors are read once and the arena is written once: streaming accesses
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 load_nt(const uint32_t* p) {
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void store_nt(uint32_t* p, const uint4 v) {
    u32x4 w;
    w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
    __builtin_nontemporal_store(w, reinterpret_cast<u32x4*>(p));
}

// words [q, q + 4) of a block of which `cnt` exist: loaded one by one, mixed, stored as one 16-byte quad with zeros past cnt
__device__ __forceinline__ u64 quad_by_words(const uint32_t* __restrict__ w, uint32_t* __restrict__ dst, int q, int cnt, u64 g0) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    const u64 g = g0 + G * (u64)q;
    u64 s = 0;
    v.x = w[q];
    s += mix(v.x + g);
    if (q + 1 < cnt) { v.y = w[q + 1]; s += mix(v.y + (g + G)); }
    if (q + 2 < cnt) { v.z = w[q + 2]; s += mix(v.z + (g + 2 * G)); }
    if (q + 3 < cnt) { v.w = w[q + 3]; s += mix(v.w + (g + 3 * G)); }
    *reinterpret_cast<uint4*>(dst + q) = v;
    return s;
}

__global__ __launch_bounds__(FP_THREADS) void snapshot_partials_kernel(const umi_optim_desc* __restrict__ descs, int n_desc,
                                                                       u64* __restrict__ ws) {
    __shared__ u64 sh[FP_THREADS / 32];
    const int blk = blockIdx.x;
    const umi_optim_desc d = descs[find_desc(descs, n_desc, blk)];
    const long base = (long)(blk - d.blk0) * FP_BLOCK;
    const long left = d.n - base;
    const int cnt = left < FP_BLOCK ? (int)left : FP_BLOCK;
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(d.p) + base;
    uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(d.s0) + base;
    const u64 g0 = G * (u64)(base + 1);                                // G * (i + 1) of the block's first word
    u64 s = 0;
    int tail = 0;                             // first word the word-by-word loop takes
    if (((uintptr_t)w & 15) == 0) {
        if (cnt == FP_BLOCK) {                // a full block: the four loads of a thread in flight together
            uint4 v[FP_QUADS];
#pragma unroll
            for (int j = 0; j < FP_QUADS; ++j)
                v[j] = load_nt(w + threadIdx.x * 4 + 4 * FP_THREADS * j);
#pragma unroll
            for (int j = 0; j < FP_QUADS; ++j) {
                s += four(v[j], g0 + G * (u64)(threadIdx.x * 4 + 4 * FP_THREADS * j));
                store_nt(dst + threadIdx.x * 4 + 4 * FP_THREADS * j, v[j]);
            }
        } else {
            for (int i = threadIdx.x * 4; i + 4 <= cnt; i += 4 * FP_THREADS) {
                const uint4 v = load_nt(w + i);
                s += four(v, g0 + G * (u64)i);
                store_nt(dst + i, v);
            }
        }
        tail = cnt & ~3;
    }
    for (int q = tail + threadIdx.x * 4; q < cnt; q += 4 * FP_THREADS) s += quad_by_words(w, dst, q, cnt, g0);
    s = block_sum(s, sh);
    if (threadIdx.x == 0) ws[blk] = s;
}

__global__ __launch_bounds__(FP_THREADS) void restore_kernel(const umi_optim_desc* __restrict__ descs, int n_desc) {
    const int blk = blockIdx.x;
    const umi_optim_desc d = descs[find_desc(descs, n_desc, blk)];
    const long base = (long)(blk - d.blk0) * FP_BLOCK;
    const long left = d.n - base;
    const int cnt = left < FP_BLOCK ? (int)left : FP_BLOCK;
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(d.s0) + base;
    uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(d.p) + base;
    if (((uintptr_t)dst & 15) == 0) {
        if (cnt == FP_BLOCK) {
            uint4 v[FP_QUADS];
#pragma unroll
            for (int j = 0; j < FP_QUADS; ++j)
                v[j] = *reinterpret_cast<const uint4*>(src + threadIdx.x * 4 + 4 * FP_THREADS * j);
#pragma unroll
            for (int j = 0; j < FP_QUADS; ++j)
                *reinterpret_cast<uint4*>(dst + threadIdx.x * 4 + 4 * FP_THREADS * j) = v[j];
        } else {
            for (int i = threadIdx.x * 4; i + 4 <= cnt; i += 4 * FP_THREADS)
                *reinterpret_cast<uint4*>(dst + i) = *reinterpret_cast<const uint4*>(src + i);
            const int i = (cnt & ~3) + threadIdx.x;
            if (i < cnt) dst[i] = src[i];                              // nothing past word n of the tensor
        }
    } else {
        for (int i = threadIdx.x; i < cnt; i += FP_THREADS) dst[i] = src[i];
    }
}

}  // namespace

extern "C" size_t umi_snapshot_ws_bytes(int total_blocks) {
    return total_blocks > 0 ? (size_t)total_blocks * sizeof(u64) : 0;
}

extern "C" int umi_snapshot_multi(const void* descs, int n_desc, int total_blocks, void* ws, size_t ws_bytes,
                                  unsigned long long* out, umi_stream_t stream) {
    if (!out || ((uintptr_t)out & 7) || n_desc < 0 || total_blocks < 0) return UMI_ERR_BADARG;
    if (n_desc > 0 && !descs) return UMI_ERR_BADARG;
    if (total_blocks > 0 && (n_desc == 0 || !ws || ((uintptr_t)ws & 7))) return UMI_ERR_BADARG;
    if (umi_optim_block_elems() != FP_BLOCK) return UMI_ERR_UNSUPPORTED;
    if (ws_bytes < umi_snapshot_ws_bytes(total_blocks)) return UMI_ERR_WORKSPACE;
    if (total_blocks > 0) {
        hipLaunchKernelGGL(snapshot_partials_kernel, dim3(total_blocks), dim3(FP_THREADS), 0, (hipStream_t)stream,
                           (const umi_optim_desc*)descs, n_desc, (u64*)ws);
        UMI_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(fingerprint_finalize_kernel, dim3(1), dim3(FIN_THREADS), 0, (hipStream_t)stream,
                       (const umi_optim_desc*)descs, n_desc, (const u64*)ws, total_blocks, (u64*)out);    // an empty table: F = 0
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_restore_multi(const void* descs, int n_desc, int total_blocks, umi_stream_t stream) {
    if (n_desc < 0 || total_blocks < 0) return UMI_ERR_BADARG;
    if (n_desc > 0 && !descs) return UMI_ERR_BADARG;
    if (total_blocks > 0 && n_desc == 0) return UMI_ERR_BADARG;
    if (umi_optim_block_elems() != FP_BLOCK) return UMI_ERR_UNSUPPORTED;
    if (total_blocks > 0) {
        hipLaunchKernelGGL(restore_kernel, dim3(total_blocks), dim3(FP_THREADS), 0, (hipStream_t)stream,
                           (const umi_optim_desc*)descs, n_desc);
        UMI_LAUNCH_CHECK();
    }
    return UMI_OK;
}
