// The arithmetic of the replica fingerprint (include/unetmi.h, umi_fingerprint_multi), shared by the pass that only reads the
// tensors (fingerprint.hip) and the pass that also copies them into an arena (snapshot.hip):
//
//   mix(z)  the splitmix64 finaliser;  H_t = sum_i mix(w_i + G (i + 1)) over the 32-bit words of tensor t;
//   F = sum_t mix(H_t + G (t + 1)),  everything mod 2^64.
//
// Pass 1 of either file leaves one partial word per block of FP_BLOCK words in `ws`; fingerprint_finalize_kernel is pass 2 of
// both: one workgroup whose waves each take whole tensors, sum their partials, mix them with the tensor's position and add up.
#pragma once
#include "common.h"
#include <stdint.h>

namespace {

typedef unsigned long long u64;

constexpr int FP_BLOCK = 4096;       // = umi_optim_block_elems(), checked by the entry points
constexpr int FP_THREADS = 256;
constexpr int FP_QUADS = FP_BLOCK / (4 * FP_THREADS);      // 16-byte loads of one thread in a full block
constexpr int FIN_THREADS = 1024;
constexpr u64 G = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ u64 mix(u64 z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

__device__ inline int find_desc(const umi_optim_desc* d, int n, int blk) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (d[mid].blk0 <= blk) lo = mid; else hi = mid - 1;       // of equal blk0 (empty tensors) the last one owns the block
    }
    return lo;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
    for (int off = warpSize / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// sum over the workgroup; valid in thread 0.  `sh` holds one word per wave
__device__ inline u64 block_sum(u64 v, u64* sh) {
    v = wave_sum(v);
    const int wave = threadIdx.x / warpSize, nw = blockDim.x / warpSize;
    if (threadIdx.x % warpSize == 0) sh[wave] = v;
    __syncthreads();
    u64 s = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < nw; ++w) s += sh[w];
    return s;
}

__device__ __forceinline__ u64 four(const uint4 v, u64 g) {           // g = G * (index of v.x + 1)
    return mix(v.x + g) + mix(v.y + (g + G)) + mix(v.z + (g + 2 * G)) + mix(v.w + (g + 3 * G));
}

__global__ __launch_bounds__(FIN_THREADS) void fingerprint_finalize_kernel(const umi_optim_desc* __restrict__ descs, int n_desc,
                                                                           const u64* __restrict__ ws, int total_blocks,
                                                                           u64* __restrict__ out) {
    __shared__ u64 sh[FIN_THREADS / 32];
    const int lane = threadIdx.x % warpSize, wave = threadIdx.x / warpSize, nw = blockDim.x / warpSize;
    u64 f = 0;
    for (int t = wave; t < n_desc; t += nw) {                          // a wave per tensor: its lanes stride over the tensor's blocks
        const long n = descs[t].n;
        const int b0 = descs[t].blk0;
        const int nb = (int)((n + FP_BLOCK - 1) / FP_BLOCK);
        u64 h = 0;
        for (int b = lane; b < nb && b0 + b < total_blocks; b += warpSize) h += ws[b0 + b];   // never past the workspace
        h = wave_sum(h);
        if (lane == 0) f += mix(h + G * (u64)(t + 1));
    }
    f = block_sum(lane == 0 ? f : 0, sh);
    if (threadIdx.x == 0) *out = f;
}

}  // namespace
