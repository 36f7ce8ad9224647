// Replica fingerprint: one 64-bit word over every tensor of a umi_optim_desc table (include/unetmi.h, umi_fingerprint_multi).
//
//   mix(z)  the splitmix64 finaliser;  H_t = sum_i mix(w_i + G (i + 1)) over the 32-bit words of tensor t;
//   F = sum_t mix(H_t + G (t + 1)),  everything mod 2^64.
//
// Wrapping addition is associative and commutative, so the sums may be taken in any order and still give the same bits: no fixed
// tree is needed, only that every word is counted once.  Pass 1 uses the optimizer's block layout (a workgroup owns one block of
// umi_optim_block_elems() words of ONE tensor, found by binary search over blk0) and leaves one partial word per block in `ws`;
// pass 2 is one workgroup whose waves each take whole tensors, sum their partials, mix them with the tensor's position and add
// up.  Both passes only read the tensors; the stores are the block partials and the result word.  No atomics.
#include "common.h"
#include <stdint.h>

namespace {

typedef unsigned long long u64;

constexpr int FP_BLOCK = 4096;       // = umi_optim_block_elems(), checked by the entry point
constexpr int FP_THREADS = 256;
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

__global__ __launch_bounds__(FP_THREADS) void fingerprint_partials_kernel(const umi_optim_desc* __restrict__ descs, int n_desc,
                                                                          u64* __restrict__ ws) {
    __shared__ u64 sh[FP_THREADS / 32];
    const int blk = blockIdx.x;
    const umi_optim_desc d = descs[find_desc(descs, n_desc, blk)];
    const long base = (long)(blk - d.blk0) * FP_BLOCK;
    const long left = d.n - base;
    const int cnt = left < FP_BLOCK ? (int)left : FP_BLOCK;
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(d.p) + base;
    const u64 g0 = G * (u64)(base + 1);                                // G * (i + 1) of the block's first word
    u64 s = 0;
    if (((uintptr_t)w & 15) == 0) {
        if (cnt == FP_BLOCK) {                // a full block: the four loads of a thread in flight together
            uint4 v[FP_BLOCK / (4 * FP_THREADS)];
#pragma unroll
            for (int j = 0; j < FP_BLOCK / (4 * FP_THREADS); ++j)
                v[j] = *reinterpret_cast<const uint4*>(w + threadIdx.x * 4 + 4 * FP_THREADS * j);
#pragma unroll
            for (int j = 0; j < FP_BLOCK / (4 * FP_THREADS); ++j)
                s += four(v[j], g0 + G * (u64)(threadIdx.x * 4 + 4 * FP_THREADS * j));
        } else {
            for (int i = threadIdx.x * 4; i + 4 <= cnt; i += 4 * FP_THREADS)
                s += four(*reinterpret_cast<const uint4*>(w + i), g0 + G * (u64)i);
            const int i = (cnt & ~3) + threadIdx.x;
            if (i < cnt) s += mix(w[i] + (g0 + G * (u64)i));
        }
    } else {
        for (int i = threadIdx.x; i < cnt; i += FP_THREADS) s += mix(w[i] + (g0 + G * (u64)i));
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) ws[blk] = s;
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

extern "C" size_t umi_fingerprint_ws_bytes(int total_blocks) {
    return total_blocks > 0 ? (size_t)total_blocks * sizeof(u64) : 0;
}

extern "C" int umi_fingerprint_multi(const void* descs, int n_desc, int total_blocks, void* ws, size_t ws_bytes,
                                     unsigned long long* out, umi_stream_t stream) {
    if (!out || ((uintptr_t)out & 7) || n_desc < 0 || total_blocks < 0) return UMI_ERR_BADARG;
    if (n_desc > 0 && !descs) return UMI_ERR_BADARG;
    if (total_blocks > 0 && (n_desc == 0 || !ws || ((uintptr_t)ws & 7))) return UMI_ERR_BADARG;
    if (umi_optim_block_elems() != FP_BLOCK) return UMI_ERR_UNSUPPORTED;
    if (ws_bytes < umi_fingerprint_ws_bytes(total_blocks)) return UMI_ERR_WORKSPACE;
    if (total_blocks > 0) {
        hipLaunchKernelGGL(fingerprint_partials_kernel, dim3(total_blocks), dim3(FP_THREADS), 0, (hipStream_t)stream,
                           (const umi_optim_desc*)descs, n_desc, (u64*)ws);
        UMI_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(fingerprint_finalize_kernel, dim3(1), dim3(FIN_THREADS), 0, (hipStream_t)stream,
                       (const umi_optim_desc*)descs, n_desc, (const u64*)ws, total_blocks, (u64*)out);    // an empty table: F = 0
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
