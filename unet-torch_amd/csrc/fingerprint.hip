// Replica fingerprint: one 64-bit word over every tensor of a umi_optim_desc table (include/unetmi.h, umi_fingerprint_multi).
//
//   mix(z)  the splitmix64 finaliser;  H_t = sum_i mix(w_i + G (i + 1)) over the 32-bit words of tensor t;
//   F = sum_t mix(H_t + G (t + 1)),  everything mod 2^64.
//
// Wrapping addition is associative and commutative, so the sums may be taken in any order and still give the same bits: no fixed
// tree is needed, only that every word is counted once.  Pass 1 uses the optimizer's block layout (a workgroup owns one block of
// umi_optim_block_elems() words of ONE tensor, found by binary search over blk0) and leaves one partial word per block in `ws`;
// pass 2 is one workgroup whose waves each take whole tensors, sum their partials, mix them with the tensor's position and add
// up.  Both passes only read the tensors; the stores are the block partials and the result word.  No atomics.  The arithmetic
// and pass 2 live in fingerprint_mix.h, which the snapshot copy (snapshot.hip) shares.
#include "fingerprint_mix.h"

namespace {

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
