// Patch gather of the pure-ViT TransUNet variants (reference TransUnet/vit_seg_modeling.py:137-140: Conv2d(3, hidden, kernel_size=P,
// stride=P) straight on the image).  That convolution is a GEMM over non-overlapping patches; this file only lays the patches
// out as the GEMM's token-major A operand, the product itself runs on the linear path's kernels (umi_conv_fwd, 1x1):
//
//   rows[(b * gh + ty) * gw + tx][(c * P + ky) * P + kx] = x[b][c][ty * P + ky][tx * P + kx],   gh = H / P, gw = W / P
//
// The column order is PyTorch's flattening of a [hidden][C][P][P] weight, so that weight is the GEMM's [hidden][K] matrix as it
// stands.  Rows H - gh * P .. and columns W - gw * P .. of the image (what a stride-P convolution ignores) are never read.
//
// A pure streaming kernel: one thread per V consecutive output elements (V = 16 bytes of input: 4 fp32 or 8 fp16), so a wave
// writes one contiguous stretch of an output row and reads whole patch rows (P elements: 64 bytes at P = 16, fp32) of the image;
// grid-stride over 64-bit element indices.  No LDS, no atomics.  V = 1 where P, W, the row stride or an address does not allow the wide accesses.
#include "common.h"

namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_MAX_BLOCKS = 2048;                      // 8 resident blocks per CU; the loop covers the rest

template <typename T, int V> struct PrVec { typedef T type __attribute__((ext_vector_type(V))); };
template <typename T> struct PrVec<T, 1> { typedef T type; };

template <typename TI, typename TO, int V>
__device__ __forceinline__ void pr_move(const TI* __restrict__ src, TO* __restrict__ dst) {
    if constexpr (V == 1) {
        *dst = (TO)(*src);                               // fp32 -> fp16: round to nearest even
    } else {
        const typename PrVec<TI, V>::type v = *reinterpret_cast<const typename PrVec<TI, V>::type*>(src);
        typename PrVec<TO, V>::type o;
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = (TO)v[j];
        *reinterpret_cast<typename PrVec<TO, V>::type*>(dst) = o;
    }
}

// chunks = M * (K / V) pieces of V elements; K % V == 0 and P % V == 0, so a piece never leaves its patch row
template <typename TI, typename TO, int V>
__global__ __launch_bounds__(PR_THREADS) void patch_rows_kernel(const TI* __restrict__ x, TO* __restrict__ rows, long ld, long chunks,
                                                                int C, int H, int W, int P, int gh, int gw) {
    const int kv = C * P * P / V;                        // pieces per output row
    const long step = (long)gridDim.x * PR_THREADS;
    for (long i = (long)blockIdx.x * PR_THREADS + threadIdx.x; i < chunks; i += step) {
        long row, q, b;
        int piece, tx, ty;
        umi_divmod(i, kv, row, piece);
        umi_divmod(row, gw, q, tx);
        umi_divmod(q, gh, b, ty);
        const int col = piece * V;
        const int c = col / (P * P), rem = col - c * P * P;
        const int ky = rem / P, kx = rem - ky * P;
        const long src = (((b * C + c) * H + (long)ty * P + ky) * W) + (long)tx * P + kx;
        pr_move<TI, TO, V>(x + src, rows + row * ld + col);
    }
}

template <typename TI, typename TO>
int pr_launch(const void* x, void* rows, long ld, int B, int C, int H, int W, int P, hipStream_t s) {
    constexpr int V = 16 / (int)sizeof(TI);
    const int gh = H / P, gw = W / P;
    const long M = (long)B * gh * gw, K = (long)C * P * P;
    const bool wide = P % V == 0 && W % V == 0 && ld % V == 0 && ((uintptr_t)x & 15) == 0 &&
                      ((uintptr_t)rows & (V * sizeof(TO) - 1)) == 0;
    const long chunks = wide ? M * (K / V) : M * K;
    const long want = (chunks + PR_THREADS - 1) / PR_THREADS;
    const dim3 grid((unsigned)(want < PR_MAX_BLOCKS ? want : PR_MAX_BLOCKS));
    if (wide)
        hipLaunchKernelGGL((patch_rows_kernel<TI, TO, V>), grid, dim3(PR_THREADS), 0, s, (const TI*)x, (TO*)rows, ld, chunks, C, H, W,
                           P, gh, gw);
    else
        hipLaunchKernelGGL((patch_rows_kernel<TI, TO, 1>), grid, dim3(PR_THREADS), 0, s, (const TI*)x, (TO*)rows, ld, chunks, C, H, W,
                           P, gh, gw);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

}  // namespace

extern "C" int umi_patch_rows(const void* x, int in_dtype, void* rows, long ld, int out_dtype, int B, int C, int H, int W, int P,
                              umi_stream_t stream) {
    if (!x || !rows || B <= 0 || C <= 0 || H <= 0 || W <= 0 || P <= 0 || P > H || P > W) return UMI_ERR_BADARG;
    if ((in_dtype != UMI_F32 && in_dtype != UMI_F16) || (out_dtype != UMI_F32 && out_dtype != UMI_F16)) return UMI_ERR_BADARG;
    const long K = (long)C * P * P;
    if (ld < K) return UMI_ERR_BADARG;
    if (K >= (1L << 31) || (long)H * W >= (1L << 31)) return UMI_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (in_dtype == UMI_F32)
        return out_dtype == UMI_F16 ? pr_launch<float, half_t>(x, rows, ld, B, C, H, W, P, s)
                                    : pr_launch<float, float>(x, rows, ld, B, C, H, W, P, s);
    return out_dtype == UMI_F16 ? pr_launch<half_t, half_t>(x, rows, ld, B, C, H, W, P, s)
                                : pr_launch<half_t, float>(x, rows, ld, B, C, H, W, P, s);
}
