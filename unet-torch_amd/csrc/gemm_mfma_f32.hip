// fp32 pointwise convolution / nn.Linear, Y[M, Co] = X[M, Ci] . W[Ci, Co] with M = N * H * W (forward = data gradient, and weight
// gradient), on the fp32-input matrix-core instruction of gfx950, v_mfma_f32_32x32x2_f32.  Opt-in: UMI_CONV_F32_MFMA_1X1
// (include/unetmi.h); without the flag, or on a problem the predicates below refuse, the call runs exactly as before.
//
// Numerics, as in conv_mfma_f32.hip: the instruction is D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)) in fp32, so an output here is ONE
// fmaf chain; no floating-point atomics anywhere, identical inputs give identical bits.
//   forward / data gradient: one accumulator per output from the first product to the last, k ascending over 0 .. Ci - 1; the
//     bias is added once, after the chain.  (A K chunk that reaches past Ci is filled with zeros: fma(0, 0, acc) = acc.)
//   weight gradient: M is cut into contiguous splits; one accumulator per (ci, co) and split, m ascending inside the split (rows
//     past the split's end enter as zeros); the splits' slabs [split][1][ci][co] are then summed by umi_launch_wgrad_reduce in its
//     fixed order.
//   statistics: one row of part[rows][2][Co] per 128 consecutive output rows; per channel the stored values are summed in a lane
//     over its rows in ascending register order, the two half waves are added, then the waves in wave order.
#include "kernels.h"
#include "mfma_f32.h"

namespace {

// ---- forward ------------------------------------------------------------------------------------------------------------------
// The 128-row forward tile of mfma_f32.h with the identity row map: D's lanes run along co, so a store instruction writes 128
// contiguous bytes of two output rows.  The next chunk's global loads are in flight while the current one is multiplied.

template <int WM, int WN, int MT, int NT, bool HAS_TX>
__global__ __launch_bounds__(256) void gemm_f32_mfma_kernel(const float* __restrict__ x, int ldx, const float4* __restrict__ tx,
                                                            const float* __restrict__ wp, const float* __restrict__ bias,
                                                            float* __restrict__ y, int ldy, float* __restrict__ part, long M,
                                                            int Ci, int Co) {
    static_assert(WM * WN == 4 && WM * MT * 32 == P_TM, "4 waves cover 128 rows");
    constexpr int TN = WN * NT * 32;
    constexpr int WSL = P_KC * TN / 4 / 256;             // float4 weight loads per thread: 4 or 2
    __shared__ float xl[P_TM * P_XS];
    __shared__ __attribute__((aligned(16))) float wl[P_KC * TN];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, col = lane & 31, kh = lane >> 5;
    const int wm = wv % WM, wn = wv / WM;
    const long m0 = (long)blockIdx.x * P_TM;
    const int co0 = blockIdx.y * TN;

    // what this thread stages: 4 x slots (row = i * 32 + tid / 8, channel quad tid & 7) and WSL weight slots (k row, co quad)
    const int q4 = (tid & 7) * 4, xrow = tid >> 3;
    const float* xp[4];
    bool xin[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long m = m0 + i * 32 + xrow;
        xin[i] = m < M;
        xp[i] = x + (xin[i] ? m : 0) * ldx + q4;          // an address inside the tensor in every case
    }
    constexpr int WQ = TN / 4;                            // co quads per weight row
    const int wc4 = (tid % WQ) * 4, wk = tid / WQ;        // slot i: k row = i * (256 / WQ) + wk
    const bool wok = co0 + wc4 < Co;
    float4 hx[4], wx[WSL];
    auto load_chunk = [&](int ci0) {
        const bool kin = ci0 + q4 < Ci;
        float4 t[4];
        if (HAS_TX) {
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = kin ? tx[ci0 + q4 + j] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            hx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (xin[i] && kin) {
                float4 v = *reinterpret_cast<const float4*>(xp[i] + ci0);
                if (HAS_TX) { v.x = umi_tx(v.x, t[0]); v.y = umi_tx(v.y, t[1]); v.z = umi_tx(v.z, t[2]); v.w = umi_tx(v.w, t[3]); }
                hx[i] = v;                                // the transform first, the zero fill of absent rows / channels after it
            }
        }
#pragma unroll
        for (int i = 0; i < WSL; ++i) {
            const int k = ci0 + i * (256 / WQ) + wk;
            wx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (wok && k < Ci) wx[i] = *reinterpret_cast<const float4*>(wp + (long)k * Co + co0 + wc4);
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float* d = xl + (i * 32 + xrow) * P_XS + q4;
            d[0] = hx[i].x; d[1] = hx[i].y; d[2] = hx[i].z; d[3] = hx[i].w;
        }
#pragma unroll
        for (int i = 0; i < WSL; ++i) *reinterpret_cast<float4*>(wl + (i * (256 / WQ) + wk) * TN + wc4) = wx[i];
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const float* pa = xl + (wm * MT * 32 + col) * P_XS + kh;
    const float* pb = wl + kh * TN + wn * NT * 32 + col;
    load_chunk(0);
    for (int ci0 = 0; ci0 < Ci; ci0 += P_KC) {
        store_chunk();
        __syncthreads();
        if (ci0 + P_KC < Ci) load_chunk(ci0 + P_KC);
        fwd_tile_multiply<TN>(acc, pa, pb);
        __syncthreads();
    }

    // epilogue: this lane holds channel co0 + 32 (wn NT + b) + col of rows m0 + 32 (wm MT + a) + d_row(reg, kh)
    float cs[NT], cq[NT];
#pragma unroll
    for (int b = 0; b < NT; ++b) {
        const int co = co0 + (wn * NT + b) * 32 + col;
        const bool cok = co < Co;
        const float bv = (bias != nullptr && cok) ? bias[co] : 0.f;
        cs[b] = cq[b] = 0.f;
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long m = m0 + (wm * MT + a) * 32 + d_row(r, kh);
                const float v = acc[a][b][r] + bv;
                if (cok && m < M) {
                    y[m * ldy + co] = v;
                    cs[b] += v;
                    cq[b] = fmaf(v, v, cq[b]);
                }
            }
    }
    if (part == nullptr) return;
    // BatchNorm partial sums of the stored values: the two half waves hold different rows of one channel; then the WM waves that
    // share the channel, in wave order.  One row of part[rows][2][Co] per 128 output rows (blockIdx.x).
    float* red = wl;                                      // [WM][2][TN]: the weights are dead (barrier at the loop's end)
#pragma unroll
    for (int b = 0; b < NT; ++b) {
        const float s = cs[b] + __shfl_xor(cs[b], 32, 64), q = cq[b] + __shfl_xor(cq[b], 32, 64);
        if (kh == 0) {
            red[(wm * 2 + 0) * TN + (wn * NT + b) * 32 + col] = s;
            red[(wm * 2 + 1) * TN + (wn * NT + b) * 32 + col] = q;
        }
    }
    __syncthreads();
    if (tid < 2 * TN) {
        const int which = tid / TN, c = tid % TN;
        float s = red[which * TN + c];
#pragma unroll
        for (int w = 1; w < WM; ++w) s += red[(w * 2 + which) * TN + c];
        if (co0 + c < Co) part[((long)blockIdx.x * 2 + which) * Co + co0 + c] = s;
    }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
// dW[ci][co] = sum over rows of tx(x)[m][ci] * dy[m][co]: the channel-lane weight-gradient tile of mfma_f32.h over the contiguous
// rows of one split (blockIdx.y).
template <int MT, int NT, bool HAS_TX>
__global__ __launch_bounds__(256) void wgrad_gemm_f32_mfma_kernel(const float* __restrict__ x, int ldx, const float4* __restrict__ tx,
                                                                  const float* __restrict__ dy, int lddy, float* __restrict__ ws,
                                                                  long M, int Ci, int Co, int tiles_co, long rows_per_split) {
    constexpr int TI = 2 * MT * 32, TJ = 2 * NT * 32;
    constexpr int ASL = Q_KC * TI / 4 / 256, BSL = Q_KC * TJ / 4 / 256;      // float4 loads per thread: 2 or 4
    constexpr int AQ = TI / 4, BQ = TJ / 4;
    __shared__ __attribute__((aligned(16))) float xl[Q_KC * TI];
    __shared__ __attribute__((aligned(16))) float dl[Q_KC * TJ];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, col = lane & 31, kh = lane >> 5;
    const int ci0 = (blockIdx.x / tiles_co) * TI, co0 = (blockIdx.x % tiles_co) * TJ;
    const long r0 = (long)blockIdx.y * rows_per_split;
    const long r1 = r0 + rows_per_split < M ? r0 + rows_per_split : M;
    const int ac4 = (tid % AQ) * 4, arow = tid / AQ, bc4 = (tid % BQ) * 4, brow = tid / BQ;
    const bool ci_ok = ci0 + ac4 < Ci, co_ok = co0 + bc4 < Co;
    float4 t[4];
    if (HAS_TX) {
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = ci_ok ? tx[ci0 + ac4 + j] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 ax[ASL], bx[BSL];
    auto load_chunk = [&](long r) {
#pragma unroll
        for (int i = 0; i < ASL; ++i) {
            const long m = r + i * (256 / AQ) + arow;
            ax[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ci_ok && m < r1) {
                float4 v = *reinterpret_cast<const float4*>(x + m * ldx + ci0 + ac4);
                if (HAS_TX) { v.x = umi_tx(v.x, t[0]); v.y = umi_tx(v.y, t[1]); v.z = umi_tx(v.z, t[2]); v.w = umi_tx(v.w, t[3]); }
                ax[i] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < BSL; ++i) {
            const long m = r + i * (256 / BQ) + brow;
            bx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (co_ok && m < r1) bx[i] = *reinterpret_cast<const float4*>(dy + m * lddy + co0 + bc4);
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < ASL; ++i) *reinterpret_cast<float4*>(xl + (i * (256 / AQ) + arow) * TI + ac4) = ax[i];
#pragma unroll
        for (int i = 0; i < BSL; ++i) *reinterpret_cast<float4*>(dl + (i * (256 / BQ) + brow) * TJ + bc4) = bx[i];
    };

    const int wi = wv & 1, wj = wv >> 1;
    f32x16 acc[MT][NT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[a][b][q] = 0.f;

    const float* pa = xl + kh * TI + wi * MT * 32 + col;
    const float* pb = dl + kh * TJ + wj * NT * 32 + col;
    if (r0 < r1) load_chunk(r0);
    for (long r = r0; r < r1; r += Q_KC) {
        store_chunk();
        __syncthreads();
        if (r + Q_KC < r1) load_chunk(r + Q_KC);
        wgrad_tile_multiply(acc, pa, pb);
        __syncthreads();
    }
    // slab [split][ci][co]: lanes along co
#pragma unroll
    for (int b = 0; b < NT; ++b) {
        const int co = co0 + (wj * NT + b) * 32 + col;
        if (co >= Co) continue;
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int ci = ci0 + (wi * MT + a) * 32 + d_row(q, kh);
                if (ci < Ci) ws[((long)blockIdx.y * Ci + ci) * Co + co] = acc[a][b][q];
            }
    }
}

bool flags_ok(int flags) {
    return (flags & UMI_CONV_F32_MFMA_1X1) &&
           !(flags & (UMI_CONV_UPSAMPLE2 | UMI_CONV_FORCE_GENERIC | UMI_CONV_DGRAD_STRIDED | UMI_CONV_ACCUMULATE));
}

}  // namespace

bool umi_gemm_f32_mfma_ok(const ConvFwdProblem& p) {
    if (!flags_ok(p.flags)) return false;
    if (p.in_dtype != UMI_F32 || p.out_dtype != UMI_F32) return false;
    if (p.R != 1 || p.S != 1 || p.stride != 1 || p.pad != 0 || p.Ho != p.H || p.Wo != p.W) return false;
    if (p.Ci % 8 || p.Co % 8 || p.ldx % 4 || p.ldy % 4) return false;        // partial channel tiles are masked in the kernel
    // addresses are 64-bit; the row-tile index and the co-tile index are grid dimensions
    if ((long)p.N * p.H * p.W >= (1L << 31) * P_TM || umi_cdiv(p.Co, 64) > 65535) return false;
    return true;
}

int umi_gemm_f32_mfma_stat_rows(long M) { return umi_cdiv(M, P_TM); }

int umi_gemm_f32_mfma(const ConvFwdProblem& p, const void* x, const void* tx, const void* wp, const float* bias, void* y,
                      float* stat_part, hipStream_t s) {
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)wp | (uintptr_t)tx) & 15) return UMI_ERR_BADARG;
    const long M = (long)p.N * p.H * p.W;
    const bool narrow = fwd_narrow(M, p.Co, 1);
    dim3 grid((unsigned)umi_cdiv(M, P_TM), (unsigned)umi_cdiv(p.Co, narrow ? 64 : 128)), block(256);
#define UMI_GEMM_F32(WM, WN, MT, NT, TX)                                                                                      \
    hipLaunchKernelGGL((gemm_f32_mfma_kernel<WM, WN, MT, NT, TX>), grid, block, 0, s, (const float*)x, p.ldx, (const float4*)tx, \
                       (const float*)wp, bias, (float*)y, p.ldy, stat_part, M, p.Ci, p.Co)
    if (narrow) {
        if (tx) UMI_GEMM_F32(4, 1, 1, 2, true); else UMI_GEMM_F32(4, 1, 1, 2, false);
    } else {
        if (tx) UMI_GEMM_F32(2, 2, 2, 2, true); else UMI_GEMM_F32(2, 2, 2, 2, false);
    }
#undef UMI_GEMM_F32
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

bool umi_wgrad_gemm_f32_mfma_ok(const WgradProblem& p) {
    if (!flags_ok(p.flags)) return false;
    if (p.dtype != UMI_F32 || p.has_txb) return false;
    if (p.R != 1 || p.S != 1 || p.stride != 1 || p.pad != 0 || p.Ho != p.H || p.Wo != p.W) return false;
    if (p.Ci % 8 || p.Co % 8 || p.ldx % 4 || p.lddy % 4) return false;
    // addresses are 64-bit; the tile index and the split index are grid dimensions (at most 128 splits)
    if ((long)p.N * p.H * p.W >= (1L << 40) || (long)umi_cdiv(p.Ci, 64) * umi_cdiv(p.Co, 64) >= (1L << 31)) return false;
    return true;
}

size_t umi_wgrad_gemm_f32_mfma_ws_bound(const WgradProblem& facts) {
    if (!(facts.flags & UMI_CONV_F32_MFMA_1X1)) return 0;
    WgradProblem p = facts;
    p.H = p.Ho; p.W = p.Wo; p.stride = 1; p.pad = 0; p.ldx = p.lddy = 4;
    if (!umi_wgrad_gemm_f32_mfma_ok(p)) return 0;
    int ti, tj, splits;
    long rps;
    wgrad_plan((long)p.N * p.H * p.W, p.Ci, p.Co, 1, &ti, &tj, &splits, &rps);
    return (size_t)splits * p.Ci * p.Co * sizeof(float);
}

int umi_wgrad_gemm_f32_mfma(const WgradProblem& p, const void* x, const void* txa, const void* dy, const WgradOut& o, hipStream_t s) {
    const long M = (long)p.N * p.H * p.W;
    int ti, tj, splits;
    long rps;
    wgrad_plan(M, p.Ci, p.Co, 1, &ti, &tj, &splits, &rps);
    if (o.ws_bytes < (size_t)splits * p.Ci * p.Co * sizeof(float)) return UMI_ERR_WORKSPACE;
    if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)txa) & 15) return UMI_ERR_BADARG;
    const int tiles_co = umi_cdiv(p.Co, tj);
    dim3 grid((unsigned)(umi_cdiv(p.Ci, ti) * tiles_co), (unsigned)splits), block(256);
#define UMI_WGRAD_F32(MT, NT, TX)                                                                                             \
    hipLaunchKernelGGL((wgrad_gemm_f32_mfma_kernel<MT, NT, TX>), grid, block, 0, s, (const float*)x, p.ldx, (const float4*)txa, \
                       (const float*)dy, p.lddy, (float*)o.ws, M, p.Ci, p.Co, tiles_co, rps)
#define UMI_WGRAD_F32_TX(MT, NT) do { if (txa) UMI_WGRAD_F32(MT, NT, true); else UMI_WGRAD_F32(MT, NT, false); } while (0)
    if (ti == 64 && tj == 64) UMI_WGRAD_F32_TX(1, 1);
    else if (ti == 64) UMI_WGRAD_F32_TX(1, 2);
    else if (tj == 64) UMI_WGRAD_F32_TX(2, 1);
    else UMI_WGRAD_F32_TX(2, 2);
#undef UMI_WGRAD_F32_TX
#undef UMI_WGRAD_F32
    UMI_LAUNCH_CHECK();
    umi_launch_wgrad_reduce(splits, 1, p.Ci, p.Co, o, s);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
