// fp32 nn.ConvTranspose2d(k = 2, s = 2) on the fp32-input matrix-core instruction of gfx950, v_mfma_f32_32x32x2_f32: its forward
// (umi_conv_fwd with UMI_CONV_UPSAMPLE2), its data gradient (a 2x2 / stride-2 convolution over d(up)) and its weight gradient (the
// 2x2 / stride-2 weight gradient).  Opt-in: UMI_CONV_F32_MFMA_2X2 (include/unetmi.h); without the flag, or on a problem the
// predicates below refuse, the call runs exactly as before.
//
// Numerics, as in gemm_mfma_f32.hip: the instruction is D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)) in fp32, so an output here is ONE
// fmaf chain; no floating-point atomics anywhere, identical inputs give identical bits, and the images of a batch never meet in
// one accumulator of the two forward kernels.
//   forward: Y'[M, 4 Cout] = tx(X)[M, Cin] . W over umi_pack_kn's [4][Cin][Cout], M = N h w; one accumulator per output, k ascending
//     over 0 .. Cin - 1, the bias added once after the chain; row (n, h, w) of tap t = 2 dy + dx is stored at pixel
//     (2h + dy + off_h, 2w + dx + off_w) of the out_H x out_W image.
//   data gradient: dx[M, Co], K = 4 Ci; one accumulator per output, taps ascending (t = 2r + s), channels ascending inside a tap;
//     a 32-channel chunk that reaches past the tap's end is filled with zeros (fma(0, 0, acc) = acc) and the accumulator carries
//     on across the taps.
//   weight gradient: the N Ho Wo output pixels, in (n, ho, wo) order, are cut into contiguous splits; one accumulator per
//     (tap, ci, co) and split, pixels ascending inside the split (pixels past its end enter as zeros); the splits' slabs
//     [split][4][Ci][Co] are then summed by umi_launch_wgrad_reduce in its fixed order.
// Tail rows, K chunks and channel tiles are masked by loads that do not happen.
#include "kernels.h"
#include "mfma_f32.h"

namespace {

// ---- forward and data gradient ------------------------------------------------------------------------------------------------
// The 128-row forward tile of mfma_f32.h, staged as gemm_mfma_f32.hip stages it.
//   UP  (forward):      a row is an INPUT pixel, a column tile lies inside one tap, the epilogue scatters.
//   !UP (data gradient): a row is an OUTPUT pixel, the A operand is gathered from the pixels of the four taps in turn.
// Workgroups that share a row tile are neighbours in the grid (the column tile is the fast index), so x is read from memory once.

struct CtGeo { int H, W, out_H, out_W, off_h, off_w; };      // H x W: the grid the rows run over (UP: input, !UP: output pixels)

template <int WM, int WN, int MT, int NT, bool UP>
__global__ __launch_bounds__(256) void convt_f32_mfma_kernel(const float* __restrict__ x, int ldx, const float4* __restrict__ tx,
                                                             const float* __restrict__ wp, const float* __restrict__ bias,
                                                             float* __restrict__ y, int ldy, unsigned M, int K, int Nn,
                                                             int ctiles, CtGeo g) {
    static_assert(WM * WN == 4 && WM * MT * 32 == P_TM, "4 waves cover 128 rows");
    constexpr int TN = WN * NT * 32;
    constexpr int WSL = P_KC * TN / 4 / 256;             // float4 weight loads per thread: 4 or 2
    __shared__ float xl[P_TM * P_XS];
    __shared__ __attribute__((aligned(16))) float wl[P_KC * TN];
    __shared__ long orow[P_TM];                          // the output pixel of each row of the tile, -1 past the end
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, col = lane & 31, kh = lane >> 5;
    const int wm = wv % WM, wn = wv / WM;
    const unsigned ncol = UP ? 4u * ctiles : (unsigned)ctiles;
    const unsigned ct = blockIdx.x % ncol;
    const unsigned m0 = (blockIdx.x / ncol) * P_TM;
    const int tap_up = UP ? (int)(ct / ctiles) : 0;
    const int co0 = (int)(UP ? ct % ctiles : ct) * TN;

    if (tid < P_TM) {
        const unsigned m = m0 + tid;
        long o = -1;
        if (m < M) {
            o = m;
            if (UP) {
                const unsigned w = m % (unsigned)g.W, r = m / (unsigned)g.W, h = r % (unsigned)g.H, n = r / (unsigned)g.H;
                o = ((long)n * g.out_H + 2 * h + (tap_up >> 1) + g.off_h) * g.out_W + 2 * w + (tap_up & 1) + g.off_w;
            }
        }
        orow[tid] = o;                                   // read after the loop's barriers (the loop runs at least once)
    }

    // what this thread stages: 4 x slots (row = i * 32 + tid / 8, channel quad tid & 7) and WSL weight slots (k row, co quad)
    const int q4 = (tid & 7) * 4, xrow = tid >> 3;
    const float* xp[4];
    bool xin[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned m = m0 + i * 32 + xrow;
        xin[i] = m < M;
        long pix = xin[i] ? m : 0;                       // an address inside the tensor in every case
        if (!UP && xin[i]) {
            const unsigned w = m % (unsigned)g.W, r = m / (unsigned)g.W, h = r % (unsigned)g.H, n = r / (unsigned)g.H;
            pix = ((long)n * 2 * g.H + 2 * h) * (2 * g.W) + 2 * w;          // tap (0, 0) of output pixel (n, h, w)
        }
        xp[i] = x + pix * ldx + q4;
    }
    constexpr int WQ = TN / 4;                            // co quads per weight row
    const int wc4 = (tid % WQ) * 4, wk = tid / WQ;        // slot i: k row = i * (256 / WQ) + wk
    const bool wok = co0 + wc4 < Nn;
    float4 hx[4], wx[WSL];
    auto load_chunk = [&](int t, int ci0) {
        const bool kin = ci0 + q4 < K;
        const long toff = UP ? 0 : ((long)(t >> 1) * (2 * g.W) + (t & 1)) * ldx;
        float4 tq[4];
        if (tx != nullptr) {
#pragma unroll
            for (int j = 0; j < 4; ++j) tq[j] = kin ? tx[ci0 + q4 + j] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            hx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (xin[i] && kin) {
                float4 v = *reinterpret_cast<const float4*>(xp[i] + toff + ci0);
                if (tx != nullptr) { v.x = umi_tx(v.x, tq[0]); v.y = umi_tx(v.y, tq[1]); v.z = umi_tx(v.z, tq[2]); v.w = umi_tx(v.w, tq[3]); }
                hx[i] = v;                                // the transform first, the zero fill of absent rows / channels after it
            }
        }
#pragma unroll
        for (int i = 0; i < WSL; ++i) {
            const int k = ci0 + i * (256 / WQ) + wk;
            wx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (wok && k < K) wx[i] = *reinterpret_cast<const float4*>(wp + ((long)t * K + k) * Nn + co0 + wc4);
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
    const int t_end = UP ? tap_up + 1 : 4;
    int t = tap_up, ci0 = 0;
    load_chunk(t, 0);
    while (t < t_end) {
        store_chunk();
        __syncthreads();
        ci0 += P_KC;
        if (ci0 >= K) { ci0 = 0; ++t; }                   // the next chunk: the same tap's next channels, or the next tap's first
        if (t < t_end) load_chunk(t, ci0);
        fwd_tile_multiply<TN>(acc, pa, pb);
        __syncthreads();
    }

    // epilogue: this lane holds channel co0 + 32 (wn NT + b) + col of tile rows 32 (wm MT + a) + d_row(reg, kh)
#pragma unroll
    for (int b = 0; b < NT; ++b) {
        const int co = co0 + (wn * NT + b) * 32 + col;
        if (co >= Nn) continue;
        const float bv = bias != nullptr ? bias[co] : 0.f;
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long o = orow[(wm * MT + a) * 32 + d_row(r, kh)];
                if (o >= 0) y[o * ldy + co] = acc[a][b][r] + bv;
            }
    }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
// dW[t][ci][co] = sum over output pixels p = (n, ho, wo) of txa(x)[n][2 ho + r][2 wo + s][ci] * txb(dy)[p][co], t = 2 r + s: the
// channel-lane weight-gradient tile of mfma_f32.h once per tap, with the x rows gathered.  A workgroup owns one tap and the pixels
// of one split (blockIdx.y).
template <int MT, int NT>
__global__ __launch_bounds__(256) void convt_wgrad_f32_mfma_kernel(const float* __restrict__ x, int ldx, const float4* __restrict__ txa,
                                                                   const float* __restrict__ dy, int lddy,
                                                                   const float4* __restrict__ txb, float* __restrict__ ws, unsigned M,
                                                                   int Ho, int Wo, int Ci, int Co, int tiles_co, int tiles,
                                                                   unsigned rows_per_split) {
    constexpr int TI = 2 * MT * 32, TJ = 2 * NT * 32;
    constexpr int ASL = Q_KC * TI / 4 / 256, BSL = Q_KC * TJ / 4 / 256;      // float4 loads per thread: 2 or 4
    constexpr int AQ = TI / 4, BQ = TJ / 4;
    __shared__ __attribute__((aligned(16))) float xl[Q_KC * TI];
    __shared__ __attribute__((aligned(16))) float dl[Q_KC * TJ];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, col = lane & 31, kh = lane >> 5;
    const int tap = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int ci0 = (tile / tiles_co) * TI, co0 = (tile % tiles_co) * TJ;
    const unsigned r0 = blockIdx.y * rows_per_split;
    const unsigned r1 = (M - r0 > rows_per_split) ? r0 + rows_per_split : M;          // (r0 < M: the grid has no empty split)
    const int ac4 = (tid % AQ) * 4, arow = tid / AQ, bc4 = (tid % BQ) * 4, brow = tid / BQ;
    const bool ci_ok = ci0 + ac4 < Ci, co_ok = co0 + bc4 < Co;
    const int W = 2 * Wo;
    const long toff = ((long)(tap >> 1) * W + (tap & 1)) * ldx + ci0 + ac4;
    float4 ta[4], tb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ta[j] = (txa != nullptr && ci_ok) ? txa[ci0 + ac4 + j] : make_float4(0.f, 0.f, 0.f, 0.f);
        tb[j] = (txb != nullptr && co_ok) ? txb[co0 + bc4 + j] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 ax[ASL], bx[BSL];
    auto load_chunk = [&](unsigned r) {
#pragma unroll
        for (int i = 0; i < ASL; ++i) {
            const unsigned m = r + i * (256 / AQ) + arow;
            ax[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ci_ok && m < r1) {
                const unsigned wo = m % (unsigned)Wo, q = m / (unsigned)Wo, ho = q % (unsigned)Ho, n = q / (unsigned)Ho;
                const long pix = ((long)n * 2 * Ho + 2 * ho) * W + 2 * wo;
                float4 v = *reinterpret_cast<const float4*>(x + pix * ldx + toff);
                if (txa != nullptr) { v.x = umi_tx(v.x, ta[0]); v.y = umi_tx(v.y, ta[1]); v.z = umi_tx(v.z, ta[2]); v.w = umi_tx(v.w, ta[3]); }
                ax[i] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < BSL; ++i) {
            const unsigned m = r + i * (256 / BQ) + brow;
            bx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (co_ok && m < r1) {
                float4 v = *reinterpret_cast<const float4*>(dy + (long)m * lddy + co0 + bc4);
                if (txb != nullptr) { v.x = umi_tx(v.x, tb[0]); v.y = umi_tx(v.y, tb[1]); v.z = umi_tx(v.z, tb[2]); v.w = umi_tx(v.w, tb[3]); }
                bx[i] = v;
            }
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
    for (unsigned r = r0; r < r1; r += Q_KC) {
        store_chunk();
        __syncthreads();
        if (r1 - r > Q_KC) load_chunk(r + Q_KC);
        wgrad_tile_multiply(acc, pa, pb);
        __syncthreads();
    }
    // slab [split][tap][ci][co]: lanes along co
#pragma unroll
    for (int b = 0; b < NT; ++b) {
        const int co = co0 + (wj * NT + b) * 32 + col;
        if (co >= Co) continue;
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int ci = ci0 + (wi * MT + a) * 32 + d_row(q, kh);
                if (ci < Ci) ws[(((long)blockIdx.y * 4 + tap) * Ci + ci) * Co + co] = acc[a][b][q];
            }
    }
}

bool flags_ok(int flags) {
    return (flags & UMI_CONV_F32_MFMA_2X2) && !(flags & (UMI_CONV_FORCE_GENERIC | UMI_CONV_DGRAD_STRIDED | UMI_CONV_ACCUMULATE));
}

}  // namespace

bool umi_convt_f32_mfma_ok(const ConvFwdProblem& p) {
    if (!flags_ok(p.flags)) return false;
    if (p.in_dtype != UMI_F32 || p.out_dtype != UMI_F32) return false;
    if (p.R != 2 || p.S != 2 || p.stride != 2 || p.pad != 0) return false;
    if (p.flags & UMI_CONV_UPSAMPLE2) {
        if (p.Ho != p.H || p.Wo != p.W) return false;
    } else if (p.H != 2 * p.Ho || p.W != 2 * p.Wo) {
        return false;
    }
    if (p.Ci % 8 || p.Co % 8 || p.ldx % 4 || p.ldy % 4) return false;        // partial channel tiles are masked in the kernel
    // addresses are 64-bit; a row index is 32-bit and (row tile, column tile) is one grid dimension
    const long M = (long)p.N * p.Ho * p.Wo;
    if (M >= (1L << 31) - P_TM || (long)umi_cdiv(M, P_TM) * 4 * umi_cdiv(p.Co, 64) >= (1L << 31)) return false;
    return true;
}

int umi_convt_f32_mfma(const ConvFwdProblem& p, const void* x, const void* tx, const void* wp, const float* bias, void* y,
                       int off_h, int off_w, int out_H, int out_W, hipStream_t s) {
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)wp | (uintptr_t)tx) & 15) return UMI_ERR_BADARG;
    const bool up = p.flags & UMI_CONV_UPSAMPLE2;
    // the scattered window must lie inside the out_H x out_W image
    if (up && (off_h < 0 || off_w < 0 || 2L * p.H + off_h > out_H || 2L * p.W + off_w > out_W)) return UMI_ERR_BADARG;
    const long M = (long)p.N * p.Ho * p.Wo;
    const bool narrow = fwd_narrow(M, p.Co, up ? 4 : 1);
    const int ctiles = umi_cdiv(p.Co, narrow ? 64 : 128);
    const CtGeo g{p.Ho, p.Wo, out_H, out_W, off_h, off_w};
    dim3 grid((unsigned)((long)umi_cdiv(M, P_TM) * ctiles * (up ? 4 : 1))), block(256);
#define UMI_CONVT_F32(WM, WN, MT, NT, UP)                                                                                      \
    hipLaunchKernelGGL((convt_f32_mfma_kernel<WM, WN, MT, NT, UP>), grid, block, 0, s, (const float*)x, p.ldx, (const float4*)tx, \
                       (const float*)wp, bias, (float*)y, p.ldy, (unsigned)M, p.Ci, p.Co, ctiles, g)
    if (narrow) {
        if (up) UMI_CONVT_F32(4, 1, 1, 2, true); else UMI_CONVT_F32(4, 1, 1, 2, false);
    } else {
        if (up) UMI_CONVT_F32(2, 2, 2, 2, true); else UMI_CONVT_F32(2, 2, 2, 2, false);
    }
#undef UMI_CONVT_F32
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

bool umi_wgrad_convt_f32_mfma_ok(const WgradProblem& p) {
    if (!flags_ok(p.flags) || (p.flags & UMI_CONV_UPSAMPLE2)) return false;
    if (p.dtype != UMI_F32) return false;
    if (p.R != 2 || p.S != 2 || p.stride != 2 || p.pad != 0 || p.H != 2 * p.Ho || p.W != 2 * p.Wo) return false;
    if (p.Ci % 8 || p.Co % 8 || p.ldx % 4 || p.lddy % 4) return false;
    // addresses are 64-bit; a pixel index is 32-bit, (tap, tile) and the split index are grid dimensions (at most 128 splits)
    if ((long)p.N * p.Ho * p.Wo >= (1L << 31) - 64 * Q_KC || 4L * umi_cdiv(p.Ci, 64) * umi_cdiv(p.Co, 64) >= (1L << 31)) return false;
    return true;
}

size_t umi_wgrad_convt_f32_mfma_ws_bound(const WgradProblem& facts) {
    if (!(facts.flags & UMI_CONV_F32_MFMA_2X2)) return 0;
    WgradProblem p = facts;
    p.H = 2 * p.Ho; p.W = 2 * p.Wo; p.stride = 2; p.pad = 0; p.ldx = p.lddy = 4;
    if (!umi_wgrad_convt_f32_mfma_ok(p)) return 0;
    int ti, tj, splits;
    long rps;
    wgrad_plan((long)p.N * p.Ho * p.Wo, p.Ci, p.Co, 4, &ti, &tj, &splits, &rps);
    return (size_t)splits * 4 * p.Ci * p.Co * sizeof(float);
}

int umi_wgrad_convt_f32_mfma(const WgradProblem& p, const void* x, const void* txa, const void* dy, const void* txb,
                             const WgradOut& o, hipStream_t s) {
    const long M = (long)p.N * p.Ho * p.Wo;
    int ti, tj, splits;
    long rps;
    wgrad_plan(M, p.Ci, p.Co, 4, &ti, &tj, &splits, &rps);
    if (o.ws_bytes < (size_t)splits * 4 * p.Ci * p.Co * sizeof(float)) return UMI_ERR_WORKSPACE;
    if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)txa | (uintptr_t)txb) & 15) return UMI_ERR_BADARG;
    const int tiles_co = umi_cdiv(p.Co, tj), tiles = umi_cdiv(p.Ci, ti) * tiles_co;
    dim3 grid((unsigned)(4 * tiles), (unsigned)splits), block(256);
#define UMI_WGRAD_CONVT_F32(MT, NT)                                                                                            \
    hipLaunchKernelGGL((convt_wgrad_f32_mfma_kernel<MT, NT>), grid, block, 0, s, (const float*)x, p.ldx, (const float4*)txa,    \
                       (const float*)dy, p.lddy, (const float4*)txb, (float*)o.ws, (unsigned)M, p.Ho, p.Wo, p.Ci, p.Co, tiles_co, \
                       tiles, (unsigned)rps)
    if (ti == 64 && tj == 64) UMI_WGRAD_CONVT_F32(1, 1);
    else if (ti == 64) UMI_WGRAD_CONVT_F32(1, 2);
    else if (tj == 64) UMI_WGRAD_CONVT_F32(2, 1);
    else UMI_WGRAD_CONVT_F32(2, 2);
#undef UMI_WGRAD_CONVT_F32
    UMI_LAUNCH_CHECK();
    umi_launch_wgrad_reduce(splits, 4, p.Ci, p.Co, o, s);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
