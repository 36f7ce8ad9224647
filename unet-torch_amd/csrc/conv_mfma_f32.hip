// fp32 3x3 / stride 1 / pad 1 convolution (forward = data gradient, and weight gradient) on the fp32-input matrix-core
// instruction of gfx950, v_mfma_f32_32x32x2_f32.  Opt-in: UMI_CONV_F32_MFMA (include/unetmi.h); without the flag, or on a problem
// the predicates below refuse, the call runs exactly as before.
//
// Numerics.  The instruction multiplies fp32 by fp32 and accumulates in fp32 with one rounding per product: D = fma(a_k1, b_k1,
// fma(a_k0, b_k0, C)).  So an output here is ONE fmaf chain, the same arithmetic as the VALU kernels of generic_kernels.hip in
// another order; no floating-point atomics anywhere, identical inputs give identical bits.
//   forward / data gradient: k runs over input-channel chunks of 8 (ascending), inside a chunk over the 9 taps (r-major), inside a
//     tap over the chunk's 8 channels (ascending).  One accumulator per output from the first product to the last: no partial
//     sums are merged.
//   weight gradient: k runs over pixels; a split owns a contiguous range of (image, row, 32-column segment) items in that order,
//     inside an item columns ascend.  One accumulator per (tap, ci, co) and split; the splits' slabs [split][tap][ci][co] are
//     then summed by umi_launch_wgrad_reduce in its fixed order (lane l of 8 sums splits l, l + 8, ..., lanes added in order).
#include "kernels.h"
#include "mfma_f32.h"

namespace {

// ---- forward ------------------------------------------------------------------------------------------------------------------
// D[co][pixel] += W[co][k] * X[k][pixel].  A workgroup (4 waves) owns 8 rows x 32 columns of one image and 64 output channels; a
// wave owns 2 of the rows: 2 x 2 tiles of 32 co x 32 pixels = 4 independent accumulators.  Per chunk of 8 input channels the
// 10 x 34 halo tile ([pixel][channel], 9 dwords per pixel: the B operand's 32 lanes stride by one pixel and so fall on 32
// distinct banks) and the 9 x 8 x 64 weights ([tap][k][co] as packed: the A operand's lanes run along co) are staged in LDS; the
// next chunk's global loads are in flight while the current one is multiplied.
constexpr int F_TH = 8, F_TW = 32, F_HH = F_TH + 2, F_HW = F_TW + 2, F_KC = 8, F_XS = F_KC + 1, F_CO = 64;
constexpr int F_HSLOTS = F_HH * F_HW * 2;            // float4 loads of a halo chunk: 680, 3 per thread
constexpr int F_WSLOTS = 9 * F_KC * F_CO / 4;        // float4 loads of a weight chunk: 1,152, 5 per thread

template <bool HAS_TX>
__global__ __launch_bounds__(256) void conv3x3_f32_mfma_kernel(const float* __restrict__ x, int ldx, const float4* __restrict__ tx,
                                                               const float* __restrict__ wp, float* __restrict__ y, int ldy,
                                                               float* __restrict__ part, int H, int W, int Ci, int Co,
                                                               int tilesH, int tilesW) {
    __shared__ float xl[F_HH * F_HW * F_XS];
    __shared__ __attribute__((aligned(16))) float wl[9 * F_KC * F_CO];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, col = lane & 31, kh = lane >> 5;
    const int bx = blockIdx.x;
    const int tw = bx % tilesW, th = (bx / tilesW) % tilesH, n = bx / (tilesW * tilesH);
    const int h0 = th * F_TH, w0 = tw * F_TW, co0 = blockIdx.y * F_CO;
    const float* xn = x + (long)n * H * W * ldx;

    // what this thread stages: 3 halo slots (pixel, channel quad tid & 1) and 5 weight slots (row = tap * 8 + k, co quad)
    long hoff[3], woff[5];
    bool hin[3], wok[5];
    int hdst[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int slot = i * 256 + tid, pix = slot >> 1, q = slot & 1;
        const int hh = pix / F_HW, ww = pix - hh * F_HW;
        const int gh = h0 - 1 + hh, gw = w0 - 1 + ww;
        hin[i] = slot < F_HSLOTS && gh >= 0 && gh < H && gw >= 0 && gw < W;
        const int ghc = min(max(gh, 0), H - 1), gwc = min(max(gw, 0), W - 1);     // an address inside the image in every case
        hoff[i] = ((long)ghc * W + gwc) * ldx + q * 4;
        hdst[i] = slot < F_HSLOTS ? pix * F_XS + q * 4 : -1;
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int slot = i * 256 + tid, row = slot >> 4, c4 = slot & 15;
        wok[i] = slot < F_WSLOTS && co0 + c4 * 4 < Co;
        woff[i] = ((long)(row >> 3) * Ci + (row & 7)) * Co + co0 + c4 * 4;
    }
    float4 hx[3], wx[5];
    auto load_chunk = [&](int ci0) {
        float4 t[4];
        if (HAS_TX) {
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = tx[ci0 + (tid & 1) * 4 + j];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            float4 v = *reinterpret_cast<const float4*>(xn + hoff[i] + ci0);
            if (HAS_TX) { v.x = umi_tx(v.x, t[0]); v.y = umi_tx(v.y, t[1]); v.z = umi_tx(v.z, t[2]); v.w = umi_tx(v.w, t[3]); }
            hx[i] = hin[i] ? v : make_float4(0.f, 0.f, 0.f, 0.f);               // the transform first, the zero padding after it
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            wx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (wok[i]) wx[i] = *reinterpret_cast<const float4*>(wp + woff[i] + (long)ci0 * Co);
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (hdst[i] >= 0) {
                float* d = xl + hdst[i];
                d[0] = hx[i].x; d[1] = hx[i].y; d[2] = hx[i].z; d[3] = hx[i].w;
            }
#pragma unroll
        for (int i = 0; i < 5; ++i)
            if (i * 256 + tid < F_WSLOTS) *reinterpret_cast<float4*>(wl + (i * 256 + tid) * 4) = wx[i];
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][p][r] = 0.f;

    load_chunk(0);
    for (int ci0 = 0; ci0 < Ci; ci0 += F_KC) {
        store_chunk();
        __syncthreads();
        if (ci0 + F_KC < Ci) load_chunk(ci0 + F_KC);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int r = tap / 3, s = tap - r * 3;
            const float* wa = wl + (tap * F_KC + kh) * F_CO + col;
            const float* xb = xl + ((2 * wv + r) * F_HW + col + s) * F_XS + kh;
#pragma unroll
            for (int kk = 0; kk < F_KC / 2; ++kk) {
                const float a0 = wa[2 * kk * F_CO], a1 = wa[2 * kk * F_CO + 32];
                const float b0 = xb[2 * kk], b1 = xb[F_HW * F_XS + 2 * kk];
                acc[0][0] = mfma32(a0, b0, acc[0][0]);
                acc[0][1] = mfma32(a0, b1, acc[0][1]);
                acc[1][0] = mfma32(a1, b0, acc[1][0]);
                acc[1][1] = mfma32(a1, b1, acc[1][1]);
            }
        }
        __syncthreads();
    }

    // epilogue: this lane holds pixel (h0 + 2 wv + p, w0 + col), channels co0 + 32 m + d_row(reg, kh): 4 consecutive per 16-B store
    const int gw = w0 + col;
    bool pv[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int gh = h0 + 2 * wv + p;
        pv[p] = gh < H && gw < W;
        if (!pv[p]) continue;
        float* yp = y + (((long)n * H + gh) * W + gw) * ldy;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = co0 + 32 * m + 8 * g + 4 * kh;
                if (co < Co)
                    *reinterpret_cast<float4*>(yp + co) =
                        make_float4(acc[m][p][4 * g], acc[m][p][4 * g + 1], acc[m][p][4 * g + 2], acc[m][p][4 * g + 3]);
            }
    }
    if (part == nullptr) return;
    // BatchNorm partial sums of the stored values: per channel over the wave's pixels (a fixed butterfly over the 32 lanes of a
    // half wave), then over the 4 waves in wave order.  One row of part[rows][2][Co] per pixel tile.
    float* red = wl;                                  // [4 waves][2][64]: the weights are dead (barrier at the loop's end)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v0 = pv[0] ? acc[m][0][r] : 0.f, v1 = pv[1] ? acc[m][1][r] : 0.f;
            float s = v0 + v1, q = fmaf(v1, v1, v0 * v0);
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) {
                s += __shfl_xor(s, d, 64);
                q += __shfl_xor(q, d, 64);
            }
            if (col == 0) {
                red[(wv * 2 + 0) * F_CO + 32 * m + d_row(r, kh)] = s;
                red[(wv * 2 + 1) * F_CO + 32 * m + d_row(r, kh)] = q;
            }
        }
    __syncthreads();
    if (tid < 2 * F_CO) {
        const int which = tid >> 6, c = tid & 63;
        float s = red[(0 * 2 + which) * F_CO + c];
#pragma unroll
        for (int w = 1; w < 4; ++w) s += red[(w * 2 + which) * F_CO + c];
        if (co0 + c < Co) part[((long)bx * 2 + which) * Co + co0 + c] = s;
    }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
// dW[tap][ci][co] = sum over pixels of tx(x)[pixel + tap][ci] * dy[pixel][co]: M = ci, N = co, K = pixels.  Lanes run along the
// channels for both operands, so both are read straight from [pixel][channel] LDS rows.  A workgroup owns 64 ci x 64 co and the
// 3 taps of one kernel row r (blockIdx.y) over the items of one split (blockIdx.z); an item is 32 columns of one image row: dy
// [32][64] and x [34][64] (row h + r - 1, columns w0 - 1 .. w0 + 32).  Wave (ci half, co half) carries one accumulator per tap.
constexpr int G_P = 32, G_C = 64;
constexpr int G_XSLOTS = (G_P + 2) * G_C / 4;         // 544 float4, 3 per thread (the channel quad is tid & 15 in each)

template <bool HAS_TX>
__global__ __launch_bounds__(256) void wgrad3x3_f32_mfma_kernel(const float* __restrict__ x, int ldx, const float4* __restrict__ tx,
                                                                const float* __restrict__ dy, int lddy, float* __restrict__ ws,
                                                                int H, int W, int Ci, int Co, int tiles_co, int segsW, int items,
                                                                int ips) {
    __shared__ __attribute__((aligned(16))) float xl[(G_P + 2) * G_C];
    __shared__ __attribute__((aligned(16))) float dl[G_P * G_C];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, col = lane & 31, kh = lane >> 5;
    const int ci0 = (blockIdx.x / tiles_co) * G_C, co0 = (blockIdx.x % tiles_co) * G_C, r = blockIdx.y;
    const int it0 = blockIdx.z * ips, it1 = min(it0 + ips, items);
    const int c4 = (tid & 15) * 4, prow = tid >> 4;
    const bool ci_ok = ci0 + c4 < Ci, co_ok = co0 + c4 < Co;
    float4 t[4];
    if (HAS_TX) {
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = ci_ok ? tx[ci0 + c4 + j] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 ax[3], bx[2];
    auto load_item = [&](int it) {
        const int sg = it % segsW, hn = it / segsW, h = hn % H, n = hn / H;
        const int w0 = sg * G_P, hx = h + r - 1;
        const bool row_ok = hx >= 0 && hx < H;
        const float* xr = x + (((long)n * H + min(max(hx, 0), H - 1)) * W) * ldx + ci0 + c4;
        const float* dr = dy + (((long)n * H + h) * W) * lddy + co0 + c4;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int px = i * 16 + prow, wx = w0 - 1 + px;
            ax[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (px < G_P + 2 && row_ok && ci_ok && wx >= 0 && wx < W) {
                float4 v = *reinterpret_cast<const float4*>(xr + (long)wx * ldx);
                if (HAS_TX) { v.x = umi_tx(v.x, t[0]); v.y = umi_tx(v.y, t[1]); v.z = umi_tx(v.z, t[2]); v.w = umi_tx(v.w, t[3]); }
                ax[i] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int wy = w0 + i * 16 + prow;
            bx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (co_ok && wy < W) bx[i] = *reinterpret_cast<const float4*>(dr + (long)wy * lddy);
        }
    };
    auto store_item = [&]() {
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i * 16 + prow < G_P + 2) *reinterpret_cast<float4*>(xl + (i * 16 + prow) * G_C + c4) = ax[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<float4*>(dl + (i * 16 + prow) * G_C + c4) = bx[i];
    };

    const int cih = wv & 1, coh = wv >> 1;
    f32x16 acc[3];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[s][q] = 0.f;

    if (it0 < it1) load_item(it0);
    for (int it = it0; it < it1; ++it) {
        store_item();
        __syncthreads();
        if (it + 1 < it1) load_item(it + 1);
        const float* pa = xl + kh * G_C + cih * 32 + col;
        const float* pb = dl + kh * G_C + coh * 32 + col;
#pragma unroll
        for (int kk = 0; kk < G_P / 2; ++kk) {
            const float b = pb[2 * kk * G_C];
#pragma unroll
            for (int s = 0; s < 3; ++s) acc[s] = mfma32(pa[(2 * kk + s) * G_C], b, acc[s]);
        }
        __syncthreads();
    }
    // slab [split][tap][ci][co]: lanes along co
    const int co = co0 + coh * 32 + col;
    if (co < Co) {
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int ci = ci0 + cih * 32 + d_row(q, kh);
                if (ci < Ci) ws[(((long)blockIdx.z * 9 + r * 3 + s) * Ci + ci) * Co + co] = acc[s][q];
            }
    }
}

// the split of the pixel dimension: a function of the shape alone (umi_conv_wgrad_ws_bytes must give the same answer)
void wgrad_plan(int N, int H, int W, int Ci, int Co, int* segsW, int* items, int* splits, int* ips) {
    *segsW = umi_cdiv(W, G_P);
    *items = N * H * *segsW;
    const long tiles = (long)umi_cdiv(Ci, G_C) * umi_cdiv(Co, G_C) * 3;
    long want = (1024 + tiles - 1) / tiles;              // aim for >= 1,024 workgroups ...
    const long most = umi_cdiv(*items, 4);               // ... of at least 4 items each
    if (want > most) want = most;
    if (want < 1) want = 1;
    *ips = umi_cdiv(*items, want);
    *splits = umi_cdiv(*items, *ips);
}

}  // namespace

bool umi_conv3x3_f32_mfma_ok(const ConvFwdProblem& p) {
    if (!(p.flags & UMI_CONV_F32_MFMA)) return false;
    if (p.flags & (UMI_CONV_UPSAMPLE2 | UMI_CONV_FORCE_GENERIC | UMI_CONV_DGRAD_STRIDED | UMI_CONV_ACCUMULATE)) return false;
    if (p.in_dtype != UMI_F32 || p.out_dtype != UMI_F32 || p.has_bias) return false;
    if (p.R != 3 || p.S != 3 || p.stride != 1 || p.pad != 1 || p.Ho != p.H || p.Wo != p.W) return false;
    if (p.Ci % 8 || p.Co % 8 || p.ldx % 4 || p.ldy % 4) return false;       // partial 64-channel output tiles are masked in the kernel
    // addresses are 64-bit; the pixel-tile index (8 x 32 tiles) and the co-tile index are grid dimensions
    if ((long)p.N * umi_cdiv(p.H, F_TH) * umi_cdiv(p.W, F_TW) >= (1L << 31) || umi_cdiv(p.Co, F_CO) > 65535) return false;
    return true;
}

int umi_conv3x3_f32_mfma_stat_rows(int N, int H, int W) { return N * umi_cdiv(H, F_TH) * umi_cdiv(W, F_TW); }

int umi_conv3x3_f32_mfma(const ConvFwdProblem& p, const void* x, const void* tx, const void* wp, void* y, float* stat_part,
                         hipStream_t s) {
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)wp | (uintptr_t)tx) & 15) return UMI_ERR_BADARG;
    const int tilesH = umi_cdiv(p.H, F_TH), tilesW = umi_cdiv(p.W, F_TW);
    dim3 grid((unsigned)(p.N * tilesH * tilesW), (unsigned)umi_cdiv(p.Co, F_CO)), block(256);
    if (tx)
        hipLaunchKernelGGL(conv3x3_f32_mfma_kernel<true>, grid, block, 0, s, (const float*)x, p.ldx, (const float4*)tx,
                           (const float*)wp, (float*)y, p.ldy, stat_part, p.H, p.W, p.Ci, p.Co, tilesH, tilesW);
    else
        hipLaunchKernelGGL(conv3x3_f32_mfma_kernel<false>, grid, block, 0, s, (const float*)x, p.ldx, (const float4*)nullptr,
                           (const float*)wp, (float*)y, p.ldy, stat_part, p.H, p.W, p.Ci, p.Co, tilesH, tilesW);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

bool umi_wgrad3x3_f32_mfma_ok(const WgradProblem& p) {
    if (!(p.flags & UMI_CONV_F32_MFMA)) return false;
    if (p.flags & (UMI_CONV_UPSAMPLE2 | UMI_CONV_FORCE_GENERIC | UMI_CONV_DGRAD_STRIDED | UMI_CONV_ACCUMULATE)) return false;
    if (p.dtype != UMI_F32 || p.has_txb) return false;
    if (p.R != 3 || p.S != 3 || p.stride != 1 || p.pad != 1 || p.Ho != p.H || p.Wo != p.W) return false;
    if (p.Ci % 8 || p.Co % 8 || p.ldx % 4 || p.lddy % 4) return false;
    // addresses are 64-bit; the item index (image, row, 32-column segment) is an int and the tile index a grid dimension
    if ((long)p.N * p.H * umi_cdiv(p.W, G_P) >= (1L << 31) || (long)umi_cdiv(p.Ci, G_C) * umi_cdiv(p.Co, G_C) >= (1L << 31)) return false;
    return true;
}

size_t umi_wgrad3x3_f32_mfma_ws_bound(const WgradProblem& facts) {
    if (!(facts.flags & UMI_CONV_F32_MFMA)) return 0;
    WgradProblem p = facts;
    p.H = p.Ho; p.W = p.Wo; p.stride = p.pad = 1; p.ldx = p.lddy = 4;
    if (!umi_wgrad3x3_f32_mfma_ok(p)) return 0;
    int segsW, items, splits, ips;
    wgrad_plan(p.N, p.H, p.W, p.Ci, p.Co, &segsW, &items, &splits, &ips);
    return (size_t)splits * 9 * p.Ci * p.Co * sizeof(float);
}

int umi_wgrad3x3_f32_mfma(const WgradProblem& p, const void* x, const void* txa, const void* dy, const WgradOut& o, hipStream_t s) {
    int segsW, items, splits, ips;
    wgrad_plan(p.N, p.H, p.W, p.Ci, p.Co, &segsW, &items, &splits, &ips);
    if (o.ws_bytes < (size_t)splits * 9 * p.Ci * p.Co * sizeof(float)) return UMI_ERR_WORKSPACE;
    if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)txa) & 15) return UMI_ERR_BADARG;
    const int tiles_co = umi_cdiv(p.Co, G_C);
    dim3 grid((unsigned)(umi_cdiv(p.Ci, G_C) * tiles_co), 3, (unsigned)splits), block(256);
    if (txa)
        hipLaunchKernelGGL(wgrad3x3_f32_mfma_kernel<true>, grid, block, 0, s, (const float*)x, p.ldx, (const float4*)txa,
                           (const float*)dy, p.lddy, (float*)o.ws, p.H, p.W, p.Ci, p.Co, tiles_co, segsW, items, ips);
    else
        hipLaunchKernelGGL(wgrad3x3_f32_mfma_kernel<false>, grid, block, 0, s, (const float*)x, p.ldx, (const float4*)nullptr,
                           (const float*)dy, p.lddy, (float*)o.ws, p.H, p.W, p.Ci, p.Co, tiles_co, segsW, items, ips);
    UMI_LAUNCH_CHECK();
    umi_launch_wgrad_reduce(splits, 9, p.Ci, p.Co, o, s);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
