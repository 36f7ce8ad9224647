// Test-time augmentation over the eight rot90 / flip symmetries of the square, and model ensembles (statement: umi/tta.py).
//
//   umi_tta_views        x [N][C][H][W] -> the views of a list of elements, [V*N][C][H'][W'], view-major.
//   umi_tta_accumulate   acc [N][K][H][W] += the outputs [V*N][K][H'][W'] of those views, mapped back and transformed by the mode
//                        (logit: as is; relu: 0 where < 0; prob: softmax over K, sigmoid for K = 1).  Every acc pixel is owned by one
//                        thread, which walks the call's views in order with the K sums in registers: one read and one write of acc
//                        per call, no atomics, the summation order of the list.
//   umi_tta_finish       acc / float(count) in place, optionally the uint8 mask of the mean and the entropy of the mean probabilities.
//
// Element e: k = e & 3 quarter turns (np.rot90), then a flip of the last axis if e >> 2.  An element list travels by value, 4 bits per
// element in one 64-bit integer.  Elements with odd k transpose: a 32 x 32 tile goes through LDS so that the global reads run along
// the rows of the tensor read and the global writes (or the owning threads of acc) along the rows of the tensor written.  The tile
// is padded to 33 floats per row: ds_read_b32 / ds_write_b32 bank on (address / 4) % 32 within 32-lane halves, and the
// transposed read of lane l touches word l * 33 + c, bank (l + c) % 32 -- 32 distinct banks.  Elements with even k only reverse rows and
// / or columns: no LDS, and four pixels per lane as one 16-byte access (components reversed in registers) where W % 4 == 0 and the
// pointers are 16-byte aligned.
#include "common.h"

namespace {

constexpr int TT_MAX_K = 32, TT_MAX_VIEWS = 16, TT_MAX_PLANES = 65535, TT_TILE = 32;
constexpr unsigned TT_BM_CUTOFF_BITS = 0xB43FFFFEu;      // umi_binary_mask's cut-off, -0x1.7ffffcp-23

__device__ __forceinline__ int tt_elem(long long elems, int s) { return (int)((elems >> (4 * s)) & 7); }

// view pixel (i, j) of element e shows image pixel (y, x): umi.tta.view_source
__device__ __forceinline__ void tt_source(int e, int H, int W, int i, int j, int& y, int& x) {
    const int Wv = (e & 1) ? H : W;
    const int jp = (e >> 2) ? Wv - 1 - j : j;
    switch (e & 3) {
        case 0: y = i; x = jp; break;
        case 1: y = jp; x = W - 1 - i; break;
        case 2: y = H - 1 - i; x = W - 1 - jp; break;
        default: y = H - 1 - jp; x = i; break;
    }
}

// its inverse: image pixel (y, x) is view pixel (i, j)
__device__ __forceinline__ void tt_target(int e, int H, int W, int y, int x, int& i, int& j) {
    const int Wv = (e & 1) ? H : W;
    int jp;
    switch (e & 3) {
        case 0: i = y; jp = x; break;
        case 1: i = W - 1 - x; jp = y; break;
        case 2: i = H - 1 - y; jp = W - 1 - x; break;
        default: i = x; jp = H - 1 - y; break;
    }
    j = (e >> 2) ? Wv - 1 - jp : jp;
}

// ---- views ------------------------------------------------------------------------------------------------------------------------
// Any mix of elements of one output shape.  grid (tiles of the view, N * C, V), 256 threads = 32 columns x 8 rows, four rows each.
__global__ __launch_bounds__(256) void tta_view_tile_kernel(const float* __restrict__ x, int NC, int H, int W, float* __restrict__ out,
                                                            long long elems) {
    __shared__ float lds[TT_TILE][TT_TILE + 1];
    const int e = tt_elem(elems, blockIdx.z);
    const int Hv = (e & 1) ? W : H, Wv = (e & 1) ? H : W;
    const int tj = (Wv + TT_TILE - 1) / TT_TILE;
    const int i0 = (blockIdx.x / tj) * TT_TILE, j0 = (blockIdx.x % tj) * TT_TILE;
    const long HW = (long)H * W;
    const float* src = x + (long)blockIdx.y * HW;
    float* dst = out + ((long)blockIdx.z * NC + blockIdx.y) * HW;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    if (e & 1) {
        // lanes run along i: the image column x = W - 1 - i or i, so a wavefront reads two runs of 32 consecutive floats
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jl = ty + 8 * r, i = i0 + tx, j = j0 + jl;
            if (i < Hv && j < Wv) {
                int y, xx;
                tt_source(e, H, W, i, j, y, xx);
                lds[jl][tx] = src[(long)y * W + xx];
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int il = ty + 8 * r, i = i0 + il, j = j0 + tx;
            if (i < Hv && j < Wv) dst[(long)i * Wv + j] = lds[tx][il];
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + ty + 8 * r, j = j0 + tx;
            if (i < Hv && j < Wv) {
                int y, xx;
                tt_source(e, H, W, i, j, y, xx);
                dst[(long)i * Wv + j] = src[(long)y * W + xx];
            }
        }
    }
}

// Even elements only, W % 4 == 0, both pointers 16-byte aligned: a thread = four consecutive pixels of a view row, which are four
// consecutive pixels of an image row in the same or the reverse order.  grid (H * W / 4 / 256, N * C, V)
__global__ __launch_bounds__(256) void tta_view_row4_kernel(const float* __restrict__ x, int NC, int H, int W, float* __restrict__ out,
                                                            long long elems) {
    const int e = tt_elem(elems, blockIdx.z);
    const int gw = W >> 2;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= H * gw) return;
    const int i = g / gw, j0 = (g - i * gw) * 4;
    int y, xa, yb, xb;
    tt_source(e, H, W, i, j0, y, xa);
    tt_source(e, H, W, i, j0 + 3, yb, xb);
    const long HW = (long)H * W;
    const float4 q = *reinterpret_cast<const float4*>(x + (long)blockIdx.y * HW + (long)y * W + min(xa, xb));
    *reinterpret_cast<float4*>(out + ((long)blockIdx.z * NC + blockIdx.y) * HW + (long)i * W + j0) =
        xa <= xb ? q : make_float4(q.w, q.z, q.y, q.x);
}

// ---- accumulate -------------------------------------------------------------------------------------------------------------------
// One pixel's K outputs of one view -> what is added.  Every operation rounded on its own, as the statement's.
template <int KMAX>
__device__ __forceinline__ void tt_transform(float (&v)[KMAX], int K, int mode) {
#pragma clang fp contract(off)
    if (mode == 0) return;
    if (mode == 1) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) v[k] = v[k] < 0.f ? 0.f : v[k];                   // a NaN and -0.0 pass through
        return;
    }
    if (K == 1) {
        v[0] = __fdiv_rn(1.f, 1.f + expf(-v[0]));
        return;
    }
    float m = v[0];
#pragma unroll
    for (int k = 1; k < KMAX; ++k)
        if (k < K) m = fmaxf(m, v[k]);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < K) {
            v[k] = expf(v[k] - m);
            s += v[k];
        }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < K) v[k] = __fdiv_rn(v[k], s);
}

// Any mix of elements of one output shape.  grid (32 x 32 tiles of the image, N), 1024 threads, one acc pixel each: pixel (y0 + ty,
// x0 + tx) is owned, pixel (y0 + tx, x0 + ty) is what the thread stages for a transposing element -- there the lanes run along the
// view's rows.  The transform is applied before the staging, on the pixel's K values in registers.  LDS holds up to 4 channels of
// the tile at a time, twice: a staging writes the half the previous one did not, so ONE barrier per staging orders it (a thread
// writes a half again only after the barrier of the staging in between, which every thread reaches after its reads of that half).
// For K <= 8 the next view's values are loaded before this view's are used: the loads do not depend on one another, and a block
// would otherwise pay the latency of a load V times in a row.
template <int KMAX>
__global__ __launch_bounds__(1024) void tta_acc_tile_kernel(float* __restrict__ acc, int K, int H, int W, const float* __restrict__ yv,
                                                            int N, long long elems, int V, int mode) {
    constexpr int KC = KMAX < 4 ? KMAX : 4;
    constexpr bool PREFETCH = KMAX <= 8;
    __shared__ float lds[2][KC][TT_TILE][TT_TILE + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int tw = (W + TT_TILE - 1) / TT_TILE;
    const int y0 = (blockIdx.x / tw) * TT_TILE, x0 = (blockIdx.x % tw) * TT_TILE;
    const int n = blockIdx.y;
    const long HW = (long)H * W;
    const int y = y0 + ty, x = x0 + tx, ys = y0 + tx, xs = x0 + ty;
    const bool in = y < H && x < W, ins = ys < H && xs < W;
    float* ap = acc + (long)n * K * HW + (long)y * W + x;
    float a[KMAX], v[KMAX], nx[PREFETCH ? KMAX : 1];
    // the K values of view s at the pixel this thread handles for it: its own for an even element, the staged one for an odd
    auto load = [&](int s, float* dst) {
        const int e = tt_elem(elems, s);
        const float* vp = yv + ((long)s * N + n) * K * HW;
        int i, j;
        if (e & 1) {
            tt_target(e, H, W, ys, xs, i, j);                          // the view is [W][H]
#pragma unroll
            for (int k = 0; k < KMAX; ++k) dst[k] = (k < K && ins) ? vp[k * HW + (long)i * H + j] : 0.f;
        } else {
            tt_target(e, H, W, y, x, i, j);
#pragma unroll
            for (int k = 0; k < KMAX; ++k) dst[k] = (k < K && in) ? vp[k * HW + (long)i * W + j] : 0.f;
        }
    };
    if (PREFETCH) load(0, nx);
#pragma unroll
    for (int k = 0; k < KMAX; ++k) a[k] = (k < K && in) ? ap[k * HW] : 0.f;
    int half = 0;
    for (int s = 0; s < V; ++s) {
        if (PREFETCH) {
#pragma unroll
            for (int k = 0; k < KMAX; ++k) v[k] = nx[PREFETCH ? k : 0];
            if (s + 1 < V) load(s + 1, nx);
        } else load(s, v);
        tt_transform<KMAX>(v, K, mode);
        if (tt_elem(elems, s) & 1) {
#pragma unroll
            for (int c = 0; c < KMAX; c += KC) {
                if (c < K) {                                           // uniform over the block
#pragma unroll
                    for (int kk = 0; kk < KC; ++kk)
                        if (c + kk < K) lds[half][kk][ty][tx] = v[c + kk];
                    __syncthreads();
#pragma unroll
                    for (int kk = 0; kk < KC; ++kk)
                        if (c + kk < K) a[c + kk] += lds[half][kk][tx][ty];
                    half ^= 1;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < K) a[k] += v[k];
        }
    }
    if (in) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) ap[k * HW] = a[k];
    }
}

// Even elements only.  A thread = PX consecutive pixels of an image row, which are PX consecutive pixels of a view row in the same or
// the reverse order; PX = 4: W % 4 == 0 and both pointers 16-byte aligned.  grid (H * W / PX / 256, N)
template <int KMAX, int PX>
__global__ __launch_bounds__(256) void tta_acc_row_kernel(float* __restrict__ acc, int K, int H, int W, const float* __restrict__ yv,
                                                          int N, long long elems, int V, int mode) {
    const int gw = W / PX;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= H * gw) return;
    const int y = g / gw, x0 = (g - y * gw) * PX;
    const int n = blockIdx.y;
    const long HW = (long)H * W;
    float* ap = acc + (long)n * K * HW + (long)y * W + x0;
    float a[KMAX][PX], v[PX][KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
            if (PX == 4) {
                const float4 q = *reinterpret_cast<const float4*>(ap + k * HW);
                a[k][0] = q.x; a[k][PX > 1 ? 1 : 0] = q.y; a[k][PX > 2 ? 2 : 0] = q.z; a[k][PX > 3 ? 3 : 0] = q.w;
            } else a[k][0] = ap[k * HW];
        }
    }
    // the views' loads do not depend on one another: unrolled, the next views' are in flight while this one is transformed
    constexpr int UNROLL = KMAX * PX <= 8 ? 4 : KMAX * PX <= 16 ? 2 : 1;
#pragma unroll UNROLL
    for (int s = 0; s < V; ++s) {
        const int e = tt_elem(elems, s);
        int i, ja, ib, jb;
        tt_target(e, H, W, y, x0, i, ja);
        tt_target(e, H, W, y, x0 + PX - 1, ib, jb);
        const bool rev = ja > jb;
        const float* vp = yv + ((long)s * N + n) * K * HW + (long)i * W + min(ja, jb);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k < K) {
                if (PX == 4) {
                    const float4 q = *reinterpret_cast<const float4*>(vp + k * HW);
                    v[0][k] = rev ? q.w : q.x; v[PX > 1 ? 1 : 0][k] = rev ? q.z : q.y;
                    v[PX > 2 ? 2 : 0][k] = rev ? q.y : q.z; v[PX > 3 ? 3 : 0][k] = rev ? q.x : q.w;
                } else v[0][k] = vp[k * HW];
            }
        }
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            tt_transform<KMAX>(v[p], K, mode);
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < K) a[k][p] += v[p][k];
        }
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
            if (PX == 4) *reinterpret_cast<float4*>(ap + k * HW) = make_float4(a[k][0], a[k][PX > 1 ? 1 : 0], a[k][PX > 2 ? 2 : 0], a[k][PX > 3 ? 3 : 0]);
            else ap[k * HW] = a[k][0];
        }
    }
}

// ---- finish -----------------------------------------------------------------------------------------------------------------------
// A thread = PX consecutive pixels, all K planes.  grid (H * W / PX / 256, N)
template <int PX>
__global__ __launch_bounds__(256) void tta_finish_kernel(float* __restrict__ acc, int K, long HW, float count, int mode,
                                                         unsigned char* __restrict__ mask, float* __restrict__ entropy) {
#pragma clang fp contract(off)
    const long p = ((long)blockIdx.x * 256 + threadIdx.x) * PX;
    if (p >= HW) return;
    const int n = blockIdx.y;
    float* ap = acc + (long)n * K * HW + p;
    float best[PX], h[PX];
    unsigned char bi[PX];
#pragma unroll
    for (int e = 0; e < PX; ++e) { best[e] = 0.f; h[e] = 0.f; bi[e] = 0; }
    for (int k = 0; k < K; ++k) {
        float v[PX];
        if (PX == 4) {
            const float4 q = *reinterpret_cast<const float4*>(ap + k * HW);
            v[0] = q.x; v[PX > 1 ? 1 : 0] = q.y; v[PX > 2 ? 2 : 0] = q.z; v[PX > 3 ? 3 : 0] = q.w;
        } else v[0] = ap[k * HW];
#pragma unroll
        for (int e = 0; e < PX; ++e) {
            v[e] = __fdiv_rn(v[e], count);
            if (k == 0) { best[e] = v[e]; bi[e] = 0; }
            else if (v[e] > best[e]) { best[e] = v[e]; bi[e] = (unsigned char)k; }       // first maximum wins (umi_argmax_mask)
            if (entropy) {
                if (v[e] > 0.f) h[e] -= v[e] * logf(v[e]);
                if (K == 1) {
                    const float q = 1.f - v[e];
                    if (q > 0.f) h[e] -= q * logf(q);
                }
            }
        }
        if (PX == 4) *reinterpret_cast<float4*>(ap + k * HW) = make_float4(v[0], v[PX > 1 ? 1 : 0], v[PX > 2 ? 2 : 0], v[PX > 3 ? 3 : 0]);
        else ap[k * HW] = v[0];
    }
    if (mask) {
        if (K == 1) {
            const float cut = mode == 2 ? 0.5f : __builtin_bit_cast(float, TT_BM_CUTOFF_BITS);
#pragma unroll
            for (int e = 0; e < PX; ++e) bi[e] = best[e] >= cut ? 1 : 0;                 // NaN compares false: 0 (umi_binary_mask)
        }
        unsigned char* mp = mask + (long)n * HW + p;
        if (PX == 4) *reinterpret_cast<uchar4*>(mp) = make_uchar4(bi[0], bi[PX > 1 ? 1 : 0], bi[PX > 2 ? 2 : 0], bi[PX > 3 ? 3 : 0]);
        else mp[0] = bi[0];
    }
    if (entropy) {
        float* ep = entropy + (long)n * HW + p;
        if (PX == 4) *reinterpret_cast<float4*>(ep) = make_float4(h[0], h[PX > 1 ? 1 : 0], h[PX > 2 ? 2 : 0], h[PX > 3 ? 3 : 0]);
        else ep[0] = h[0];
    }
}

// the element list: V nibbles in 0..7, nothing above them; parity = 0 all even, 1 all odd, 2 mixed
int tt_elems(long long elems, int V, int& parity) {
    if (V < 1 || V > TT_MAX_VIEWS || elems < 0) return UMI_ERR_BADARG;
    if (V < 16 && (elems >> (4 * V)) != 0) return UMI_ERR_BADARG;
    int odd = 0;
    for (int s = 0; s < V; ++s) {
        const int nib = (int)((elems >> (4 * s)) & 15);
        if (nib > 7) return UMI_ERR_BADARG;
        odd += nib & 1;
    }
    parity = odd == 0 ? 0 : odd == V ? 1 : 2;
    return UMI_OK;
}

int tt_sizes(int N, int C, int H, int W, int V, long planes) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return UMI_ERR_BADARG;
    if ((__int128)V * N * C * H * W >= ((__int128)1 << 31)) return UMI_ERR_UNSUPPORTED;
    if (planes > TT_MAX_PLANES) return UMI_ERR_UNSUPPORTED;
    return UMI_OK;
}

template <int KMAX>
void tt_launch_acc(bool rows, bool wide, dim3 grid_rows, dim3 grid_tiles, hipStream_t s, float* acc, int K, int H, int W, const float* y,
                   int N, long long elems, int V, int mode) {
    if (!rows) hipLaunchKernelGGL((tta_acc_tile_kernel<KMAX>), grid_tiles, dim3(1024), 0, s, acc, K, H, W, y, N, elems, V, mode);
    else if (wide && KMAX <= 8)
        hipLaunchKernelGGL((tta_acc_row_kernel<(KMAX <= 8 ? KMAX : 1), 4>), grid_rows, dim3(256), 0, s, acc, K, H, W, y, N, elems, V, mode);
    else hipLaunchKernelGGL((tta_acc_row_kernel<KMAX, 1>), grid_rows, dim3(256), 0, s, acc, K, H, W, y, N, elems, V, mode);
}

}  // namespace

extern "C" int umi_tta_views(const float* x, int N, int C, int H, int W, float* out, long long elems, int V, umi_stream_t stream) {
    if (!x || !out || ((unsigned long)x & 3) || ((unsigned long)out & 3)) return UMI_ERR_BADARG;
    int parity = 0;
    int st = tt_elems(elems, V, parity);
    if (st) return st;
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || (parity == 2 && H != W)) return UMI_ERR_BADARG;
    st = tt_sizes(N, C, H, W, V, (long)N * C);
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    if (parity == 0 && W % 4 == 0 && (((unsigned long)x | (unsigned long)out) & 15) == 0) {
        const dim3 grid((unsigned)(((long)H * (W / 4) + 255) / 256), (unsigned)(N * C), (unsigned)V);
        hipLaunchKernelGGL(tta_view_row4_kernel, grid, dim3(256), 0, s, x, N * C, H, W, out, elems);
    } else {
        const int Hv = parity == 1 ? W : H, Wv = parity == 1 ? H : W;          // mixed: H == W
        const dim3 grid((unsigned)(umi_cdiv(Hv, TT_TILE) * umi_cdiv(Wv, TT_TILE)), (unsigned)(N * C), (unsigned)V);
        hipLaunchKernelGGL(tta_view_tile_kernel, grid, dim3(256), 0, s, x, N * C, H, W, out, elems);
    }
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_tta_accumulate(float* acc, int N, int K, int H, int W, const float* y, long long elems, int V, int mode,
                                  umi_stream_t stream) {
    if (!acc || !y || ((unsigned long)acc & 3) || ((unsigned long)y & 3) || mode < 0 || mode > 2) return UMI_ERR_BADARG;
    int parity = 0;
    int st = tt_elems(elems, V, parity);
    if (st) return st;
    if (N <= 0 || K <= 0 || H <= 0 || W <= 0 || (parity == 2 && H != W)) return UMI_ERR_BADARG;
    if (K > TT_MAX_K) return UMI_ERR_UNSUPPORTED;
    st = tt_sizes(N, K, H, W, V, (long)N);
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    const bool rows = parity == 0;
    const bool wide = W % 4 == 0 && (((unsigned long)acc | (unsigned long)y) & 15) == 0;
    const int px = wide && K <= 8 ? 4 : 1;
    const dim3 grid_rows((unsigned)(((long)H * (W / px) + 255) / 256), (unsigned)N);
    const dim3 grid_tiles((unsigned)(umi_cdiv(H, TT_TILE) * umi_cdiv(W, TT_TILE)), (unsigned)N);
    if (K == 1) tt_launch_acc<1>(rows, wide, grid_rows, grid_tiles, s, acc, K, H, W, y, N, elems, V, mode);
    else if (K == 2) tt_launch_acc<2>(rows, wide, grid_rows, grid_tiles, s, acc, K, H, W, y, N, elems, V, mode);
    else if (K <= 4) tt_launch_acc<4>(rows, wide, grid_rows, grid_tiles, s, acc, K, H, W, y, N, elems, V, mode);
    else if (K <= 8) tt_launch_acc<8>(rows, wide, grid_rows, grid_tiles, s, acc, K, H, W, y, N, elems, V, mode);
    else if (K <= 16) tt_launch_acc<16>(rows, wide, grid_rows, grid_tiles, s, acc, K, H, W, y, N, elems, V, mode);
    else tt_launch_acc<32>(rows, wide, grid_rows, grid_tiles, s, acc, K, H, W, y, N, elems, V, mode);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_tta_finish(float* acc, int N, int K, int H, int W, int count, int mode, unsigned char* mask, float* entropy,
                              umi_stream_t stream) {
    if (!acc || ((unsigned long)acc & 3) || ((unsigned long)entropy & 3) || mode < 0 || mode > 2 || count < 1) return UMI_ERR_BADARG;
    if (N <= 0 || K <= 0 || H <= 0 || W <= 0 || (entropy && mode != 2)) return UMI_ERR_BADARG;
    if (K > TT_MAX_K) return UMI_ERR_UNSUPPORTED;
    const int st = tt_sizes(N, K, H, W, 1, (long)N);
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    const long HW = (long)H * W;
    const bool wide = HW % 4 == 0 && (((unsigned long)acc | (unsigned long)entropy) & 15) == 0 && ((unsigned long)mask & 3) == 0;
    const dim3 grid((unsigned)(((wide ? HW / 4 : HW) + 255) / 256), (unsigned)N);
    if (wide) hipLaunchKernelGGL((tta_finish_kernel<4>), grid, dim3(256), 0, s, acc, K, HW, (float)count, mode, mask, entropy);
    else hipLaunchKernelGGL((tta_finish_kernel<1>), grid, dim3(256), 0, s, acc, K, HW, (float)count, mode, mask, entropy);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
