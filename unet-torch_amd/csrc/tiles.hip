// Overlap-tile / sliding-window inference over an image larger than the network input (statement: umi/tiles.py).
//
//   umi_tile_gather   image [C][H][W] -> a chunk of tiles [n][C][th][tw], samples outside the image reflected (numpy.pad 'reflect',
//                     any pad width) or a constant; an empty slot (id < 0) is written as zeros.
//   umi_tile_blend    the chunk's logits [n][K][th][tw] -> the canvas [K][H][W]: acc += fp32(w * logit), w = fp32(wy[i] * wx[j]),
//                     tiles with w == 0 at a pixel skipped.  No atomics: the thread of the FIRST slot of the chunk that
//                     geometrically contains a canvas pixel owns it for the launch and adds the chunk's tiles in slot order, so
//                     every pixel sees its tiles in the order of the id list whatever the chunking.
//   umi_tile_finish   acc / fp32(sy[y] * sx[x]) in place, and optionally the uint8 mask of the quotient (umi_binary_mask's rule for
//                     K = 1, umi_argmax_mask's for K >= 2).
//
// Origins, windows, sums and the chunk's ids are DEVICE arrays: a captured chunk replays with other ids copied into the same
// buffer.  All three are streaming kernels: a wavefront covers contiguous runs along W, four pixels per lane where tw % 4 == 0,
// with 16-byte accesses on the tile side, and on the image side too where the four pixels start at a multiple of 4 of a
// 16-byte-aligned row (tile origins are arbitrary: otherwise dwords).  Every product, sum and quotient is rounded on its own (no
// contraction), as the NumPy statement does.
#include "common.h"

namespace {

constexpr int TL_MAX_TILE = 4096, TL_MAX_GRID = 1024, TL_MAX_CHUNK = 64;
constexpr unsigned TL_BM_CUTOFF_BITS = 0xB43FFFFEu;      // umi_binary_mask's cut-off, -0x1.7ffffcp-23

__device__ __forceinline__ int tl_reflect(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

__device__ __forceinline__ float tl_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float tl_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// origin of the tile in chunk slot s, false for an empty slot or an id outside the grid
__device__ __forceinline__ bool tl_origin(const int* __restrict__ ids, int s, const int* __restrict__ oy, const int* __restrict__ ox,
                                          int ny, int nx, int& y0, int& x0) {
    const int id = ids[s];
    if (id < 0 || id >= ny * nx) return false;
    y0 = oy[id / nx];
    x0 = ox[id % nx];
    return true;
}

// blockIdx.y = slot * C + channel; a thread = V consecutive pixels of one tile row.  `al`: x is 16-byte aligned and W % 4 == 0, so four
// in-image samples starting at a multiple of 4 are one 16-byte load
template <int V>
__global__ __launch_bounds__(256) void tile_gather_kernel(const float* __restrict__ x, int C, int H, int W, float* __restrict__ tiles,
                                                          int th, int tw, const int* __restrict__ oy, const int* __restrict__ ox,
                                                          int ny, int nx, const int* __restrict__ ids, int pad_mode, float pad_value,
                                                          int al) {
    const int gw = (tw + V - 1) / V;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= th * gw) return;
    const int i = g / gw, j0 = (g - i * gw) * V;
    const int slot = blockIdx.y / C, c = blockIdx.y - slot * C;
    float* dst = tiles + (((long)slot * C + c) * th + i) * tw + j0;
    float v[V];
    int y0 = 0, x0 = 0;
    if (!tl_origin(ids, slot, oy, ox, ny, nx, y0, x0)) {
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = 0.f;
    } else {
        const int y = y0 + i, xs = x0 + j0;
        const bool row_in = y >= 0 && y < H;
        const float* src = x + ((long)c * H + (pad_mode == 0 ? tl_reflect(y, H) : (row_in ? y : 0))) * W;
        if (V == 4 && al && xs >= 0 && xs + 3 < W && (xs & 3) == 0 && (row_in || pad_mode == 0)) {
            const float4 q = *reinterpret_cast<const float4*>(src + xs);
            v[0] = q.x; v[V > 1 ? 1 : 0] = q.y; v[V > 2 ? 2 : 0] = q.z; v[V > 3 ? 3 : 0] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int xx = xs + e;
                const bool in = xx >= 0 && xx < W;
                if (pad_mode == 0) v[e] = src[in ? xx : tl_reflect(xx, W)];
                else v[e] = (row_in && in) ? src[xx] : pad_value;
            }
        }
    }
    if (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[V > 1 ? 1 : 0], v[V > 2 ? 2 : 0], v[V > 3 ? 3 : 0]);   // tw % 4 == 0, aligned base
    else dst[0] = v[0];
}

// blockIdx.y = slot; a thread = V consecutive pixels of one tile row, i.e. of one canvas row.  The chunk's origins are read once per
// block into LDS (an empty slot gets a row origin no pixel reaches).  `al`: logits, acc and wx are 16-byte aligned and W % 4 == 0;
// four pixels that start at a multiple of 4 on both sides then move as 16-byte accesses (origins that are multiples of 4, the
// usual case), everything else as dwords.
template <int V>
__global__ __launch_bounds__(256) void tile_blend_kernel(const float* __restrict__ logits, int K, int th, int tw, float* __restrict__ acc,
                                                         int H, int W, const int* __restrict__ oy, const int* __restrict__ ox, int ny,
                                                         int nx, const float* __restrict__ wy, const float* __restrict__ wx,
                                                         const int* __restrict__ ids, int n, int al) {
    __shared__ int s_y[TL_MAX_CHUNK], s_x[TL_MAX_CHUNK];
    if ((int)threadIdx.x < n) {
        int ty = 0, tx = 0;
        const bool live = tl_origin(ids, threadIdx.x, oy, ox, ny, nx, ty, tx);
        s_y[threadIdx.x] = live ? ty : 0x7fffffff;
        s_x[threadIdx.x] = tx;
    }
    __syncthreads();
    const int gw = (tw + V - 1) / V;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= th * gw) return;
    const int i = g / gw, j0 = (g - i * gw) * V;
    const int slot = blockIdx.y;
    const int y0 = s_y[slot], x0 = s_x[slot];
    if (y0 == 0x7fffffff) return;
    const int y = y0 + i, xb = x0 + j0;
    if (y < 0 || y >= H) return;
    bool own[V];
    bool any = false, all = true;
#pragma unroll
    for (int e = 0; e < V; ++e) own[e] = xb + e >= 0 && xb + e < W;
    for (int s = 0; s < slot; ++s) {                        // an earlier slot that contains the pixel owns it
        const int ty = s_y[s], tx = s_x[s];
        if (y < ty || y >= ty + th) continue;
#pragma unroll
        for (int e = 0; e < V; ++e)
            if (xb + e >= tx && xb + e < tx + tw) own[e] = false;
    }
#pragma unroll
    for (int e = 0; e < V; ++e) { any = any || own[e]; all = all && own[e]; }
    if (!any) return;
    const bool wide = V == 4 && al && all && (xb & 3) == 0;
    const long HW = (long)H * W;
    for (int k = 0; k < K; ++k) {
        float* row = acc + (long)k * HW + (long)y * W;
        float a[V];
        if (wide) {
            const float4 q = *reinterpret_cast<const float4*>(row + xb);
            a[0] = q.x; a[V > 1 ? 1 : 0] = q.y; a[V > 2 ? 2 : 0] = q.z; a[V > 3 ? 3 : 0] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) a[e] = own[e] ? row[xb + e] : 0.f;
        }
        for (int s = slot; s < n; ++s) {
            const int ty = s_y[s], tx = s_x[s];
            if (y < ty || y >= ty + th) continue;
            const float wr = wy[y - ty];
            const float* lrow = logits + (((long)s * K + k) * th + (y - ty)) * tw;
            const int jj0 = xb - tx;
            if (wide && jj0 >= 0 && jj0 + 3 < tw && (jj0 & 3) == 0) {
                const float4 lq = *reinterpret_cast<const float4*>(lrow + jj0), wq = *reinterpret_cast<const float4*>(wx + jj0);
                const float l[4] = {lq.x, lq.y, lq.z, lq.w}, wc[4] = {wq.x, wq.y, wq.z, wq.w};
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float w = tl_mul(wr, wc[e]);
                    if (w > 0.f) a[e] = tl_add(a[e], tl_mul(w, l[e]));
                }
                continue;
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int jj = jj0 + e;
                if (!own[e] || jj < 0 || jj >= tw) continue;
                const float w = tl_mul(wr, wx[jj]);
                if (w > 0.f) a[e] = tl_add(a[e], tl_mul(w, lrow[jj]));
            }
        }
        if (wide) *reinterpret_cast<float4*>(row + xb) = make_float4(a[0], a[V > 1 ? 1 : 0], a[V > 2 ? 2 : 0], a[V > 3 ? 3 : 0]);
        else {
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (own[e]) row[xb + e] = a[e];
        }
    }
}

// a thread = V consecutive pixels of one canvas row, all K planes
template <int V>
__global__ __launch_bounds__(256) void tile_finish_kernel(float* __restrict__ acc, int K, int H, int W, const float* __restrict__ sy,
                                                          const float* __restrict__ sx, unsigned char* __restrict__ mask) {
#pragma clang fp contract(off)
    const int gw = (W + V - 1) / V;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long)H * gw) return;
    const int y = (int)(g / gw), x0 = (int)(g - (long)y * gw) * V;
    const long HW = (long)H * W, p = (long)y * W + x0;
    const float ry = sy[y];
    const float cut = __builtin_bit_cast(float, TL_BM_CUTOFF_BITS);
    float d[V], best[V];
    unsigned char bi[V];
#pragma unroll
    for (int e = 0; e < V; ++e) d[e] = tl_mul(ry, sx[x0 + e]);
    for (int k = 0; k < K; ++k) {
        float v[V];
        if (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(acc + (long)k * HW + p);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else v[0] = acc[(long)k * HW + p];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            v[e] = __fdiv_rn(v[e], d[e]);
            if (k == 0) { best[e] = v[e]; bi[e] = 0; }
            else if (v[e] > best[e]) { best[e] = v[e]; bi[e] = (unsigned char)k; }       // first maximum wins (umi_argmax_mask)
        }
        if (V == 4) *reinterpret_cast<float4*>(acc + (long)k * HW + p) = make_float4(v[0], v[1], v[2], v[3]);
        else acc[(long)k * HW + p] = v[0];
    }
    if (!mask) return;
    if (K == 1) {
#pragma unroll
        for (int e = 0; e < V; ++e) bi[e] = best[e] >= cut ? 1 : 0;                      // NaN compares false: 0 (umi_binary_mask)
    }
    if (V == 4) *reinterpret_cast<uchar4*>(mask + p) = make_uchar4(bi[0], bi[1], bi[2], bi[3]);
    else mask[p] = bi[0];
}

// sizes shared by the three entry points; `ch` = channels of the tile tensor
int tl_check(int ch, int H, int W, int th, int tw, int ny, int nx, int n) {
    if (ch <= 0 || H <= 0 || W <= 0 || th <= 0 || tw <= 0 || ny <= 0 || nx <= 0 || n <= 0) return UMI_ERR_BADARG;
    if (th > TL_MAX_TILE || tw > TL_MAX_TILE || ny > TL_MAX_GRID || nx > TL_MAX_GRID || n > TL_MAX_CHUNK) return UMI_ERR_UNSUPPORTED;
    if ((__int128)ch * H * W >= ((__int128)1 << 31) || (__int128)n * ch * th * tw >= ((__int128)1 << 31)) return UMI_ERR_UNSUPPORTED;
    if ((long)n * ch > 65535) return UMI_ERR_UNSUPPORTED;                                // grid.y
    return UMI_OK;
}

}  // namespace

extern "C" int umi_tile_gather(const float* x, int C, int H, int W, float* tiles, int th, int tw, const int* oy, const int* ox, int ny,
                               int nx, const int* ids, int n, int pad_mode, float pad_value, umi_stream_t stream) {
    if (!x || !tiles || !oy || !ox || !ids || (pad_mode != 0 && pad_mode != 1)) return UMI_ERR_BADARG;
    if (((unsigned long)x & 3) || ((unsigned long)tiles & 3)) return UMI_ERR_BADARG;
    const int st = tl_check(C, H, W, th, tw, ny, nx, n);
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    const bool wide = tw % 4 == 0 && ((unsigned long)tiles & 15) == 0;
    const int al = W % 4 == 0 && ((unsigned long)x & 15) == 0 ? 1 : 0;
    const int gw = wide ? tw / 4 : tw;
    const dim3 grid((unsigned)(((long)th * gw + 255) / 256), (unsigned)(n * C));
    if (wide)
        hipLaunchKernelGGL((tile_gather_kernel<4>), grid, dim3(256), 0, s, x, C, H, W, tiles, th, tw, oy, ox, ny, nx, ids, pad_mode,
                           pad_value, al);
    else
        hipLaunchKernelGGL((tile_gather_kernel<1>), grid, dim3(256), 0, s, x, C, H, W, tiles, th, tw, oy, ox, ny, nx, ids, pad_mode,
                           pad_value, 0);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_tile_blend(const float* logits, int K, int th, int tw, float* acc, int H, int W, const int* oy, const int* ox, int ny,
                              int nx, const float* wy, const float* wx, const int* ids, int n, umi_stream_t stream) {
    if (!logits || !acc || !oy || !ox || !wy || !wx || !ids) return UMI_ERR_BADARG;
    if (((unsigned long)logits & 3) || ((unsigned long)acc & 3)) return UMI_ERR_BADARG;
    const int st = tl_check(K, H, W, th, tw, ny, nx, n);
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    const bool quad = tw % 4 == 0;                          // four pixels per lane
    const int al = W % 4 == 0 && (((unsigned long)logits | (unsigned long)acc | (unsigned long)wx) & 15) == 0 ? 1 : 0;
    const int gw = quad ? tw / 4 : tw;
    const dim3 grid((unsigned)(((long)th * gw + 255) / 256), (unsigned)n);
    if (quad)
        hipLaunchKernelGGL((tile_blend_kernel<4>), grid, dim3(256), 0, s, logits, K, th, tw, acc, H, W, oy, ox, ny, nx, wy, wx, ids, n, al);
    else
        hipLaunchKernelGGL((tile_blend_kernel<1>), grid, dim3(256), 0, s, logits, K, th, tw, acc, H, W, oy, ox, ny, nx, wy, wx, ids, n, 0);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_tile_finish(float* acc, int K, int H, int W, const float* sy, const float* sx, unsigned char* mask,
                               umi_stream_t stream) {
    if (!acc || !sy || !sx || K <= 0 || H <= 0 || W <= 0 || ((unsigned long)acc & 3)) return UMI_ERR_BADARG;
    if ((__int128)K * H * W >= ((__int128)1 << 31) || K > 256) return UMI_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const bool wide = W % 4 == 0 && ((unsigned long)acc & 15) == 0 && ((unsigned long)mask & 3) == 0;
    const int gw = wide ? W / 4 : W;
    const dim3 grid((unsigned)(((long)H * gw + 255) / 256));
    if (wide) hipLaunchKernelGGL((tile_finish_kernel<4>), grid, dim3(256), 0, s, acc, K, H, W, sy, sx, mask);
    else hipLaunchKernelGGL((tile_finish_kernel<1>), grid, dim3(256), 0, s, acc, K, H, W, sy, sx, mask);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
