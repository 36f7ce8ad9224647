// fp32 multi-head softmax attention, head dim 64, on the fp32-input matrix-core instruction of gfx950, v_mfma_f32_32x32x2_f32
// (reference TransUnet/vit_seg_modeling.py:73-91: softmax(Q K^T / sqrt(64)) V).  Opt-in: UMI_ATTN_F32_MFMA (include/unetmi.h);
// without the flag, or on a call the predicate below refuses, umi_attn_fwd_flags / umi_attn_bwd_flags run exactly as before.
//
// The decomposition of attention_mfma.hip (fp16) with one-dword operands.  Scores are never materialised, every kernel
// recomputes P from the saved log-sum-exp (max + log(sum exp(s - max)) of the scaled scores, the VALU kernel's definition),
// there are no atomics (identical inputs give identical bits) and nothing is allocated at launch.
//   forward      : workgroup = 128 queries (4 waves x 32) of one (batch, head); K / V streamed in 64-key chunks.
//   backward dQ  : the same decomposition; also writes delta = rowsum(dO * O).
//   backward dKV : workgroup = 128 keys (4 waves x 32) of one (batch, head); Q / dO streamed in 32-query tiles.
//
// With the operand maps A[i][k], B[k][j], D[row][col] of the 32x32x2 form (mfma_f32.h):
//   scores  S^T[key][query] = K . Q^T: a lane owns ONE query column, so the row statistics are register reductions plus one
//            exchange with lane ^ 32.  B = the lane's own (pre-scaled) Q row in 32 VGPRs; the contraction runs over the head
//            dimension in the order d = 32 * (l >> 5) + t for step t, so that a lane loads 32 consecutive floats.  A =
//            K[key = l & 31][d] from a row-major LDS tile of 65 dwords per row: the 32 lanes of a half stride by one row and
//            fall on 32 distinct banks.
//   output   O^T[d][query] += V^T . P^T: accumulator register t of the score tile holds keys d_row(t, 0) / d_row(t, 1) in the
//            two lane halves, which IS the B operand [k = l >> 5][j = query] of a k-step over those two keys: P goes from the
//            accumulator into the next product without touching LDS.  A = V[that key][d0 + (l & 31)]: a plain row read of the
//            same kind of tile (consecutive dwords, conflict-free).  dQ^T = K^T . dS^T, dV^T = dO^T . P and dK^T = Q^T . dS
//            work the same way.
//   Rows past N enter the LDS tiles as zeros and their probabilities are forced to zero: no unknown memory is multiplied.
// DROP (all three kernels): attention-probability dropout, O = (P o Z) V, Z = keep / (1 - p): as in attention_mfma.hip, a lane
// regenerates the 16 keep bits of its tile column from the stream (common.h: umi_stream_keep); statistics and lse are undropped.
// Independent accumulators in flight per wave: forward 2 (the score chain is split in two halves of the head dimension, the two
// 32-channel halves of O), backward 2 (S and dP) and 2 / 4 (dQ halves; dK and dV halves).
#include "kernels.h"
#include "mfma_f32.h"

namespace {

constexpr int D = 64;
constexpr int PITCH = D + 1;       // dwords per LDS row
constexpr int KC = 64;             // keys per staged chunk (query-side kernels)
constexpr int QT = 32;             // queries per staged tile (key-side kernel)
constexpr int TILE = 128;          // queries / keys per workgroup

__device__ __forceinline__ float lane_xchg32(float v) { return __shfl_xor(v, 32); }

// ROWS rows of one head slice of a token tensor -> a [ROWS][PITCH] LDS tile; rows at or past row_limit enter as zeros
template <int ROWS>
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, int ld, long row0, long row_limit, float* tile, int tid) {
    constexpr int IT = ROWS * (D / 4) / 256;
    float4 v[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int r = (i * 256 + tid) >> 4, c4 = (tid & 15) * 4;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + r < row_limit) v[i] = *reinterpret_cast<const float4*>(src + (row0 + r) * ld + c4);
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int r = (i * 256 + tid) >> 4, c4 = (tid & 15) * 4;
        float* d = tile + r * PITCH + c4;
        d[0] = v[i].x; d[1] = v[i].y; d[2] = v[i].z; d[3] = v[i].w;
    }
}

// the lane's B operand of a score product: 32 consecutive floats of its own row (zeros for a row past the end), times mul
__device__ __forceinline__ void load_row_half(const float* __restrict__ p, bool valid, float mul, float (&dst)[32]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid) v = *reinterpret_cast<const float4*>(p + 4 * j);
        dst[4 * j + 0] = v.x * mul; dst[4 * j + 1] = v.y * mul; dst[4 * j + 2] = v.z * mul; dst[4 * j + 3] = v.w * mul;
    }
}

// transposed accumulator (rows = channels, lane = token) -> 64 floats of the lane's token row, 16 bytes per store
__device__ __forceinline__ void store_row(float* __restrict__ dst, const f32x16 (&acc)[2], float mul, int lh) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(dst + mt * 32 + g * 8 + lh * 4) =
                make_float4(acc[mt][4 * g] * mul, acc[mt][4 * g + 1] * mul, acc[mt][4 * g + 2] * mul, acc[mt][4 * g + 3] * mul);
}

// ---- forward (BWD = false) and backward query side (BWD = true) ---------------------------------------------------------------
template <bool BWD, typename... DA>
__global__ __launch_bounds__(256, 2) void attn_f32_q_side_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                 const float* __restrict__ v, int ld,
                                                                 float* __restrict__ o /*fwd: out; bwd: forward output (read)*/,
                                                                 const float* __restrict__ dO, int ldo, float* __restrict__ lse,
                                                                 float* __restrict__ dq, int lddq, float* __restrict__ delta,
                                                                 int N, int Hh, int tiles, float scale, DA... da) {
    constexpr bool DROP = sizeof...(DA) != 0;
    const UmiAttnDrop drop = umi_attn_drop_of(da...);
    __shared__ float ks[KC * PITCH], vs[KC * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lq = lane & 31, lh = lane >> 5;
    const int bh = blockIdx.x / tiles, b = bh / Hh, h = bh % Hh;
    const long tok0 = (long)b * N;
    const int q0 = (blockIdx.x % tiles) * TILE + wave * 32, qi = q0 + lq;
    const bool qv = qi < N, wave_on = q0 < N;          // a wave with no query only helps staging
    const float* kh = k + h * D;
    const float* vh = v + h * D;
    const unsigned dseed = DROP ? umi_stream_seed(drop) : 0u;
    const unsigned long erow = DROP ? ((unsigned long)bh * N + qi) * N : 0ul;          // dense index of P[qi][0]

    float qr[32], dor[32];
    float dl = 0.f, L = 0.f;
    load_row_half(q + (tok0 + qi) * ld + h * D + lh * 32, qv, scale, qr);
    if (BWD) {
        float orow[32];
        load_row_half(dO + (tok0 + qi) * ldo + h * D + lh * 32, qv, 1.f, dor);
        load_row_half(o + (tok0 + qi) * ldo + h * D + lh * 32, qv, 1.f, orow);
        // delta in the order of the dP chain below (d = 0, 32, 1, 33, ...: the instruction adds the k = 0 product, then the
        // k = 1 one), so that dP - delta is exactly zero where it is zero in exact arithmetic (a single key: O = V).  The two
        // lane halves hold the two halves of one query's row and end up with the same value.
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            const float d2 = lane_xchg32(dor[t]), o2 = lane_xchg32(orow[t]);
            dl = fmaf(lh ? d2 : dor[t], lh ? o2 : orow[t], dl);
            dl = fmaf(lh ? dor[t] : d2, lh ? orow[t] : o2, dl);
        }
        L = qv ? lse[(long)bh * N + qi] : 0.f;
    }

    f32x16 acc[2] = {zero16(), zero16()};               // fwd: O^T [d half][.]; bwd: dQ^T
    float mx = -INFINITY, lsum = 0.f;

    for (int kc0 = 0; kc0 < N; kc0 += KC) {
        __syncthreads();
        stage_rows<KC>(kh, ld, tok0 + kc0, tok0 + N, ks, tid);
        stage_rows<KC>(vh, ld, tok0 + kc0, tok0 + N, vs, tid);
        __syncthreads();
        if (!wave_on) continue;
        const int kend = (N - kc0) < KC ? (N - kc0) : KC;
        for (int kt = 0; kt < kend; kt += 32) {
            const float* ka = ks + (kt + lq) * PITCH + lh * 32;
            unsigned keepbits = 0;                      // bit r: keep of P[qi][key of register r]; independent of the products
            if (DROP) {                                 // below, so the hashes run under their latency
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    keepbits |= (unsigned)umi_stream_keep(erow + (kc0 + kt + d_row(r, lh)), dseed, drop.thr) << r;
            }
            f32x16 p;
            if (!BWD) {
                // S^T tile [32 keys][32 queries] of the scaled scores, as two chains over the even and the odd steps
                f32x16 s = zero16(), s1 = zero16();
#pragma unroll
                for (int t = 0; t < 32; t += 2) {
                    s = mfma32(ka[t], qr[t], s);
                    s1 = mfma32(ka[t + 1], qr[t + 1], s1);
                }
                float tmax = -INFINITY;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[r] = kt + d_row(r, lh) < kend ? s[r] + s1[r] : -INFINITY;
                    tmax = fmaxf(tmax, s[r]);
                }
                tmax = fmaxf(tmax, lane_xchg32(tmax));  // finite: key kt of the tile is always inside the sequence
                const float mn = fmaxf(mx, tmax);
                const float corr = __expf(mx - mn);
                float ps = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) { p[r] = __expf(s[r] - mn); ps += p[r]; }
                ps += lane_xchg32(ps);
                lsum = lsum * corr + ps;
                mx = mn;
                if (DROP) {                             // only the operand of P . V is masked
#pragma unroll
                    for (int r = 0; r < 16; ++r) p[r] = (keepbits >> r & 1) ? p[r] : 0.f;
                }
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[a][r] *= corr;
            } else {
                // S^T and dP^T = V . dO^T tiles, then dS^T = P * (dP - delta)
                const float* va = vs + (kt + lq) * PITCH + lh * 32;
                f32x16 s = zero16(), dp = zero16();
#pragma unroll
                for (int t = 0; t < 32; ++t) {
                    s = mfma32(ka[t], qr[t], s);
                    dp = mfma32(va[t], dor[t], dp);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float pr = kt + d_row(r, lh) < kend ? __expf(s[r] - L) : 0.f;
                    if (DROP) p[r] = pr * (((keepbits >> r & 1) ? dp[r] * drop.inv_keep : 0.f) - dl);   // dS = P o (Z o dP - delta)
                    else p[r] = pr * (dp[r] - dl);
                }
            }
            // acc^T[d][query] += X^T . p, X = V (forward) or K (backward): step t covers the two keys that register t holds
            const float* xa = (BWD ? ks : vs) + (kt + 4 * lh) * PITCH + lq;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const float* xr = xa + d_row(t, 0) * PITCH;
                acc[0] = mfma32(xr[0], p[t], acc[0]);
                acc[1] = mfma32(xr[32], p[t], acc[1]);
            }
        }
    }
    if (qv) {
        if (BWD) store_row(dq + (tok0 + qi) * lddq + h * D, acc, scale, lh);
        else store_row(o + (tok0 + qi) * ldo + h * D, acc, DROP ? drop.inv_keep / lsum : 1.f / lsum, lh);
        if (lh == 0) {
            if (BWD) delta[(long)bh * N + qi] = dl;
            else lse[(long)bh * N + qi] = mx + __logf(lsum);
        }
    }
}

// ---- backward key side --------------------------------------------------------------------------------------------------------
// A wave owns 32 keys (lane = key column of S[query][key]); its K (pre-scaled) and V rows are the B operands of S = Q . K^T and
// dP = dO . V^T, whose A operands are rows of the staged Q and dO tiles.  P and dS = P * (dP - delta) * scale then feed
// dV^T[d][key] += dO^T . P and dK^T[d][key] += Q^T . dS from the accumulator, with row reads of the same two tiles.
template <typename... DA>
__global__ __launch_bounds__(256, 2) void attn_f32_kv_side_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                  const float* __restrict__ v, int ld,
                                                                  const float* __restrict__ dO, int ldo,
                                                                  const float* __restrict__ lse, const float* __restrict__ delta,
                                                                  float* __restrict__ dk, float* __restrict__ dv, int lddk, int N,
                                                                  int Hh, int tiles, float scale, DA... da) {
    constexpr bool DROP = sizeof...(DA) != 0;
    const UmiAttnDrop drop = umi_attn_drop_of(da...);
    __shared__ float qs[QT * PITCH], os[QT * PITCH];
    __shared__ float lse_s[QT], del_s[QT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lk = lane & 31, lh = lane >> 5;
    const int bh = blockIdx.x / tiles, b = bh / Hh, h = bh % Hh;
    const long tok0 = (long)b * N;
    const int k0 = (blockIdx.x % tiles) * TILE + wave * 32, ki = k0 + lk;
    const bool kv = ki < N, wave_on = k0 < N;
    const float* qh = q + h * D;
    const float* oh = dO + h * D;
    const unsigned dseed = DROP ? umi_stream_seed(drop) : 0u;
    const unsigned long ecol = DROP ? (unsigned long)bh * N * N + ki : 0ul;            // dense index of P[0][ki]

    float kf[32], vf[32];
    load_row_half(k + (tok0 + ki) * ld + h * D + lh * 32, kv, scale, kf);
    load_row_half(v + (tok0 + ki) * ld + h * D + lh * 32, kv, 1.f, vf);
    f32x16 dkT[2] = {zero16(), zero16()}, dvT[2] = {zero16(), zero16()};

    for (int q0 = 0; q0 < N; q0 += QT) {
        __syncthreads();
        stage_rows<QT>(qh, ld, tok0 + q0, tok0 + N, qs, tid);
        stage_rows<QT>(oh, ldo, tok0 + q0, tok0 + N, os, tid);
        if (tid < QT) {
            const bool in = q0 + tid < N;
            lse_s[tid] = in ? lse[(long)bh * N + q0 + tid] : 0.f;
            del_s[tid] = in ? delta[(long)bh * N + q0 + tid] : 0.f;
        }
        __syncthreads();
        if (!wave_on) continue;
        const float* qa = qs + lk * PITCH + lh * 32;
        const float* oa = os + lk * PITCH + lh * 32;
        unsigned keepbits = 0;                          // bit r: keep of P[query of register r][ki]
        if (DROP) {
            // four hashes at a time, NOT unrolled further: this kernel has no registers to spare (16 hashes in flight spill)
#pragma unroll 1
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    keepbits |= (unsigned)umi_stream_keep(ecol + (unsigned long)(q0 + d_row(4 * g + j, lh)) * N, dseed, drop.thr)
                                << (4 * g + j);
        }
        f32x16 s = zero16(), dp = zero16();
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            s = mfma32(qa[t], kf[t], s);                // S[query][key], scaled
            dp = mfma32(oa[t], vf[t], dp);              // dP[query][key]
        }
        f32x16 p, ds;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qq = d_row(r, lh);                // query row of this register
            const float pr = (q0 + qq < N && kv) ? __expf(s[r] - lse_s[qq]) : 0.f;
            if (DROP) {                                 // dV takes P o Z, dK takes dS
                const bool keep = keepbits >> r & 1;
                p[r] = keep ? pr * drop.inv_keep : 0.f;
                ds[r] = pr * ((keep ? dp[r] * drop.inv_keep : 0.f) - del_s[qq]) * scale;
                continue;
            }
            p[r] = pr;
            ds[r] = pr * (dp[r] - del_s[qq]) * scale;
        }
        const float* qx = qs + 4 * lh * PITCH + lk;
        const float* ox = os + 4 * lh * PITCH + lk;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int ro = d_row(t, 0) * PITCH;
            dvT[0] = mfma32(ox[ro], p[t], dvT[0]);
            dvT[1] = mfma32(ox[ro + 32], p[t], dvT[1]);
            dkT[0] = mfma32(qx[ro], ds[t], dkT[0]);
            dkT[1] = mfma32(qx[ro + 32], ds[t], dkT[1]);
        }
    }
    if (kv) {
        store_row(dk + (tok0 + ki) * lddk + h * D, dkT, 1.f, lh);
        store_row(dv + (tok0 + ki) * lddk + h * D, dvT, 1.f, lh);
    }
}

// one workgroup per (batch, head, 128-token tile), all in grid dimension x
bool grid_of(int B, int N, int Hh, int* tiles, unsigned* blocks) {
    *tiles = umi_cdiv(N, TILE);
    const long n = (long)B * Hh * *tiles;
    *blocks = (unsigned)n;
    return n < (1L << 31);
}

}  // namespace

bool umi_attn_f32_mfma_ok(int D_, int ld, int ldo, int ldd, int dtype, int flags, uintptr_t ptrs) {
    // addresses are 64-bit, so the tensors' sizes add no condition
    return (flags & UMI_ATTN_F32_MFMA) && dtype == UMI_F32 && D_ == D && ld % 4 == 0 && ldo % 4 == 0 && ldd % 4 == 0 &&
           (ptrs & 15) == 0;
}

int umi_attn_fwd_f32_mfma(const void* q, const void* k, const void* v, int ld, void* o, int ldo, float* lse, int B, int N, int Hh,
                          const UmiAttnDrop* drop, hipStream_t s) {
    int tiles;
    unsigned blocks;
    if (!grid_of(B, N, Hh, &tiles, &blocks)) return UMI_ERR_BADARG;
#define UMI_ARGS (const float*)q, (const float*)k, (const float*)v, ld, (float*)o, (const float*)nullptr, ldo, lse, (float*)nullptr, 0, \
                 (float*)nullptr, N, Hh, tiles, 0.125f
    if (drop) hipLaunchKernelGGL(attn_f32_q_side_kernel<false>, dim3(blocks), dim3(256), 0, s, UMI_ARGS, *drop);
    else hipLaunchKernelGGL(attn_f32_q_side_kernel<false>, dim3(blocks), dim3(256), 0, s, UMI_ARGS);
#undef UMI_ARGS
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

int umi_attn_bwd_f32_mfma(const void* q, const void* k, const void* v, int ld, const void* o, const void* dO, int ldo,
                          const float* lse, void* dq, void* dk, void* dv, int ldd, float* delta, int B, int N, int Hh,
                          const UmiAttnDrop* drop, hipStream_t s) {
    int tiles;
    unsigned blocks;
    if (!grid_of(B, N, Hh, &tiles, &blocks)) return UMI_ERR_BADARG;
#define UMI_Q_ARGS (const float*)q, (const float*)k, (const float*)v, ld, (float*)o, (const float*)dO, ldo, (float*)lse, (float*)dq, ldd, \
                   delta, N, Hh, tiles, 0.125f
#define UMI_KV_ARGS (const float*)q, (const float*)k, (const float*)v, ld, (const float*)dO, ldo, lse, (const float*)delta, (float*)dk, \
                    (float*)dv, ldd, N, Hh, tiles, 0.125f
    if (drop) hipLaunchKernelGGL(attn_f32_q_side_kernel<true>, dim3(blocks), dim3(256), 0, s, UMI_Q_ARGS, *drop);
    else hipLaunchKernelGGL(attn_f32_q_side_kernel<true>, dim3(blocks), dim3(256), 0, s, UMI_Q_ARGS);
    UMI_LAUNCH_CHECK();
    if (drop) hipLaunchKernelGGL(attn_f32_kv_side_kernel, dim3(blocks), dim3(256), 0, s, UMI_KV_ARGS, *drop);
    else hipLaunchKernelGGL(attn_f32_kv_side_kernel, dim3(blocks), dim3(256), 0, s, UMI_KV_ARGS);
#undef UMI_Q_ARGS
#undef UMI_KV_ARGS
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
