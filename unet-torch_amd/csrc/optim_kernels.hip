// Multi-tensor parameter update and weight re-pack: one launch per training step each instead of one per tensor.
//
//   umi_optim_sgd_multi / umi_optim_adam_multi   torch.optim.SGD / Adam arithmetic (reference train.py:341-347: SGD lr 0.01
//       momentum 0.9 wd 1e-4, Adam lr 5e-4 wd 1e-4), fp32, same operation order and roundings as torch's foreach kernels.
//   umi_pack_kn_multi                            umi_pack_kn / umi_pack_kn8 of every convolution weight of a model.
//
// All three walk a descriptor table that lives in device memory.  A workgroup owns one fixed-size block of ONE tensor
// (`blk0` = first block of a descriptor, found by binary search), so the grid is balanced however unequal the tensors
// are (a U-Net has 3x3x1024x1024 weights next to 64-element BatchNorm vectors).  HBM-bound streaming work: 16-byte
// accesses whenever the four pointers of a tensor allow it.
#include "common.h"
#include <stdint.h>

namespace {

constexpr int OPT_BLOCK = 4096;      // elements per workgroup (256 threads x 4 x float4)
constexpr int PACK_BLOCK = 2048;     // packed elements per workgroup

template <typename D>
__device__ inline int find_desc(const D* d, int n, int blk) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (d[mid].blk0 <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Device-resident hyper-parameters of one param group (mirrors umi_optim_hyper, include/unetmi.h): what a captured HIP graph
// must NOT freeze.  The doubles are the state; the floats are what the update kernel reads, derived by hyper_pre_kernel
// with the roundings torch applies to its Python doubles.
struct Hyper {
    double lr, base_lr, iter, max_iter, power, adam_t, beta1, beta2;
    float lr_f, step_size_f, bc2_sqrt_f;
    int kind;                            // UMI_SCHED_*: what hyper_schedule_kernel applies (0: none installed)
    double warmup, final_ratio;
};
static_assert(sizeof(Hyper) == 96, "umi_optim_hyper is 96 bytes");

struct SgdArgs { float lr, momentum, omd, wd; int nesterov, first; const Hyper* hp; };   // omd = 1 - dampening

__device__ inline void sgd_one(float& p, float g, float& m, const SgdArgs a) {
    if (a.wd != 0.f) g = fmaf(a.wd, p, g);                            // grad.add(param, alpha=wd)
    if (a.momentum != 0.f) {
        if (a.first) m = g;                                            // buf = clone(grad)
        else {
            float mm = __fmul_rn(m, a.momentum);                       // buf.mul_(momentum)
            m = a.omd == 1.f ? __fadd_rn(mm, g) : fmaf(a.omd, g, mm);   // .add_(grad, alpha=1-dampening)
        }
        g = a.nesterov ? fmaf(a.momentum, m, g) : m;
    }
    p = fmaf(-a.lr, g, p);                                             // param.add_(grad, alpha=-lr)
}

struct AdamArgs { float step_size, omb1, beta2, omb2, bc2_sqrt, eps, wd; const Hyper* hp; };   // omb = 1 - beta, rounded from double

// AdamW (decoupled weight decay): the Adam arguments with wd = 0, plus what the decay factor is formed from, in double.  `lr` is
// this step's learning rate when there is no hyper block (step_size = lr / bc1 does not determine it).
struct AdamWArgs { float step_size, omb1, beta2, omb2, bc2_sqrt, eps, wd; const Hyper* hp; double lr, wd_d; };

// (float)(1 - lr * wd) with the two roundings of the Python doubles torch forms it from: no fused multiply-add
__device__ inline float adamw_decay(double lr, double wd) {
#pragma clang fp contract(off)
    const double prod = lr * wd;
    return (float)(1.0 - prod);
}

template <typename A>
__device__ inline void adam_one(float& p, float g, float& m, float& v, const A a) {
    if (a.wd != 0.f) g = fmaf(a.wd, p, g);                            // grad.add(param, alpha=wd)  (L2, not AdamW)
    m = fmaf(a.omb1, g - m, m);                                        // exp_avg.lerp_(grad, 1-beta1)
    v = fmaf(a.omb2 * g, g, __fmul_rn(v, a.beta2));                   // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1-beta2)
    const float denom = __fdiv_rn(__fsqrt_rn(v), a.bc2_sqrt) + a.eps;
    p = fmaf(-a.step_size, __fdiv_rn(m, denom), p);                    // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// GUARD: the step is conditional on the device guard block (umi_grad_guard_finalize): nothing is stored on a skipped step, and
// every gradient is multiplied by (float)COEF -- one fp32 rounding, as a torch multiply of the gradient would make -- before the
// unchanged sgd_one / adam_one.  Without GUARD the body is the one the unguarded entry points have always run.
// DECOUPLED (AdamW, A = AdamWArgs): param.mul_(1 - lr * weight_decay) first -- the factor formed in double from THIS step's
// learning rate (the block's `lr` when there is one) and rounded once -- then adam_one with wd = 0.  A skipped step returns
// before it: no decay either.
template <bool ADAM, bool GUARD, typename A, bool DECOUPLED = false>
__device__ __forceinline__ void optim_multi_body(const umi_optim_desc* __restrict__ descs, int n_desc, A a,
                                                 const double* __restrict__ guard) {
    bool skip = false;
    float cf = 1.f;
    if constexpr (GUARD) {
        skip = guard[UMI_GUARD_SKIP] != 0.0;
        cf = (float)guard[UMI_GUARD_COEF];
    }
    const auto gs = [cf](float g) { return (GUARD && cf != 1.f) ? __fmul_rn(g, cf) : g; };
    if (a.hp) {                               // learning rate / bias corrections from device memory (graph-safe)
        if constexpr (ADAM) { a.step_size = a.hp->step_size_f; a.bc2_sqrt = a.hp->bc2_sqrt_f; }
        else a.lr = a.hp->lr_f;
    }
    float decay = 1.f;
    bool decays = false;
    if constexpr (DECOUPLED) {
        decays = a.wd_d != 0.0;
        if (decays) decay = adamw_decay(a.hp ? a.hp->lr : a.lr, a.wd_d);
    }
    const auto dk = [decay, decays](float p) { return (DECOUPLED && decays) ? __fmul_rn(p, decay) : p; };
    const int blk = blockIdx.x;
    const umi_optim_desc d = descs[find_desc(descs, n_desc, blk)];
    const long base = (long)(blk - d.blk0) * OPT_BLOCK;
    const long left = d.n - base;
    const int cnt = left < OPT_BLOCK ? (int)left : OPT_BLOCK;
    float* p = d.p + base;
    const float* g = d.g + base;
    float* s0 = d.s0 ? d.s0 + base : nullptr;
    float* s1 = d.s1 ? d.s1 + base : nullptr;
    if constexpr (GUARD) {
        if (skip) {                           // (uniform) a skipped FIRST SGD step still owes the momentum buffer its zeros
            if constexpr (!ADAM) {
                if (a.first && s0)
                    for (int i = threadIdx.x; i < cnt; i += 256) s0[i] = 0.f;
            }
            return;
        }
    }
    const unsigned long al = (unsigned long)p | (unsigned long)g | (unsigned long)s0 | (unsigned long)s1;
    if ((al & 15) == 0) {
        for (int i = threadIdx.x * 4; i + 4 <= cnt; i += 1024) {
            float4 pv = *reinterpret_cast<float4*>(p + i);
            float4 gv = *reinterpret_cast<const float4*>(g + i);
            if constexpr (GUARD) gv = make_float4(gs(gv.x), gs(gv.y), gs(gv.z), gs(gv.w));
            float4 mv = s0 ? *reinterpret_cast<float4*>(s0 + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            float4 vv = (ADAM && s1) ? *reinterpret_cast<float4*>(s1 + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (ADAM) {
                if constexpr (DECOUPLED) pv = make_float4(dk(pv.x), dk(pv.y), dk(pv.z), dk(pv.w));
                adam_one(pv.x, gv.x, mv.x, vv.x, a); adam_one(pv.y, gv.y, mv.y, vv.y, a);
                adam_one(pv.z, gv.z, mv.z, vv.z, a); adam_one(pv.w, gv.w, mv.w, vv.w, a);
                *reinterpret_cast<float4*>(s1 + i) = vv;
            } else {
                sgd_one(pv.x, gv.x, mv.x, a); sgd_one(pv.y, gv.y, mv.y, a);
                sgd_one(pv.z, gv.z, mv.z, a); sgd_one(pv.w, gv.w, mv.w, a);
            }
            *reinterpret_cast<float4*>(p + i) = pv;
            if (s0) *reinterpret_cast<float4*>(s0 + i) = mv;
        }
        const int tail0 = cnt & ~3;
        const int i = tail0 + threadIdx.x;
        if (i < cnt) {
            float pv = p[i], mv = s0 ? s0[i] : 0.f;
            if constexpr (ADAM) { float vv = s1[i]; pv = dk(pv); adam_one(pv, gs(g[i]), mv, vv, a); s1[i] = vv; }
            else sgd_one(pv, gs(g[i]), mv, a);
            p[i] = pv;
            if (s0) s0[i] = mv;
        }
    } else {
        for (int i = threadIdx.x; i < cnt; i += 256) {
            float pv = p[i], mv = s0 ? s0[i] : 0.f;
            if constexpr (ADAM) { float vv = s1[i]; pv = dk(pv); adam_one(pv, gs(g[i]), mv, vv, a); s1[i] = vv; }
            else sgd_one(pv, gs(g[i]), mv, a);
            p[i] = pv;
            if (s0) s0[i] = mv;
        }
    }
}

template <bool ADAM, typename A, bool DECOUPLED = false>
__global__ __launch_bounds__(256) void optim_multi_kernel(const umi_optim_desc* __restrict__ descs, int n_desc, A a) {
    optim_multi_body<ADAM, false, A, DECOUPLED>(descs, n_desc, a, nullptr);
}

template <bool ADAM, typename A, bool DECOUPLED = false>
__global__ __launch_bounds__(256) void optim_multi_guarded_kernel(const umi_optim_desc* __restrict__ descs, int n_desc, A a,
                                                                  const double* __restrict__ guard) {
    optim_multi_body<ADAM, true, A, DECOUPLED>(descs, n_desc, a, guard);
}

// ---- gradient guard: per-block sum of squares and non-finite count, then one workgroup that decides the step ----------------
__device__ inline void guard_acc(float g, double& s, int& k) {
    const double x = (double)g;
    s += x * x;                                                        // fp32 squared is exact in double
    k += (__float_as_uint(g) & 0x7f800000u) == 0x7f800000u;           // inf or NaN
}

// fixed-order tree over the NT threads of a workgroup; the result is valid in thread 0
template <int NT>
__device__ inline void guard_block_sum(double& s, double& k, double* sh_s, double* sh_k) {
    sh_s[threadIdx.x] = s;
    sh_k[threadIdx.x] = k;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sh_s[threadIdx.x] += sh_s[threadIdx.x + w];
            sh_k[threadIdx.x] += sh_k[threadIdx.x + w];
        }
        __syncthreads();
    }
    s = sh_s[0];
    k = sh_k[0];
}

__global__ __launch_bounds__(256) void grad_norm_partials_kernel(const umi_optim_desc* __restrict__ descs, int n_desc,
                                                                 int block_offset, double* __restrict__ ws) {
    __shared__ double sh_s[256], sh_k[256];
    const int blk = blockIdx.x;
    const umi_optim_desc d = descs[find_desc(descs, n_desc, blk)];
    const long base = (long)(blk - d.blk0) * OPT_BLOCK;
    const long left = d.n - base;
    const int cnt = left < OPT_BLOCK ? (int)left : OPT_BLOCK;
    const float* g = d.g + base;
    double s = 0.0;
    int k = 0;
    if (((unsigned long)g & 15) == 0) {
        if (cnt == OPT_BLOCK) {               // a full block: the four loads of a thread in flight together, summed in loop order
            float4 gv[OPT_BLOCK / 1024];
#pragma unroll
            for (int j = 0; j < OPT_BLOCK / 1024; ++j) gv[j] = *reinterpret_cast<const float4*>(g + threadIdx.x * 4 + 1024 * j);
#pragma unroll
            for (int j = 0; j < OPT_BLOCK / 1024; ++j) {
                guard_acc(gv[j].x, s, k); guard_acc(gv[j].y, s, k); guard_acc(gv[j].z, s, k); guard_acc(gv[j].w, s, k);
            }
        } else {
            for (int i = threadIdx.x * 4; i + 4 <= cnt; i += 1024) {
                const float4 gv = *reinterpret_cast<const float4*>(g + i);
                guard_acc(gv.x, s, k); guard_acc(gv.y, s, k); guard_acc(gv.z, s, k); guard_acc(gv.w, s, k);
            }
            const int i = (cnt & ~3) + threadIdx.x;
            if (i < cnt) guard_acc(g[i], s, k);
        }
    } else {
        for (int i = threadIdx.x; i < cnt; i += 256) guard_acc(g[i], s, k);
    }
    double kd = (double)k;
    guard_block_sum<256>(s, kd, sh_s, sh_k);
    if (threadIdx.x == 0)
        *reinterpret_cast<double2*>(ws + 2 * (long)(block_offset + blk)) = make_double2(s, kd);
}

// One workgroup of 1,024 threads: thread t sums rows t, t + 1024, ... in that order (four 16-byte row loads in flight per trip: a
// U-Net has 30 k rows, a R50-ViT-B/16 103 k, and a loop of one dependent load per trip would run at the memory latency), then the tree.
constexpr int FIN_THREADS = 1024;
__global__ __launch_bounds__(FIN_THREADS) void grad_guard_finalize_kernel(const double* __restrict__ ws, int rows, double* st) {
    __shared__ double sh_s[FIN_THREADS], sh_k[FIN_THREADS];
    const double2* __restrict__ w2 = reinterpret_cast<const double2*>(ws);
    double S = 0.0, K = 0.0;
    for (int r = threadIdx.x; r < rows; r += 4 * FIN_THREADS) {
        double2 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int rr = r + j * FIN_THREADS;
            v[j] = rr < rows ? w2[rr] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (r + j * FIN_THREADS < rows) { S += v[j].x; K += v[j].y; }
    }
    guard_block_sum<FIN_THREADS>(S, K, sh_s, sh_k);
    if (threadIdx.x != 0) return;
    double d = st[UMI_GUARD_SCALE];
    const double norm = sqrt(S) / d;
    st[UMI_GUARD_NORM] = norm;
    st[UMI_GUARD_NONFINITE] = K;
    const bool skip = K > 0.0;
    st[UMI_GUARD_SKIP] = skip ? 1.0 : 0.0;
    if (!skip) {
        const double mn = st[UMI_GUARD_MAX_NORM];
        double clip = 1.0;
        if (mn > 0.0) {
            const double r = mn / (norm + 1e-6);
            clip = r < 1.0 ? r : 1.0;
        }
        st[UMI_GUARD_COEF] = clip / d;
        if (clip < 1.0) st[UMI_GUARD_CLIPPED] += 1.0;
    } else {
        st[UMI_GUARD_COEF] = 0.0;
        st[UMI_GUARD_SKIPPED] += 1.0;
    }
    st[UMI_GUARD_STEPS] += 1.0;
    const double gi = st[UMI_GUARD_GROWTH_INTERVAL];
    if (gi > 0.0) {                                                    // torch.amp.GradScaler.update
        if (skip) {
            const double b = d * st[UMI_GUARD_BACKOFF], lo = st[UMI_GUARD_MIN_SCALE];
            d = b > lo ? b : lo;
            st[UMI_GUARD_STREAK] = 0.0;
        } else {
            const double streak = st[UMI_GUARD_STREAK] + 1.0;
            if (streak >= gi) {
                const double b = d * st[UMI_GUARD_GROWTH], hi = st[UMI_GUARD_MAX_SCALE];
                d = b < hi ? b : hi;
                st[UMI_GUARD_STREAK] = 0.0;
            } else {
                st[UMI_GUARD_STREAK] = streak;
            }
        }
        st[UMI_GUARD_SCALE] = d;
    }
}

// (a variant with one thread per 8 outputs of the k8 layout -- coalesced reads for the data-gradient layouts -- measured
// slower: 227 vs 173 us per launch on a TransUNet's 105 M parameters; the launch moves 1.26 GB, 0.31 ms at 4 TB/s)
// k8 layouts of matrices with T <= 9 taps go through an LDS tile of 32 n x 32 k x T (round 3): the source is read in ITS order
// (runs of 32 T consecutive floats along whichever of k / n is its inner index: OIHW conv weights, [out][in] linears and their
// transposes alike), the destination is written in 512-byte runs (32 n x 8 k per tap and k-group).  One element per thread in
// destination order -- the path below -- reads 4 bytes per 36-byte stride at best and a different line per lane at worst
// (1.26 GB in 0.50 ms on the TransUNet's 105 M parameters, 0.18 ms on the U-Net's 31 M).
constexpr int PT = 32;
template <typename T, int U>
__device__ __forceinline__ void pack_stage(const umi_pack_desc& d, T* tl, int k0, int n0, bool k_inner) {
    const int TT = d.T;
    for (int e0 = threadIdx.x; e0 < PT * PT * TT; e0 += 256 * U) {
        float v[U];
        int li[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + 256 * u;
            const int o_ = e / (PT * TT), r = e - o_ * (PT * TT);
            const int i_ = r / TT, t = r - i_ * TT;
            const int kl = k_inner ? i_ : o_, nl = k_inner ? o_ : i_;
            const int k = k0 + kl, n = n0 + nl;
            ok[u] = e < PT * PT * TT && k < d.K && n < d.N;
            li[u] = e < PT * PT * TT ? (t * PT + kl) * (PT + 2) + nl : -1;
            // unconditional loads from clamped (in-range) addresses, selected afterwards: `ok ? src[..] : 0` compiles to a
            // branch per load with a wait of its own, i.e. ONE load in flight per thread instead of U
            const int tc = t < TT ? t : TT - 1, kc = k < d.K ? k : d.K - 1, nc = n < d.N ? n : d.N - 1;
            v[u] = d.src[(long)(d.flip_t ? TT - 1 - tc : tc) * d.st + (long)kc * d.sk + (long)nc * d.sn];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) asm volatile("" : "+v"(v[u]));       // (keeps hipcc from sinking the loads under `ok`)
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = ok[u] ? v[u] : 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (li[u] >= 0) tl[li[u]] = (T)v[u];
    }
}

template <typename T>
__device__ void pack_tiles_k8(const umi_pack_desc& d, int my_blk, int n_blk) {
    __shared__ T tl[9 * PT * (PT + 2)];                       // [t][k][n], row pad 2
    const int nkt = (d.Kpad + PT - 1) / PT, nnt = (d.Npad + PT - 1) / PT;
    const int kb8 = d.Kpad >> 3, ldn = d.ldn ? d.ldn : d.Npad, TT = d.T;
    const bool k_inner = d.sk <= d.sn;                        // the source's inner index among (k, n)
    T* dst = (T*)d.dst;
    for (int tile = my_blk; tile < nkt * nnt; tile += n_blk) {
        const int k0 = (tile % nkt) * PT, n0 = (tile / nkt) * PT;
        // U loads in flight per thread (a one-load loop runs at the memory latency: 36 trips per tile at T = 9): 12 for the
        // 3 x 3 convs' tiles (three trips), 4 otherwise (a T = 1 tile is one trip of four)
        if (TT == 9) pack_stage<T, 12>(d, tl, k0, n0, k_inner);
        else pack_stage<T, 4>(d, tl, k0, n0, k_inner);
        __syncthreads();
        // pieces of 8 k for one (t, k-group, n): 16 bytes (fp16) each, 32 n adjacent
        for (int e = threadIdx.x; e < TT * (PT / 8) * PT; e += 256) {
            const int nl = e % PT, r = e / PT, kg = r % (PT / 8), t = r / (PT / 8);
            const int k = k0 + kg * 8, n = n0 + nl;
            if (k >= d.Kpad || n >= d.Npad) continue;
            T pk[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) pk[j] = tl[(t * PT + kg * 8 + j) * (PT + 2) + nl];
            T* o = dst + (((long)t * kb8 + (k >> 3)) * ldn + n) * 8;
            typedef T vec8 __attribute__((ext_vector_type(8)));
            vec8 pv;
#pragma unroll
            for (int j = 0; j < 8; ++j) pv[j] = pk[j];
            *reinterpret_cast<vec8*>(o) = pv;
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(256) void pack_multi_kernel(const umi_pack_desc* __restrict__ descs, int n_desc) {
    const int blk = blockIdx.x;
    const umi_pack_desc d = descs[find_desc(descs, n_desc, blk)];
    const long total = (long)d.T * d.Kpad * d.Npad;
    if (d.k8 && d.T <= 9 && sizeof(T) == 2) {                 // (uniform per workgroup)
        pack_tiles_k8<T>(d, blk - d.blk0, (int)((total + PACK_BLOCK - 1) / PACK_BLOCK));
        return;
    }
    const long base = (long)(blk - d.blk0) * PACK_BLOCK;
    T* dst = (T*)d.dst;
    const int kb8 = d.Kpad >> 3;
    const int ldn = d.ldn ? d.ldn : d.Npad;
#pragma unroll 2
    for (int j = 0; j < PACK_BLOCK / 256; ++j) {
        const long i = base + j * 256 + threadIdx.x;
        if (i >= total) break;
        int n, k, t;
        long o;                          // destination index (== i unless the entry is a column slice: ldn > Npad)
        if (d.k8) {                      // dst[t][k/8][n][k%8]
            const int k8 = (int)(i & 7);
            long r = i >> 3;
            n = (int)(r % d.Npad); r /= d.Npad;
            const int kb = (int)(r % kb8);
            t = (int)(r / kb8);
            k = kb * 8 + k8;
            o = (((long)t * kb8 + kb) * ldn + n) * 8 + k8;
        } else {                         // dst[t][k][n]
            n = (int)(i % d.Npad);
            const long r = i / d.Npad;
            k = (int)(r % d.Kpad);
            t = (int)(r / d.Kpad);
            o = ((long)t * d.Kpad + k) * ldn + n;
        }
        float v = 0.f;
        if (k < d.K && n < d.N) {
            const int ts = d.flip_t ? (d.T - 1 - t) : t;
            v = d.src[ts * d.st + k * d.sk + n * d.sn];
        }
        dst[o] = (T)v;
    }
}

}  // namespace

// Descriptor-table upload as a KERNEL: `src` is pinned host memory (device-mapped), `dst` the device copy the update /
// pack kernels read.  Inside a HIP-graph capture this is an ordinary kernel node that re-reads the host buffer on every
// replay; a captured host-to-device memcpy of a torch pinned buffer did not replay reliably on ROCm 7.2 (the replayed
// optimizer step saw a stale table).
__global__ __launch_bounds__(256) void table_upload_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int n16) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n16; i += gridDim.x * 256) dst[i] = src[i];
}
extern "C" int umi_table_upload(const void* host_pinned, void* dev, size_t nbytes, umi_stream_t stream) {
    if (!host_pinned || !dev || nbytes == 0 || (nbytes & 15) || (((uintptr_t)host_pinned | (uintptr_t)dev) & 15)) return UMI_ERR_BADARG;
    const int n16 = (int)(nbytes / 16);
    int grid = (n16 + 255) / 256;
    if (grid > 64) grid = 64;
    hipLaunchKernelGGL(table_upload_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint4*)host_pinned, (uint4*)dev, n16);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_optim_block_elems(void) { return OPT_BLOCK; }
extern "C" int umi_pack_block_elems(void) { return PACK_BLOCK; }

// Hyper-parameters arrive as doubles and are rounded to fp32 exactly where torch rounds them (1 - dampening and 1 - beta
// are formed in double first: 1 - 0.999 is 0.001f there, not 1.f - 0.999f).
extern "C" int umi_optim_sgd_multi(const void* descs, int n_desc, int total_blocks, double lr, double momentum,
                                   double dampening, double weight_decay, int nesterov, int first_step,
                                   umi_stream_t stream) {
    if (!descs || n_desc <= 0 || total_blocks <= 0) return UMI_ERR_BADARG;
    SgdArgs a{(float)lr, (float)momentum, (float)(1.0 - dampening), (float)weight_decay, nesterov, first_step, nullptr};
    hipLaunchKernelGGL((optim_multi_kernel<false, SgdArgs>), dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const umi_optim_desc*)descs, n_desc, a);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_optim_adam_multi(const void* descs, int n_desc, int total_blocks, double step_size, double beta1,
                                    double beta2, double bc2_sqrt, double eps, double weight_decay, umi_stream_t stream) {
    if (!descs || n_desc <= 0 || total_blocks <= 0) return UMI_ERR_BADARG;
    AdamArgs a{(float)step_size, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)bc2_sqrt, (float)eps,
               (float)weight_decay, nullptr};
    hipLaunchKernelGGL((optim_multi_kernel<true, AdamArgs>), dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const umi_optim_desc*)descs, n_desc, a);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

// ---- device-resident hyper-parameters (graph-safe learning rate / Adam step count) ------------------------------------
__global__ void hyper_pre_kernel(Hyper* h, int adam, const double* guard) {
    if (adam && !(guard && guard[UMI_GUARD_SKIP] != 0.0)) {                                   // torch.optim.Adam: step += 1; bias corrections in double, then rounded
        const double t = h->adam_t + 1.0;
        h->adam_t = t;
        const double bc1 = 1.0 - pow(h->beta1, t), bc2 = 1.0 - pow(h->beta2, t);
        h->step_size_f = (float)(h->lr / bc1);
        h->bc2_sqrt_f = (float)sqrt(bc2);
    }
    h->lr_f = (float)h->lr;
}
// reference Trainer.py:722-726: lr = base_lr * (1 - iter_num / max_iterations) ** 0.9 with the PRE-increment iter_num, written
// after the optimizer step; then iter_num += 1
__global__ void hyper_poly_kernel(Hyper* h) {
    h->lr = h->base_lr * pow(1.0 - h->iter / h->max_iter, h->power);
    h->iter += 1.0;
}

// The schedule rule of include/unetmi.h, after the update: iter += 1; lr = base_lr * factor(iter).  No lag: step k (from 0) runs
// on base_lr * factor(k), which device_schedule wrote for k = iter_num and this kernel writes for every later k.
__global__ void hyper_schedule_kernel(Hyper* h) {
    const double k = h->iter + 1.0;
    h->iter = k;
    const double w = h->warmup > 0.0 ? fmin(1.0, (k + 1.0) / h->warmup) : 1.0;
    const double x = fmin(k, h->max_iter) / h->max_iter;
    double s = 1.0;
    if (h->kind == UMI_SCHED_POLY) s = pow(1.0 - x, h->power);
    else if (h->kind == UMI_SCHED_COSINE) s = 0.5 * (1.0 + cos(3.141592653589793 * x));
    h->lr = h->base_lr * (w * (h->final_ratio + (1.0 - h->final_ratio) * s));
}

extern "C" size_t umi_optim_hyper_bytes(void) { return sizeof(Hyper); }

extern "C" int umi_optim_hyper_pre(void* hyper, int adam, umi_stream_t stream) {
    if (!hyper || ((uintptr_t)hyper & 7)) return UMI_ERR_BADARG;
    hipLaunchKernelGGL(hyper_pre_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (Hyper*)hyper, adam, (const double*)nullptr);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_optim_hyper_poly(void* hyper, umi_stream_t stream) {
    if (!hyper || ((uintptr_t)hyper & 7)) return UMI_ERR_BADARG;
    hipLaunchKernelGGL(hyper_poly_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (Hyper*)hyper);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_optim_hyper_schedule(void* hyper, umi_stream_t stream) {
    if (!hyper || ((uintptr_t)hyper & 7)) return UMI_ERR_BADARG;
    hipLaunchKernelGGL(hyper_schedule_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (Hyper*)hyper);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_optim_sgd_multi_dev(const void* descs, int n_desc, int total_blocks, const void* hyper, double momentum,
                                       double dampening, double weight_decay, int nesterov, int first_step,
                                       umi_stream_t stream) {
    if (!descs || !hyper || n_desc <= 0 || total_blocks <= 0) return UMI_ERR_BADARG;
    SgdArgs a{0.f, (float)momentum, (float)(1.0 - dampening), (float)weight_decay, nesterov, first_step, (const Hyper*)hyper};
    hipLaunchKernelGGL((optim_multi_kernel<false, SgdArgs>), dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const umi_optim_desc*)descs, n_desc, a);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_optim_adam_multi_dev(const void* descs, int n_desc, int total_blocks, const void* hyper, double beta1,
                                        double beta2, double eps, double weight_decay, umi_stream_t stream) {
    if (!descs || !hyper || n_desc <= 0 || total_blocks <= 0) return UMI_ERR_BADARG;
    AdamArgs a{0.f, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), 1.f, (float)eps, (float)weight_decay,
               (const Hyper*)hyper};
    hipLaunchKernelGGL((optim_multi_kernel<true, AdamArgs>), dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const umi_optim_desc*)descs, n_desc, a);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

// ---- guarded step (include/unetmi.h) ------------------------------------------------------------------------------------------
extern "C" size_t umi_grad_guard_ws_bytes(int total_blocks) {
    return total_blocks > 0 ? (size_t)total_blocks * 2 * sizeof(double) : 0;
}

extern "C" int umi_grad_norm_partials(const void* descs, int n_desc, int total_blocks, int block_offset, void* ws,
                                      size_t ws_bytes, umi_stream_t stream) {
    if (!descs || !ws || ((uintptr_t)ws & 15) || n_desc <= 0 || total_blocks <= 0 || block_offset < 0) return UMI_ERR_BADARG;
    if ((long)block_offset + total_blocks > 0x7fffffffL) return UMI_ERR_BADARG;
    if (ws_bytes < umi_grad_guard_ws_bytes(block_offset + total_blocks)) return UMI_ERR_WORKSPACE;
    hipLaunchKernelGGL(grad_norm_partials_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const umi_optim_desc*)descs, n_desc, block_offset, (double*)ws);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_grad_guard_finalize(const void* ws, int total_blocks, double* state, umi_stream_t stream) {
    if (!ws || !state || ((uintptr_t)ws & 15) || ((uintptr_t)state & 7) || total_blocks <= 0) return UMI_ERR_BADARG;
    hipLaunchKernelGGL(grad_guard_finalize_kernel, dim3(1), dim3(FIN_THREADS), 0, (hipStream_t)stream, (const double*)ws, total_blocks,
                       state);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_optim_hyper_pre_guarded(void* hyper, int adam, const double* guard, umi_stream_t stream) {
    if (!hyper || !guard || (((uintptr_t)hyper | (uintptr_t)guard) & 7)) return UMI_ERR_BADARG;
    hipLaunchKernelGGL(hyper_pre_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (Hyper*)hyper, adam, guard);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_optim_sgd_multi_guarded(const void* descs, int n_desc, int total_blocks, const void* hyper, double lr,
                                           double momentum, double dampening, double weight_decay, int nesterov,
                                           int first_step, const double* guard, umi_stream_t stream) {
    if (!descs || !guard || ((uintptr_t)guard & 7) || n_desc <= 0 || total_blocks <= 0 || dampening != 0.0) return UMI_ERR_BADARG;
    SgdArgs a{(float)lr, (float)momentum, 1.f, (float)weight_decay, nesterov, first_step, (const Hyper*)hyper};
    hipLaunchKernelGGL((optim_multi_guarded_kernel<false, SgdArgs>), dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const umi_optim_desc*)descs, n_desc, a, guard);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_optim_adam_multi_guarded(const void* descs, int n_desc, int total_blocks, const void* hyper,
                                            double step_size, double beta1, double beta2, double bc2_sqrt, double eps,
                                            double weight_decay, const double* guard, umi_stream_t stream) {
    if (!descs || !guard || ((uintptr_t)guard & 7) || n_desc <= 0 || total_blocks <= 0) return UMI_ERR_BADARG;
    AdamArgs a{(float)step_size, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)bc2_sqrt, (float)eps,
               (float)weight_decay, (const Hyper*)hyper};
    hipLaunchKernelGGL((optim_multi_guarded_kernel<true, AdamArgs>), dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const umi_optim_desc*)descs, n_desc, a, guard);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

// ---- AdamW: the Adam entry points with decoupled weight decay (include/unetmi.h) ---------------------------------------------
extern "C" int umi_optim_adamw_multi(const void* descs, int n_desc, int total_blocks, double lr, double step_size, double beta1,
                                     double beta2, double bc2_sqrt, double eps, double weight_decay, umi_stream_t stream) {
    if (!descs || n_desc <= 0 || total_blocks <= 0) return UMI_ERR_BADARG;
    AdamWArgs a{(float)step_size, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)bc2_sqrt, (float)eps, 0.f,
                nullptr, lr, weight_decay};
    hipLaunchKernelGGL((optim_multi_kernel<true, AdamWArgs, true>), dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const umi_optim_desc*)descs, n_desc, a);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_optim_adamw_multi_dev(const void* descs, int n_desc, int total_blocks, const void* hyper, double beta1,
                                         double beta2, double eps, double weight_decay, umi_stream_t stream) {
    if (!descs || !hyper || n_desc <= 0 || total_blocks <= 0) return UMI_ERR_BADARG;
    AdamWArgs a{0.f, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), 1.f, (float)eps, 0.f, (const Hyper*)hyper, 0.0,
                weight_decay};
    hipLaunchKernelGGL((optim_multi_kernel<true, AdamWArgs, true>), dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const umi_optim_desc*)descs, n_desc, a);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_optim_adamw_multi_guarded(const void* descs, int n_desc, int total_blocks, const void* hyper, double lr,
                                             double step_size, double beta1, double beta2, double bc2_sqrt, double eps,
                                             double weight_decay, const double* guard, umi_stream_t stream) {
    if (!descs || !guard || ((uintptr_t)guard & 7) || n_desc <= 0 || total_blocks <= 0) return UMI_ERR_BADARG;
    AdamWArgs a{(float)step_size, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)bc2_sqrt, (float)eps, 0.f,
                (const Hyper*)hyper, lr, weight_decay};
    hipLaunchKernelGGL((optim_multi_guarded_kernel<true, AdamWArgs, true>), dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const umi_optim_desc*)descs, n_desc, a, guard);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_pack_kn_multi(const void* descs, int n_desc, int total_blocks, int dtype, umi_stream_t stream) {
    if (!descs || n_desc <= 0 || total_blocks <= 0) return UMI_ERR_BADARG;
    if (dtype == UMI_F16)
        hipLaunchKernelGGL((pack_multi_kernel<half_t>), dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                           (const umi_pack_desc*)descs, n_desc);
    else if (dtype == UMI_F32)
        hipLaunchKernelGGL((pack_multi_kernel<float>), dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                           (const umi_pack_desc*)descs, n_desc);
    else return UMI_ERR_BADARG;
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
