// 8-connected component labelling of a batch of binary masks on the device (reference loss.py:422-440 `MRAccuracy`:
// cv2.connectedComponents(connectivity=8) per image after a device -> host copy).  Exact and deterministic: label numbers
// follow the raster order of each component's first pixel (SciPy's numbering for ndimage.label with a full 3x3 structure).
//
// A union-find whose representative is the component's minimum flat index (cc_unionfind.h), in separate launches on the
// caller's stream, the whole batch in every launch.  Kernel boundaries are the only ordering between passes: no workgroup
// waits for another one, nothing depends on dispatch order, timing or placement.
//
//   1. tile     one workgroup per 64 x 64 tile: row masks by ballot, every row run starts as one set (its first pixel), links
//               to the row above by atomicMin on LDS words, then parent[p] = flat index of the tile-local root (-1: background).
//   2. seam     one thread per pixel of a tile's last row / last column: union with its neighbours across the seam on the
//               global parent map.  Workgroups touch the same words here, so EVERY access is an agent-scope atomic (relaxed
//               load in find, atomicMin to link): a plain load could be served from a CU's L1 that no other CU's write refreshes.
//   3. flatten  root[p] = find(p), written to a second array (the labels output) so that no thread reads a word that another
//               thread of the launch rewrites; the roots (root[p] == p) of every 1024-pixel block are counted.
//               Counting alone needs no find: after pass 2 the roots are the pixels with parent[p] == p.
//   4. scan     per image, a fixed-order exclusive scan of the block counts; the total is counts[n].
//   5. rank     each root's number = block offset + its raster position among the block's roots, written over parent[root].
//   6. relabel  labels[p] = number of root[p]; area / sum_y / sum_x by INTEGER atomic adds, one per label that a 64-pixel wave chunk
//               meets, and one per up to 16 chunks while the label stays the same (one huge component would otherwise send
//               every add to one address).
//
// Every find / union loop is capped by the image's pixel count; a reached cap or a broken chain stores a UMI_CC_FAULT_* code
// in the first word of the workspace (an ordinary vector store) and the thread stops following the map, so a corrupted map
// cannot hang the device.  The launch functions clear that word, and the statistics, on every call.
//
// Class-valued masks (umi_count_class_components / umi_label_class_components: values 0 .. K - 1, K <= 8, two pixels in one
// component iff 8-connected through pixels of the SAME non-zero value) run the same passes over all classes at once:
//   1. tile     one ballot per class and row (K - 1 row masks per tile row in LDS); a lane picks the masks of its own class and
//               the row-run / link helpers apply to them unchanged, so a run is a run of one class and links stay in the class.
//   2. seam     a neighbour across the seam counts when its mask value equals the pixel's.
//   3..6        unchanged (a root is a root whatever its class); the rank pass also tallies the roots per class (integer adds)
//               and stores each label's class, and the relabel pass keeps statistics for the labels 1 .. cap only, cap being the
//               caller's: more labels than that leave counts and the label map exact and set UMI_CC_FAULT_CAP.
// A mask value >= K is background and sets UMI_CC_FAULT_CLASS; it is compared, never used as an index.
#include "common.h"
#include "cc_unionfind.h"

namespace {

constexpr int CC_T = 64;               // tile edge == wavefront width: one ballot is one row mask
constexpr int CC_BLK = 1024;           // pixels per block of the flatten / rank passes
constexpr int CC_HEAD = 256;           // bytes reserved for the fault word in front of the workspace
constexpr int CC_CHUNKS = 16;          // 64-pixel chunks per wave in the relabel pass
constexpr int CC_MAX_CLASSES = 8;      // class values 0 .. 7: 8 x 64 row masks of 8 bytes = 4 KB of LDS per tile

struct CcLds {                         // one workgroup's LDS words
    static __device__ __forceinline__ int load(const int* p) {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    static __device__ __forceinline__ int fetch_min(int* p, int v) {
        return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};
struct CcAgent {                       // global words that other workgroups link concurrently
    static __device__ __forceinline__ int load(const int* p) {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ int fetch_min(int* p, int v) {
        return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
struct CcPlain {                       // global words nobody writes during the launch
    static __device__ __forceinline__ int load(const int* p) { return *p; }
};

__global__ __launch_bounds__(256) void cc_tile_kernel(const unsigned char* __restrict__ mask, int* __restrict__ parent, int H,
                                                      int W, int* __restrict__ err) {
    __shared__ unsigned long long rows[CC_T];
    __shared__ int lab[CC_T * CC_T];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x0 = blockIdx.x * CC_T, y0 = blockIdx.y * CC_T, x = x0 + lane;
    const long img = (long)blockIdx.z * H * W;
    int fault = 0;
    for (int r = wv; r < CC_T; r += 4) {
        const int y = y0 + r;
        const bool fg = y < H && x < W && mask[img + (long)y * W + x] != 0;
        const unsigned long long m = __ballot(fg);
        if (lane == 0) rows[r] = m;
        lab[r * CC_T + lane] = fg ? r * CC_T + umi_cc_run_start(m, lane) : -1;
    }
    __syncthreads();
    for (int r = wv < 1 ? 4 : wv; r < CC_T; r += 4) {          // rows 1..63
        const unsigned long long m = rows[r], a = rows[r - 1];
        if (!((m >> lane) & 1ull)) continue;
        const int p = r * CC_T + lane, k = umi_cc_links_above(m, a, lane);
        if (k & 1) umi_cc_union<CcLds>(lab, p, p - CC_T, CC_T * CC_T, &fault);
        if (k & 2) umi_cc_union<CcLds>(lab, p, p - CC_T - 1, CC_T * CC_T, &fault);
        if (k & 4) umi_cc_union<CcLds>(lab, p, p - CC_T + 1, CC_T * CC_T, &fault);
    }
    __syncthreads();
    for (int r = wv; r < CC_T; r += 4) {
        const int y = y0 + r;
        if (y >= H || x >= W) continue;
        int g = -1;
        if ((rows[r] >> lane) & 1ull) {
            const int root = umi_cc_find<CcLds>(lab, r * CC_T + lane, CC_T * CC_T, &fault);
            if (root >= 0) g = (int)(img + (long)(y0 + (root >> 6)) * W + x0 + (root & 63));
        }
        parent[img + (long)y * W + x] = g;
    }
    if (fault) *err = fault;
}

// Stores a fault code.  The union-find codes (corrupted map, results invalid) are stored unconditionally; UMI_CC_FAULT_CLASS and
// UMI_CC_FAULT_CAP (results valid as documented) only into a word that is still 0, so they never hide a union-find code and the
// first of them stays.
__device__ __forceinline__ void cc_report(int* err, int fault) {
    if (fault >= UMI_CC_FAULT_CLASS) atomicCAS(err, 0, fault);
    else *err = fault;
}

// mask value -> class: values >= K are background (callers that report it set UMI_CC_FAULT_CLASS)
__device__ __forceinline__ int cc_class(unsigned char v, int K) { return v < K ? v : 0; }

// Adds the number of this wave's lanes of each class (c: the class of a root lane, 0 elsewhere) to the workgroup's LDS tally:
// integer adds, one per class that the wave meets.  Called by whole waves.
__device__ __forceinline__ void cc_class_tally(int* tally, int c, int K, int lane) {
    for (int q = 1; q < K; ++q) {
        const int cnt = __popcll(__ballot(c == q));
        if (cnt && lane == 0) atomicAdd(tally + q, cnt);
    }
}

// The tile pass for class values 0 .. K - 1 (2 <= K <= CC_MAX_CLASSES).  rows[k][r] is the row mask of class k; a lane works
// on the masks of its own class, which it keeps for its 16 rows in 4-bit fields of one register.
__global__ __launch_bounds__(256) void cc_class_tile_kernel(const unsigned char* __restrict__ mask, int* __restrict__ parent, int H,
                                                            int W, int K, int* __restrict__ err) {
    __shared__ unsigned long long rows[CC_MAX_CLASSES][CC_T];
    __shared__ int lab[CC_T * CC_T];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x0 = blockIdx.x * CC_T, y0 = blockIdx.y * CC_T, x = x0 + lane;
    const long img = (long)blockIdx.z * H * W;
    int fault = 0;
    bool foreign = false;
    unsigned long long cls = 0;                                  // bits 4j .. 4j + 3: class of (row wv + 4j, column lane)
    for (int j = 0; j < CC_T / 4; ++j) {
        const int r = wv + 4 * j, y = y0 + r;
        int c = 0;
        if (y < H && x < W) {
            const unsigned char v = mask[img + (long)y * W + x];
            c = cc_class(v, K);
            if (v >= K) foreign = true;
        }
        unsigned long long m = 0;
        for (int k = 1; k < K; ++k) {
            const unsigned long long b = __ballot(c == k);
            if (lane == 0) rows[k][r] = b;
            if (c == k) m = b;
        }
        cls |= (unsigned long long)c << (4 * j);
        lab[r * CC_T + lane] = c ? r * CC_T + umi_cc_run_start(m, lane) : -1;
    }
    __syncthreads();
    for (int j = 0; j < CC_T / 4; ++j) {
        const int r = wv + 4 * j, c = (int)((cls >> (4 * j)) & 15ull);
        if (r == 0 || !c) continue;
        const unsigned long long m = rows[c][r], a = rows[c][r - 1];
        const int p = r * CC_T + lane, k = umi_cc_links_above(m, a, lane);
        if (k & 1) umi_cc_union<CcLds>(lab, p, p - CC_T, CC_T * CC_T, &fault);
        if (k & 2) umi_cc_union<CcLds>(lab, p, p - CC_T - 1, CC_T * CC_T, &fault);
        if (k & 4) umi_cc_union<CcLds>(lab, p, p - CC_T + 1, CC_T * CC_T, &fault);
    }
    __syncthreads();
    for (int j = 0; j < CC_T / 4; ++j) {
        const int r = wv + 4 * j, y = y0 + r;
        if (y >= H || x >= W) continue;
        int g = -1;
        if ((cls >> (4 * j)) & 15ull) {
            const int root = umi_cc_find<CcLds>(lab, r * CC_T + lane, CC_T * CC_T, &fault);
            if (root >= 0) g = (int)(img + (long)(y0 + (root >> 6)) * W + x0 + (root & 63));
        }
        parent[img + (long)y * W + x] = g;
    }
    if (foreign) cc_report(err, UMI_CC_FAULT_CLASS);
    if (fault) cc_report(err, fault);
}

// nhs / nvs: horizontal / vertical seams of one image, (H - 1) / 64 and (W - 1) / 64.  CLS: a neighbour counts when its mask
// value is the pixel's own class (mask and parent share flat indices); otherwise when it is foreground.
template <bool CLS>
__global__ __launch_bounds__(256) void cc_seam_kernel(const unsigned char* __restrict__ mask, int K, int* parent, int N, int H, int W,
                                                      int nhs, int nvs, int* __restrict__ err) {
    const long per = (long)nhs * W + (long)nvs * H;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= per * N) return;
    const int n = (int)(t / per);
    long r = t - (long)n * per;
    const int cap = H * W;
    const long img = (long)n * H * W;
    int fault = 0;
    int p, step;            // the pixel, and the distance between its three neighbours across the seam
    int q;                  // the neighbour straight across
    bool lo_in, hi_in;
    if (r < (long)nhs * W) {
        const int s = (int)(r / W), x = (int)(r - (long)s * W), y = s * CC_T + CC_T - 1;
        p = (int)(img + (long)y * W + x);
        q = p + W;
        step = 1;
        lo_in = x > 0;
        hi_in = x + 1 < W;
    } else {
        r -= (long)nhs * W;
        const int s = (int)(r / H), y = (int)(r - (long)s * H), x = s * CC_T + CC_T - 1;
        p = (int)(img + (long)y * W + x);
        q = p + 1;
        step = W;
        lo_in = y > 0;
        hi_in = y + 1 < H;
    }
    bool mid, lo, hi;
    if (CLS) {
        const int c = cc_class(mask[p], K);
        if (!c) return;
        mid = cc_class(mask[q], K) == c;
        lo = lo_in && cc_class(mask[q - step], K) == c;
        hi = hi_in && cc_class(mask[q + step], K) == c;
    } else {
        if (CcAgent::load(parent + p) < 0) return;
        mid = CcAgent::load(parent + q) >= 0;
        lo = lo_in && CcAgent::load(parent + q - step) >= 0;
        hi = hi_in && CcAgent::load(parent + q + step) >= 0;
    }
    const int k = umi_cc_links_across(lo, mid, hi);
    if (k & 1) umi_cc_union<CcAgent>(parent, p, q, cap, &fault);
    if (k & 2) umi_cc_union<CcAgent>(parent, p, q - step, cap, &fault);
    if (k & 4) umi_cc_union<CcAgent>(parent, p, q + step, cap, &fault);
    if (fault) *err = fault;
}

// blockIdx.x = 1024-pixel block of image blockIdx.y.  FULL: root[p] = find(p) (or -1) as well as the count of roots.
template <bool FULL>
__global__ __launch_bounds__(256) void cc_flatten_kernel(const int* __restrict__ parent, int* __restrict__ root, int HW, int nblk,
                                                         int* __restrict__ blockcnt, int* __restrict__ err) {
    __shared__ int wsum[4];
    const long img = (long)blockIdx.y * HW;
    int fault = 0, mine = 0;
    for (int k = 0; k < CC_BLK / 256; ++k) {
        const int i = blockIdx.x * CC_BLK + k * 256 + threadIdx.x;
        bool is_root = false;
        if (i < HW) {
            const int p = (int)(img + i);
            const int par = parent[p];
            int rt = par;
            if (FULL) {
                if (par >= 0) rt = umi_cc_find<CcPlain>(parent, p, HW, &fault);
                root[p] = rt;
                is_root = rt == p;
            } else is_root = par == p;
        }
        mine += __popcll(__ballot(is_root));
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) blockcnt[(long)blockIdx.y * nblk + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (fault) *err = fault;
}

// one workgroup per image: blockcnt -> exclusive prefix in raster order (in place), counts[n] = total.  Thread t owns the
// contiguous segment [t * seg, (t + 1) * seg); the 256 segment sums are scanned by thread 0.
__global__ __launch_bounds__(256) void cc_scan_kernel(int* __restrict__ blockcnt, int nblk, int* __restrict__ counts) {
    __shared__ int part[256];
    int* c = blockcnt + (long)blockIdx.x * nblk;
    const int seg = (nblk + 255) / 256, b0 = threadIdx.x * seg, b1 = min(b0 + seg, nblk);
    int s = 0;
    for (int b = b0; b < b1; ++b) s += c[b];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) {
            const int v = part[t];
            part[t] = run;
            run += v;
        }
        counts[blockIdx.x] = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int b = b0; b < b1; ++b) {
        const int v = c[b];
        c[b] = run;
        run += v;
    }
}

// number[root] = 1 + block offset + raster position among the block's roots, written over parent[root] (parent is dead after
// the flatten pass; only root words are written, and only root words are read back by the relabel pass).  CLS: the roots
// of each class are also added to class_counts[image][class] (integer adds, through an LDS tally per workgroup: the total
// does not depend on their order) and
// label_class[image][number - 1] = the root's class for the numbers 1 .. cap.
template <bool CLS>
__global__ __launch_bounds__(256) void cc_rank_kernel(const int* __restrict__ root, int* __restrict__ number, int HW, int nblk,
                                                      const int* __restrict__ blockoff, const unsigned char* __restrict__ mask, int K,
                                                      int cap, unsigned char* __restrict__ label_class, int* __restrict__ class_counts) {
    __shared__ int wcnt[CC_BLK / 64];
    __shared__ int tally[CC_MAX_CLASSES];
    const long img = (long)blockIdx.y * HW;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bool flag[CC_BLK / 256];
    int before[CC_BLK / 256];
    if (CLS) {
        if (threadIdx.x < CC_MAX_CLASSES) tally[threadIdx.x] = 0;
        __syncthreads();
    }
    for (int k = 0; k < CC_BLK / 256; ++k) {
        const int i = blockIdx.x * CC_BLK + k * 256 + threadIdx.x;
        flag[k] = i < HW && root[img + i] == (int)(img + i);
        const unsigned long long b = __ballot(flag[k]);
        before[k] = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[k * 4 + wv] = __popcll(b);
        if (CLS && b) cc_class_tally(tally, flag[k] ? cc_class(mask[img + i], K) : 0, K, lane);        // b is wave-uniform
    }
    __syncthreads();
    if (CLS && threadIdx.x >= 1 && (int)threadIdx.x < K && tally[threadIdx.x])
        atomicAdd(class_counts + (long)blockIdx.y * K + threadIdx.x, tally[threadIdx.x]);
    const int off = blockoff[(long)blockIdx.y * nblk + blockIdx.x];
    for (int k = 0; k < CC_BLK / 256; ++k) {
        if (!flag[k]) continue;
        int pre = 0;
        for (int j = 0; j < k * 4 + wv; ++j) pre += wcnt[j];
        const int i = blockIdx.x * CC_BLK + k * 256 + threadIdx.x, num = off + pre + before[k] + 1;
        number[img + i] = num;
        if (CLS && num >= 1 && num <= cap) label_class[(long)blockIdx.y * cap + num - 1] = (unsigned char)cc_class(mask[img + i], K);
    }
}

// counts only: the roots (parent[p] == p after the seam pass) of each class, added to class_counts[image][class]
__global__ __launch_bounds__(256) void cc_class_count_kernel(const int* __restrict__ parent, const unsigned char* __restrict__ mask,
                                                             int HW, int K, int* __restrict__ class_counts) {
    __shared__ int tally[CC_MAX_CLASSES];
    const long img = (long)blockIdx.y * HW;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < CC_MAX_CLASSES) tally[threadIdx.x] = 0;
    __syncthreads();
    for (int k = 0; k < CC_BLK / 256; ++k) {
        const int i = blockIdx.x * CC_BLK + k * 256 + threadIdx.x;
        const bool is_root = i < HW && parent[img + i] == (int)(img + i);
        if (__ballot(is_root)) cc_class_tally(tally, is_root ? cc_class(mask[img + i], K) : 0, K, lane);
    }
    __syncthreads();
    if (threadIdx.x >= 1 && (int)threadIdx.x < K && tally[threadIdx.x])
        atomicAdd(class_counts + (long)blockIdx.y * K + threadIdx.x, tally[threadIdx.x]);
}

__device__ __forceinline__ void cc_stat_add(int* area, long long* sy, long long* sx, long slot, int a, long long y, long long x) {
    atomicAdd(area + slot, a);
    atomicAdd((unsigned long long*)(sy + slot), (unsigned long long)y);
    atomicAdd((unsigned long long*)(sx + slot), (unsigned long long)x);
}

// sum of the lane numbers of the set bits of m
__device__ __forceinline__ int cc_lane_sum(unsigned long long m) {
    return __popcll(m & 0xAAAAAAAAAAAAAAAAull) + 2 * __popcll(m & 0xCCCCCCCCCCCCCCCCull) + 4 * __popcll(m & 0xF0F0F0F0F0F0F0F0ull) +
           8 * __popcll(m & 0xFF00FF00FF00FF00ull) + 16 * __popcll(m & 0xFFFF0000FFFF0000ull) + 32 * __popcll(m & 0xFFFFFFFF00000000ull);
}

// labels holds root[] on entry.  Each wave walks CC_CHUNKS consecutive 64-pixel chunks of one image and adds per LABEL, not per
// pixel: the lanes of a chunk that carry one label are found by ballot and their area and coordinate sums follow from the lane
// mask alone (a chunk of an image at least 64 pixels wide meets at most two rows), and sums for the label the wave met last stay
// in registers until another label turns up.  All of that is wave-uniform; lane 0 issues the adds.
// CLS: cap is the caller's and may be smaller than the number of labels; a label above it is still written to the map, gets
// no statistics (nothing is stored at or beyond entry cap) and sets UMI_CC_FAULT_CAP.
template <bool CLS>
__global__ __launch_bounds__(256) void cc_relabel_kernel(int* __restrict__ labels, const int* __restrict__ number, int HW, int W,
                                                         int cap, int* __restrict__ area, long long* __restrict__ sum_y,
                                                         long long* __restrict__ sum_x, int* __restrict__ err) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long img = (long)blockIdx.y * HW, stat0 = (long)blockIdx.y * cap;
    const int base = (blockIdx.x * 4 + wv) * (CC_CHUNKS * 64);
    int pend_lbl = 0, pend_area = 0;             // wave-uniform: sums of the label met last, not yet added
    long long pend_y = 0, pend_x = 0;
    int fault = 0;
    bool over = false;
    for (int k = 0; k < CC_CHUNKS; ++k) {
        const int i0 = base + k * 64;
        if (i0 >= HW) break;                      // wave-uniform
        const int i = i0 + lane;
        int lbl = 0;
        if (i < HW) {
            const int rt = labels[img + i];
            if (rt >= 0) lbl = number[rt];
            if (lbl < 0 || lbl > (CLS ? HW : cap)) {
                fault = UMI_CC_FAULT_RANK;
                lbl = 0;
            }
            labels[img + i] = lbl;
            if (CLS && lbl > cap) {
                over = true;
                lbl = 0;                                         // no statistics for this label
            }
        }
        const int y0 = i0 / W;
        const long next_row = (long)(y0 + 1) * W - i0;          // first lane of the chunk on row y0 + 1 (>= 1)
        if (next_row + W > 63) {                                 // the chunk meets rows y0 and y0 + 1 only
            const unsigned long long upper = next_row >= 64 ? 0ull : ~0ull << next_row;
            unsigned long long rem = __ballot(lbl > 0);
            while (rem) {                                        // one turn per distinct label of the chunk
                const int l = __shfl(lbl, __builtin_ctzll(rem), 64);
                const unsigned long long mk = __ballot(lbl == l);
                rem &= ~mk;
                const int cnt = __popcll(mk);
                const long long sy = (long long)y0 * cnt + __popcll(mk & upper);
                const long long sx = (long long)i0 * cnt + cc_lane_sum(mk) - (long long)W * sy;
                if (l != pend_lbl) {
                    if (pend_lbl && lane == 0) cc_stat_add(area, sum_y, sum_x, stat0 + pend_lbl - 1, pend_area, pend_y, pend_x);
                    pend_lbl = l;
                    pend_area = 0;
                    pend_y = pend_x = 0;
                }
                pend_area += cnt;
                pend_y += sy;
                pend_x += sx;
            }
            continue;
        }
        // images narrower than 64 pixels: one add per run of equal labels on one row
        if (pend_lbl) {
            if (lane == 0) cc_stat_add(area, sum_y, sum_x, stat0 + pend_lbl - 1, pend_area, pend_y, pend_x);
            pend_lbl = 0;
        }
        const int y = i / W, x = i - y * W;
        const int prev = __shfl_up(lbl, 1, 64);
        const bool bound = lane == 0 || prev != lbl || x == 0 || i >= HW;
        const unsigned long long bm = __ballot(bound);
        if (bound && lbl > 0) {
            const unsigned long long rest = lane < 63 ? bm >> (lane + 1) : 0ull;
            const long long len = rest ? __builtin_ctzll(rest) + 1 : 64 - lane;
            cc_stat_add(area, sum_y, sum_x, stat0 + lbl - 1, (int)len, len * y, len * x + len * (len - 1) / 2);
        }
    }
    if (pend_lbl && lane == 0) cc_stat_add(area, sum_y, sum_x, stat0 + pend_lbl - 1, pend_area, pend_y, pend_x);
    if (CLS && over) cc_report(err, UMI_CC_FAULT_CAP);
    if (fault) *err = fault;
}

struct CcPlan {
    long nhw;
    int hw, nblk;
    size_t off_parent, off_blk, total;
};
// 0 on success
int cc_plan(int N, int H, int W, CcPlan* pl) {
    if (N <= 0 || H <= 0 || W <= 0) return UMI_ERR_BADARG;
    const long nhw = (long)N * H * W;
    if ((long)H * W >= (1L << 31) || nhw >= (1L << 31) || N > 65535) return UMI_ERR_UNSUPPORTED;
    pl->nhw = nhw;
    pl->hw = H * W;
    pl->nblk = (pl->hw + CC_BLK - 1) / CC_BLK;
    pl->off_parent = CC_HEAD;
    pl->off_blk = pl->off_parent + (((size_t)nhw * sizeof(int) + 255) & ~(size_t)255);
    pl->total = pl->off_blk + (((size_t)N * pl->nblk * sizeof(int) + 255) & ~(size_t)255);
    return UMI_OK;
}

// passes 1 and 2
void cc_build(const unsigned char* mask, int* parent, int* err, int N, int H, int W, hipStream_t s) {
    const dim3 tiles((W + CC_T - 1) / CC_T, (H + CC_T - 1) / CC_T, N);
    hipLaunchKernelGGL(cc_tile_kernel, tiles, dim3(256), 0, s, mask, parent, H, W, err);
    const int nhs = (H - 1) / CC_T, nvs = (W - 1) / CC_T;
    const long seam = ((long)nhs * W + (long)nvs * H) * N;
    if (seam > 0)
        hipLaunchKernelGGL(cc_seam_kernel<false>, dim3((unsigned)((seam + 255) / 256)), dim3(256), 0, s, (const unsigned char*)nullptr,
                           0, parent, N, H, W, nhs, nvs, err);
}

// passes 1 and 2 for class values 0 .. K - 1
void cc_class_build(const unsigned char* mask, int* parent, int* err, int N, int H, int W, int K, hipStream_t s) {
    const dim3 tiles((W + CC_T - 1) / CC_T, (H + CC_T - 1) / CC_T, N);
    hipLaunchKernelGGL(cc_class_tile_kernel, tiles, dim3(256), 0, s, mask, parent, H, W, K, err);
    const int nhs = (H - 1) / CC_T, nvs = (W - 1) / CC_T;
    const long seam = ((long)nhs * W + (long)nvs * H) * N;
    if (seam > 0)
        hipLaunchKernelGGL(cc_seam_kernel<true>, dim3((unsigned)((seam + 255) / 256)), dim3(256), 0, s, mask, K, parent, N, H, W, nhs,
                           nvs, err);
}

}  // namespace

extern "C" size_t umi_components_ws_bytes(int N, int H, int W) {
    CcPlan pl;
    return cc_plan(N, H, W, &pl) == UMI_OK ? pl.total : 0;
}

extern "C" int umi_components_cap(int H, int W) {
    if (H <= 0 || W <= 0) return UMI_ERR_BADARG;
    const long cap = (long)((H + 1) / 2) * ((W + 1) / 2);
    return cap >= (1L << 31) ? UMI_ERR_UNSUPPORTED : (int)cap;
}

extern "C" int umi_count_components(const unsigned char* mask, int* counts, int N, int H, int W, void* ws, size_t ws_bytes,
                                    umi_stream_t stream) {
    if (!mask || !counts || N <= 0 || H <= 0 || W <= 0) return UMI_ERR_BADARG;
    CcPlan pl;
    const int st = cc_plan(N, H, W, &pl);
    if (st != UMI_OK) return st;
    if (!ws || ws_bytes < pl.total) return UMI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int* err = (int*)ws;
    int* parent = (int*)((char*)ws + pl.off_parent);
    int* blk = (int*)((char*)ws + pl.off_blk);
    hipError_t e = hipMemsetAsync(err, 0, CC_HEAD, s);
    if (e != hipSuccess) return (int)e;
    cc_build(mask, parent, err, N, H, W, s);
    hipLaunchKernelGGL((cc_flatten_kernel<false>), dim3(pl.nblk, N), dim3(256), 0, s, parent, (int*)nullptr, pl.hw, pl.nblk, blk, err);
    hipLaunchKernelGGL(cc_scan_kernel, dim3(N), dim3(256), 0, s, blk, pl.nblk, counts);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_label_components(const unsigned char* mask, int* labels, int* counts, int* area, long long* sum_y,
                                    long long* sum_x, int N, int H, int W, void* ws, size_t ws_bytes, umi_stream_t stream) {
    if (!mask || !labels || !counts || !area || !sum_y || !sum_x || N <= 0 || H <= 0 || W <= 0) return UMI_ERR_BADARG;
    CcPlan pl;
    const int st = cc_plan(N, H, W, &pl);
    if (st != UMI_OK) return st;
    if (!ws || ws_bytes < pl.total) return UMI_ERR_WORKSPACE;
    const int cap = umi_components_cap(H, W);
    if (cap < 0) return cap;
    hipStream_t s = (hipStream_t)stream;
    int* err = (int*)ws;
    int* parent = (int*)((char*)ws + pl.off_parent);
    int* blk = (int*)((char*)ws + pl.off_blk);
    hipError_t e = hipMemsetAsync(err, 0, CC_HEAD, s);
    if (e == hipSuccess) e = hipMemsetAsync(area, 0, (size_t)N * cap * sizeof(int), s);
    if (e == hipSuccess) e = hipMemsetAsync(sum_y, 0, (size_t)N * cap * sizeof(long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(sum_x, 0, (size_t)N * cap * sizeof(long long), s);
    if (e != hipSuccess) return (int)e;
    cc_build(mask, parent, err, N, H, W, s);
    hipLaunchKernelGGL((cc_flatten_kernel<true>), dim3(pl.nblk, N), dim3(256), 0, s, parent, labels, pl.hw, pl.nblk, blk, err);
    hipLaunchKernelGGL(cc_scan_kernel, dim3(N), dim3(256), 0, s, blk, pl.nblk, counts);
    hipLaunchKernelGGL(cc_rank_kernel<false>, dim3(pl.nblk, N), dim3(256), 0, s, labels, parent, pl.hw, pl.nblk, blk,
                       (const unsigned char*)nullptr, 0, 0, (unsigned char*)nullptr, (int*)nullptr);
    const int per_wg = 4 * CC_CHUNKS * 64;
    hipLaunchKernelGGL(cc_relabel_kernel<false>, dim3((pl.hw + per_wg - 1) / per_wg, N), dim3(256), 0, s, labels, parent, pl.hw, W, cap,
                       area, sum_y, sum_x, err);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" size_t umi_class_components_ws_bytes(int N, int H, int W, int n_classes) {
    CcPlan pl;
    if (n_classes < 2 || n_classes > CC_MAX_CLASSES) return 0;
    return cc_plan(N, H, W, &pl) == UMI_OK ? pl.total : 0;
}

extern "C" int umi_count_class_components(const unsigned char* mask, int* class_counts, int N, int H, int W, int n_classes, void* ws,
                                          size_t ws_bytes, umi_stream_t stream) {
    if (!mask || !class_counts || N <= 0 || H <= 0 || W <= 0 || n_classes < 2) return UMI_ERR_BADARG;
    if (n_classes > CC_MAX_CLASSES) return UMI_ERR_UNSUPPORTED;
    CcPlan pl;
    const int st = cc_plan(N, H, W, &pl);
    if (st != UMI_OK) return st;
    if (!ws || ws_bytes < pl.total) return UMI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int* err = (int*)ws;
    int* parent = (int*)((char*)ws + pl.off_parent);
    hipError_t e = hipMemsetAsync(err, 0, CC_HEAD, s);
    if (e == hipSuccess) e = hipMemsetAsync(class_counts, 0, (size_t)N * n_classes * sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    cc_class_build(mask, parent, err, N, H, W, n_classes, s);
    hipLaunchKernelGGL(cc_class_count_kernel, dim3(pl.nblk, N), dim3(256), 0, s, parent, mask, pl.hw, n_classes, class_counts);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}

extern "C" int umi_label_class_components(const unsigned char* mask, int* labels, int* counts, int* class_counts,
                                          unsigned char* label_class, int* area, long long* sum_y, long long* sum_x, int N, int H, int W,
                                          int n_classes, int cap, void* ws, size_t ws_bytes, umi_stream_t stream) {
    if (!mask || !labels || !counts || !class_counts || !label_class || !area || !sum_y || !sum_x || N <= 0 || H <= 0 || W <= 0 ||
        n_classes < 2 || cap <= 0)
        return UMI_ERR_BADARG;
    if (n_classes > CC_MAX_CLASSES) return UMI_ERR_UNSUPPORTED;
    CcPlan pl;
    const int st = cc_plan(N, H, W, &pl);
    if (st != UMI_OK) return st;
    if (cap > pl.hw) return UMI_ERR_BADARG;
    if (!ws || ws_bytes < pl.total) return UMI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int* err = (int*)ws;
    int* parent = (int*)((char*)ws + pl.off_parent);
    int* blk = (int*)((char*)ws + pl.off_blk);
    hipError_t e = hipMemsetAsync(err, 0, CC_HEAD, s);
    if (e == hipSuccess) e = hipMemsetAsync(class_counts, 0, (size_t)N * n_classes * sizeof(int), s);
    if (e == hipSuccess) e = hipMemsetAsync(label_class, 0, (size_t)N * cap, s);
    if (e == hipSuccess) e = hipMemsetAsync(area, 0, (size_t)N * cap * sizeof(int), s);
    if (e == hipSuccess) e = hipMemsetAsync(sum_y, 0, (size_t)N * cap * sizeof(long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(sum_x, 0, (size_t)N * cap * sizeof(long long), s);
    if (e != hipSuccess) return (int)e;
    cc_class_build(mask, parent, err, N, H, W, n_classes, s);
    hipLaunchKernelGGL((cc_flatten_kernel<true>), dim3(pl.nblk, N), dim3(256), 0, s, parent, labels, pl.hw, pl.nblk, blk, err);
    hipLaunchKernelGGL(cc_scan_kernel, dim3(N), dim3(256), 0, s, blk, pl.nblk, counts);
    hipLaunchKernelGGL(cc_rank_kernel<true>, dim3(pl.nblk, N), dim3(256), 0, s, labels, parent, pl.hw, pl.nblk, blk, mask, n_classes, cap,
                       label_class, class_counts);
    const int per_wg = 4 * CC_CHUNKS * 64;
    hipLaunchKernelGGL(cc_relabel_kernel<true>, dim3((pl.hw + per_wg - 1) / per_wg, N), dim3(256), 0, s, labels, parent, pl.hw, W, cap,
                       area, sum_y, sum_x, err);
    UMI_LAUNCH_CHECK();
    return UMI_OK;
}
