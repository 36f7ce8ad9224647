// Union-find pieces of the connected-component labelling (components.hip): pure integer code, no HIP types, so the same
// text compiles as plain C++ (a sequential rehearsal of the passes on the host) and as device code.
//
// Representation: parent[p] is a flat pixel index <= p (background: -1); the representative of a set is its MINIMUM
// index, parent[root] == root.  Links only ever lower a root's parent, so every chain is strictly decreasing and a
// valid chain is shorter than the pixel count; `cap` bounds every loop all the same, and a violated invariant
// (parent > index, parent < 0, cap reached) is reported through `*fault` instead of being followed.
//
// `M` says how a word of `parent` is read and linked:
//   M::load(const int*)            the value of the word
//   M::fetch_min(int*, int)        atomically word = min(word, v), returns the old value
// Where several workgroups link concurrently both must be agent-scope atomics (components.hip: CcAgent).
#pragma once

#if defined(__HIPCC__)
#define UMI_CC_HD __host__ __device__ __forceinline__
#else
#define UMI_CC_HD inline
#endif

// UMI_CC_FAULT_CLASS: a mask value >= n_classes was met (taken as background); UMI_CC_FAULT_CAP: an image has more components
// than the caller's statistics rows hold (counts and the label map stay exact, the rows hold the first `cap` labels).
enum { UMI_CC_OK = 0, UMI_CC_FAULT_FIND_CAP = 1, UMI_CC_FAULT_UNION_CAP = 2, UMI_CC_FAULT_CHAIN = 3, UMI_CC_FAULT_RANK = 4,
       UMI_CC_FAULT_CLASS = 5, UMI_CC_FAULT_CAP = 6 };

template <class M>
UMI_CC_HD int umi_cc_find(const int* parent, int a, int cap, int* fault) {
    for (int it = 0; it <= cap; ++it) {
        const int p = M::load(parent + a);
        if (p == a) return a;
        if (p < 0 || p > a) {
            *fault = UMI_CC_FAULT_CHAIN;
            return -1;
        }
        a = p;
    }
    *fault = UMI_CC_FAULT_FIND_CAP;
    return -1;
}

// Lock-free union by minimum index.  A failed fetch_min (another linker got to root b first) leaves parent[b] =
// min(old, a): the set that `old` heads still has to meet a's, so the loop goes on with (a, old).
template <class M>
UMI_CC_HD void umi_cc_union(int* parent, int a, int b, int cap, int* fault) {
    for (int it = 0; it <= cap; ++it) {
        a = umi_cc_find<M>(parent, a, cap, fault);
        if (a < 0) return;
        b = umi_cc_find<M>(parent, b, cap, fault);
        if (b < 0) return;
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = M::fetch_min(parent + b, a);
        if (old == b) return;
        b = old;
    }
    *fault = UMI_CC_FAULT_UNION_CAP;
}

// Column at which the run of set bits containing bit x of row mask m begins (bit x must be set).
UMI_CC_HD int umi_cc_run_start(unsigned long long m, int x) {
    const unsigned long long below = ~m & ((1ull << x) - 1ull);
    return below ? 64 - __builtin_clzll(below) : 0;
}

// Which of the three 8-neighbours in the row above a foreground pixel (column x of row mask m; `a` = the row above)
// need a union once every row run already is one set: bit 0 = straight up, bit 1 = up-left, bit 2 = up-right.
//   up set:    up-left / up-right lie in up's run.  With left and up-left both set the pair (left, up-left) is vertically
//              adjacent and left belongs to this pixel's run, so left's own link (or, by induction towards the run's first
//              pixel, an earlier one) already joins the two runs.
//   up clear:  up-left and up-right are different runs of the row above; left set makes (left, up-left) a vertical pair
//              that left links itself.
UMI_CC_HD int umi_cc_links_above(unsigned long long m, unsigned long long a, int x) {
    const bool up = (a >> x) & 1ull;
    const bool ul = x > 0 && ((a >> (x - 1)) & 1ull);
    const bool ur = x < 63 && ((a >> (x + 1)) & 1ull);
    const bool left = x > 0 && ((m >> (x - 1)) & 1ull);
    if (up) return (ul && left) ? 0 : 1;
    return ((ul && !left) ? 2 : 0) | (ur ? 4 : 0);
}

// Seam form of the same choice for a pixel on a tile's last row (or column) and its three neighbours across the seam,
// `mid` the one straight across, `lo` / `hi` the two diagonal ones: bit 0 = mid, bit 1 = lo, bit 2 = hi.  With mid set,
// lo and hi are 4-adjacent to mid on the far side: inside mid's tile the tile pass joined them, across a tile corner the
// other seam direction's own straight link does.
UMI_CC_HD int umi_cc_links_across(bool lo, bool mid, bool hi) {
    if (mid) return 1;
    return (lo ? 2 : 0) | (hi ? 4 : 0);
}
