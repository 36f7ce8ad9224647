// SciPy's order-0 zoom along one axis (scipy.ndimage.zoom(order=0), mode 'constant'): the rule of umi_zoom_nearest, shared with
// the label gather of the training-batch transform (augment.hip), which composes it with its geometry.
#pragma once
#include <hip/hip_runtime.h>

// source index of output i, or -1 where SciPy's mode 'constant' gives 0: sample coordinate x = i * ((in - 1) / (out - 1)) in
// float64 (0 for out == 1), index floor(x + 0.5)
__device__ inline int zn_src(int i, int n_in, int n_out) {
#pragma clang fp contract(off)
    const double x = (double)i * (n_out > 1 ? (double)(n_in - 1) / (double)(n_out - 1) : 0.0);
    if (x < 0.0 || x > (double)(n_in - 1)) return -1;
    const int s = (int)floor(x + 0.5);
    return s > n_in - 1 ? n_in - 1 : s;
}
