// Largest error of the device expf and logf against float64, in units in the last place of the float64 value rounded to fp32, over
// the ranges the 'prob' mode of csrc/tta.hip and its tests use: expf on [-60, 20] (softmax arguments v - max <= 0, sigmoid's -v),
// logf on (0, 1] (mean probabilities).  A stand-alone program, built with the library's flags by tools/bench_tta.py:
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/tta_math_ulp.hip -o tta_math_ulp && ./tta_math_ulp
// prints one JSON line.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>

__global__ void eval_kernel(const float* __restrict__ xe, const float* __restrict__ xl, float* __restrict__ e, float* __restrict__ l, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    e[i] = expf(xe[i]);
    l[i] = logf(xl[i]);
}

static double ulps(float got, double want) {
    if (want == 0.0) return got == 0.f ? 0.0 : INFINITY;
    int ex;
    frexp(want, &ex);                                        // |want| in [2^(ex-1), 2^ex)
    double ulp = ldexp(1.0, ex - 24);
    if (fabs(want) < FLT_MIN) ulp = ldexp(1.0, -149);
    return fabs((double)got - want) / ulp;
}

#define CHECK(call)                                                                   \
    do {                                                                              \
        hipError_t e__ = (call);                                                      \
        if (e__ != hipSuccess) {                                                      \
            fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e__));               \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

int main() {
    const int n = 1 << 24;
    std::vector<float> xe(n), xl(n), e(n), l(n);
    unsigned long long s = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const double u = (double)(s >> 11) / 9007199254740992.0;                 // [0, 1)
        xe[i] = (float)(-60.0 + 80.0 * u);
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const double w = (double)(s >> 11) / 9007199254740992.0;
        // a third uniform in (0, 1], a third log-uniform down to 2^-60, a third within 2^-10 of 1
        xl[i] = i % 3 == 0 ? (float)(1.0 - w) : i % 3 == 1 ? (float)exp2(-60.0 * w) : (float)(1.0 - w / 1024.0);
        if (!(xl[i] > 0.f)) xl[i] = 1.f;
    }
    float *dxe, *dxl, *de, *dl;
    const size_t bytes = (size_t)n * sizeof(float);
    CHECK(hipMalloc(&dxe, bytes));
    CHECK(hipMalloc(&dxl, bytes));
    CHECK(hipMalloc(&de, bytes));
    CHECK(hipMalloc(&dl, bytes));
    CHECK(hipMemcpy(dxe, xe.data(), bytes, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dxl, xl.data(), bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(eval_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dxe, dxl, de, dl, n);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(e.data(), de, bytes, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(l.data(), dl, bytes, hipMemcpyDeviceToHost));
    double we = 0, wl = 0;
    for (int i = 0; i < n; ++i) {
        we = fmax(we, ulps(e[i], exp((double)xe[i])));
        wl = fmax(wl, ulps(l[i], log((double)xl[i])));
    }
    printf("{\"samples\": %d, \"expf_range\": [-60, 20], \"expf_max_ulp\": %.4f, \"logf_range\": \"(0, 1]\", \"logf_max_ulp\": %.4f}\n",
           n, we, wl);
    for (float* p : {dxe, dxl, de, dl}) (void)hipFree(p);
    return 0;
}
