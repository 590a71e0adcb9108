// The tail of the one-workgroup-per-window gathers (k_gather_windows of f2_gather.hip, k_gather_windows_mixed of
// f2_gather_mix.hip): the window's values lie in LDS, every thread holds the minimum and maximum of the values it put there, and
// what follows - the reduction, the flag rule and the (ln v - ln min) / range epilogue - is this one function, so that the two
// kernels cannot drift apart. GT threads, all of which call it; `win` holds `total` values with c fastest, the layout of the output.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

template <int GT>
__device__ __forceinline__ void gather_window_tail(const double* win, int total, double mn, double mx, int normalize, float* __restrict__ o,
                                                   int* __restrict__ flag, double* red_min, double* red_max) {
    const int tid = threadIdx.x;
    if (!normalize) {
        __syncthreads();
        for (int idx = tid; idx < total; idx += GT) o[idx] = (float)win[idx];
        return;
    }
    for (int d = 32; d > 0; d >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, d));
        mx = fmax(mx, __shfl_xor(mx, d));
    }
    if ((tid & 63) == 0) {
        red_min[tid >> 6] = mn;
        red_max[tid >> 6] = mx;
    }
    __syncthreads();
    mn = red_min[0];
    mx = red_max[0];
    for (int w = 1; w < GT / 64; ++w) {
        mn = fmin(mn, red_min[w]);
        mx = fmax(mx, red_max[w]);
    }
    if (!(mn > 0.0)) {   // also catches NaN
        if (tid == 0) atomicOr(flag, 1);
        for (int idx = tid; idx < total; idx += GT) o[idx] = 0.f;
        return;
    }
    if (mn == mx) {
        for (int idx = tid; idx < total; idx += GT) o[idx] = 0.f;
        return;
    }
    const double lmn = log(mn);
    const double range = log(mx) - lmn;
    for (int idx = tid; idx < total; idx += GT) o[idx] = (float)((log(win[idx]) - lmn) / range);
}
