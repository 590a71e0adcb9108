// Fixed-order sums over a workgroup and the owner of a sample of a ragged batch, shared by the noise kernels (f2_noise.hip) and the
// masker kernels (f2_masker.hip): the same tree, so the same bits, in both. gfx950, wave64.
#ifndef F2_BLOCK_SUM_H
#define F2_BLOCK_SUM_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

template <typename T>
__device__ inline T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;   // lane 0 holds the sum; the tree is the same on every call
}

// sum over the workgroup, valid in thread 0: lanes by shuffles, waves through LDS in wave order
template <typename T, int THREADS>
__device__ inline T block_sum(T v, T* lds) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T total = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < THREADS / 64; ++w) total += lds[w];
    return total;
}

// utterance of sample p of the batch: the last b with offsets[b] <= p (empty utterances are stepped over)
__device__ inline int utterance_of(const int64_t* __restrict__ offsets, int B, int64_t p) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace

#endif
