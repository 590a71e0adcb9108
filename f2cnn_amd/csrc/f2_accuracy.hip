// Kernel of f2_label_accuracy (include/f2cnn_hip.h): the labels of a strided evaluation held against the VTR-derived labels.
//   k_label_accuracy  per utterance: rows whose timepoint lies within a step of a reference timepoint, by reference sign and label
// gfx950, wave64. Everything that reaches memory is written by vector integer atomics on a buffer the caller zeroed.
#include "f2_internal.h"

namespace {

constexpr int ACC_THREADS = 256;

__device__ inline unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;   // lane 0 holds the sum
}

// Workgroups (u, blockIdx.y) share the rows of utterance u, which is scored against reference set r = u % R: timepoints
// T[0..n) strictly increasing, signs s[0..n). Row j stands for sample t = origin + j * hop. With k the last label before t
// (binary search: the set stays in global memory, so any size works, and the ~log2 n reads per row of a set of a few hundred
// labels come from the cache), the row is counted when T[k] < t < T[k+1] and one of the two is less than `step` away; the
// nearer one gives the reference sign, the earlier one on a tie (Evaluating.py:96-107). The distances are formed in uint64:
// exact for any int64 timepoints with T[k] < t < T[k+1].
// counts[4u + 2 ref + pred] += rows: lanes by shuffles, waves through LDS, then one 64-bit integer atomic per counter that is
// not zero. Integer sums do not depend on the order: the same bits on every call.
__global__ __launch_bounds__(ACC_THREADS) void k_label_accuracy(const uint8_t* __restrict__ labels, const int64_t* __restrict__ wo,
                                                                 const int64_t* __restrict__ ref_off,
                                                                 const int64_t* __restrict__ ref_t, const uint8_t* __restrict__ ref_s,
                                                                 int R, int64_t origin, int hop, int step,
                                                                 unsigned long long* __restrict__ counts) {
    __shared__ unsigned lds[ACC_THREADS / 64][4];
    const int u = blockIdx.x, r = u % R;
    const int64_t first = wo[u], rows = wo[u + 1] - first;
    const int64_t n = ref_off[r + 1] - ref_off[r];
    const int64_t* T = ref_t + ref_off[r];
    const uint8_t* s = ref_s + ref_off[r];
    unsigned c[4] = {0, 0, 0, 0};
    if (n >= 2) {
        const int64_t t_first = T[0], t_last = T[n - 1];
        for (int64_t j = (int64_t)blockIdx.y * ACC_THREADS + threadIdx.x; j < rows; j += (int64_t)gridDim.y * ACC_THREADS) {
            const int64_t t = origin + j * (int64_t)hop;
            if (t <= t_first || t >= t_last) continue;
            int64_t lo = 0, hi = n - 1;   // T[lo] < t <= T[hi]
            while (hi - lo > 1) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (T[mid] < t) lo = mid; else hi = mid;
            }
            const int64_t after = T[hi];
            if (after == t) continue;     // on a timepoint
            const uint64_t da = (uint64_t)t - (uint64_t)T[lo], db = (uint64_t)after - (uint64_t)t;
            if (da >= (uint64_t)step && db >= (uint64_t)step) continue;
            const unsigned ref = da <= db ? s[lo] : s[hi];
            const unsigned cell = 2 * ref + (labels[first + j] != 0);
#pragma unroll
            for (unsigned i = 0; i < 4; ++i) c[i] += cell == i;   // (no indexed register array)
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned w = wave_sum(c[i]);
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6][i] = w;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long total = 0;
        for (int w = 0; w < ACC_THREADS / 64; ++w) total += lds[w][threadIdx.x];
        if (total) atomicAdd(&counts[4 * (size_t)u + threadIdx.x], total);
    }
}

}  // namespace

int f2_launch_label_accuracy(f2_ctx* ctx, const uint8_t* d_labels, const int64_t* d_window_offsets, int U, const int64_t* d_ref_offsets,
                             const int64_t* d_ref_timepoints, const uint8_t* d_ref_signs, int R, int64_t origin, int hop, int step,
                             int64_t max_rows, int64_t* d_counts) {
    if (U == 0 || max_rows == 0) return F2_OK;
    const int64_t per = (max_rows + ACC_THREADS - 1) / ACC_THREADS;
    const dim3 grid((unsigned)U, (unsigned)(per < 64 ? per : 64));
    k_label_accuracy<<<grid, dim3(ACC_THREADS), 0, ctx->stream>>>(d_labels, d_window_offsets, d_ref_offsets, d_ref_timepoints,
                                                                  d_ref_signs, R, origin, hop, step, (unsigned long long*)d_counts);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}
