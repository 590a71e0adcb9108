// Input range of f2_cnn_forward (K4): one bandwidth-bound pass over the window tensor that finds max |x| over its finite values,
// the max |x| of its quietest window and whether it holds inf / NaN, so that the host can pick the split path's scale set for the
// inputs it was given (f2_pipeline.hip; the scales: f2_cnn.hip, f2_cnn_split.h).
#include "f2_internal.h"

namespace {

constexpr int RANGE_THREADS = 256;
constexpr int RANGE_BLOCKS_PER_CU = 8;

// max |x| as the bit pattern of a non-negative float (orders like the value), non-finite values flagged apart
__device__ __forceinline__ void range_take(float v, unsigned& m, unsigned& bad) {
    const unsigned u = __float_as_uint(v) & 0x7fffffffu;
    if (u >= 0x7f800000u) bad = 1u;
    else m = u > m ? u : m;
}

__device__ __forceinline__ void range_take4(const float4 v, unsigned& m, unsigned& bad) {
    range_take(v.x, m, bad);
    range_take(v.y, m, bad);
    range_take(v.z, m, bad);
    range_take(v.w, m, bad);
}

// One wave per window (grid-stride over windows), 16-byte vectors where the windows allow, four in flight per lane. Per window
// the wave's max |x| over finite values; over the windows of a workgroup their maximum and their minimum (the quietest window),
// then ONE atomicMax per workgroup for each: words[0] = bit pattern of max |x|, words[2] = its complement of the quietest window's
// max |x| (so that the zeroed word works as the start of a maximum); words[1] = 1 if a value was inf / NaN.
__global__ __launch_bounds__(RANGE_THREADS) void k_cnn_input_range(const float* __restrict__ x, int64_t nwin, int S, int vec,
                                                                    unsigned* __restrict__ words) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nwaves = (int64_t)gridDim.x * (RANGE_THREADS / 64);
    unsigned gmax = 0u, quiet_c = 0u, bad = 0u;
    for (int64_t w = (int64_t)blockIdx.x * (RANGE_THREADS / 64) + wave; w < nwin; w += nwaves) {
        const float* p = x + w * S;
        unsigned m = 0u;
        if (vec) {
            const float4* p4 = reinterpret_cast<const float4*>(p);
            const int n4 = S >> 2;
            for (int i0 = 0; i0 < n4; i0 += 256) {
                float4 v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int idx = i0 + 64 * k + lane;
                    v[k] = idx < n4 ? p4[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) range_take4(v[k], m, bad);
            }
        } else {
            for (int i = lane; i < S; i += 64) range_take(p[i], m, bad);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned mo = __shfl_xor(m, o);
            m = mo > m ? mo : m;
        }
        gmax = m > gmax ? m : gmax;
        quiet_c = ~m > quiet_c ? ~m : quiet_c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o);
    __shared__ unsigned wm[RANGE_THREADS / 64], wq[RANGE_THREADS / 64], wb[RANGE_THREADS / 64];
    if (lane == 0) {
        wm[wave] = gmax;
        wq[wave] = quiet_c;
        wb[wave] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < RANGE_THREADS / 64; ++k) {
            gmax = wm[k] > gmax ? wm[k] : gmax;
            quiet_c = wq[k] > quiet_c ? wq[k] : quiet_c;
            bad |= wb[k];
        }
        atomicMax(&words[0], gmax);
        atomicMax(&words[2], quiet_c);
        if (bad) words[1] = 1u;
    }
}

}  // namespace

int f2_launch_cnn_input_range(f2_ctx* ctx, const float* d_x, int64_t nwin, int S, unsigned* d_words) {
    if (nwin <= 0 || S <= 0) return F2_OK;
    const int vec = ((uintptr_t)d_x & 15) == 0 && S % 4 == 0;
    const int64_t want = (nwin + RANGE_THREADS / 64 - 1) / (RANGE_THREADS / 64);
    const int64_t cap = (int64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * RANGE_BLOCKS_PER_CU;
    const unsigned blocks = (unsigned)(want < cap ? want : cap);
    hipLaunchKernelGGL(k_cnn_input_range, dim3(blocks), dim3(RANGE_THREADS), 0, ctx->stream, d_x, nwin, S, vec, d_words);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}
