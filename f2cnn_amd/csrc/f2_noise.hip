// Kernels of f2_eval_noise_sweep and f2_noise_pick (include/f2cnn_hip.h): the noise levels of a ragged batch and the tally of its labels.
//   k_noise_sigma  sum of squares of every clean utterance (one workgroup per row, fixed order) -> sigma per (level, utterance)
//   k_noise_levels the (K+1) x batch float64 waveform: clean + sigma * z, z from Philox4x32-10 per sample; level K is the clean one
//   k_noise_pick_sigma, k_noise_pick  the same two for a batch in which every utterance has one level of its own
//   k_label_tally  per (level, utterance): windows labelled rising, windows whose label is the clean level's
// gfx950, wave64. Everything that reaches memory is written by plain C++ stores or vector integer atomics.
#include "f2_internal.h"
#include "f2_block_sum.h"
#include "f2_philox.h"

#include <type_traits>

namespace {

constexpr int SIGMA_THREADS = 1024, NOISE_THREADS = 256, TALLY_THREADS = 256;

// (wave_sum, block_sum and utterance_of live in f2_block_sum.h: the masker kernels of f2_masker.hip sum with the same tree)

// RMS of row b of the clean batch, valid in thread 0. int16: the squares are summed in int64 (exact, so the order does not matter),
// then sqrt((double)sum / n). float64: thread t adds samples t, t + THREADS, ... in that order, then the fixed tree of block_sum.
template <typename T>
__device__ inline double row_rms(const T* __restrict__ wave, const int64_t* __restrict__ offsets, int b) {
    using acc_t = typename std::conditional<std::is_same<T, int16_t>::value, long long, double>::type;
    __shared__ acc_t lds[SIGMA_THREADS / 64];
    const int64_t n = offsets[b + 1] - offsets[b];
    const T* x = wave + offsets[b];
    acc_t acc = 0;
    for (int64_t i = threadIdx.x; i < n; i += SIGMA_THREADS) {
        const acc_t v = (acc_t)x[i];
        acc += v * v;
    }
    const acc_t total = block_sum<acc_t, SIGMA_THREADS>(acc, lds);
    return n > 0 ? sqrt((double)total / (double)n) : 0.0;
}
// sigma of an utterance of that RMS at the level whose 10^(snr_db / 10) is lin; an empty utterance has none
__device__ inline double sigma_of(double rms, double lin, bool empty) { return empty ? 0.0 : rms / lin; }

// sigma[l * B + b] = rms / lin[l] for l < K (lin[l] = 10^(snr_db[l] / 10), from the host) and 0 for the clean level l = K.
template <typename T>
__global__ __launch_bounds__(SIGMA_THREADS) void k_noise_sigma(const T* __restrict__ wave, const int64_t* __restrict__ offsets,
                                                                const double* __restrict__ lin, int B, int K,
                                                                double* __restrict__ sigma) {
    const int b = blockIdx.x;
    const double rms = row_rms(wave, offsets, b);
    if (threadIdx.x != 0) return;
    const bool empty = offsets[b + 1] == offsets[b];
    for (int l = 0; l < K; ++l) sigma[(size_t)l * B + b] = sigma_of(rms, lin[l], empty);
    sigma[(size_t)K * B + b] = 0.0;
}

// The same for a batch whose utterance b runs at level level[b] alone: sigma[b], 0 for the clean level K
template <typename T>
__global__ __launch_bounds__(SIGMA_THREADS) void k_noise_pick_sigma(const T* __restrict__ wave, const int64_t* __restrict__ offsets,
                                                                     const double* __restrict__ lin, const int32_t* __restrict__ level,
                                                                     int K, double* __restrict__ sigma) {
    const int b = blockIdx.x;
    const int l = level[b];
    if (l >= K) {   // (the whole workgroup: no barrier is skipped by a part of it)
        if (threadIdx.x == 0) sigma[b] = 0.0;
        return;
    }
    const double rms = row_rms(wave, offsets, b);
    if (threadIdx.x == 0) sigma[b] = sigma_of(rms, lin[l], offsets[b + 1] == offsets[b]);
}

// (noise_deviate, the standard normal deviate of (seed, level, utterance, sample), lives in f2_philox.h: k_shaped_noise_levels of
// f2_noise_shaped.hip draws from the same function)

// One thread per sample of one level (blockIdx.y strides over the levels): out[l * total + p] = clean[p] + sigma[l * B + b] * z,
// product and sum rounded separately; where sigma is 0 (the clean level, an all-zero row) the sample itself, exactly.
// Consecutive lanes write consecutive float64 values: 512 bytes per wave and store instruction.
template <typename T>
__global__ __launch_bounds__(NOISE_THREADS) void k_noise_levels(const T* __restrict__ wave, const int64_t* __restrict__ offsets,
                                                                 const double* __restrict__ sigma, int B, int levels, int64_t total,
                                                                 uint64_t seed, double* __restrict__ out) {
#pragma clang fp contract(off)
    for (int64_t p = (int64_t)blockIdx.x * NOISE_THREADS + threadIdx.x; p < total; p += (int64_t)gridDim.x * NOISE_THREADS) {
        const int b = utterance_of(offsets, B, p);
        const uint64_t i = (uint64_t)(p - offsets[b]);
        const double clean = (double)wave[p];
        for (int l = blockIdx.y; l < levels; l += gridDim.y) {
            const double s = sigma[(size_t)l * B + b];
            double v = clean;
            if (s != 0.0) {
                const double nz = s * noise_deviate(seed, (uint32_t)l, (uint32_t)b, i);
                v = clean + nz;
            }
            out[(size_t)l * (size_t)total + (size_t)p] = v;
        }
    }
}

// One thread per sample of a batch whose utterance b runs at level[b] and is utterance first_utt + b of its corpus:
// out[p] = clean[p] + sigma[b] * z(seed, level[b], first_utt + b, i), what k_noise_levels writes for that level of that utterance.
// sigma == NULL: every utterance is clean (the conversion to float64 alone). Consecutive lanes write consecutive float64 values.
template <typename T>
__global__ __launch_bounds__(NOISE_THREADS) void k_noise_pick(const T* __restrict__ wave, const int64_t* __restrict__ offsets,
                                                               const double* __restrict__ sigma, const int32_t* __restrict__ level, int B,
                                                               int64_t total, uint32_t first_utt, uint64_t seed, double* __restrict__ out) {
#pragma clang fp contract(off)
    for (int64_t p = (int64_t)blockIdx.x * NOISE_THREADS + threadIdx.x; p < total; p += (int64_t)gridDim.x * NOISE_THREADS) {
        double v = (double)wave[p];
        if (sigma) {
            const int b = utterance_of(offsets, B, p);
            const double s = sigma[b];
            if (s != 0.0) {
                const double nz = s * noise_deviate(seed, (uint32_t)level[b], first_utt + (uint32_t)b, (uint64_t)(p - offsets[b]));
                v = v + nz;
            }
        }
        out[p] = v;
    }
}

// Workgroups (u, blockIdx.y) share the windows of utterance u = l * B + b; window j is held against window j of the clean level's
// utterance K * B + b (the same count: the levels share their offsets). One pair of 64-bit integer atomics per workgroup that
// counted something, on a zeroed buffer: integer sums do not depend on the order.
__global__ __launch_bounds__(TALLY_THREADS) void k_label_tally(const uint8_t* __restrict__ labels, const int64_t* __restrict__ wo,
                                                               int B, int K, unsigned long long* __restrict__ stats) {
    __shared__ unsigned lds[TALLY_THREADS / 64];
    const int u = blockIdx.x, b = u % B;
    const int64_t first = wo[u], n = wo[u + 1] - first, first_clean = wo[(size_t)K * B + b];
    unsigned rising = 0, agree = 0;
    for (int64_t j = (int64_t)blockIdx.y * TALLY_THREADS + threadIdx.x; j < n; j += (int64_t)gridDim.y * TALLY_THREADS) {
        const uint8_t mine = labels[first + j];
        rising += mine != 0;
        agree += mine == labels[first_clean + j];
    }
    const unsigned r = block_sum<unsigned, TALLY_THREADS>(rising, lds);
    __syncthreads();
    const unsigned a = block_sum<unsigned, TALLY_THREADS>(agree, lds);
    if (threadIdx.x == 0) {
        if (r) atomicAdd(&stats[2 * (size_t)u], (unsigned long long)r);
        if (a) atomicAdd(&stats[2 * (size_t)u + 1], (unsigned long long)a);
    }
}

}  // namespace

int f2_launch_noise_sigma(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const double* d_lin, int B,
                          int K, double* d_sigma) {
    if (B == 0) return F2_OK;
    if (wave_dtype == F2_WAVE_I16)
        k_noise_sigma<int16_t><<<dim3(B), dim3(SIGMA_THREADS), 0, ctx->stream>>>((const int16_t*)d_wave, d_offsets, d_lin, B, K, d_sigma);
    else
        k_noise_sigma<double><<<dim3(B), dim3(SIGMA_THREADS), 0, ctx->stream>>>((const double*)d_wave, d_offsets, d_lin, B, K, d_sigma);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

int f2_launch_noise_levels(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const double* d_sigma, int B,
                           int K, int64_t total, uint64_t seed, double* d_out) {
    if (B == 0 || total == 0) return F2_OK;
    const int64_t blocks = (total + NOISE_THREADS - 1) / NOISE_THREADS;
    const dim3 grid((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)), (unsigned)(K + 1 < 1024 ? K + 1 : 1024));
    if (wave_dtype == F2_WAVE_I16)
        k_noise_levels<int16_t><<<grid, dim3(NOISE_THREADS), 0, ctx->stream>>>((const int16_t*)d_wave, d_offsets, d_sigma, B, K + 1, total,
                                                                              seed, d_out);
    else
        k_noise_levels<double><<<grid, dim3(NOISE_THREADS), 0, ctx->stream>>>((const double*)d_wave, d_offsets, d_sigma, B, K + 1, total,
                                                                             seed, d_out);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

int f2_launch_noise_pick_sigma(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const double* d_lin,
                               const int32_t* d_level, int B, int K, double* d_sigma) {
    if (B == 0) return F2_OK;
    if (wave_dtype == F2_WAVE_I16)
        k_noise_pick_sigma<int16_t><<<dim3(B), dim3(SIGMA_THREADS), 0, ctx->stream>>>((const int16_t*)d_wave, d_offsets, d_lin, d_level, K, d_sigma);
    else
        k_noise_pick_sigma<double><<<dim3(B), dim3(SIGMA_THREADS), 0, ctx->stream>>>((const double*)d_wave, d_offsets, d_lin, d_level, K, d_sigma);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

int f2_launch_noise_pick(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const double* d_lin,
                         const int32_t* d_level, int B, int K, int64_t total, uint32_t first_utterance, uint64_t seed, double* d_sigma,
                         double* d_out) {
    if (B == 0) return F2_OK;
    const bool i16 = wave_dtype == F2_WAVE_I16;
    if (d_sigma) F2_TRY(f2_launch_noise_pick_sigma(ctx, d_wave, wave_dtype, d_offsets, d_lin, d_level, B, K, d_sigma));
    if (total == 0) return F2_OK;
    const int64_t blocks = (total + NOISE_THREADS - 1) / NOISE_THREADS;
    const dim3 grid((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)));
    if (i16)
        k_noise_pick<int16_t><<<grid, dim3(NOISE_THREADS), 0, ctx->stream>>>((const int16_t*)d_wave, d_offsets, d_sigma, d_level, B, total,
                                                                            first_utterance, seed, d_out);
    else
        k_noise_pick<double><<<grid, dim3(NOISE_THREADS), 0, ctx->stream>>>((const double*)d_wave, d_offsets, d_sigma, d_level, B, total,
                                                                           first_utterance, seed, d_out);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

int f2_launch_label_tally(f2_ctx* ctx, const uint8_t* d_labels, const int64_t* d_window_offsets, int B, int K, int64_t max_windows,
                          int64_t* d_stats) {
    if (B == 0 || max_windows == 0) return F2_OK;
    const int64_t per = (max_windows + TALLY_THREADS - 1) / TALLY_THREADS;
    const dim3 grid((unsigned)((int64_t)(K + 1) * B), (unsigned)(per < 64 ? per : 64));
    k_label_tally<<<grid, dim3(TALLY_THREADS), 0, ctx->stream>>>(d_labels, d_window_offsets, B, K, (unsigned long long*)d_stats);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}
