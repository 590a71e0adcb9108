// Recorded maskers on a ragged batch (include/f2cnn_hip.h: f2_masker_levels, f2_masker_pick; the kernels of f2_eval_masker_sweep and
// of the masker stage of f2_input_batch_masked / f2_trainer_render_masked). A level l < K is a pair (recording masker_of[l],
// snr_db[l]); the masker of utterance number `utt` at that level is a cyclic segment of the recording, scaled to sigma[l].
//   k_masker_gain_levels  one workgroup per (utterance, level): the start of the segment (mk_start, a Philox4x32-10 draw of its own
//                         stream), P = sum of the segment's squares in a fixed order, gain = sigma / sqrt(P / n) (mk_gain)
//   k_masker_levels       the (K+1) x batch float64 waveform: clean + gain * m[(start + i) mod M]; level K is the clean one
//   k_masker_gain_pick, k_masker_pick   the same two for a batch in which every utterance has one level of its own and is number
//                         first_utt + b of its corpus, in the layout of the waves
// The start and the sum are one device function for both gain kernels, the segment and mix arithmetic one (mk_sample) for both mix
// kernels: the same bits. sigma comes from k_noise_sigma / k_noise_pick_sigma (f2_noise.hip), unchanged. No atomics; product and sum
// rounded separately. gfx950, wave64; plain vector stores only.
#include "f2_internal.h"
#include "f2_block_sum.h"
#include "f2_philox.h"

#include <cmath>

namespace {

constexpr int MK_SUM_THREADS = 1024, MK_MIX_THREADS = 256;
constexpr uint32_t MK_STREAM = 0x4D41534Bu;   // second counter word of the draw: no deviate has it (theirs is the high half of a sample index)

// first sample of the segment of recording r (M samples) for utterance number utt: depends on nothing else
__device__ inline int64_t mk_start(uint64_t seed, uint32_t r, uint32_t utt, int64_t M) {
    const philox_words w = philox4x32_10(r, MK_STREAM, 0u, utt, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (int64_t)((((uint64_t)w.w1 << 32) | (uint64_t)w.w0) % (uint64_t)M);
}

// gain of the segment m[(start + i) mod M], i < n, at sigma; valid in thread 0. Thread t adds the squares of i = t, t + THREADS, ...
// in that order (its index reduced once, then stepped by compare and subtract), then the fixed tree of block_sum. 0 where n == 0,
// sigma == 0 or the segment is silent. Every thread of the workgroup calls it (a barrier inside, skipped by all or none).
__device__ inline double mk_gain(const double* __restrict__ m, int64_t M, int64_t start, int64_t n, double sigma, double* lds) {
#pragma clang fp contract(off)
    if (n == 0 || sigma == 0.0) return 0.0;
    int64_t k = (int64_t)(((uint64_t)start + threadIdx.x) % (uint64_t)M);
    const int64_t step = (int64_t)MK_SUM_THREADS % M;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += MK_SUM_THREADS) {
        const double v = m[k];
        const double sq = v * v;
        acc = acc + sq;
        k += step;
        if (k >= M) k -= M;
    }
    const double P = block_sum<double, MK_SUM_THREADS>(acc, lds);
    if (!(P > 0.0)) return 0.0;
    return sigma / sqrt(P / (double)n);
}

// sample i of an utterance at one level: clean + gain * m_r[(start + i) mod M_r], product and sum rounded separately; where gain is
// 0 (the clean level, a silent segment, an all-zero utterance) the clean sample itself, exactly, and nothing of the recording is read.
// i is reduced once (M_r <= 2^26: a 32-bit remainder wherever i fits), start < M_r is added by compare and subtract.
template <typename T>
__device__ inline double mk_sample(T clean, double gain, int64_t start, const double* __restrict__ masker, const int64_t* __restrict__ moff,
                                   int r, uint64_t i) {
#pragma clang fp contract(off)
    const double c = (double)clean;
    if (gain == 0.0) return c;
    const int64_t m0 = moff[r];
    const uint64_t M = (uint64_t)(moff[r + 1] - m0);
    uint64_t k = (i >> 32) == 0 ? (uint64_t)((uint32_t)i % (uint32_t)M) : i % M;
    k += (uint64_t)start;
    if (k >= M) k -= M;
    const double nz = gain * masker[m0 + (int64_t)k];
    return c + nz;
}

// Workgroup (b, l): gain[l * B + b] and start[l * B + b] of utterance b at level l; level K (the clean one) holds 0 in both.
__global__ __launch_bounds__(MK_SUM_THREADS) void k_masker_gain_levels(const int64_t* __restrict__ offsets, const double* __restrict__ sigma,
                                                                      const double* __restrict__ masker, const int64_t* __restrict__ moff,
                                                                      const int32_t* __restrict__ masker_of, int B, int K, uint64_t seed,
                                                                      double* __restrict__ gain, int64_t* __restrict__ start) {
    __shared__ double lds[MK_SUM_THREADS / 64];
    const int b = blockIdx.x, l = blockIdx.y;
    const size_t u = (size_t)l * B + b;
    if (l >= K) {   // (the whole workgroup)
        if (threadIdx.x == 0) gain[u] = 0.0, start[u] = 0;
        return;
    }
    const int r = masker_of[l];
    const int64_t m0 = moff[r], M = moff[r + 1] - m0;
    const int64_t s = mk_start(seed, (uint32_t)r, (uint32_t)b, M);
    const double g = mk_gain(masker + m0, M, s, offsets[b + 1] - offsets[b], sigma[u], lds);
    if (threadIdx.x == 0) gain[u] = g, start[u] = s;
}

// The same for a batch whose utterance b runs at level level[b] alone and is utterance first_utt + b of its corpus: gain[b], start[b]
__global__ __launch_bounds__(MK_SUM_THREADS) void k_masker_gain_pick(const int64_t* __restrict__ offsets, const double* __restrict__ sigma,
                                                                    const int32_t* __restrict__ level, const double* __restrict__ masker,
                                                                    const int64_t* __restrict__ moff, const int32_t* __restrict__ masker_of,
                                                                    int K, uint32_t first_utt, uint64_t seed, double* __restrict__ gain,
                                                                    int64_t* __restrict__ start) {
    __shared__ double lds[MK_SUM_THREADS / 64];
    const int b = blockIdx.x, l = level[b];
    if (l >= K) {   // (the whole workgroup)
        if (threadIdx.x == 0) gain[b] = 0.0, start[b] = 0;
        return;
    }
    const int r = masker_of[l];
    const int64_t m0 = moff[r], M = moff[r + 1] - m0;
    const int64_t s = mk_start(seed, (uint32_t)r, first_utt + (uint32_t)b, M);
    const double g = mk_gain(masker + m0, M, s, offsets[b + 1] - offsets[b], sigma[b], lds);
    if (threadIdx.x == 0) gain[b] = g, start[b] = s;
}

// One thread per sample of one level (blockIdx.y strides over the levels): out[l * total + p] = mk_sample of utterance b at level l.
// Consecutive lanes read consecutive samples of the wave and (up to the wrap) of the recording and write consecutive float64
// values: 512 bytes per wave and store instruction, as k_noise_levels.
template <typename T>
__global__ __launch_bounds__(MK_MIX_THREADS) void k_masker_levels(const T* __restrict__ wave, const int64_t* __restrict__ offsets,
                                                                  const double* __restrict__ gain, const int64_t* __restrict__ start,
                                                                  const double* __restrict__ masker, const int64_t* __restrict__ moff,
                                                                  const int32_t* __restrict__ masker_of, int B, int K, int64_t total,
                                                                  double* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * MK_MIX_THREADS + threadIdx.x; p < total; p += (int64_t)gridDim.x * MK_MIX_THREADS) {
        const int b = utterance_of(offsets, B, p);
        const uint64_t i = (uint64_t)(p - offsets[b]);
        const T clean = wave[p];
        for (int l = blockIdx.y; l <= K; l += gridDim.y) {
            const size_t u = (size_t)l * B + b;
            out[(size_t)l * (size_t)total + (size_t)p] = mk_sample(clean, gain[u], start[u], masker, moff, l < K ? masker_of[l] : 0, i);
        }
    }
}

// One thread per sample of a batch whose utterance b runs at level[b]: out[p] = what k_masker_levels writes for that level of
// utterance number first_utt + b (which the gain kernel put into gain[b] and start[b]). gain == NULL: every utterance is clean (the
// conversion to float64 alone).
template <typename T>
__global__ __launch_bounds__(MK_MIX_THREADS) void k_masker_pick(const T* __restrict__ wave, const int64_t* __restrict__ offsets,
                                                                const double* __restrict__ gain, const int64_t* __restrict__ start,
                                                                const int32_t* __restrict__ level, const double* __restrict__ masker,
                                                                const int64_t* __restrict__ moff, const int32_t* __restrict__ masker_of, int B,
                                                                int K, int64_t total, double* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * MK_MIX_THREADS + threadIdx.x; p < total; p += (int64_t)gridDim.x * MK_MIX_THREADS) {
        const T clean = wave[p];
        double v = (double)clean;
        if (gain) {
            const int b = utterance_of(offsets, B, p);
            const int l = level[b];
            v = mk_sample(clean, gain[b], start[b], masker, moff, l < K ? masker_of[l] : 0, (uint64_t)(p - offsets[b]));
        }
        out[p] = v;
    }
}

dim3 mix_grid(int64_t total, int levels) {
    const int64_t blocks = (total + MK_MIX_THREADS - 1) / MK_MIX_THREADS;
    return dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)), (unsigned)(levels < 1024 ? levels : 1024));
}

}  // namespace

int f2_check_maskers(f2_ctx* ctx, const double* masker, const int64_t* masker_offsets, int R, const int32_t* masker_of, int K) {
    F2_CHECK(ctx, masker && masker_offsets && masker_of, F2_ERR_INVALID,
             "maskers need their samples (masker), masker_offsets and the recording of each of the %d levels (masker_of)", K);
    F2_CHECK(ctx, R >= 1, F2_ERR_INVALID, "maskers need at least one recording (R=%d)", R);
    F2_CHECK(ctx, R <= F2_MASKER_MAX_RECORDINGS, F2_ERR_UNSUPPORTED, "%d recordings (at most %d)", R, F2_MASKER_MAX_RECORDINGS);
    F2_CHECK(ctx, K <= F2_MASKER_MAX_LEVELS, F2_ERR_UNSUPPORTED, "%d masker levels (at most %d)", K, F2_MASKER_MAX_LEVELS);
    F2_CHECK(ctx, masker_offsets[0] == 0, F2_ERR_INVALID, "masker_offsets[0] must be 0 (recording 0)");
    for (int r = 0; r < R; ++r) {
        const int64_t M = masker_offsets[r + 1] - masker_offsets[r];
        F2_CHECK(ctx, M >= 0, F2_ERR_INVALID, "masker_offsets must be non-decreasing (recording %d)", r);
        F2_CHECK(ctx, M >= 1, F2_ERR_INVALID, "recording %d is empty", r);
        F2_CHECK(ctx, M <= F2_MASKER_MAX_SAMPLES, F2_ERR_UNSUPPORTED, "recording %d has %lld samples (at most %lld)", r, (long long)M,
                 (long long)F2_MASKER_MAX_SAMPLES);
    }
    for (int r = 0; r < R; ++r)
        for (int64_t i = masker_offsets[r]; i < masker_offsets[r + 1]; ++i)
            F2_CHECK(ctx, std::isfinite(masker[i]), F2_ERR_INVALID, "recording %d: sample %lld is not finite", r,
                     (long long)(i - masker_offsets[r]));
    for (int l = 0; l < K; ++l)
        F2_CHECK(ctx, masker_of[l] >= 0 && masker_of[l] < R, F2_ERR_INVALID, "level %d: recording %d is outside [0, %d)", l, (int)masker_of[l], R);
    return F2_OK;
}

int f2_check_masker_levels(f2_ctx* ctx, const double* snr_db, const double* masker, const int64_t* masker_offsets, int R,
                           const int32_t* masker_of, int K) {
    F2_CHECK(ctx, K >= 1 && snr_db, F2_ERR_INVALID, "a sweep needs at least one masker level (K=%d) and their snr_db", K);
    for (int k = 0; k < K; ++k) F2_CHECK(ctx, std::isfinite(snr_db[k]), F2_ERR_INVALID, "snr_db[%d] is not finite", k);
    return f2_check_maskers(ctx, masker, masker_offsets, R, masker_of, K);
}

int f2_check_masker_pick(f2_ctx* ctx, int B, f2_masker_pick_args* M) {
    F2_TRY(f2_check_noise_pick(ctx, B, {M->snr_db, M->K, M->level_of, M->first_utterance, M->seed}));
    bool all_clean = M->silent();
    if (!all_clean) {
        all_clean = true;
        for (int b = 0; b < B; ++b) all_clean = all_clean && M->level_of[b] == M->K;
    }
    if (all_clean) {   // nothing reads a recording: the stage converts alone, or is skipped
        M->K = 0, M->level_of = nullptr;
        return F2_OK;
    }
    return f2_check_maskers(ctx, M->masker, M->masker_offsets, M->R, M->masker_of, M->K);
}

int f2_upload_maskers(f2_ctx* ctx, f2_scratch& area, const double* masker, const int64_t* masker_offsets, int R, const int64_t** d_moff,
                      const double** d_masker) {
    const size_t obytes = sizeof(int64_t) * ((size_t)R + 1), sbytes = sizeof(double) * (size_t)masker_offsets[R];
    F2_TRY(f2_reserve(ctx, area, obytes + sbytes));
    F2_TRY(f2_upload_async(ctx, area.ptr, masker_offsets, obytes));
    F2_TRY(f2_upload_async(ctx, (char*)area.ptr + obytes, masker, sbytes));
    *d_moff = (const int64_t*)area.ptr, *d_masker = (const double*)((const char*)area.ptr + obytes);
    return F2_OK;
}

void f2_masker_meta(f2_meta_carve* meta, int B, int K, f2_masker_arrays* A) {
    const size_t U = ((size_t)K + 1) * (size_t)B;
    meta->add(&A->d_sigma, 3 * U), meta->add(&A->d_lin, (size_t)K), meta->add(&A->d_masker_of, ((size_t)K + 1) / 2);
    A->d_gain = nullptr, A->d_start = nullptr;   // (behind d_sigma: set by the launch, once reserve() has placed it)
}

int f2_launch_masker_levels(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const int64_t* h_offsets, int B,
                            const double* snr_db, const double* masker, const int64_t* masker_offsets, int R, const int32_t* masker_of,
                            int K, uint64_t seed, f2_masker_arrays& A, double* d_out) {
    const int64_t total = h_offsets[B];
    if (B == 0 || total == 0) return F2_OK;
    const size_t U = ((size_t)K + 1) * (size_t)B;
    A.d_gain = A.d_sigma + U, A.d_start = (int64_t*)(A.d_sigma + 2 * U);
    std::vector<double> lin;   // 10^(snr / 10) per level, as f2_eval_noise_sweep forms it
    for (int k = 0; k < K; ++k) lin.push_back(std::pow(10.0, snr_db[k] / 10.0));
    F2_TRY(f2_upload_async(ctx, A.d_lin, lin.data(), sizeof(double) * (size_t)K));
    F2_TRY(f2_upload_async(ctx, A.d_masker_of, masker_of, sizeof(int32_t) * (size_t)K));
    const int64_t* d_moff;
    const double* d_masker;
    F2_TRY(f2_upload_maskers(ctx, ctx->masker, masker, masker_offsets, R, &d_moff, &d_masker));
    F2_TRY(f2_launch_noise_sigma(ctx, d_wave, wave_dtype, d_offsets, A.d_lin, B, K, A.d_sigma));
    k_masker_gain_levels<<<dim3((unsigned)B, (unsigned)(K + 1)), dim3(MK_SUM_THREADS), 0, ctx->stream>>>(
        d_offsets, A.d_sigma, d_masker, d_moff, (const int32_t*)A.d_masker_of, B, K, seed, A.d_gain, A.d_start);
    F2_HIP(ctx, hipGetLastError());
    if (wave_dtype == F2_WAVE_I16)
        k_masker_levels<int16_t><<<mix_grid(total, K + 1), dim3(MK_MIX_THREADS), 0, ctx->stream>>>(
            (const int16_t*)d_wave, d_offsets, A.d_gain, A.d_start, d_masker, d_moff, (const int32_t*)A.d_masker_of, B, K, total, d_out);
    else
        k_masker_levels<double><<<mix_grid(total, K + 1), dim3(MK_MIX_THREADS), 0, ctx->stream>>>(
            (const double*)d_wave, d_offsets, A.d_gain, A.d_start, d_masker, d_moff, (const int32_t*)A.d_masker_of, B, K, total, d_out);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

void f2_masker_pick_meta(f2_meta_carve* meta, int B, const f2_masker_pick_args& M, f2_masker_pick_arrays* A) {
    if (M.silent()) return;
    meta->add(&A->d_sigma, 3 * (size_t)B), meta->add(&A->d_lin, (size_t)M.K);
    meta->add(&A->d_level, ((size_t)B + 1) / 2), meta->add(&A->d_masker_of, ((size_t)M.K + 1) / 2);
}

int f2_launch_masker_pick(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, int B, int64_t total,
                          const f2_masker_pick_args& M, f2_masker_pick_arrays& A, double* d_out) {
    if (B == 0) return F2_OK;
    const double* d_masker = M.d_masker;
    const int64_t* d_moff = M.d_moff;
    if (!M.silent()) {
        A.d_gain = A.d_sigma + B, A.d_start = (int64_t*)(A.d_sigma + 2 * (size_t)B);
        std::vector<double> lin;
        for (int k = 0; k < M.K; ++k) lin.push_back(std::pow(10.0, M.snr_db[k] / 10.0));
        F2_TRY(f2_upload_async(ctx, A.d_lin, lin.data(), sizeof(double) * (size_t)M.K));
        F2_TRY(f2_upload_async(ctx, A.d_level, M.level_of, sizeof(int32_t) * (size_t)B));
        F2_TRY(f2_upload_async(ctx, A.d_masker_of, M.masker_of, sizeof(int32_t) * (size_t)M.K));
        // (a caller that serves several launches from one upload hands the device copies in)
        if (!d_masker) F2_TRY(f2_upload_maskers(ctx, ctx->masker, M.masker, M.masker_offsets, M.R, &d_moff, &d_masker));
        F2_TRY(f2_launch_noise_pick_sigma(ctx, d_wave, wave_dtype, d_offsets, A.d_lin, (const int32_t*)A.d_level, B, M.K, A.d_sigma));
        k_masker_gain_pick<<<dim3((unsigned)B), dim3(MK_SUM_THREADS), 0, ctx->stream>>>(
            d_offsets, A.d_sigma, (const int32_t*)A.d_level, d_masker, d_moff, (const int32_t*)A.d_masker_of, M.K, M.first_utterance, M.seed,
            A.d_gain, A.d_start);
        F2_HIP(ctx, hipGetLastError());
    }
    if (total == 0) return F2_OK;
    if (wave_dtype == F2_WAVE_I16)
        k_masker_pick<int16_t><<<mix_grid(total, 1), dim3(MK_MIX_THREADS), 0, ctx->stream>>>(
            (const int16_t*)d_wave, d_offsets, A.d_gain, A.d_start, (const int32_t*)A.d_level, d_masker, d_moff, (const int32_t*)A.d_masker_of, B,
            M.K, total, d_out);
    else
        k_masker_pick<double><<<mix_grid(total, 1), dim3(MK_MIX_THREADS), 0, ctx->stream>>>(
            (const double*)d_wave, d_offsets, A.d_gain, A.d_start, (const int32_t*)A.d_level, d_masker, d_moff, (const int32_t*)A.d_masker_of, B,
            M.K, total, d_out);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

namespace {

// sigma, gain and start of a call come back as one run of 3 n values ([sigma | gain | start], as the carve placed them) and are
// handed out here; a caller that wants none of them does not wait for them
struct masker_small_outputs {
    double *sigma, *gain;
    int64_t* start;
    size_t n;
    std::vector<double> all;
    double* buffer() {
        if (!sigma && !gain && !start) return nullptr;
        all.assign(3 * n, 0.0);
        return all.data();
    }
    void hand_out() const {
        if (all.empty()) return;
        if (sigma) memcpy(sigma, all.data(), sizeof(double) * n);
        if (gain) memcpy(gain, all.data() + n, sizeof(double) * n);
        if (start) memcpy(start, all.data() + 2 * n, sizeof(int64_t) * n);
    }
};

}  // namespace

// f2_masker_levels: the clean samples and the recordings go up, the sigma kernel and the two masker kernels run, the float64 levels
// and sigma / gain / start come back. A device call waits only for those three.
extern "C" int f2_masker_levels(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, int B, const double* snr_db,
                                const double* masker, const int64_t* masker_offsets, int R, const int32_t* masker_of, int K, uint64_t seed,
                                double* noisy, double* sigma_or_null, double* gain_or_null, int64_t* start_or_null, int mem_space) {
    f2_masker_arrays A;
    // (a K the checks refuse sizes nothing)
    masker_small_outputs S = {sigma_or_null, gain_or_null, start_or_null,
                              ((size_t)(K > 0 && K <= F2_MASKER_MAX_LEVELS ? K : 0) + 1) * (size_t)(B > 0 ? B : 0), {}};
    const int rc = f2_stage_call(
        ctx, offsets, B, mem_space,
        [&]() -> int {
            F2_TRY(f2_check_wave_batch(ctx, wave_dtype, offsets, B, mem_space));
            F2_TRY(f2_check_masker_levels(ctx, snr_db, masker, masker_offsets, R, masker_of, K));
            F2_CHECK(ctx, ((int64_t)K + 1) * (B > 0 ? B : 1) <= INT32_MAX / 2, F2_ERR_UNSUPPORTED, "%d levels of %d utterances", K + 1, B);
            return F2_OK;
        },
        [&](f2_meta_carve* meta) {
            f2_masker_meta(meta, B, K, &A);
            return F2_OK;
        },
        wave, [&](int64_t total, const void** d_wave) { return f2_stage_wave(ctx, wave, wave_dtype, total, mem_space, d_wave); },
        &f2_ctx::levels, noisy, sizeof(double) * ((size_t)K + 1),
        [&](const void* d_wave, const int64_t* d_offsets, int64_t, double* d_out) {
            return f2_launch_masker_levels(ctx, d_wave, wave_dtype, d_offsets, offsets, B, snr_db, masker, masker_offsets, R, masker_of, K, seed,
                                           A, d_out);
        },
        S.buffer(), 3 * S.n, &A.d_sigma);
    if (rc == F2_OK) S.hand_out();
    return rc;
}

// f2_masker_pick: the same for one level per utterance, in the layout of the waves
extern "C" int f2_masker_pick(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, int B, const double* snr_db,
                              const double* masker, const int64_t* masker_offsets, int R, const int32_t* masker_of, int K,
                              const int32_t* level_of, uint32_t first_utterance, uint64_t seed, double* noisy, double* sigma_or_null,
                              double* gain_or_null, int64_t* start_or_null, int mem_space) {
    f2_masker_pick_args M = {snr_db, masker, masker_offsets, R, masker_of, K, level_of, first_utterance, seed, nullptr, nullptr};
    f2_masker_pick_arrays A;
    masker_small_outputs S = {sigma_or_null, gain_or_null, start_or_null, (size_t)(B > 0 ? B : 0), {}};
    const int rc = f2_stage_call(
        ctx, offsets, B, mem_space,
        [&]() -> int {   // (f2_noise_pick's order: the dtype before B, the offsets only where there is an utterance)
            F2_TRY(f2_check_wave_dtype(ctx, wave_dtype));
            F2_CHECK(ctx, B >= 0, F2_ERR_INVALID, "bad batch size (B=%d)", B);
            F2_TRY(f2_check_mem_space(ctx, mem_space, false));
            F2_TRY(f2_check_masker_pick(ctx, B, &M));
            if (B > 0) F2_TRY(f2_check_offsets(ctx, offsets, B, "offsets"));
            return F2_OK;
        },
        [&](f2_meta_carve* meta) {
            f2_masker_pick_meta(meta, B, M, &A);
            return F2_OK;
        },
        wave, [&](int64_t total, const void** d_wave) { return f2_stage_wave(ctx, wave, wave_dtype, total, mem_space, d_wave); },
        &f2_ctx::levels, noisy, sizeof(double),
        [&](const void* d_wave, const int64_t* d_offsets, int64_t total, double* d_out) {
            return f2_launch_masker_pick(ctx, d_wave, wave_dtype, d_offsets, B, total, M, A, d_out);
        },
        S.buffer(), 3 * S.n, &A.d_sigma);
    if (rc == F2_OK) S.hand_out();
    return rc;
}
