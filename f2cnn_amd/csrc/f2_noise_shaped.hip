// Coloured noise on a ragged batch at K levels in one pass (include/f2cnn_hip.h: f2_shaped_noise_levels; the kernel of
// f2_eval_shaped_noise_sweep).
//   k_shaped_noise_levels  noisy[l][b][i] = clean_b[i] + sigma[l][b] * sum_{t < T_l} h_l[t] z(seed, l, b, i - t), the direct form in
//                          float64. One workgroup per (output tile of F2_SHAPED_BLOCK samples, level); level K, and a level whose
//                          sigma is 0, copies the clean samples. The deviates of the tile's whole span [k0 - (T_l - 1), k0 + nk) are
//                          generated once into LDS as float64 (the index wraps below zero as a 64-bit counter: deviates like any
//                          others), then every lane walks them with ft_walk (f2_fir_tile.h), the walk of k_reverb_levels, over one
//                          chunk that holds every tap.
//   k_shaped_noise_pick    noisy[b][i] for the one level level[b] of every utterance (f2_shaped_noise_pick; the noise stage of
//                          f2_input_batch_coloured / f2_trainer_render_coloured), in the layout of the waves, utterance b being
//                          number first_utt + b of its corpus. The grid is the tiles alone, in the order of a list the host
//                          uploads (most taps first, f2_tile_list); sigma[b] comes from k_noise_pick_sigma (f2_noise.hip). The
//                          tile body (sn_tile) and the epilogue (sn_finish) are the sweep's: the same bits as level level[b].
// Arithmetic contract of the header: one float64 accumulator per output, taps in ascending t, acc = fma(h[t], z[i - t], acc), no
// atomics, no sum split across lanes; then clean + sigma * acc, product and sum rounded separately. sigma comes from k_noise_sigma
// (f2_noise.hip), unchanged. gfx950, wave64; plain vector stores only.
#include "f2_internal.h"
#include "f2_fir_tile.h"
#include "f2_philox.h"
#include "f2_tile_owner.h"

#include <cmath>

namespace {

constexpr int SN_SPAN = FT_BLOCK + F2_SHAPED_MAX_TAPS;   // most staged deviates: zs[j] = z[k0 - tc + j], tc = taps rounded up to FT_R
constexpr int SN_PLANE = SN_SPAN / FT_R + 1;             // pitch of the LDS image (f2_fir_tile.h)
static_assert(F2_SHAPED_BLOCK == FT_BLOCK, "a lane owns FT_R consecutive outputs of the tile");
static_assert(F2_SHAPED_MAX_TAPS % FT_R == 0, "the rounded tap count stays inside the span");
static_assert(FT_R * SN_PLANE * sizeof(double) <= 64 * 1024, "one span in LDS");

// The work of one tile: c[k] = sum_{t < taps} h[t] z(seed, level, utt, k - t) for the outputs k0 .. k0 + nk - 1 (1 <= nk <= FT_BLOCK)
// of utterance number `utt` at `level`, lane L owning k0 + 4 L + c, c < 4, in a0 .. a3 (which enter as 0; those of outputs from nk
// on are not meaningful). zs: the workgroup's FT_R * SN_PLANE doubles of LDS. Every thread of the workgroup calls it (a barrier
// inside). 1 <= taps <= F2_SHAPED_MAX_TAPS; no tap at or beyond `taps` is read.
__device__ __forceinline__ void sn_tile(double* __restrict__ zs, uint64_t seed, uint32_t level, uint32_t utt, int64_t k0, int nk,
                                        const double* __restrict__ h, int taps, double& a0, double& a1, double& a2, double& a3) {
    const int tid = threadIdx.x;
    const int o = FT_R * tid;                                // first output of this lane inside the tile
    const int tc = (taps + FT_R - 1) & ~(FT_R - 1);          // the register window turns once per FT_R taps
    const uint64_t lo = (uint64_t)k0 - (uint64_t)tc;         // sample index of zs[0], modulo 2^64
    const int span = tc + nk;
    for (int j = tid; j < span; j += FT_NT) zs[ft_at<SN_PLANE>(j)] = noise_deviate(seed, level, utt, lo + (uint64_t)j);
    __syncthreads();
    if (o >= nk) return;                                     // (behind the only barrier)
    ft_walk<SN_PLANE>(zs, tc, o, h, taps, a0, a1, a2, a3);
}

// The epilogue of one tile: y[o + c] = x[o + c] + s * a[c] for the lane's outputs below nk, product and sum rounded separately
// (x, y: at the tile's first output).
template <typename T>
__device__ __forceinline__ void sn_finish(const T* __restrict__ x, double* __restrict__ y, int o, int nk, double s,
                                          const double (&a)[FT_R]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < FT_R; ++c)
        if (o + c < nk) {
            const double nz = s * a[c];
            y[o + c] = (double)x[o + c] + nz;
        }
}

// Workgroup (blockIdx.x, l = blockIdx.y) serves outputs k0 .. k0 + FT_BLOCK - 1 of the utterance that owns tile blockIdx.x
// (tile_owner over `first`). Lane L owns k0 + 4 L + c, c < 4.
template <typename T>
__global__ __launch_bounds__(FT_NT) void k_shaped_noise_levels(const T* __restrict__ wave, const int64_t* __restrict__ offsets,
                                                                const int64_t* __restrict__ first, int B,
                                                                const double* __restrict__ sigma, const double* __restrict__ fir,
                                                                const int64_t* __restrict__ fir_offsets, int K, int64_t total,
                                                                uint64_t seed, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double zs[FT_R * SN_PLANE];
    const int tid = threadIdx.x;
    const int l = blockIdx.y;
    const int64_t blk = blockIdx.x;
    const int b = tile_owner(first, B, blk);
    const int64_t n = offsets[b + 1] - offsets[b];
    const int64_t k0 = (blk - first[b]) * FT_BLOCK;
    const int nk = (int)min((int64_t)FT_BLOCK, n - k0);      // outputs of this workgroup, >= 1
    const T* __restrict__ x = wave + offsets[b] + k0;
    double* __restrict__ y = out + (size_t)l * (size_t)total + (size_t)offsets[b] + (size_t)k0;
    const int o = FT_R * tid;                                // first output of this lane inside the tile
    const double s = l < K ? sigma[(size_t)l * B + b] : 0.0;
    if (s == 0.0) {                                          // the clean level, an all-zero utterance: the samples themselves
        ft_copy(x, 0, y, o, nk);
        return;
    }
    double a[FT_R] = {0.0, 0.0, 0.0, 0.0};
    sn_tile(zs, seed, (uint32_t)l, (uint32_t)b, k0, nk, fir + fir_offsets[l], (int)(fir_offsets[l + 1] - fir_offsets[l]), a[0], a[1], a[2],
            a[3]);
    sn_finish(x, y, o, nk, s, a);
}

// One level per utterance, the output in the layout of the waves. Workgroup blockIdx.x serves the tile tiles[blockIdx.x] =
// utterance << 32 | tile index of the utterance (f2_tile_list: no workgroup searches, the expensive tiles start first); utterance b
// runs at level[b] in [0, K], K the clean one, with sigma[b] (k_noise_pick_sigma: 0 for the clean level) and the deviates of
// utterance number first_utt + b. The same tile body and epilogue, the same bits as level level[b] of k_shaped_noise_levels.
template <typename T>
__global__ __launch_bounds__(FT_NT) void k_shaped_noise_pick(const T* __restrict__ wave, const int64_t* __restrict__ offsets,
                                                              const int64_t* __restrict__ tiles, const double* __restrict__ sigma,
                                                              const int32_t* __restrict__ level, const double* __restrict__ fir,
                                                              const int64_t* __restrict__ fir_offsets, int K, uint32_t first_utt,
                                                              uint64_t seed, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double zs[FT_R * SN_PLANE];
    const int64_t entry = tiles[blockIdx.x];
    const int b = (int)(entry >> 32);
    const int l = level[b];
    const int64_t n = offsets[b + 1] - offsets[b];
    const int64_t k0 = (entry & 0xffffffffll) * FT_BLOCK;
    const int nk = (int)min((int64_t)FT_BLOCK, n - k0);      // outputs of this workgroup, >= 1
    const T* __restrict__ x = wave + offsets[b] + k0;
    double* __restrict__ y = out + (size_t)offsets[b] + (size_t)k0;
    const int o = FT_R * threadIdx.x;                        // first output of this lane inside the tile
    const double s = l < K ? sigma[b] : 0.0;
    if (s == 0.0) {                                          // a clean utterance, an all-zero one: the samples themselves
        ft_copy(x, 0, y, o, nk);
        return;
    }
    double a[FT_R] = {0.0, 0.0, 0.0, 0.0};
    sn_tile(zs, seed, (uint32_t)l, first_utt + (uint32_t)b, k0, nk, fir + fir_offsets[l], (int)(fir_offsets[l + 1] - fir_offsets[l]), a[0],
            a[1], a[2], a[3]);
    sn_finish(x, y, o, nk, s, a);
}

}  // namespace

int f2_check_fir(f2_ctx* ctx, const double* snr_db, const double* fir, const int64_t* fir_offsets, int K) {
    F2_CHECK(ctx, K >= 1 && snr_db, F2_ERR_INVALID, "a sweep needs at least one noise level (K=%d) and their snr_db", K);
    for (int k = 0; k < K; ++k) F2_CHECK(ctx, std::isfinite(snr_db[k]), F2_ERR_INVALID, "snr_db[%d] is not finite", k);
    return f2_check_fir_taps(ctx, fir, fir_offsets, K, "a coloured sweep");
}

int f2_check_fir_taps(f2_ctx* ctx, const double* fir, const int64_t* fir_offsets, int K, const char* who) {
    F2_CHECK(ctx, fir && fir_offsets, F2_ERR_INVALID, "%s needs the taps of its %d levels (fir) and their fir_offsets", who, K);
    static const f2_tap_words words = {"noise levels", "fir_offsets", " (level 0)", "level ", "the filter of level"};
    return f2_check_taps(ctx, fir, fir_offsets, K, F2_SHAPED_MAX_LEVELS, F2_SHAPED_MAX_TAPS, words);
}

void f2_shaped_meta(f2_meta_carve* meta, int B, const int64_t* fir_offsets, int K, f2_shaped_arrays* A) {
    meta->add(&A->d_sigma, ((size_t)K + 1) * (size_t)B), meta->add(&A->d_lin, (size_t)K);
    meta->add(&A->d_first, (size_t)B + 1), meta->add(&A->d_fir_off, (size_t)K + 1), meta->add(&A->d_fir, (size_t)fir_offsets[K]);
}

int f2_launch_shaped_noise_levels(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const int64_t* h_offsets,
                                  int B, const double* snr_db, const double* fir, const int64_t* fir_offsets, int K, uint64_t seed,
                                  const f2_shaped_arrays& A, double* d_out) {
    const int64_t total = h_offsets[B];
    if (B == 0 || total == 0) return F2_OK;
    std::vector<int64_t> first;
    const int64_t tiles = f2_tile_table(h_offsets, B, FT_BLOCK, &first);
    F2_TRY(f2_check_workgroups(ctx, tiles, "coloured noise", " per level"));
    std::vector<double> lin;   // 10^(snr / 10) per level, as f2_eval_noise_sweep forms it
    for (int k = 0; k < K; ++k) lin.push_back(std::pow(10.0, snr_db[k] / 10.0));
    F2_TRY(f2_upload_async(ctx, A.d_lin, lin.data(), sizeof(double) * (size_t)K));
    F2_TRY(f2_launch_noise_sigma(ctx, d_wave, wave_dtype, d_offsets, A.d_lin, B, K, A.d_sigma));
    // d_first and d_fir_off were named in a row (f2_shaped_meta): one upload for both
    first.insert(first.end(), fir_offsets, fir_offsets + K + 1);
    F2_TRY(f2_upload_async(ctx, A.d_first, first.data(), sizeof(int64_t) * first.size()));
    F2_TRY(f2_upload_async(ctx, A.d_fir, fir, sizeof(double) * (size_t)fir_offsets[K]));
    const dim3 grid((unsigned)tiles, (unsigned)(K + 1));
    if (wave_dtype == F2_WAVE_I16)
        k_shaped_noise_levels<int16_t><<<grid, dim3(FT_NT), 0, ctx->stream>>>((const int16_t*)d_wave, d_offsets, A.d_first, B, A.d_sigma,
                                                                             A.d_fir, A.d_fir_off, K, total, seed, d_out);
    else
        k_shaped_noise_levels<double><<<grid, dim3(FT_NT), 0, ctx->stream>>>((const double*)d_wave, d_offsets, A.d_first, B, A.d_sigma,
                                                                            A.d_fir, A.d_fir_off, K, total, seed, d_out);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

// ---- one level per utterance: f2_shaped_noise_pick, the noise stage of f2_input_batch_coloured / f2_trainer_render_coloured ----

int f2_check_noise_colours(f2_ctx* ctx, int B, f2_noise_pick_args* N, bool need_fir) {
    bool all_clean = N->clean();
    if (!all_clean) {
        all_clean = true;
        for (int b = 0; b < B; ++b) all_clean = all_clean && N->level_of[b] == N->K;
    }
    if (all_clean) {   // nothing reads a tap: the white stage converts alone
        N->fir = nullptr, N->fir_offsets = nullptr;
        return F2_OK;
    }
    if (!N->fir && !need_fir) return F2_OK;
    return f2_check_fir_taps(ctx, N->fir, N->fir_offsets, N->K, "coloured noise");
}

void f2_shaped_pick_meta(f2_meta_carve* meta, int B, const int64_t* h_offsets, const f2_noise_pick_args& N, f2_shaped_pick_arrays* A) {
    meta->add(&A->d_tiles, (size_t)f2_tile_table(h_offsets, B, FT_BLOCK));
    if (!N.d_fir) meta->add(&A->d_fir_off, (size_t)N.K + 1), meta->add(&A->d_fir, (size_t)N.fir_offsets[N.K]);
}

int f2_launch_shaped_noise_pick(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const int64_t* h_offsets, int B,
                                const f2_noise_pick_args& N, const f2_shaped_pick_arrays& A, const int32_t* d_level,
                                const double* d_sigma, double* d_out) {
    if (B == 0 || h_offsets[B] == 0) return F2_OK;
    const int64_t ntiles = f2_tile_table(h_offsets, B, FT_BLOCK);
    F2_TRY(f2_check_workgroups(ctx, ntiles, "coloured noise", ""));
    // a tile costs the taps of its utterance's level, and nothing when clean
    std::vector<int64_t> tiles;
    f2_tile_list(h_offsets, B, FT_BLOCK, ctx->opt_noise_pick_sort != 0, &tiles, [&](int b, int64_t, int64_t) {
        const int l = N.level_of[b];
        return (int32_t)(l < N.K ? N.fir_offsets[l + 1] - N.fir_offsets[l] : 0);
    });
    F2_TRY(f2_upload_async(ctx, A.d_tiles, tiles.data(), sizeof(int64_t) * tiles.size()));
    const double* d_fir = N.d_fir;
    const int64_t* d_fir_off = N.d_fir_off;
    if (!d_fir) {   // (a caller that serves several launches from one upload hands the device copies in)
        F2_TRY(f2_upload_async(ctx, A.d_fir_off, N.fir_offsets, sizeof(int64_t) * ((size_t)N.K + 1)));
        F2_TRY(f2_upload_async(ctx, A.d_fir, N.fir, sizeof(double) * (size_t)N.fir_offsets[N.K]));
        d_fir = A.d_fir, d_fir_off = A.d_fir_off;
    }
    const dim3 grid((unsigned)ntiles);
    if (wave_dtype == F2_WAVE_I16)
        k_shaped_noise_pick<int16_t><<<grid, dim3(FT_NT), 0, ctx->stream>>>((const int16_t*)d_wave, d_offsets, A.d_tiles, d_sigma, d_level,
                                                                           d_fir, d_fir_off, N.K, N.first_utterance, N.seed, d_out);
    else
        k_shaped_noise_pick<double><<<grid, dim3(FT_NT), 0, ctx->stream>>>((const double*)d_wave, d_offsets, A.d_tiles, d_sigma, d_level,
                                                                          d_fir, d_fir_off, N.K, N.first_utterance, N.seed, d_out);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

// f2_shaped_noise_levels: the clean samples and the taps go up, the two kernels run, the float64 levels and sigma come back. A device
// call waits only for sigma.
extern "C" int f2_shaped_noise_levels(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, int B, const double* snr_db,
                                      const double* fir, const int64_t* fir_offsets, int K, uint64_t seed, double* noisy,
                                      double* sigma_or_null, int mem_space) {
    f2_shaped_arrays A;
    return f2_stage_call(
        ctx, offsets, B, mem_space,
        [&]() -> int {
            F2_TRY(f2_check_wave_batch(ctx, wave_dtype, offsets, B, mem_space));
            F2_TRY(f2_check_fir(ctx, snr_db, fir, fir_offsets, K));
            F2_CHECK(ctx, ((int64_t)K + 1) * (B > 0 ? B : 1) <= INT32_MAX / 2, F2_ERR_UNSUPPORTED, "%d levels of %d utterances", K + 1, B);
            return F2_OK;
        },
        [&](f2_meta_carve* meta) {
            f2_shaped_meta(meta, B, fir_offsets, K, &A);
            return F2_OK;
        },
        wave, [&](int64_t total, const void** d_wave) { return f2_stage_wave(ctx, wave, wave_dtype, total, mem_space, d_wave); },
        &f2_ctx::levels, noisy, sizeof(double) * ((size_t)K + 1),
        [&](const void* d_wave, const int64_t* d_offsets, int64_t, double* d_out) {
            return f2_launch_shaped_noise_levels(ctx, d_wave, wave_dtype, d_offsets, offsets, B, snr_db, fir, fir_offsets, K, seed, A, d_out);
        },
        sigma_or_null, ((size_t)K + 1) * (size_t)B, &A.d_sigma);
}
