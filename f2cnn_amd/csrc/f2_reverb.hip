// Reverberation of a ragged batch at K impulse responses in one pass (include/f2cnn_hip.h: f2_reverb_levels; the kernel of
// f2_eval_reverb_sweep).
//   k_reverb_levels  wet[l][b][k] = sum_{t <= k, t < T_l} h_l[t] x_b[k - t], the direct form in float64. One workgroup per (output
//                    tile of F2_REVERB_BLOCK samples, level); level K copies the dry samples. The taps are walked in chunks of
//                    F2_REVERB_TAP_CHUNK: per chunk the input span of the tile is staged in LDS as float64 (zero before the
//                    utterance's start, as k_resample does), then every lane walks it with ft_walk (f2_fir_tile.h), the walk
//                    k_shaped_noise_levels shares.
//   k_reverb_pick    wet[b][k] for the one room room[b] of every utterance (f2_reverb_pick; the reverberant stage of
//                    f2_input_batch_wet / f2_trainer_render_wet), in the layout of the waves. The grid is the tiles alone, in the
//                    order of a list the host uploads (most taps first); the per-tile tap walk is rv_walk, shared with the sweep.
// Arithmetic contract of the header: one float64 accumulator per output, taps in ascending t, acc = fma(h[t], x[k - t], acc), no
// atomics, no sum split across lanes. gfx950, wave64; plain vector stores only.
#include "f2_internal.h"
#include "f2_fir_tile.h"
#include "f2_tile_owner.h"

#include <algorithm>

namespace {

constexpr int RV_TC = F2_REVERB_TAP_CHUNK;         // taps per staged span
constexpr int RV_SPAN = FT_BLOCK + RV_TC;          // staged samples of a chunk: xs[j] = x[k0 - t0 - RV_TC + j]
constexpr int RV_PLANE = RV_SPAN / FT_R + 1;       // pitch of the LDS image (f2_fir_tile.h)
static_assert(F2_REVERB_BLOCK == FT_BLOCK, "a lane owns FT_R consecutive outputs of the tile");
static_assert(RV_TC % FT_R == 0 && RV_TC >= FT_R, "the register window turns once per FT_R taps");
static_assert(FT_R * RV_PLANE * sizeof(double) <= 64 * 1024, "one span in LDS");

// The tap walk of one tile: outputs k0 .. k0 + nk - 1 (nk >= 1) of the utterance x of n samples under the response h of `taps` taps,
// lane L owning k0 + 4 L + c, c < 4, in a0 .. a3 (which enter as 0).
// Chunk t0 needs x[k0 - t0 - (RV_TC - 1)] .. x[k0 + FT_BLOCK - 1 - t0]; samples before the utterance are staged as 0 (a tap
// beyond k adds fma(h, 0, acc), which leaves acc as it is), samples from n on - read only by outputs that are not stored - too.
// Chunks whose span lies before the utterance altogether are not walked, and no tap at or beyond `taps` is ever read.
// xs: the workgroup's FT_R * RV_PLANE doubles of LDS. Every thread of the workgroup calls it (barriers inside).
template <typename T>
__device__ __forceinline__ void rv_walk(double* __restrict__ xs, const T* __restrict__ x, int64_t n, int64_t k0, int nk,
                                        const double* __restrict__ h, int64_t taps, double& a0, double& a1, double& a2, double& a3) {
    const int tid = threadIdx.x;
    // taps that reach a sample of the utterance for some stored output of the tile: t <= k0 + nk - 1
    const int t_end = (int)min(taps, k0 + (int64_t)nk);
    for (int t0 = 0; t0 < t_end; t0 += RV_TC) {
        const int ns = min(RV_TC, t_end - t0);               // taps of this chunk
        const int64_t lo = k0 - (int64_t)t0 - RV_TC;         // utterance index of xs[0]
        __syncthreads();                                     // the previous chunk's readers are done
        for (int j = tid; j < RV_SPAN; j += FT_NT) {
            const int64_t i = lo + j;
            xs[ft_at<RV_PLANE>(j)] = i >= 0 && i < n ? (double)x[i] : 0.0;
        }
        __syncthreads();
        ft_walk<RV_PLANE>(xs, RV_TC, FT_R * tid, h + t0, ns, a0, a1, a2, a3);
    }
}

// Workgroup (blockIdx.x, l = blockIdx.y) serves outputs k0 .. k0 + FT_BLOCK - 1 of the utterance that owns tile blockIdx.x
// (tile_owner over `first`). Lane L owns k0 + 4 L + c, c < 4.
template <typename T>
__global__ __launch_bounds__(FT_NT) void k_reverb_levels(const T* __restrict__ wave, const int64_t* __restrict__ offsets,
                                                          const int64_t* __restrict__ first, int B, const double* __restrict__ rir,
                                                          const int64_t* __restrict__ rir_offsets, int K, int64_t total,
                                                          double* __restrict__ out) {
    __shared__ double xs[FT_R * RV_PLANE];
    const int l = blockIdx.y;
    const int64_t blk = blockIdx.x;
    const int b = tile_owner(first, B, blk);
    const int64_t n = offsets[b + 1] - offsets[b];
    const int64_t k0 = (blk - first[b]) * FT_BLOCK;
    const int nk = (int)min((int64_t)FT_BLOCK, n - k0);      // outputs of this workgroup, >= 1
    const T* __restrict__ x = wave + offsets[b];
    double* __restrict__ y = out + (size_t)l * (size_t)total + (size_t)offsets[b] + (size_t)k0;
    const int o = FT_R * threadIdx.x;                        // first output of this lane inside the tile
    if (l == K) {                                            // the dry level: the samples themselves
        ft_copy(x, k0, y, o, nk);
        return;
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    rv_walk(xs, x, n, k0, nk, rir + rir_offsets[l], rir_offsets[l + 1] - rir_offsets[l], a0, a1, a2, a3);
    ft_store(y, o, nk, a0, a1, a2, a3);
}

// One room per utterance, the output in the layout of the waves. Workgroup blockIdx.x serves the tile tiles[blockIdx.x] =
// utterance << 32 | tile index of the utterance (a list from the host, so that no workgroup searches and the expensive tiles can
// start first); the utterance runs at room[b] in [0, K], K the dry one; room == NULL: every utterance is dry. The same walk, the
// same bits as level room[b] of k_reverb_levels.
template <typename T>
__global__ __launch_bounds__(FT_NT) void k_reverb_pick(const T* __restrict__ wave, const int64_t* __restrict__ offsets,
                                                        const int64_t* __restrict__ tiles, const double* __restrict__ rir,
                                                        const int64_t* __restrict__ rir_offsets, const int32_t* __restrict__ room, int K,
                                                        double* __restrict__ out) {
    __shared__ double xs[FT_R * RV_PLANE];
    const int64_t entry = tiles[blockIdx.x];
    const int b = (int)(entry >> 32);
    const int l = room ? room[b] : K;
    const int64_t n = offsets[b + 1] - offsets[b];
    const int64_t k0 = (entry & 0xffffffffll) * FT_BLOCK;
    const int nk = (int)min((int64_t)FT_BLOCK, n - k0);      // outputs of this workgroup, >= 1
    const T* __restrict__ x = wave + offsets[b];
    double* __restrict__ y = out + (size_t)offsets[b] + (size_t)k0;
    const int o = FT_R * threadIdx.x;
    if (l == K) {                                            // a dry utterance: the samples themselves
        ft_copy(x, k0, y, o, nk);
        return;
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    rv_walk(xs, x, n, k0, nk, rir + rir_offsets[l], rir_offsets[l + 1] - rir_offsets[l], a0, a1, a2, a3);
    ft_store(y, o, nk, a0, a1, a2, a3);
}

}  // namespace

int f2_check_rir(f2_ctx* ctx, const double* rir, const int64_t* rir_offsets, int K) {
    F2_CHECK(ctx, K >= 1 && rir && rir_offsets, F2_ERR_INVALID,
             "a sweep needs at least one impulse response (K=%d), their taps and their rir_offsets", K);
    static const f2_tap_words words = {"impulse responses", "rir_offsets", "", "l=", "impulse response"};
    return f2_check_taps(ctx, rir, rir_offsets, K, F2_REVERB_MAX_LEVELS, F2_REVERB_MAX_TAPS, words);
}

void f2_reverb_meta(f2_meta_carve* meta, int B, const int64_t* rir_offsets, int K, f2_reverb_arrays* A) {
    meta->add(&A->d_first, (size_t)B + 1), meta->add(&A->d_rir_off, (size_t)K + 1), meta->add(&A->d_rir, (size_t)rir_offsets[K]);
}

int f2_launch_reverb_levels(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const int64_t* h_offsets, int B,
                            const double* rir, const int64_t* rir_offsets, int K, const f2_reverb_arrays& A, double* d_out) {
    const int64_t total = h_offsets[B];
    if (B == 0 || total == 0) return F2_OK;
    std::vector<int64_t> first;
    const int64_t tiles = f2_tile_table(h_offsets, B, FT_BLOCK, &first);
    F2_TRY(f2_check_workgroups(ctx, tiles, "reverberation", " per level"));
    // d_first and d_rir_off were named in a row (f2_reverb_meta): one upload for both
    first.insert(first.end(), rir_offsets, rir_offsets + K + 1);
    F2_TRY(f2_upload_async(ctx, A.d_first, first.data(), sizeof(int64_t) * first.size()));
    F2_TRY(f2_upload_async(ctx, A.d_rir, rir, sizeof(double) * (size_t)rir_offsets[K]));
    const dim3 grid((unsigned)tiles, (unsigned)(K + 1));
    if (wave_dtype == F2_WAVE_I16)
        k_reverb_levels<int16_t><<<grid, dim3(FT_NT), 0, ctx->stream>>>((const int16_t*)d_wave, d_offsets, A.d_first, B, A.d_rir,
                                                                       A.d_rir_off, K, total, d_out);
    else
        k_reverb_levels<double><<<grid, dim3(FT_NT), 0, ctx->stream>>>((const double*)d_wave, d_offsets, A.d_first, B, A.d_rir,
                                                                      A.d_rir_off, K, total, d_out);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

extern "C" int f2_reverb_levels(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, int B, const double* rir,
                                const int64_t* rir_offsets, int K, double* levels, int mem_space) {
    f2_reverb_arrays A;
    return f2_stage_call(
        ctx, offsets, B, mem_space,
        [&]() -> int {
            F2_TRY(f2_check_wave_batch(ctx, wave_dtype, offsets, B, mem_space));
            F2_TRY(f2_check_rir(ctx, rir, rir_offsets, K));
            F2_CHECK(ctx, ((int64_t)K + 1) * (B > 0 ? B : 1) <= INT32_MAX / 2, F2_ERR_UNSUPPORTED, "%d levels of %d utterances", K + 1, B);
            return F2_OK;
        },
        [&](f2_meta_carve* meta) {
            f2_reverb_meta(meta, B, rir_offsets, K, &A);
            return F2_OK;
        },
        wave,
        [&](int64_t total, const void** d_wave) { return f2_stage_wave(ctx, wave, wave_dtype, total, mem_space, d_wave); },
        &f2_ctx::levels, levels, sizeof(double) * ((size_t)K + 1),
        [&](const void* d_wave, const int64_t* d_offsets, int64_t, double* d_out) {
            return f2_launch_reverb_levels(ctx, d_wave, wave_dtype, d_offsets, offsets, B, rir, rir_offsets, K, A, d_out);
        });
}

// ---- one room per utterance: f2_reverb_pick, the reverberant stage of f2_input_batch_wet / f2_trainer_render_wet ----

int f2_check_reverb_pick(f2_ctx* ctx, int B, const f2_reverb_pick_args& R) {
    F2_CHECK(ctx, R.K >= 0, F2_ERR_INVALID, "negative number of rooms (K=%d)", R.K);
    if (R.dry()) return F2_OK;
    F2_CHECK(ctx, R.rir, F2_ERR_INVALID, "room_of is given for K=%d rooms, but rir is NULL", R.K);
    F2_TRY(f2_check_rir(ctx, R.rir, R.rir_offsets, R.K));
    for (int b = 0; b < B; ++b)
        F2_CHECK(ctx, R.room_of[b] >= 0 && R.room_of[b] <= R.K, F2_ERR_INVALID, "utterance %d: room %d is outside [0, %d]", b,
                 (int)R.room_of[b], R.K);
    return F2_OK;
}

void f2_reverb_pick_meta(f2_meta_carve* meta, int B, const int64_t* h_offsets, const f2_reverb_pick_args& R, f2_reverb_pick_arrays* A) {
    meta->add(&A->d_tiles, (size_t)f2_tile_table(h_offsets, B, FT_BLOCK));
    if (R.dry()) return;
    meta->add(&A->d_room, ((size_t)B + 1) / 2);
    if (!R.d_rir) meta->add(&A->d_rir_off, (size_t)R.K + 1), meta->add(&A->d_rir, (size_t)R.rir_offsets[R.K]);
}

int f2_launch_reverb_pick(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const int64_t* h_offsets, int B,
                          const f2_reverb_pick_args& R, const f2_reverb_pick_arrays& A, double* d_out) {
    if (B == 0 || h_offsets[B] == 0) return F2_OK;
    const int64_t ntiles = f2_tile_table(h_offsets, B, FT_BLOCK);
    F2_TRY(f2_check_workgroups(ctx, ntiles, "reverberation", ""));
    const bool dry = R.dry();
    // the tile list (f2_tile_list), most taps first: a tile walks min(T_room, k0 + nk) taps, none for a dry utterance
    std::vector<int64_t> tiles;
    f2_tile_list(h_offsets, B, FT_BLOCK, !dry && ctx->opt_reverb_pick_sort, &tiles, [&](int b, int64_t n, int64_t i) {
        const int l = R.room_of[b];
        const int64_t taps = l < R.K ? R.rir_offsets[l + 1] - R.rir_offsets[l] : 0;
        return (int32_t)std::min(taps, std::min(n, (i + 1) * FT_BLOCK));
    });
    F2_TRY(f2_upload_async(ctx, A.d_tiles, tiles.data(), sizeof(int64_t) * tiles.size()));
    const double* d_rir = nullptr;
    const int64_t* d_rir_off = nullptr;
    if (!dry) {
        F2_TRY(f2_upload_async(ctx, A.d_room, R.room_of, sizeof(int32_t) * (size_t)B));
        d_rir = R.d_rir, d_rir_off = R.d_rir_off;
        if (!d_rir) {   // (a caller that serves several launches from one upload hands the device copies in)
            F2_TRY(f2_upload_async(ctx, A.d_rir_off, R.rir_offsets, sizeof(int64_t) * ((size_t)R.K + 1)));
            F2_TRY(f2_upload_async(ctx, A.d_rir, R.rir, sizeof(double) * (size_t)R.rir_offsets[R.K]));
            d_rir = A.d_rir, d_rir_off = A.d_rir_off;
        }
    }
    const int32_t* d_room = dry ? nullptr : (const int32_t*)A.d_room;
    const dim3 grid((unsigned)ntiles);
    if (wave_dtype == F2_WAVE_I16)
        k_reverb_pick<int16_t><<<grid, dim3(FT_NT), 0, ctx->stream>>>((const int16_t*)d_wave, d_offsets, A.d_tiles, d_rir, d_rir_off, d_room,
                                                                     R.K, d_out);
    else
        k_reverb_pick<double><<<grid, dim3(FT_NT), 0, ctx->stream>>>((const double*)d_wave, d_offsets, A.d_tiles, d_rir, d_rir_off, d_room,
                                                                    R.K, d_out);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

extern "C" int f2_reverb_pick(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, int B, const double* rir,
                              const int64_t* rir_offsets, int K, const int32_t* room_of, double* wet, int mem_space) {
    const f2_reverb_pick_args R = {rir, rir_offsets, K, room_of, nullptr, nullptr};
    f2_reverb_pick_arrays A;
    return f2_stage_call(
        ctx, offsets, B, mem_space,
        [&]() -> int {
            F2_TRY(f2_check_wave_batch(ctx, wave_dtype, offsets, B, mem_space));
            return f2_check_reverb_pick(ctx, B, R);
        },
        [&](f2_meta_carve* meta) {
            f2_reverb_pick_meta(meta, B, offsets, R, &A);
            return F2_OK;
        },
        wave,
        [&](int64_t total, const void** d_wave) { return f2_stage_wave(ctx, wave, wave_dtype, total, mem_space, d_wave); },
        &f2_ctx::wet, wet, sizeof(double),
        [&](const void* d_wave, const int64_t* d_offsets, int64_t, double* d_out) {
            return f2_launch_reverb_pick(ctx, d_wave, wave_dtype, d_offsets, offsets, B, R, A, d_out);
        });
}
