// Reverberation of a ragged batch at K impulse responses in one pass (include/f2cnn_hip.h: f2_reverb_levels; the kernel of
// f2_eval_reverb_sweep).
//   k_reverb_levels  wet[l][b][k] = sum_{t <= k, t < T_l} h_l[t] x_b[k - t], the direct form in float64. One workgroup per (output
//                    tile of F2_REVERB_BLOCK samples, level); level K copies the dry samples. The taps are walked in chunks of
//                    F2_REVERB_TAP_CHUNK: per chunk the input span of the tile is staged in LDS as float64 (zero before the
//                    utterance's start, as k_resample does), then every lane slides a register window of its RV_R consecutive
//                    outputs over it - one 8-byte LDS read and RV_R FMAs per tap, the tap itself a wave-uniform load from global
//                    memory.
//   k_reverb_pick    wet[b][k] for the one room room[b] of every utterance (f2_reverb_pick; the reverberant stage of
//                    f2_input_batch_wet / f2_trainer_render_wet), in the layout of the waves. The grid is the tiles alone, in the
//                    order of a list the host uploads (most taps first); the per-tile tap walk is rv_walk, shared with the sweep.
// Arithmetic contract of the header: one float64 accumulator per output, taps in ascending t, acc = fma(h[t], x[k - t], acc), no
// atomics, no sum split across lanes. gfx950, wave64; plain vector stores only.
#include "f2_internal.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int RV_NT = 256;                         // threads of a workgroup
constexpr int RV_R = 4;                            // consecutive outputs of a lane
constexpr int RV_BLOCK = F2_REVERB_BLOCK;          // outputs of a workgroup
constexpr int RV_TC = F2_REVERB_TAP_CHUNK;         // taps per staged span
constexpr int RV_SPAN = RV_BLOCK + RV_TC;          // staged samples of a chunk: xs[j] = x[k0 - t0 - RV_TC + j]
// LDS image: sample j at plane j % RV_R, place j / RV_R. The odd pitch keeps the compiler from pairing the four reads of a step
// into ds_read2st64_b64, which the LDS serves at a quarter of the rate of single ds_read_b64.
constexpr int RV_PLANE = RV_SPAN / RV_R + 1;
static_assert(RV_BLOCK == RV_NT * RV_R, "a lane owns RV_R consecutive outputs of the tile");
static_assert(RV_TC % RV_R == 0 && RV_TC >= RV_R, "the register window turns once per RV_R taps");
static_assert(RV_R * RV_PLANE * sizeof(double) <= 64 * 1024, "one span in LDS");

// Sample j of the span. Lane L reads j = const - 4 L at every tap: with the samples of equal j % 4 side by side the lanes of a
// wave read consecutive doubles (conflict-free ds_read_b64) although each owns four consecutive outputs.
__device__ __forceinline__ int rv_at(int j) { return (j & (RV_R - 1)) * RV_PLANE + (j >> 2); }
static_assert(RV_R == 4, "rv_at and the unrolled window below are written for four outputs per lane");

// The tap walk of one tile: outputs k0 .. k0 + nk - 1 (nk >= 1) of the utterance x of n samples under the response h of `taps` taps,
// lane L owning k0 + 4 L + c, c < 4, in a0 .. a3 (which enter as 0).
// Chunk t0 needs x[k0 - t0 - (RV_TC - 1)] .. x[k0 + RV_BLOCK - 1 - t0]; samples before the utterance are staged as 0 (a tap
// beyond k adds fma(h, 0, acc), which leaves acc as it is), samples from n on - read only by outputs that are not stored - too.
// Chunks whose span lies before the utterance altogether are not walked, and no tap at or beyond `taps` is ever read.
// xs: the workgroup's RV_R * RV_PLANE doubles of LDS. Every thread of the workgroup calls it (barriers inside).
template <typename T>
__device__ __forceinline__ void rv_walk(double* __restrict__ xs, const T* __restrict__ x, int64_t n, int64_t k0, int nk,
                                        const double* __restrict__ h, int64_t taps, double& a0, double& a1, double& a2, double& a3) {
    const int tid = threadIdx.x;
    const int o = RV_R * tid;                                // first output of this lane inside the tile
    // taps that reach a sample of the utterance for some stored output of the tile: t <= k0 + nk - 1
    const int t_end = (int)min(taps, k0 + (int64_t)nk);
    for (int t0 = 0; t0 < t_end; t0 += RV_TC) {
        const int ns = min(RV_TC, t_end - t0);               // taps of this chunk
        const int64_t lo = k0 - (int64_t)t0 - RV_TC;         // utterance index of xs[0]
        __syncthreads();                                     // the previous chunk's readers are done
        for (int j = tid; j < RV_SPAN; j += RV_NT) {
            const int64_t i = lo + j;
            xs[rv_at(j)] = i >= 0 && i < n ? (double)x[i] : 0.0;
        }
        __syncthreads();
        // window at tap s of the chunk: w_c = xs[RV_TC + o + c - s]
        double w0 = xs[rv_at(RV_TC + o)], w1 = xs[rv_at(RV_TC + o + 1)], w2 = xs[rv_at(RV_TC + o + 2)],
               w3 = xs[rv_at(RV_TC + o + 3)];
        const double* __restrict__ hc = h + t0;
        // sample RV_TC + o - s - 1 enters at the bottom after tap s: plane (3 - s) & 3, place (RV_TC + o) / 4 - 1 - s / 4
        // Four taps from tap s of the chunk (s a multiple of four) with the four samples that enter at place q
        auto step4 = [&](int s, int q) {
            const double h0 = hc[s], h1 = hc[s + 1], h2 = hc[s + 2], h3 = hc[s + 3];
            const double n3 = xs[q + 3 * RV_PLANE], n2 = xs[q + 2 * RV_PLANE], n1 = xs[q + RV_PLANE], n0 = xs[q];
            a0 = fma(h0, w0, a0), a1 = fma(h0, w1, a1), a2 = fma(h0, w2, a2), a3 = fma(h0, w3, a3);
            a0 = fma(h1, n3, a0), a1 = fma(h1, w0, a1), a2 = fma(h1, w1, a2), a3 = fma(h1, w2, a3);
            a0 = fma(h2, n2, a0), a1 = fma(h2, n3, a1), a2 = fma(h2, w0, a2), a3 = fma(h2, w1, a3);
            a0 = fma(h3, n1, a0), a1 = fma(h3, n2, a1), a2 = fma(h3, n3, a2), a3 = fma(h3, w0, a3);
            w3 = n3, w2 = n2, w1 = n1, w0 = n0;
        };
        // Two steps per turn, so that the window comes back to its registers without moves. The second step's place goes
        // through an address register of its own that the compiler cannot relate to the first (the empty asm): it would pair
        // reads 8 bytes apart into ds_read2_b64, a quarter of the rate again.
        int qa = (RV_TC + o) / RV_R - 1, qb = qa - 1;
        asm volatile("" : "+v"(qb));
        int s = 0;
        for (; s + 2 * RV_R <= ns; s += 2 * RV_R, qa -= 2, qb -= 2) {
            step4(s, qa);
            step4(s + RV_R, qb);
        }
        if (s + RV_R <= ns) {
            step4(s, qa);
            s += RV_R;
        }
        for (; s < ns; ++s) {                                // the last taps of a response that is no multiple of four
            const double hs = hc[s];
            a0 = fma(hs, w0, a0), a1 = fma(hs, w1, a1), a2 = fma(hs, w2, a2), a3 = fma(hs, w3, a3);
            w3 = w2, w2 = w1, w1 = w0, w0 = xs[rv_at(RV_TC + o - s - 1)];
        }
    }
}

// Workgroup (blockIdx.x, l = blockIdx.y) serves outputs k0 .. k0 + RV_BLOCK - 1 of the utterance b with first[b] <= blockIdx.x <
// first[b + 1] (first: running sums of the utterances' tiles; an empty utterance has none). Lane L owns k0 + 4 L + c, c < 4.
template <typename T>
__global__ __launch_bounds__(RV_NT) void k_reverb_levels(const T* __restrict__ wave, const int64_t* __restrict__ offsets,
                                                          const int64_t* __restrict__ first, int B, const double* __restrict__ rir,
                                                          const int64_t* __restrict__ rir_offsets, int K, int64_t total,
                                                          double* __restrict__ out) {
    __shared__ double xs[RV_R * RV_PLANE];
    const int tid = threadIdx.x;
    const int l = blockIdx.y;
    const int64_t blk = blockIdx.x;
    int b = 0, hi = B;      // first[b] <= blk < first[hi]
    while (hi - b > 1) {
        const int mid = (b + hi) >> 1;
        if (first[mid] <= blk) b = mid;
        else hi = mid;
    }
    const int64_t n = offsets[b + 1] - offsets[b];
    const int64_t k0 = (blk - first[b]) * RV_BLOCK;
    const int nk = (int)min((int64_t)RV_BLOCK, n - k0);      // outputs of this workgroup, >= 1
    const T* __restrict__ x = wave + offsets[b];
    double* __restrict__ y = out + (size_t)l * (size_t)total + (size_t)offsets[b] + (size_t)k0;
    const int o = RV_R * tid;                                // first output of this lane inside the tile
    if (l == K) {                                            // the dry level: the samples themselves
#pragma unroll
        for (int c = 0; c < RV_R; ++c)
            if (o + c < nk) y[o + c] = (double)x[k0 + o + c];
        return;
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    rv_walk(xs, x, n, k0, nk, rir + rir_offsets[l], rir_offsets[l + 1] - rir_offsets[l], a0, a1, a2, a3);
    if (o < nk) y[o] = a0;
    if (o + 1 < nk) y[o + 1] = a1;
    if (o + 2 < nk) y[o + 2] = a2;
    if (o + 3 < nk) y[o + 3] = a3;
}

// One room per utterance, the output in the layout of the waves. Workgroup blockIdx.x serves the tile tiles[blockIdx.x] =
// utterance << 32 | tile index of the utterance (a list from the host, so that no workgroup searches and the expensive tiles can
// start first); the utterance runs at room[b] in [0, K], K the dry one; room == NULL: every utterance is dry. The same walk, the
// same bits as level room[b] of k_reverb_levels.
template <typename T>
__global__ __launch_bounds__(RV_NT) void k_reverb_pick(const T* __restrict__ wave, const int64_t* __restrict__ offsets,
                                                        const int64_t* __restrict__ tiles, const double* __restrict__ rir,
                                                        const int64_t* __restrict__ rir_offsets, const int32_t* __restrict__ room, int K,
                                                        double* __restrict__ out) {
    __shared__ double xs[RV_R * RV_PLANE];
    const int tid = threadIdx.x;
    const int64_t entry = tiles[blockIdx.x];
    const int b = (int)(entry >> 32);
    const int l = room ? room[b] : K;
    const int64_t n = offsets[b + 1] - offsets[b];
    const int64_t k0 = (entry & 0xffffffffll) * RV_BLOCK;
    const int nk = (int)min((int64_t)RV_BLOCK, n - k0);      // outputs of this workgroup, >= 1
    const T* __restrict__ x = wave + offsets[b];
    double* __restrict__ y = out + (size_t)offsets[b] + (size_t)k0;
    const int o = RV_R * tid;
    if (l == K) {                                            // a dry utterance: the samples themselves
#pragma unroll
        for (int c = 0; c < RV_R; ++c)
            if (o + c < nk) y[o + c] = (double)x[k0 + o + c];
        return;
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    rv_walk(xs, x, n, k0, nk, rir + rir_offsets[l], rir_offsets[l + 1] - rir_offsets[l], a0, a1, a2, a3);
    if (o < nk) y[o] = a0;
    if (o + 1 < nk) y[o + 1] = a1;
    if (o + 2 < nk) y[o + 2] = a2;
    if (o + 3 < nk) y[o + 3] = a3;
}

}  // namespace

int f2_check_rir(f2_ctx* ctx, const double* rir, const int64_t* rir_offsets, int K) {
    F2_CHECK(ctx, K >= 1 && rir && rir_offsets, F2_ERR_INVALID,
             "a sweep needs at least one impulse response (K=%d), their taps and their rir_offsets", K);
    F2_CHECK(ctx, K <= F2_REVERB_MAX_LEVELS, F2_ERR_UNSUPPORTED, "%d impulse responses (at most %d)", K, F2_REVERB_MAX_LEVELS);
    F2_CHECK(ctx, rir_offsets[0] == 0, F2_ERR_INVALID, "rir_offsets[0] must be 0");
    for (int l = 0; l < K; ++l) {
        const int64_t taps = rir_offsets[l + 1] - rir_offsets[l];
        F2_CHECK(ctx, taps >= 0, F2_ERR_INVALID, "rir_offsets must be non-decreasing (l=%d)", l);
        F2_CHECK(ctx, taps >= 1, F2_ERR_INVALID, "impulse response %d has no taps", l);
    }
    for (int l = 0; l < K; ++l) {
        const int64_t taps = rir_offsets[l + 1] - rir_offsets[l];
        F2_CHECK(ctx, taps <= F2_REVERB_MAX_TAPS, F2_ERR_UNSUPPORTED, "impulse response %d has %lld taps (at most %d)", l,
                 (long long)taps, F2_REVERB_MAX_TAPS);
    }
    for (int l = 0; l < K; ++l)
        for (int64_t t = rir_offsets[l]; t < rir_offsets[l + 1]; ++t)
            F2_CHECK(ctx, std::isfinite(rir[t]), F2_ERR_INVALID, "tap %lld of impulse response %d is not finite",
                     (long long)(t - rir_offsets[l]), l);
    return F2_OK;
}

void f2_reverb_meta(f2_meta_carve* meta, int B, const int64_t* rir_offsets, int K, f2_reverb_arrays* A) {
    meta->add(&A->d_first, (size_t)B + 1), meta->add(&A->d_rir_off, (size_t)K + 1), meta->add(&A->d_rir, (size_t)rir_offsets[K]);
}

int f2_launch_reverb_levels(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const int64_t* h_offsets, int B,
                            const double* rir, const int64_t* rir_offsets, int K, const f2_reverb_arrays& A, double* d_out) {
    const int64_t total = h_offsets[B];
    if (B == 0 || total == 0) return F2_OK;
    std::vector<int64_t> first((size_t)B + 1, 0);
    for (int b = 0; b < B; ++b) first[(size_t)b + 1] = first[(size_t)b] + (h_offsets[b + 1] - h_offsets[b] + RV_BLOCK - 1) / RV_BLOCK;
    const int64_t tiles = first[(size_t)B];
    F2_CHECK(ctx, tiles < (int64_t(1) << 31), F2_ERR_UNSUPPORTED, "reverberation needs %lld workgroups per level (at most 2^31 - 1)",
             (long long)tiles);
    // d_first and d_rir_off were named in a row (f2_reverb_meta): one upload for both
    first.insert(first.end(), rir_offsets, rir_offsets + K + 1);
    F2_TRY(f2_upload_async(ctx, A.d_first, first.data(), sizeof(int64_t) * first.size()));
    F2_TRY(f2_upload_async(ctx, A.d_rir, rir, sizeof(double) * (size_t)rir_offsets[K]));
    const dim3 grid((unsigned)tiles, (unsigned)(K + 1));
    if (wave_dtype == F2_WAVE_I16)
        k_reverb_levels<int16_t><<<grid, dim3(RV_NT), 0, ctx->stream>>>((const int16_t*)d_wave, d_offsets, A.d_first, B, A.d_rir,
                                                                       A.d_rir_off, K, total, d_out);
    else
        k_reverb_levels<double><<<grid, dim3(RV_NT), 0, ctx->stream>>>((const double*)d_wave, d_offsets, A.d_first, B, A.d_rir,
                                                                      A.d_rir_off, K, total, d_out);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

extern "C" int f2_reverb_levels(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, int B, const double* rir,
                                const int64_t* rir_offsets, int K, double* levels, int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_CHECK(ctx, B >= 0, F2_ERR_INVALID, "bad batch size (B=%d)", B);
    F2_TRY(f2_check_wave_dtype(ctx, wave_dtype));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_TRY(f2_check_offsets(ctx, offsets, B, "offsets"));
    F2_TRY(f2_check_rir(ctx, rir, rir_offsets, K));
    F2_CHECK(ctx, ((int64_t)K + 1) * (B > 0 ? B : 1) <= INT32_MAX / 2, F2_ERR_UNSUPPORTED, "%d levels of %d utterances", K + 1, B);
    const int64_t total = offsets[B];
    if (B == 0 || total == 0) return F2_OK;
    F2_CHECK(ctx, wave && levels, F2_ERR_INVALID, "null data pointer");
    f2_reverb_arrays A;
    f2_meta_carve meta;
    f2_reverb_meta(&meta, B, rir_offsets, K, &A);
    F2_TRY(meta.reserve(ctx));
    f2_output out;
    F2_TRY(f2_place(ctx, ctx->levels, levels, sizeof(double) * ((size_t)K + 1) * (size_t)total, mem_space, true, &out));
    const void* d_wave;
    F2_TRY(f2_stage_wave(ctx, wave, wave_dtype, total, mem_space, &d_wave));
    F2_TRY(f2_upload_offsets(ctx, offsets, B));
    F2_TRY(f2_launch_reverb_levels(ctx, d_wave, wave_dtype, (const int64_t*)ctx->offsets.ptr, offsets, B, rir, rir_offsets, K, A,
                                   out.as<double>()));
    F2_TRY(f2_copy_back(ctx, out));
    return f2_host_wait(ctx, mem_space);
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

static int64_t rv_tiles(const int64_t* h_offsets, int B) {
    int64_t tiles = 0;
    for (int b = 0; b < B; ++b) tiles += (h_offsets[b + 1] - h_offsets[b] + RV_BLOCK - 1) / RV_BLOCK;
    return tiles;
}

void f2_reverb_pick_meta(f2_meta_carve* meta, int B, const int64_t* h_offsets, const f2_reverb_pick_args& R, f2_reverb_pick_arrays* A) {
    meta->add(&A->d_tiles, (size_t)rv_tiles(h_offsets, B));
    if (R.dry()) return;
    meta->add(&A->d_room, ((size_t)B + 1) / 2);
    if (!R.d_rir) meta->add(&A->d_rir_off, (size_t)R.K + 1), meta->add(&A->d_rir, (size_t)R.rir_offsets[R.K]);
}

int f2_launch_reverb_pick(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const int64_t* h_offsets, int B,
                          const f2_reverb_pick_args& R, const f2_reverb_pick_arrays& A, double* d_out) {
    if (B == 0 || h_offsets[B] == 0) return F2_OK;
    const int64_t ntiles = rv_tiles(h_offsets, B);
    F2_CHECK(ctx, ntiles < (int64_t(1) << 31), F2_ERR_UNSUPPORTED, "reverberation needs %lld workgroups (at most 2^31 - 1)",
             (long long)ntiles);
    const bool dry = R.dry();
    // the tile list, utterance << 32 | tile, in (utterance, tile) order ...
    std::vector<int64_t> tiles;
    std::vector<int32_t> cost;   // taps the tile walks: min(T_room, k0 + nk), 0 for a dry utterance
    tiles.reserve((size_t)ntiles);
    for (int b = 0; b < B; ++b) {
        const int64_t n = h_offsets[b + 1] - h_offsets[b], nt = (n + RV_BLOCK - 1) / RV_BLOCK;
        const int l = dry ? R.K : R.room_of[b];
        const int64_t taps = l < R.K ? R.rir_offsets[l + 1] - R.rir_offsets[l] : 0;
        for (int64_t i = 0; i < nt; ++i) {
            tiles.push_back((int64_t)b << 32 | i);
            if (!dry && ctx->opt_reverb_pick_sort) cost.push_back((int32_t)std::min(taps, std::min(n, (i + 1) * RV_BLOCK)));
        }
    }
    // ... or most taps first, ties in that order: the tiles that run longest do not start last. The results do not depend on it.
    if (!cost.empty()) {
        std::vector<int32_t> idx((size_t)ntiles);
        for (int64_t i = 0; i < ntiles; ++i) idx[(size_t)i] = (int32_t)i;
        std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t c) { return cost[(size_t)a] > cost[(size_t)c]; });
        std::vector<int64_t> sorted((size_t)ntiles);
        for (int64_t i = 0; i < ntiles; ++i) sorted[(size_t)i] = tiles[(size_t)idx[(size_t)i]];
        tiles.swap(sorted);
    }
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
        k_reverb_pick<int16_t><<<grid, dim3(RV_NT), 0, ctx->stream>>>((const int16_t*)d_wave, d_offsets, A.d_tiles, d_rir, d_rir_off, d_room,
                                                                     R.K, d_out);
    else
        k_reverb_pick<double><<<grid, dim3(RV_NT), 0, ctx->stream>>>((const double*)d_wave, d_offsets, A.d_tiles, d_rir, d_rir_off, d_room,
                                                                    R.K, d_out);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

extern "C" int f2_reverb_pick(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, int B, const double* rir,
                              const int64_t* rir_offsets, int K, const int32_t* room_of, double* wet, int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_CHECK(ctx, B >= 0, F2_ERR_INVALID, "bad batch size (B=%d)", B);
    F2_TRY(f2_check_wave_dtype(ctx, wave_dtype));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_TRY(f2_check_offsets(ctx, offsets, B, "offsets"));
    const f2_reverb_pick_args R = {rir, rir_offsets, K, room_of, nullptr, nullptr};
    F2_TRY(f2_check_reverb_pick(ctx, B, R));
    const int64_t total = offsets[B];
    if (B == 0 || total == 0) return F2_OK;
    F2_CHECK(ctx, wave && wet, F2_ERR_INVALID, "null data pointer");
    f2_reverb_pick_arrays A;
    f2_meta_carve meta;
    f2_reverb_pick_meta(&meta, B, offsets, R, &A);
    F2_TRY(meta.reserve(ctx));
    f2_output out;
    F2_TRY(f2_place(ctx, ctx->wet, wet, sizeof(double) * (size_t)total, mem_space, true, &out));
    const void* d_wave;
    F2_TRY(f2_stage_wave(ctx, wave, wave_dtype, total, mem_space, &d_wave));
    F2_TRY(f2_upload_offsets(ctx, offsets, B));
    F2_TRY(f2_launch_reverb_pick(ctx, d_wave, wave_dtype, (const int64_t*)ctx->offsets.ptr, offsets, B, R, A, out.as<double>()));
    F2_TRY(f2_copy_back(ctx, out));
    return f2_host_wait(ctx, mem_space);
}
