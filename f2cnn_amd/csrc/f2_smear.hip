// Linear maps across the channels of envelopes that are already in memory, at K mixing matrices in one pass (include/f2cnn_hip.h:
// f2_channel_mix_levels; the kernel of f2_eval_smear_sweep).
//   k_channel_mix_levels  out[l][b][c][i] = sum_{c'} mix[l][c][c'] env[b][c'][i] in float64. One workgroup per (tile of
//                         F2_SMEAR_TILE_SAMPLES samples of one utterance, level, tile of F2_SMEAR_TILE_CHANNELS output channels);
//                         level K copies the tile. Lanes run along time: a lane owns SM_SPL samples, SM_NT apart, and
//                         F2_SMEAR_TILE_CHANNELS accumulators for each. Per input channel c' of the tile's span - the union of the
//                         supports of its rows - it loads its SM_SPL envelope values once (consecutive lanes, consecutive doubles:
//                         rows may start at any 8-byte boundary) and feeds them to all its accumulators; the weights of that step,
//                         mix[l][c0 .. c0 + 15][c'], are wave-uniform and lie side by side in the transposed, zero-padded image the
//                         host uploads, so they come through the scalar load path and enter the FMAs as the scalar operand.
// Arithmetic contract of the header: one float64 accumulator per output starting from +0.0, c' ascending, acc = fma(w, x, acc), no
// atomics, no sum split across lanes. The span of a tile can be wider than the support of a row; outside its support the row's
// weights are zero by the definition of a support, and fma(0, x, acc) leaves acc as it is for finite x - up to the sign of a zero,
// which the closing acc + 0.0 settles (a zero is stored as +0.0). gfx950, wave64; plain vector stores only.
#include "f2_internal.h"
#include "f2_tile_owner.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int SM_NT = 256;                              // threads of a workgroup
constexpr int SM_SPL = 2;                               // samples of a lane, SM_NT apart
constexpr int SM_TS = F2_SMEAR_TILE_SAMPLES;            // samples of a workgroup
constexpr int SM_TC = F2_SMEAR_TILE_CHANNELS;           // output channels of a workgroup = accumulators per lane and sample
static_assert(SM_TS == SM_NT * SM_SPL, "a lane owns SM_SPL samples of the tile");
static_assert(SM_SPL == 2, "the two accumulator rows below are written out");
constexpr unsigned SM_XCDS = 8;                         // dies a launch is dealt over

// Tile id = (time tile * (K + 1) + l) * nct + ct, channel tiles fastest: the workgroups that read the same input tile - all channel
// tiles of all levels - have neighbouring ids. Workgroups are dealt round-robin over the chip's SM_XCDS dies, each with an L2 of its
// own, so workgroup w takes tile id (w % SM_XCDS) * (gridDim.x / SM_XCDS) + w / SM_XCDS: one die then walks a contiguous range of
// ids, and an input tile is fetched into one L2 instead of all of them (for speed only: any placement computes the same; the grid is
// padded to a multiple of SM_XCDS and ids from `tiles` on have nothing to do). Time tile t serves samples k0 .. k0 + SM_TS - 1 of the utterance that owns it
// (tile_owner over `first`). Lane L owns k0 + L and k0 + L + SM_NT; a lane beyond the
// utterance's end reads its last sample instead (never stored). wT: per level C rows of Cpad doubles, wT[l][c'][c] =
// mix[l][c][c'], zero for c >= C; spans[l * nct + ct] = lo | hi << 32, the input channels lo .. hi - 1 the tile walks.
__global__ __launch_bounds__(SM_NT) void k_channel_mix_levels(const double* __restrict__ env, const int64_t* __restrict__ offsets,
                                                               const int64_t* __restrict__ first, int B, int C, int Cpad, int nct,
                                                               const double* __restrict__ wT, const int64_t* __restrict__ spans,
                                                               int K, unsigned tiles, int64_t level_stride, double* __restrict__ out) {
    const int tid = threadIdx.x;
    const unsigned id = (blockIdx.x % SM_XCDS) * (gridDim.x / SM_XCDS) + blockIdx.x / SM_XCDS;
    if (id >= tiles) return;
    const unsigned per = (unsigned)nct * (unsigned)(K + 1);
    const unsigned t = id / per, r = id - t * per;
    const int l = (int)(r / (unsigned)nct), ct = (int)(r - (unsigned)l * (unsigned)nct);
    const int b = tile_owner(first, B, (int64_t)t);
    const int64_t n = offsets[b + 1] - offsets[b];
    const int64_t k0 = ((int64_t)t - first[b]) * SM_TS;
    const int64_t i0 = k0 + tid, i1 = i0 + SM_NT;                  // k0 < n: the tile has at least one sample
    const int64_t j0 = i0 < n ? i0 : n - 1, j1 = i1 < n ? i1 : n - 1;
    const double* __restrict__ x = env + (size_t)C * (size_t)offsets[b];          // row c' at x + c' * n
    double* __restrict__ y = out + (size_t)l * (size_t)level_stride + (size_t)C * (size_t)offsets[b];
    const int c0 = ct * SM_TC;
    if (l == K) {                                                  // the copy level
#pragma unroll 4
        for (int q = 0; q < SM_TC; ++q) {
            const int c = c0 + q;
            if (c >= C) break;
            const double v0 = x[(size_t)c * (size_t)n + (size_t)j0], v1 = x[(size_t)c * (size_t)n + (size_t)j1];
            if (i0 < n) y[(size_t)c * (size_t)n + (size_t)i0] = v0;
            if (i1 < n) y[(size_t)c * (size_t)n + (size_t)i1] = v1;
        }
        return;
    }
    const int64_t span = spans[(size_t)l * (size_t)nct + (size_t)ct];
    const int lo = (int)(span & 0xffffffff), hi = (int)(span >> 32);
    const double* __restrict__ w = wT + (size_t)l * (size_t)C * (size_t)Cpad + (size_t)c0;   // weights of step c' at w + c' * Cpad
    double a0[SM_TC], a1[SM_TC];
#pragma unroll
    for (int q = 0; q < SM_TC; ++q) a0[q] = a1[q] = 0.0;
    const double* __restrict__ x0 = x + (size_t)j0;
    const double* __restrict__ x1 = x + (size_t)j1;
    // two steps per turn: their four loads are issued together, and the second step's are in flight while the first is summed
#pragma unroll 2
    for (int cp = lo; cp < hi; ++cp) {
        const double v0 = x0[(size_t)cp * (size_t)n], v1 = x1[(size_t)cp * (size_t)n];
        const double* __restrict__ wr = w + (size_t)cp * (size_t)Cpad;
#pragma unroll
        for (int q = 0; q < SM_TC; ++q) {
            const double wq = wr[q];
            a0[q] = fma(wq, v0, a0[q]);
            a1[q] = fma(wq, v1, a1[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < SM_TC; ++q) {
        const int c = c0 + q;
        if (c < C) {
            if (i0 < n) y[(size_t)c * (size_t)n + (size_t)i0] = a0[q] + 0.0;
            if (i1 < n) y[(size_t)c * (size_t)n + (size_t)i1] = a1[q] + 0.0;
        }
    }
}

}  // namespace

int f2_check_mix(f2_ctx* ctx, const double* mix, int K, int C, f2_smear_plan* P) {
    F2_CHECK(ctx, K >= 1 && mix, F2_ERR_INVALID, "a sweep needs at least one mixing matrix (K=%d) and their weights", K);
    F2_CHECK(ctx, K <= F2_SMEAR_MAX_LEVELS, F2_ERR_UNSUPPORTED, "%d mixing matrices (at most %d)", K, F2_SMEAR_MAX_LEVELS);
    F2_CHECK(ctx, C <= F2_SMEAR_MAX_CHANNELS, F2_ERR_UNSUPPORTED, "mixing matrices of %d channels (at most %d)", C, F2_SMEAR_MAX_CHANNELS);
    const int nct = (C + SM_TC - 1) / SM_TC, Cpad = nct * SM_TC;
    P->K = K, P->C = C, P->Cpad = Cpad, P->nct = nct;
    P->wT.assign((size_t)K * (size_t)C * (size_t)Cpad, 0.0);
    P->spans.assign((size_t)K * (size_t)nct, 0);
    for (int l = 0; l < K; ++l)
        for (int ct = 0; ct < nct; ++ct) {
            int64_t ulo = C, uhi = 0;                   // union of the supports of the tile's rows
            for (int c = ct * SM_TC; c < C && c < (ct + 1) * SM_TC; ++c) {
                const double* row = mix + ((size_t)l * (size_t)C + (size_t)c) * (size_t)C;
                int64_t lo = C, hi = 0;                 // the row's support: first and one past the last non-zero weight
                for (int cp = 0; cp < C; ++cp) {
                    F2_CHECK(ctx, std::isfinite(row[cp]), F2_ERR_INVALID, "weight [%d][%d][%d] of the mixing matrices is not finite", l, c, cp);
                    if (row[cp] != 0.0) {
                        lo = std::min(lo, (int64_t)cp), hi = cp + 1;
                        P->wT[((size_t)l * (size_t)C + (size_t)cp) * (size_t)Cpad + (size_t)c] = row[cp];
                    }
                }
                ulo = std::min(ulo, lo), uhi = std::max(uhi, hi);
            }
            if (uhi <= ulo) ulo = uhi = 0;              // rows of zeros only: nothing to walk
            P->spans[(size_t)l * (size_t)nct + (size_t)ct] = ulo | (uhi << 32);
        }
    return F2_OK;
}

int f2_smear_reserve(f2_ctx* ctx, const f2_smear_plan& P, int B) {
    return f2_reserve(ctx, ctx->mix, sizeof(int64_t) * ((size_t)B + 1 + P.spans.size()) + sizeof(double) * P.wT.size());
}

int f2_launch_channel_mix_levels(f2_ctx* ctx, const double* d_env, const int64_t* d_offsets, const int64_t* h_offsets, int B,
                                 const f2_smear_plan& P, double* d_levels) {
    const int64_t total = h_offsets[B];
    if (B == 0 || total == 0) return F2_OK;
    std::vector<int64_t> small;                        // [running sums of the utterances' tiles | spans]
    const int64_t tiles = f2_tile_table(h_offsets, B, SM_TS, &small) * (int64_t)P.nct * (P.K + 1);
    const int64_t blocks = (tiles + SM_XCDS - 1) / SM_XCDS * SM_XCDS;
    F2_TRY(f2_check_workgroups(ctx, blocks, "the channel mix", ""));
    small.insert(small.end(), P.spans.begin(), P.spans.end());
    int64_t* d_first = (int64_t*)ctx->mix.ptr;
    int64_t* d_spans = d_first + B + 1;
    double* d_wT = (double*)(d_spans + P.spans.size());
    F2_TRY(f2_upload_async(ctx, d_first, small.data(), sizeof(int64_t) * small.size()));
    F2_TRY(f2_upload_async(ctx, d_wT, P.wT.data(), sizeof(double) * P.wT.size()));
    k_channel_mix_levels<<<dim3((unsigned)blocks), dim3(SM_NT), 0, ctx->stream>>>(d_env, d_offsets, d_first, B, P.C, P.Cpad, P.nct, d_wT,
                                                                                 d_spans, P.K, (unsigned)tiles, (int64_t)P.C * total, d_levels);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

extern "C" int f2_channel_mix_levels(f2_ctx* ctx, const double* env, const int64_t* offsets, int B, int C, const double* mix, int K,
                                     double* levels, int mem_space) {
    f2_smear_plan P;
    return f2_stage_call(
        ctx, offsets, B, mem_space,
        [&]() -> int {
            F2_TRY(f2_check_batch(ctx, offsets, B, C, mem_space, true));
            F2_TRY(f2_check_mix(ctx, mix, K, C, &P));
            F2_CHECK(ctx, (int64_t)B * C <= INT32_MAX, F2_ERR_UNSUPPORTED, "%d utterances of %d channels", B, C);
            return F2_OK;
        },
        [&](f2_meta_carve*) { return f2_smear_reserve(ctx, P, B); }, env,
        [&](int64_t total, const void** d_env) { return f2_stage_input(ctx, env, sizeof(double) * (size_t)C * (size_t)total, mem_space, d_env); },
        &f2_ctx::levels, levels, sizeof(double) * (size_t)C * ((size_t)K + 1),
        [&](const void* d_env, const int64_t* d_offsets, int64_t, double* d_out) {
            return f2_launch_channel_mix_levels(ctx, (const double*)d_env, d_offsets, offsets, B, P, d_out);
        });
}
