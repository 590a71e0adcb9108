// Coloured noise on a ragged batch at K levels in one pass (include/f2cnn_hip.h: f2_shaped_noise_levels; the kernel of
// f2_eval_shaped_noise_sweep).
//   k_shaped_noise_levels  noisy[l][b][i] = clean_b[i] + sigma[l][b] * sum_{t < T_l} h_l[t] z(seed, l, b, i - t), the direct form in
//                          float64. One workgroup per (output tile of F2_SHAPED_BLOCK samples, level); level K, and a level whose
//                          sigma is 0, copies the clean samples. The deviates of the tile's whole span [k0 - (T_l - 1), k0 + nk) are
//                          generated once into LDS as float64 (the index wraps below zero as a 64-bit counter: deviates like any
//                          others), then every lane slides a register window of its SN_R consecutive outputs over them - one 8-byte
//                          LDS read and SN_R FMAs per tap, the tap itself a wave-uniform load from global memory: the walk of rv_walk
//                          (f2_reverb.hip) over one chunk that holds every tap.
// Arithmetic contract of the header: one float64 accumulator per output, taps in ascending t, acc = fma(h[t], z[i - t], acc), no
// atomics, no sum split across lanes; then clean + sigma * acc, product and sum rounded separately. sigma comes from k_noise_sigma
// (f2_noise.hip), unchanged. gfx950, wave64; plain vector stores only.
#include "f2_internal.h"
#include "f2_philox.h"

#include <cmath>

namespace {

constexpr int SN_NT = 256;                          // threads of a workgroup
constexpr int SN_R = 4;                             // consecutive outputs of a lane
constexpr int SN_BLOCK = F2_SHAPED_BLOCK;           // outputs of a workgroup
constexpr int SN_SPAN = SN_BLOCK + F2_SHAPED_MAX_TAPS;   // most staged deviates: zs[j] = z[k0 - tc + j], tc = taps rounded up to SN_R
// LDS image as in f2_reverb.hip: deviate j at plane j % SN_R, place j / SN_R; the odd pitch keeps the compiler from pairing the four
// reads of a step into ds_read2st64_b64.
constexpr int SN_PLANE = SN_SPAN / SN_R + 1;
static_assert(SN_BLOCK == SN_NT * SN_R, "a lane owns SN_R consecutive outputs of the tile");
static_assert(F2_SHAPED_MAX_TAPS % SN_R == 0, "the rounded tap count stays inside the span");
static_assert(SN_R * SN_PLANE * sizeof(double) <= 64 * 1024, "one span in LDS");
static_assert(SN_R == 4, "sn_at and the unrolled window below are written for four outputs per lane");

__device__ __forceinline__ int sn_at(int j) { return (j & (SN_R - 1)) * SN_PLANE + (j >> 2); }

// The work of one tile: c[k] = sum_{t < taps} h[t] z(seed, level, utt, k - t) for the outputs k0 .. k0 + nk - 1 (1 <= nk <= SN_BLOCK)
// of utterance number `utt` at `level`, lane L owning k0 + 4 L + c, c < 4, in a0 .. a3 (which enter as 0; those of outputs from nk
// on are not meaningful). zs: the workgroup's SN_R * SN_PLANE doubles of LDS. Every thread of the workgroup calls it (a barrier
// inside). 1 <= taps <= F2_SHAPED_MAX_TAPS; no tap at or beyond `taps` is read.
__device__ __forceinline__ void sn_tile(double* __restrict__ zs, uint64_t seed, uint32_t level, uint32_t utt, int64_t k0, int nk,
                                        const double* __restrict__ h, int taps, double& a0, double& a1, double& a2, double& a3) {
    const int tid = threadIdx.x;
    const int o = SN_R * tid;                                // first output of this lane inside the tile
    const int tc = (taps + SN_R - 1) & ~(SN_R - 1);          // the register window turns once per SN_R taps
    const uint64_t lo = (uint64_t)k0 - (uint64_t)tc;         // sample index of zs[0], modulo 2^64
    const int span = tc + nk;
    for (int j = tid; j < span; j += SN_NT) zs[sn_at(j)] = noise_deviate(seed, level, utt, lo + (uint64_t)j);
    __syncthreads();
    if (o >= nk) return;                                     // (behind the only barrier)
    // window at tap s: w_c = zs[tc + o + c - s]
    double w0 = zs[sn_at(tc + o)], w1 = zs[sn_at(tc + o + 1)], w2 = zs[sn_at(tc + o + 2)], w3 = zs[sn_at(tc + o + 3)];
    // Four taps from tap s (a multiple of four) with the four deviates that enter at place q
    auto step4 = [&](int s, int q) {
        const double h0 = h[s], h1 = h[s + 1], h2 = h[s + 2], h3 = h[s + 3];
        const double n3 = zs[q + 3 * SN_PLANE], n2 = zs[q + 2 * SN_PLANE], n1 = zs[q + SN_PLANE], n0 = zs[q];
        a0 = fma(h0, w0, a0), a1 = fma(h0, w1, a1), a2 = fma(h0, w2, a2), a3 = fma(h0, w3, a3);
        a0 = fma(h1, n3, a0), a1 = fma(h1, w0, a1), a2 = fma(h1, w1, a2), a3 = fma(h1, w2, a3);
        a0 = fma(h2, n2, a0), a1 = fma(h2, n3, a1), a2 = fma(h2, w0, a2), a3 = fma(h2, w1, a3);
        a0 = fma(h3, n1, a0), a1 = fma(h3, n2, a1), a2 = fma(h3, n3, a2), a3 = fma(h3, w0, a3);
        w3 = n3, w2 = n2, w1 = n1, w0 = n0;
    };
    // Two steps per turn, the second through an address register of its own (the empty asm), as in rv_walk: the reads stay single
    // ds_read_b64.
    int qa = (tc + o) / SN_R - 1, qb = qa - 1;
    asm volatile("" : "+v"(qb));
    int s = 0;
    for (; s + 2 * SN_R <= taps; s += 2 * SN_R, qa -= 2, qb -= 2) {
        step4(s, qa);
        step4(s + SN_R, qb);
    }
    if (s + SN_R <= taps) {
        step4(s, qa);
        s += SN_R;
    }
    for (; s < taps; ++s) {                                  // the last taps of a filter that is no multiple of four
        const double hs = h[s];
        a0 = fma(hs, w0, a0), a1 = fma(hs, w1, a1), a2 = fma(hs, w2, a2), a3 = fma(hs, w3, a3);
        w3 = w2, w2 = w1, w1 = w0, w0 = zs[sn_at(tc + o - s - 1)];
    }
}

// Workgroup (blockIdx.x, l = blockIdx.y) serves outputs k0 .. k0 + SN_BLOCK - 1 of the utterance b with first[b] <= blockIdx.x <
// first[b + 1] (first: running sums of the utterances' tiles; an empty utterance has none). Lane L owns k0 + 4 L + c, c < 4.
template <typename T>
__global__ __launch_bounds__(SN_NT) void k_shaped_noise_levels(const T* __restrict__ wave, const int64_t* __restrict__ offsets,
                                                                const int64_t* __restrict__ first, int B,
                                                                const double* __restrict__ sigma, const double* __restrict__ fir,
                                                                const int64_t* __restrict__ fir_offsets, int K, int64_t total,
                                                                uint64_t seed, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double zs[SN_R * SN_PLANE];
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
    const int64_t k0 = (blk - first[b]) * SN_BLOCK;
    const int nk = (int)min((int64_t)SN_BLOCK, n - k0);      // outputs of this workgroup, >= 1
    const T* __restrict__ x = wave + offsets[b] + k0;
    double* __restrict__ y = out + (size_t)l * (size_t)total + (size_t)offsets[b] + (size_t)k0;
    const int o = SN_R * tid;                                // first output of this lane inside the tile
    const double s = l < K ? sigma[(size_t)l * B + b] : 0.0;
    if (s == 0.0) {                                          // the clean level, an all-zero utterance: the samples themselves
#pragma unroll
        for (int c = 0; c < SN_R; ++c)
            if (o + c < nk) y[o + c] = (double)x[o + c];
        return;
    }
    double a[SN_R] = {0.0, 0.0, 0.0, 0.0};
    sn_tile(zs, seed, (uint32_t)l, (uint32_t)b, k0, nk, fir + fir_offsets[l], (int)(fir_offsets[l + 1] - fir_offsets[l]), a[0], a[1], a[2],
            a[3]);
#pragma unroll
    for (int c = 0; c < SN_R; ++c)
        if (o + c < nk) {
            const double nz = s * a[c];
            y[o + c] = (double)x[o + c] + nz;
        }
}

}  // namespace

int f2_check_fir(f2_ctx* ctx, const double* snr_db, const double* fir, const int64_t* fir_offsets, int K) {
    F2_CHECK(ctx, K >= 1 && snr_db, F2_ERR_INVALID, "a sweep needs at least one noise level (K=%d) and their snr_db", K);
    for (int k = 0; k < K; ++k) F2_CHECK(ctx, std::isfinite(snr_db[k]), F2_ERR_INVALID, "snr_db[%d] is not finite", k);
    F2_CHECK(ctx, fir && fir_offsets, F2_ERR_INVALID, "a coloured sweep needs the taps of its %d levels (fir) and their fir_offsets", K);
    F2_CHECK(ctx, K <= F2_SHAPED_MAX_LEVELS, F2_ERR_UNSUPPORTED, "%d noise levels (at most %d)", K, F2_SHAPED_MAX_LEVELS);
    F2_CHECK(ctx, fir_offsets[0] == 0, F2_ERR_INVALID, "fir_offsets[0] must be 0 (level 0)");
    for (int l = 0; l < K; ++l) {
        const int64_t taps = fir_offsets[l + 1] - fir_offsets[l];
        F2_CHECK(ctx, taps >= 0, F2_ERR_INVALID, "fir_offsets must be non-decreasing (level %d)", l);
        F2_CHECK(ctx, taps >= 1, F2_ERR_INVALID, "the filter of level %d has no taps", l);
    }
    for (int l = 0; l < K; ++l) {
        const int64_t taps = fir_offsets[l + 1] - fir_offsets[l];
        F2_CHECK(ctx, taps <= F2_SHAPED_MAX_TAPS, F2_ERR_UNSUPPORTED, "the filter of level %d has %lld taps (at most %d)", l,
                 (long long)taps, F2_SHAPED_MAX_TAPS);
    }
    for (int l = 0; l < K; ++l)
        for (int64_t t = fir_offsets[l]; t < fir_offsets[l + 1]; ++t)
            F2_CHECK(ctx, std::isfinite(fir[t]), F2_ERR_INVALID, "tap %lld of the filter of level %d is not finite",
                     (long long)(t - fir_offsets[l]), l);
    return F2_OK;
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
    std::vector<int64_t> first((size_t)B + 1, 0);
    for (int b = 0; b < B; ++b) first[(size_t)b + 1] = first[(size_t)b] + (h_offsets[b + 1] - h_offsets[b] + SN_BLOCK - 1) / SN_BLOCK;
    const int64_t tiles = first[(size_t)B];
    F2_CHECK(ctx, tiles < (int64_t(1) << 31), F2_ERR_UNSUPPORTED, "coloured noise needs %lld workgroups per level (at most 2^31 - 1)",
             (long long)tiles);
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
        k_shaped_noise_levels<int16_t><<<grid, dim3(SN_NT), 0, ctx->stream>>>((const int16_t*)d_wave, d_offsets, A.d_first, B, A.d_sigma,
                                                                             A.d_fir, A.d_fir_off, K, total, seed, d_out);
    else
        k_shaped_noise_levels<double><<<grid, dim3(SN_NT), 0, ctx->stream>>>((const double*)d_wave, d_offsets, A.d_first, B, A.d_sigma,
                                                                            A.d_fir, A.d_fir_off, K, total, seed, d_out);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

// f2_shaped_noise_levels: the clean samples and the taps go up, the two kernels run, the float64 levels and sigma come back. A device
// call waits only for sigma.
extern "C" int f2_shaped_noise_levels(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, int B, const double* snr_db,
                                      const double* fir, const int64_t* fir_offsets, int K, uint64_t seed, double* noisy,
                                      double* sigma_or_null, int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_CHECK(ctx, B >= 0, F2_ERR_INVALID, "bad batch size (B=%d)", B);
    F2_TRY(f2_check_wave_dtype(ctx, wave_dtype));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_TRY(f2_check_offsets(ctx, offsets, B, "offsets"));
    F2_TRY(f2_check_fir(ctx, snr_db, fir, fir_offsets, K));
    F2_CHECK(ctx, ((int64_t)K + 1) * (B > 0 ? B : 1) <= INT32_MAX / 2, F2_ERR_UNSUPPORTED, "%d levels of %d utterances", K + 1, B);
    const int64_t total = offsets[B];
    const size_t U = ((size_t)K + 1) * (size_t)B;
    if (B == 0 || total == 0) {
        if (sigma_or_null) std::fill(sigma_or_null, sigma_or_null + U, 0.0);
        return F2_OK;
    }
    F2_CHECK(ctx, wave && noisy, F2_ERR_INVALID, "null data pointer");
    f2_shaped_arrays A;
    f2_meta_carve meta;
    f2_shaped_meta(&meta, B, fir_offsets, K, &A);
    F2_TRY(meta.reserve(ctx));
    f2_output out;
    F2_TRY(f2_place(ctx, ctx->levels, noisy, sizeof(double) * ((size_t)K + 1) * (size_t)total, mem_space, true, &out));
    const void* d_wave;
    F2_TRY(f2_stage_wave(ctx, wave, wave_dtype, total, mem_space, &d_wave));
    F2_TRY(f2_upload_offsets(ctx, offsets, B));
    F2_TRY(f2_launch_shaped_noise_levels(ctx, d_wave, wave_dtype, (const int64_t*)ctx->offsets.ptr, offsets, B, snr_db, fir, fir_offsets,
                                         K, seed, A, out.as<double>()));
    F2_TRY(f2_copy_back(ctx, out));
    if (sigma_or_null) {
        F2_HIP(ctx, hipMemcpyAsync(sigma_or_null, A.d_sigma, sizeof(double) * U, hipMemcpyDeviceToHost, ctx->stream));
        F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return F2_OK;
    }
    return f2_host_wait(ctx, mem_space);
}
