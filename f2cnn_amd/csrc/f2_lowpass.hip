// Stand-alone first-order low-pass of envelopes that are already in memory, at K cutoffs in one pass (include/f2cnn_hip.h:
// f2_lowpass_levels; the kernel of f2_eval_cutoff_sweep).
//   k_lowpass_levels  one workgroup per row (utterance, channel) walks it in segments of LP_SEG samples; a segment is read once
//                     (16-byte loads) into registers, written out as the copy level and filtered K times from those registers by
//                     lowpass_pairs_store<double> (f2_envelope_core.h: pair -> weighted DPP scan over the wave in float64 -> wave
//                     totals through LDS -> block chain), with the one-pole state of every cutoff carried from segment to segment
//                     (as k_split_lowpass does for one cutoff).
//   k_lowpass_pick    the same walk with one cutoff per utterance, or none (f2_lowpass_pick; the cutoff stage of
//                     f2_input_batch_filtered / f2_trainer_render_filtered), out of place or in place.
// The segmentation depends on the row length alone and every sum has a fixed order: the bits of a filtered row depend on its
// samples and its cutoff, not on the batch around it, on K or on the other cutoffs. gfx950, wave64; plain vector stores only.
#include "f2_envelope_core.h"

#include <cmath>

namespace {

using namespace f2fft;

constexpr int LP_NT = 256, LP_NBLK = 8;
constexpr int LP_SEG = 2 * LP_NT * LP_NBLK;   // samples per segment: 16 per thread, 8 blocks of 512 consecutive samples

// One segment of a row, the code the two kernels share: its nseg samples at x are read once (16-byte loads) into registers, stored
// as they are to y + copy_at (COPY) and filtered with the pairs coef[k0 .. k1), level k to y + k * level_stride, the one-pole state of
// level k entering from carry[k - k0] and left there for the next segment. A row starts at C * offsets[b] + c * n_b doubles - on a
// 16-byte boundary only when that is even: pairs move through the under-aligned 16-byte types of f2_envelope_core.h (global memory
// takes dword-aligned wide accesses), the last sample of an odd tail on its own.
// x and y + k * level_stride may be the same row (k_lowpass_pick in place): a thread stores exactly the pairs (and the odd last
// sample) it loaded - lowpass_pairs_store's index and tests are the load's - and stores them behind the barrier that precedes
// the filter call, when every load of the segment has landed in registers.
template <bool COPY>
__device__ __forceinline__ void lowpass_segment(const double* x, double* y, int64_t copy_at, int64_t level_stride, const double* coef, int k0,
                                                int k1, double* lds, double* carry, int nseg, int tid) {
    double er[LP_NBLK], ei[LP_NBLK];
#pragma unroll
    for (int jj = 0; jj < LP_NBLK; ++jj) {
        const int i0 = 2 * (tid + LP_NT * jj);
        // (a block inside the segment - a wave-uniform test - loads and stores without a test per lane)
        if (2 * LP_NT * (jj + 1) <= nseg || i0 + 1 < nseg) {
            const f2_d2 t = load_pair_f64(x + i0);
            er[jj] = t.x, ei[jj] = t.y;
            if (COPY) store_pair(y + copy_at + i0, t.x, t.y);
        } else {
            er[jj] = ei[jj] = 0.0;
            if (i0 < nseg) {
                er[jj] = x[i0];
                if (COPY) y[copy_at + i0] = er[jj];
            }
        }
    }
    for (int k = k0; k < k1; ++k) {
        __syncthreads();   // lds free again; carry[k - k0] of the previous segment visible; the segment's loads done
        const double s = lowpass_pairs_store<double, LP_NT, LP_NBLK>(er, ei, coef[2 * k + 1], coef[2 * k], (unsigned char*)lds,
                                                                    y + (int64_t)k * level_stride, nseg, tid, carry[k - k0]);
        if (tid == 0) carry[k - k0] = s;   // (every thread read it before the barriers inside the call)
    }
}

// coef: K x {b0, a1}.
__global__ __launch_bounds__(LP_NT) void k_lowpass_levels(const double* __restrict__ env, const int64_t* __restrict__ offsets, int C,
                                                          const double* __restrict__ coef, int K, int64_t level_stride,
                                                          double* __restrict__ out) {
    __shared__ double lds[lowpass_lds_bytes<double, LP_NT, LP_NBLK>() / sizeof(double)];
    __shared__ double carry[F2_LOWPASS_MAX_CUTOFFS];   // s at the end of the previous segment, per cutoff
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)C), c = (int)(blockIdx.x - (unsigned)b * (unsigned)C);
    const int64_t n = offsets[b + 1] - offsets[b];
    if (n == 0) return;
    const int64_t row = (int64_t)C * offsets[b] + (int64_t)c * n;
    if (tid < K) carry[tid] = 0.0;
    for (int64_t base = 0; base < n; base += LP_SEG) {
        const int nseg = (int)(n - base < LP_SEG ? n - base : LP_SEG);
        double* y = out + row + base;
        lowpass_segment<true>(env + row + base, y, (int64_t)K * level_stride, level_stride, coef, 0, K, lds, carry, nseg, tid);
    }
}

// Utterance b at level cutoff_of[b] in [0, K] (K: unfiltered): its rows are bit for bit that level's rows of k_lowpass_levels - the
// same segments, loads, filter call and carried state, with the one pair {b0, a1} of its level. src and dst may be the same buffer
// (no __restrict__ on the two): lowpass_segment says why that is safe; an unfiltered row is then left alone - its workgroup returns
// at once - and copied segment by segment where they differ.
__global__ __launch_bounds__(LP_NT) void k_lowpass_pick(const double* src, const int64_t* __restrict__ offsets, int C,
                                                        const double* __restrict__ coef, int K, const int32_t* __restrict__ cutoff_of,
                                                        double* dst) {
    __shared__ double lds[lowpass_lds_bytes<double, LP_NT, LP_NBLK>() / sizeof(double)];
    __shared__ double carry[1];
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)C), c = (int)(blockIdx.x - (unsigned)b * (unsigned)C);
    const int64_t n = offsets[b + 1] - offsets[b];
    if (n == 0) return;
    const int l = cutoff_of[b];
    const bool plain = l < 0 || l >= K;   // (the host checked [0, K]; nothing outside it indexes coef)
    if (plain && src == dst) return;
    const int64_t row = (int64_t)C * offsets[b] + (int64_t)c * n;
    if (tid == 0) carry[0] = 0.0;
    for (int64_t base = 0; base < n; base += LP_SEG) {
        const int nseg = (int)(n - base < LP_SEG ? n - base : LP_SEG);
        const double* x = src + row + base;
        double* y = dst + row + base;
        if (plain) lowpass_segment<true>(x, y, 0, 0, coef, 0, 0, lds, carry, nseg, tid);
        else lowpass_segment<false>(x, y, 0, 0, coef, l, l + 1, lds, carry, nseg, tid);   // (level stride 0: level l lands on y)
    }
}

}  // namespace

int f2_check_cutoffs(f2_ctx* ctx, const double* cutoff_hz, int K) {
    F2_CHECK(ctx, K >= 1 && cutoff_hz, F2_ERR_INVALID, "a sweep needs at least one cutoff (K=%d) and their cutoff_hz", K);
    F2_CHECK(ctx, K <= F2_LOWPASS_MAX_CUTOFFS, F2_ERR_UNSUPPORTED, "%d cutoffs (at most %d)", K, F2_LOWPASS_MAX_CUTOFFS);
    for (int k = 0; k < K; ++k)
        F2_CHECK(ctx, std::isfinite(cutoff_hz[k]) && cutoff_hz[k] > 0 && cutoff_hz[k] < 8000, F2_ERR_INVALID,
                 "cutoff_hz[%d] = %g Hz outside (0, 8000)", k, cutoff_hz[k]);
    return F2_OK;
}

int f2_upload_lowpass_coefs(f2_ctx* ctx, const double* cutoff_hz, int K, double* d_coef) {
    double host[2 * F2_LOWPASS_MAX_CUTOFFS];
    for (int k = 0; k < K; ++k) {
        // butter(1, cutoff/8000): bilinear transform of 1/(s+1), pre-warped (EnvelopeExtraction.py:47)
        const double t = tan(3.14159265358979323846 * cutoff_hz[k] / 16000.0);
        host[2 * k] = t / (1.0 + t);
        host[2 * k + 1] = (t - 1.0) / (t + 1.0);
    }
    return f2_upload_async(ctx, d_coef, host, sizeof(double) * 2 * (size_t)K);
}

int f2_launch_lowpass_levels(f2_ctx* ctx, const double* d_env, const int64_t* d_offsets, int B, int C, int64_t total,
                             const double* d_coef, int K, double* d_levels) {
    if (B == 0 || total == 0) return F2_OK;
    k_lowpass_levels<<<dim3((unsigned)B * (unsigned)C), dim3(LP_NT), 0, ctx->stream>>>(d_env, d_offsets, C, d_coef, K,
                                                                                      (int64_t)C * total, d_levels);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

int f2_check_lowpass_pick(f2_ctx* ctx, int B, int C, const f2_lowpass_pick_args& P) {
    F2_CHECK(ctx, P.K >= 0, F2_ERR_INVALID, "negative number of cutoffs (K=%d)", P.K);
    if (P.unfiltered()) return F2_OK;
    F2_CHECK(ctx, P.cutoff_hz, F2_ERR_INVALID, "cutoff_of is given for K=%d cutoffs, but cutoff_hz is NULL", P.K);
    F2_TRY(f2_check_cutoffs(ctx, P.cutoff_hz, P.K));
    for (int b = 0; b < B; ++b)
        F2_CHECK(ctx, P.cutoff_of[b] >= 0 && P.cutoff_of[b] <= P.K, F2_ERR_INVALID, "utterance %d: cutoff %d is outside [0, %d]", b,
                 (int)P.cutoff_of[b], P.K);
    F2_CHECK(ctx, (int64_t)B * C <= INT32_MAX, F2_ERR_UNSUPPORTED, "%d utterances of %d channels", B, C);
    return F2_OK;
}

void f2_lowpass_pick_meta(f2_meta_carve* meta, int B, const f2_lowpass_pick_args& P, f2_lowpass_pick_arrays* A) {
    if (P.unfiltered()) return;
    if (!P.d_coef) meta->add(&A->d_coef, 2 * (size_t)P.K);
    meta->add(&A->d_cutoff_of, ((size_t)B + 1) / 2);
}

int f2_launch_lowpass_pick(f2_ctx* ctx, const double* d_src, const int64_t* d_offsets, int B, int C, int64_t total,
                           const f2_lowpass_pick_args& P, const f2_lowpass_pick_arrays& A, double* d_dst) {
    if (B == 0 || total == 0) return F2_OK;
    if (P.unfiltered()) {
        if (d_src != d_dst)
            F2_HIP(ctx, hipMemcpyAsync(d_dst, d_src, sizeof(double) * (size_t)C * (size_t)total, hipMemcpyDeviceToDevice, ctx->stream));
        return F2_OK;
    }
    const double* d_coef = P.d_coef;
    if (!d_coef) {
        F2_TRY(f2_upload_lowpass_coefs(ctx, P.cutoff_hz, P.K, A.d_coef));
        d_coef = A.d_coef;
    }
    F2_TRY(f2_upload_async(ctx, A.d_cutoff_of, P.cutoff_of, sizeof(int32_t) * (size_t)B));
    k_lowpass_pick<<<dim3((unsigned)B * (unsigned)C), dim3(LP_NT), 0, ctx->stream>>>(d_src, d_offsets, C, d_coef, P.K,
                                                                                    (const int32_t*)A.d_cutoff_of, d_dst);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

extern "C" int f2_lowpass_pick(f2_ctx* ctx, const double* env, const int64_t* offsets, int B, int C, const double* cutoff_hz, int K,
                               const int32_t* cutoff_of, double* filtered, int mem_space) {
    f2_lowpass_pick_args P;
    P.cutoff_hz = cutoff_hz, P.K = K, P.cutoff_of = cutoff_of;
    f2_lowpass_pick_arrays A;
    return f2_stage_call(
        ctx, offsets, B, mem_space,
        [&]() -> int {
            F2_TRY(f2_check_batch(ctx, offsets, B, C, mem_space, true));
            return f2_check_lowpass_pick(ctx, B, C, P);
        },
        [&](f2_meta_carve* meta) {
            f2_lowpass_pick_meta(meta, B, P, &A);
            return F2_OK;
        },
        env, [&](int64_t total, const void** d_env) { return f2_stage_input(ctx, env, sizeof(double) * (size_t)C * (size_t)total, mem_space, d_env); },
        &f2_ctx::levels, filtered, sizeof(double) * (size_t)C,
        [&](const void* d_env, const int64_t* d_offsets, int64_t total, double* d_out) -> int {
            return f2_launch_lowpass_pick(ctx, (const double*)d_env, d_offsets, B, C, total, P, A, d_out);
        });
}

extern "C" int f2_lowpass_levels(f2_ctx* ctx, const double* env, const int64_t* offsets, int B, int C, const double* cutoff_hz, int K,
                                 double* levels, int mem_space) {
    double* d_coef;
    return f2_stage_call(
        ctx, offsets, B, mem_space,
        [&]() -> int {
            F2_TRY(f2_check_batch(ctx, offsets, B, C, mem_space, true));
            F2_TRY(f2_check_cutoffs(ctx, cutoff_hz, K));
            F2_CHECK(ctx, (int64_t)B * C <= INT32_MAX, F2_ERR_UNSUPPORTED, "%d utterances of %d channels", B, C);
            return F2_OK;
        },
        [&](f2_meta_carve* meta) {
            meta->add(&d_coef, 2 * (size_t)K);
            return F2_OK;
        },
        env, [&](int64_t total, const void** d_env) { return f2_stage_input(ctx, env, sizeof(double) * (size_t)C * (size_t)total, mem_space, d_env); },
        &f2_ctx::levels, levels, sizeof(double) * (size_t)C * ((size_t)K + 1),
        [&](const void* d_env, const int64_t* d_offsets, int64_t total, double* d_out) -> int {
            F2_TRY(f2_upload_lowpass_coefs(ctx, cutoff_hz, K, d_coef));
            return f2_launch_lowpass_levels(ctx, (const double*)d_env, d_offsets, B, C, total, d_coef, K, d_out);
        });
}
