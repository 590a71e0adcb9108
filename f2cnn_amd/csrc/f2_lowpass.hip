// Stand-alone first-order low-pass of envelopes that are already in memory, at K cutoffs in one pass (include/f2cnn_hip.h:
// f2_lowpass_levels; the kernel of f2_eval_cutoff_sweep).
//   k_lowpass_levels  one workgroup per row (utterance, channel) walks it in segments of LP_SEG samples; a segment is read once
//                     (16-byte loads) into registers, written out as the copy level and filtered K times from those registers by
//                     lowpass_pairs_store<double> (f2_envelope_core.h: pair -> weighted DPP scan over the wave in float64 -> wave
//                     totals through LDS -> block chain), with the one-pole state of every cutoff carried from segment to segment
//                     (as k_split_lowpass does for one cutoff).
// The segmentation depends on the row length alone and every sum has a fixed order: the bits of a filtered row depend on its
// samples and its cutoff, not on the batch around it, on K or on the other cutoffs. gfx950, wave64; plain vector stores only.
#include "f2_envelope_core.h"

#include <cmath>

namespace {

using namespace f2fft;

constexpr int LP_NT = 256, LP_NBLK = 8;
constexpr int LP_SEG = 2 * LP_NT * LP_NBLK;   // samples per segment: 16 per thread, 8 blocks of 512 consecutive samples

// coef: K x {b0, a1}. A row starts at C * offsets[b] + c * n_b doubles - on an 8-byte boundary only when n_b or offsets[b] is odd:
// pairs move through the under-aligned 16-byte types of f2_envelope_core.h (global memory takes dword-aligned wide accesses), the
// last sample of an odd tail on its own.
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
        const double* x = env + row + base;
        double* y = out + row + base;
        double er[LP_NBLK], ei[LP_NBLK];
#pragma unroll
        for (int jj = 0; jj < LP_NBLK; ++jj) {
            const int i0 = 2 * (tid + LP_NT * jj);
            // (a block inside the segment - a wave-uniform test - loads and stores without a test per lane)
            if (2 * LP_NT * (jj + 1) <= nseg || i0 + 1 < nseg) {
                const f2_d2 t = load_pair_f64(x + i0);
                er[jj] = t.x, ei[jj] = t.y;
                store_pair(y + (int64_t)K * level_stride + i0, t.x, t.y);
            } else {
                er[jj] = ei[jj] = 0.0;
                if (i0 < nseg) {
                    er[jj] = x[i0];
                    y[(int64_t)K * level_stride + i0] = er[jj];
                }
            }
        }
        for (int k = 0; k < K; ++k) {
            __syncthreads();   // lds free again; carry[k] of the previous segment visible
            const double s = lowpass_pairs_store<double, LP_NT, LP_NBLK>(er, ei, coef[2 * k + 1], coef[2 * k], (unsigned char*)lds,
                                                                        y + (int64_t)k * level_stride, nseg, tid, carry[k]);
            if (tid == 0) carry[k] = s;   // (every thread read carry[k] before the barriers inside the call)
        }
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
