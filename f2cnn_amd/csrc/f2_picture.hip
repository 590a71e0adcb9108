// Kernels of f2_envelope_picture / f2_gammatonegram_batch (include/f2cnn_hip.h): the envelopes of a ragged batch reduced to
// pictures of `width` columns.
//   k_picture_pool    pooled[b][c][x] = mean or maximum of the samples of row c that column x covers, float64; per utterance the
//                     smallest and largest pixel > 0
//   k_picture_levels  levels[b][c][x] = matplotlib's LogNorm() over the picture, quantised to 1..255 (0 = masked pixel)
// gfx950, wave64. Everything that reaches memory is written by plain C++ stores or vector integer atomics.
#include "f2_internal.h"

namespace {

constexpr int PT = 256;          // threads of a workgroup (4 waves)
constexpr int RUNS = 8;          // runs of columns a wave takes, their first loads issued together
constexpr int TASKS = 4;         // (row, RUNS runs) tasks a wave takes one after the other
constexpr int LT = 256;          // threads = pixels of a k_picture_levels workgroup

// One wave per (row, RUNS consecutive runs of columns). A run is 64 / G consecutive columns, G = 2^lg lanes per column, G the
// smallest power of two that holds the longest bin of the utterance (64 for longer bins: the lanes then stride through the bin).
// Lane l works for column l / G of the run with sample phase l % G, so the lanes of a wave read consecutive samples of one row
// whatever the bin size: a run of short bins is one contiguous stretch, a long bin is walked 64 samples (512 bytes) at a time.
// Rows start wherever C * offsets[b] + c * n_b puts them: 8-byte loads only.
//   mean     every lane adds its own samples in index order, then a butterfly over the G lanes (lane ^ G/2, ..., lane ^ 1) whose
//            two operands are the same pair in both partners: the order is fixed by (m, W) alone - no atomics, the same bits on
//            every call. A NaN sample makes the sum NaN.
//   maximum  fmax drops NaNs, so a lane that meets one remembers it and the pixel becomes NaN.
//   range    pixels > 0 (a NaN is not): minimum and maximum over the wave by shuffles, over the workgroup through LDS, then one
//            atomicMin / atomicMax per workgroup on the bit patterns (positive doubles order as their bit patterns do) of
//            range[2b] / range[2b + 1], preset by the caller to the bits of +inf and to 0.
// Workgroup blockIdx.x serves utterance blockIdx.x / bpu (bpu: the most workgroups any utterance of the call needs; the spare ones of
// the others leave at once): utt[4b .. 4b + 3] = {s_b, m_b, q = m_b / W, (m_b % W) << 8 | lg}. Each wave takes TASKS consecutive
// (row, RUNS runs) tasks, so that what it has to find out before its first load is paid once per 4 RUNS TASKS lines of samples.
// m_b == 0: every pixel of the utterance is 0.0.
template <int POOL>
__global__ __launch_bounds__(PT) void k_picture_pool(const double* __restrict__ env, const int64_t* __restrict__ offsets,
                                                      const int64_t* __restrict__ utt, int C, int W, unsigned bpu,
                                                      double* __restrict__ pooled, unsigned long long* __restrict__ range) {
    __shared__ double red_min[PT / 64], red_max[PT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned b = blockIdx.x / bpu, local = blockIdx.x % bpu;
    const int64_t s = utt[4 * (size_t)b], m = utt[4 * (size_t)b + 1], q = utt[4 * (size_t)b + 2];
    const unsigned r = (unsigned)(utt[4 * (size_t)b + 3] >> 8);
    const int lg = (int)(utt[4 * (size_t)b + 3] & 255);
    const int G = 1 << lg, per = 64 >> lg;              // lanes per column, columns per run
    const int runs = (W + per - 1) / per;               // per row
    const unsigned groups = (unsigned)(runs + RUNS - 1) / RUNS, tasks = (unsigned)C * groups;      // wave tasks per row, per utterance
    const int64_t o0 = offsets[b], nb = offsets[b + 1] - o0;
    const int sub = lane & (G - 1), col = lane >> lg;
    // floor(x m / W) = x q + floor(x r / W) with m = q W + r: x, r < 2^16, so the second term is a 32-bit division - made once per
    // task, for the lane's first column x0 (and x0 + 1, the bin's end); from run to run x grows by `per` and quotient / remainder
    // follow by additions (per r = dq W + dr)
    const unsigned Wu = (unsigned)W;
    const int64_t xq_step = (int64_t)per * q;
    const unsigned dq = (unsigned)per * r / Wu, dr = (unsigned)per * r % Wu;

    double vmin = INFINITY, vmax = 0.0;
    for (int it = 0; it < TASKS; ++it) {
        const unsigned task = (local * (PT / 64) + wv) * TASKS + it;
        if (task >= tasks) break;                           // (the whole wave)
        const int c = (int)(task / groups), r0 = (int)(task % groups) * RUNS;
        const double* row = env + (size_t)C * (size_t)o0 + (size_t)c * (size_t)nb;
        double* prow = pooled + ((size_t)b * C + c) * (size_t)W;
        const unsigned x0 = min((unsigned)(r0 * per + col), Wu - 1);      // (columns past the row's end are never used)
        unsigned qa = x0 * r / Wu, ra = x0 * r % Wu;                      // of x r
        unsigned qb = qa, rb = ra + r;                                    // of (x + 1) r
        if (rb >= Wu) rb -= Wu, ++qb;
        int64_t xq = (int64_t)x0 * q;
        // first the one sample every lane owns in each run (all of a bin when it fits the G lanes): RUNS independent loads in flight
        int64_t lo[RUNS], hi[RUNS];
        double first[RUNS];
#pragma unroll
        for (int k = 0; k < RUNS; ++k) {
            const int x = (r0 + k) * per + col;
            lo[k] = hi[k] = 0;
            if (r0 + k < runs && x < W && m > 0) {
                lo[k] = s + xq + qa;
                hi[k] = s + xq + q + qb;
                if (hi[k] == lo[k]) hi[k] = lo[k] + 1;
            }
            first[k] = lo[k] + sub < hi[k] ? row[lo[k] + sub] : (POOL ? -INFINITY : 0.0);
            xq += xq_step;
            qa += dq, ra += dr;
            if (ra >= Wu) ra -= Wu, ++qa;
            qb += dq, rb += dr;
            if (rb >= Wu) rb -= Wu, ++qb;
        }

#pragma unroll
        for (int k = 0; k < RUNS; ++k) {
            const int x = (r0 + k) * per + col;
            const bool has = r0 + k < runs && x < W;
            double acc = first[k];
            int nan = POOL ? acc != acc : 0;
            for (int64_t i = lo[k] + sub + G; i < hi[k]; i += G) {   // bins longer than a wave (G = 64): the lane's further samples
                const double v = row[i];
                if (POOL) {
                    nan |= v != v;
                    acc = fmax(acc, v);
                } else {
                    acc += v;
                }
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                if (d >= G) continue;      // (uniform: G belongs to the utterance)
                const double o = __shfl_xor(acc, d);
                if (POOL) {
                    acc = fmax(acc, o);
                    nan |= __shfl_xor(nan, d);
                } else {
                    acc += o;
                }
            }
            if (has && sub == 0) {
                double v = 0.0;
                if (m > 0) v = POOL ? (nan ? (double)NAN : acc) : acc / (double)(hi[k] - lo[k]);
                prow[x] = v;
                if (v > 0.0) {
                    vmin = fmin(vmin, v);
                    vmax = fmax(vmax, v);
                }
            }
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        vmin = fmin(vmin, __shfl_xor(vmin, d));
        vmax = fmax(vmax, __shfl_xor(vmax, d));
    }
    if (lane == 0) {
        red_min[wv] = vmin;
        red_max[wv] = vmax;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PT / 64; ++w) {
            vmin = fmin(vmin, red_min[w]);
            vmax = fmax(vmax, red_max[w]);
        }
        if (vmax > 0.0) {
            atomicMin(&range[2 * (size_t)b], (unsigned long long)__double_as_longlong(vmin));
            atomicMax(&range[2 * (size_t)b + 1], (unsigned long long)__double_as_longlong(vmax));
        }
    }
}

// One thread per pixel p of the (B, C, W) picture stack; utterance p / (C W) with the range words k_picture_pool left. v > 0:
// level 1 + (int)(254 t + 0.5), t = (ln v - ln vmin) / (ln vmax - ln vmin) in float64, t = 0 when vmax == vmin; v <= 0 or NaN:
// level 0 (LogNorm masks the pixel). vmin <= v <= vmax holds for every v > 0, so t lies in [0, 1] (kept there against the
// logarithm's rounding and an infinite vmax).
__global__ __launch_bounds__(LT) void k_picture_levels(const double* __restrict__ pooled, const unsigned long long* __restrict__ range,
                                                        size_t per_utt, size_t total, uint8_t* __restrict__ levels) {
    const size_t p = (size_t)blockIdx.x * LT + threadIdx.x;
    if (p >= total) return;
    const size_t b = p / per_utt;
    const double v = pooled[p];
    int level = 0;
    if (v > 0.0) {
        const double vmin = __longlong_as_double((long long)range[2 * b]), vmax = __longlong_as_double((long long)range[2 * b + 1]);
        double t = 0.0;
        if (vmax != vmin) {
            const double lmin = log(vmin);
            t = v == vmax ? 1.0 : (log(v) - lmin) / (log(vmax) - lmin);
            t = fmin(fmax(t, 0.0), 1.0);
        }
        level = 1 + (int)(254.0 * t + 0.5);
    }
    levels[p] = (uint8_t)level;
}

}  // namespace

int f2_picture_lanes_log2(int64_t m, int width) {
    const int64_t longest = m > width ? (m + width - 1) / width : 1;
    int lg = 0;
    while (lg < 6 && (int64_t(1) << lg) < longest) ++lg;
    return lg;
}

int64_t f2_picture_pool_blocks(int C, int width, int lg) {
    const int per = 64 >> lg;
    const int64_t runs = (width + per - 1) / per, groups = (runs + RUNS - 1) / RUNS;
    constexpr int64_t PER_BLOCK = PT / 64 * TASKS;
    return ((int64_t)C * groups + PER_BLOCK - 1) / PER_BLOCK;
}

int f2_launch_picture_pool(f2_ctx* ctx, const double* d_env, const int64_t* d_offsets, const int64_t* d_utt, int B, int C, int width,
                           int pool, int64_t blocks_per_utt, double* d_pooled, uint64_t* d_range) {
    if (B <= 0 || blocks_per_utt <= 0) return F2_OK;
    // (tasks of an utterance are counted in 32 bits by the kernel: at most (blocks_per_utt + 1) * 4 TASKS of them)
    F2_CHECK(ctx, blocks_per_utt * B < (int64_t(1) << 31) && blocks_per_utt < (int64_t(1) << 26), F2_ERR_UNSUPPORTED,
             "picture of %d x %d x %d pixels needs too many workgroups", B, C, width);
    const dim3 grid((unsigned)(blocks_per_utt * B));
    if (pool)
        k_picture_pool<1><<<grid, dim3(PT), 0, ctx->stream>>>(d_env, d_offsets, d_utt, C, width, (unsigned)blocks_per_utt, d_pooled,
                                                             (unsigned long long*)d_range);
    else
        k_picture_pool<0><<<grid, dim3(PT), 0, ctx->stream>>>(d_env, d_offsets, d_utt, C, width, (unsigned)blocks_per_utt, d_pooled,
                                                             (unsigned long long*)d_range);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

int f2_launch_picture_levels(f2_ctx* ctx, const double* d_pooled, const uint64_t* d_range, int B, int C, int width, uint8_t* d_levels) {
    const size_t per_utt = (size_t)C * (size_t)width, total = per_utt * (size_t)B;
    if (total == 0) return F2_OK;
    const size_t blocks = (total + LT - 1) / LT;
    F2_CHECK(ctx, blocks < (size_t(1) << 31), F2_ERR_UNSUPPORTED, "picture of %d x %d x %d pixels needs too many workgroups", B, C, width);
    k_picture_levels<<<dim3((unsigned)blocks), dim3(LT), 0, ctx->stream>>>(d_pooled, (const unsigned long long*)d_range, per_utt, total,
                                                                          d_levels);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}
