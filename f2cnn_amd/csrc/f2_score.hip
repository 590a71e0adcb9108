// Kernels of f2_cnn_score_windows (include/f2cnn_hip.h): a model scored on stored, labelled windows.
//   k_normalize_windows  float32 (n, rows*C) raw envelope windows -> normalised float32 windows, K3's arithmetic (f2_gather.hip)
//   k_score_tally        per window: counts[4g + 2 sign + label] and the float64 loss term; per workgroup and group a loss partial
//   k_score_loss_fold    loss[g] += the partials of a launch, workgroup by workgroup
// gfx950, wave64. Everything that reaches memory is written by plain C++ stores or vector integer atomics.
#include "f2_internal.h"

namespace {

constexpr int NT = 256;      // threads of k_normalize_windows (one workgroup per window)
constexpr int ST = 256;      // threads = windows of a k_score_tally workgroup
constexpr int SCORE_MAX_GROUPS = 1024;

// One workgroup per window: a window is ONE contiguous run of `total` = rows * C float32 values (5.6 KB for 11 x 128), so lane l of
// a wave reads and writes value base + l - whole 256-byte runs per instruction for any `total`; the run starts wherever e * total
// puts it, hence 4-byte accesses. The window is read once and kept in LDS as float32 between the min / max reduction and the
// logarithms. The arithmetic is k_gather_windows' (f2_gather.hip), operation for operation, on the values widened to float64
// (exact): min / max over the window, ln min and ln max - ln min once per window, (ln v - ln min) / range per value, rounded to
// float32 once - the same bits as K3 gives for the same window held in an envelope. All values equal: zeros. A value <= 0 or a NaN
// (which fmin / fmax would drop: it is turned into 0 for the minimum) anywhere: zeros and one atomicOr on the flag per window.
__global__ __launch_bounds__(NT) void k_normalize_windows(const float* __restrict__ in, int total, float* __restrict__ out,
                                                           int* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* win = reinterpret_cast<float*>(smem_raw);
    __shared__ double red_min[NT / 64], red_max[NT / 64];

    const int tid = threadIdx.x;
    const float* x = in + (size_t)blockIdx.x * (size_t)total;
    float* o = out + (size_t)blockIdx.x * (size_t)total;
    double mn = INFINITY, mx = -INFINITY;
    for (int idx = tid; idx < total; idx += NT) {
        const float f = x[idx];
        win[idx] = f;
        const double v = (double)f;
        mn = fmin(mn, v > 0.0 ? v : 0.0);
        mx = fmax(mx, v);
    }
    for (int d = 32; d > 0; d >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, d));
        mx = fmax(mx, __shfl_xor(mx, d));
    }
    if ((tid & 63) == 0) {
        red_min[tid >> 6] = mn;
        red_max[tid >> 6] = mx;
    }
    __syncthreads();
    mn = red_min[0];
    mx = red_max[0];
    for (int w = 1; w < NT / 64; ++w) {
        mn = fmin(mn, red_min[w]);
        mx = fmax(mx, red_max[w]);
    }
    if (!(mn > 0.0) || mn == mx) {
        if (!(mn > 0.0) && tid == 0) atomicOr(flag, 1);
        for (int idx = tid; idx < total; idx += NT) o[idx] = 0.f;
        return;
    }
    const double lmn = log(mn);
    const double range = log(mx) - lmn;
    // (every thread reads back the LDS words it wrote itself: no second barrier)
    for (int idx = tid; idx < total; idx += NT) o[idx] = (float)((log((double)win[idx]) - lmn) / range);
}

// Thread t of workgroup b owns window i = b * ST + t of the launch's m. sign = signs[i] (0 falling, 1 rising), g = groups[i]
// (groups == NULL: 0), pred = labels[i] != 0, term = -ln(min(max((double)scores[i][sign], 1e-7), 1)) (Training.py:217-218).
//   counts  cnt[4g + 2 sign + pred] in LDS by integer atomics, then one 64-bit integer atomic on the caller-zeroed global array per
//           counter that is not zero: integer sums do not depend on the order;
//   loss    no floating-point atomics. The terms and groups of the workgroup's windows go to LDS; thread g' (g' = t, t + ST, ...)
//           adds the terms of group g' in window order - only if the workgroup counted a window of that group, else 0 - and writes
//           partial[b * G + g']. k_score_loss_fold then adds the partials in workgroup order: the same bits on every call;
//   flag    a sign above 1 sets bit 0, a group outside [0, G) bit 1 of *flag (one atomicOr per workgroup that met one); such a
//           window is counted nowhere.
__global__ __launch_bounds__(ST) void k_score_tally(const float* __restrict__ scores, const uint8_t* __restrict__ labels,
                                                     const uint8_t* __restrict__ signs, const int* __restrict__ groups, int G,
                                                     int64_t m, unsigned long long* __restrict__ counts,
                                                     double* __restrict__ partial, int* __restrict__ flag) {
    __shared__ double term[ST];
    __shared__ int grp[ST];
    __shared__ unsigned cnt[4 * SCORE_MAX_GROUPS];
    __shared__ int bad;
    const int tid = threadIdx.x;
    for (int c = tid; c < 4 * G; c += ST) cnt[c] = 0;
    if (tid == 0) bad = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * ST + tid;
    double t = 0.0;
    int g = -1;
    if (i < m) {
        const unsigned sign = signs[i];
        const int gi = groups ? groups[i] : 0;
        const int wrong = (sign > 1u ? 1 : 0) | (gi < 0 || gi >= G ? 2 : 0);
        if (wrong) {
            atomicOr(&bad, wrong);
        } else {
            g = gi;
            const double p = (double)scores[2 * i + sign];
            t = -log(fmin(fmax(p, 1e-7), 1.0));
            atomicAdd(&cnt[4 * g + 2 * sign + (labels[i] != 0)], 1u);
        }
    }
    term[tid] = t;
    grp[tid] = g;
    __syncthreads();
    for (int c = tid; c < 4 * G; c += ST)
        if (cnt[c]) atomicAdd(&counts[c], (unsigned long long)cnt[c]);
    for (int gg = tid; gg < G; gg += ST) {
        double acc = 0.0;
        if (cnt[4 * gg] | cnt[4 * gg + 1] | cnt[4 * gg + 2] | cnt[4 * gg + 3])
            for (int k = 0; k < ST; ++k)
                if (grp[k] == gg) acc += term[k];
        partial[(size_t)blockIdx.x * G + gg] = acc;
    }
    if (tid == 0 && bad) atomicOr(flag, bad);
}

// One thread per group: loss[g] += partial[0][g], then [1][g], ... in that order. Launches follow each other on the stream, so
// loss[g] is one chain of float64 additions fixed by (n, the launch sizes): no atomics.
__global__ __launch_bounds__(ST) void k_score_loss_fold(const double* __restrict__ partial, int blocks, int G, double* __restrict__ loss) {
    const int g = blockIdx.x * ST + threadIdx.x;
    if (g >= G) return;
    double acc = loss[g];
    for (int b = 0; b < blocks; ++b) acc += partial[(size_t)b * G + g];
    loss[g] = acc;
}

}  // namespace

int f2_launch_normalize_windows(f2_ctx* ctx, const float* d_in, int64_t n, int total, float* d_out, int* d_flag) {
    if (n <= 0 || total <= 0) return F2_OK;
    const size_t lds = sizeof(float) * (size_t)total;
    F2_CHECK(ctx, lds <= 150 * 1024, F2_ERR_UNSUPPORTED, "window of %d values does not fit in LDS", total);
    F2_CHECK(ctx, n < (int64_t(1) << 31), F2_ERR_UNSUPPORTED, "too many windows (%lld)", (long long)n);
    if (lds > 64 * 1024)
        F2_HIP(ctx, hipFuncSetAttribute((const void*)k_normalize_windows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // Timed as window-stage time (F2_K_GATHER): it does K3's normalising, and the F2_K_* ids are part of what callers see. The
    // tally and fold kernels below have no id, like k_label_tally and the noise kernels ("Noise sweep").
    F2_TRY(f2_prof_begin(ctx, F2_K_GATHER));
    hipLaunchKernelGGL(k_normalize_windows, dim3((unsigned)n), dim3(NT), lds, ctx->stream, d_in, total, d_out, d_flag);
    F2_HIP(ctx, hipGetLastError());
    F2_TRY(f2_prof_end(ctx, F2_K_GATHER));
    return F2_OK;
}

size_t f2_score_partial_doubles(int64_t max_windows, int G) { return (size_t)((max_windows + ST - 1) / ST) * (size_t)G; }

int f2_launch_score_tally(f2_ctx* ctx, const float* d_scores, const uint8_t* d_labels, const uint8_t* d_signs, const int* d_groups,
                          int G, int64_t m, int64_t* d_counts, double* d_partial, double* d_loss, int* d_flag) {
    if (m <= 0) return F2_OK;
    F2_CHECK(ctx, G >= 1 && G <= SCORE_MAX_GROUPS, F2_ERR_UNSUPPORTED, "%d groups (at most %d)", G, SCORE_MAX_GROUPS);
    const int64_t blocks = (m + ST - 1) / ST;
    F2_CHECK(ctx, blocks < (int64_t(1) << 31), F2_ERR_UNSUPPORTED, "too many windows (%lld)", (long long)m);
    k_score_tally<<<dim3((unsigned)blocks), dim3(ST), 0, ctx->stream>>>(d_scores, d_labels, d_signs, d_groups, G, m,
                                                                        (unsigned long long*)d_counts, d_partial, d_flag);
    F2_HIP(ctx, hipGetLastError());
    k_score_loss_fold<<<dim3((unsigned)((G + ST - 1) / ST)), dim3(ST), 0, ctx->stream>>>(d_partial, (int)blocks, G, d_loss);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}
