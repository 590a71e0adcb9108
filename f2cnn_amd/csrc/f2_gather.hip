// K3 -- window gather + per-window log min-max normalisation.
// Reference: scripts/processing/InputGenerator.py:73-80 (gather at given centres, cast to float32 at :83),
// scripts/CNN/Evaluating.py:76-80 (every-sample windows) and scripts/CNN/Training.py:13-28 (normalizeInput).
//
//   out[e, k, c] = env[c, centre_e + step*(k - radius)]           k < 2*radius+1, c < C
//   normalize:     (ln v - ln min)/(ln max - ln min) over the whole window, in float64, then float32;
//                  all-equal window -> zeros; any value <= 0 -> error flag (the reference raises ValueError)
//
// One 256-thread workgroup per window. The window (R*C float64 values, 11 KiB for 11x128) is gathered
// into LDS once, reduced for min/max there, and written out with c fastest, i.e. fully coalesced float32
// rows. In `cnn eval` mode consecutive windows read consecutive samples of the same envelope rows, so
// the strided gather is served by L2.
//
// RAGGED (f2_input_batch): the windows of a whole ragged batch in one launch. Window e lies in utterance
// win_utt[e], whose (C, n_b) block starts at env + C * offsets[b]; everything after that is the kernel above,
// except that without normalisation the values go straight from the envelope to the output (no LDS stage, no
// barrier). The windows of neighbouring labelled timepoints share most of their tap columns in L2.
#include "f2_internal.h"
#include "f2_gather_tail.h"

namespace {

constexpr int GT = 256;

template <bool RAGGED>
__global__ __launch_bounds__(GT) void k_gather_windows(const double* __restrict__ env, int C, int64_t N,
                                                       const int64_t* __restrict__ centers, int64_t first_center,
                                                       int radius, int step, int normalize,
                                                       float* __restrict__ out, int* __restrict__ flag,
                                                       const int64_t* __restrict__ offsets, const int* __restrict__ win_utt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* win = reinterpret_cast<double*>(smem_raw);
    __shared__ double red_min[GT / 64], red_max[GT / 64];

    const int tid = threadIdx.x;
    const int64_t e = blockIdx.x;
    const int R = 2 * radius + 1;
    const int total = R * C;
    if (RAGGED) {
        const int64_t o0 = offsets[win_utt[e]];
        env += (size_t)C * (size_t)o0;
        N = offsets[win_utt[e] + 1] - o0;
    }
    const int64_t centre = centers ? centers[e] : first_center + e;
    if (RAGGED && !normalize) {
        float* o = out + (size_t)e * (size_t)total;
        for (int idx = tid; idx < total; idx += GT) {
            const int k = idx / C, c = idx - k * C;
            o[idx] = (float)env[(size_t)c * (size_t)N + (size_t)(centre + (int64_t)step * (k - radius))];
        }
        return;
    }

    double mn = INFINITY, mx = -INFINITY;
    for (int idx = tid; idx < total; idx += GT) {
        const int k = idx / C, c = idx - k * C;
        const double v = env[(size_t)c * (size_t)N + (size_t)(centre + (int64_t)step * (k - radius))];
        win[idx] = v;
        mn = fmin(mn, v);
        mx = fmax(mx, v);
    }
    gather_window_tail<GT>(win, total, mn, mx, normalize, out + (size_t)e * (size_t)total, flag, red_min, red_max);
}

// ---- every-sample windows (`cnn eval`: centres first_center + e, normalised): two passes over coalesced data ----
// A sample of the envelope matrix appears in 2 * radius + 1 windows per channel; the per-window kernel above reads it with
// an 8-byte strided access and takes its logarithm (float64) each time. Here:
//   k_log_columns:   L[c][t] = ln env[c][t] once per sample (coalesced in t), with the minimum / maximum over each group of 16
//                    channels - a window's minimum is the minimum of R x groups of those;
//   k_window_stats:  (ln min, range) of every window from those partial minima, once;
//   k_eval_windows:  a workgroup = WB consecutive windows x one tap k; it reads, per channel, the WB consecutive values
//                    L[c][centre_0 + w + step (k - radius)] (one 256-byte run instead of 32 strided reads), normalises with
//                    the window's (ln min, range) and turns the (window, channel) tile through LDS into 512-byte output rows.
// Same arithmetic as k_gather_windows - ln v, ln min, (ln v - ln min) / range in float64, then float32 - so the results are
// bit-identical to it (tests/test_gpu_windows_cnn.py compares the two).
//
// Each of the three is ONE __forceinline__ body with two __global__ entry points that differ in their address prologue only:
// k_X takes its columns, windows and output rows from the block index (every-sample windows of one utterance), k_X_strided
// from a host-built table (strided windows of a ragged batch, below). The entry points stay apart because the every-sample
// kernels must not wait for a table entry before their first load ("Strided windows of a ragged batch").
constexpr int WB = 32;      // consecutive windows per workgroup
constexpr int LCH = 16;     // channels per thread of k_log_columns (its grid's second dimension walks the channel groups)

// Column j of L / pmin / pmax for the channels of `group`: src is channel 0's sample of this thread, rows N samples apart; a
// sample that does not exist leaves the column's minimum / maximum at +-infinity
__device__ __forceinline__ void log_columns_body(const double* __restrict__ src, size_t N, bool exists, size_t j, size_t span,
                                                 int C, int group, double* __restrict__ L, double* __restrict__ pmin,
                                                 double* __restrict__ pmax) {
    const int c0 = group * LCH, c1 = min(C, c0 + LCH);
    double mn = INFINITY, mx = -INFINITY;
    if (exists) {
        if (c1 - c0 == LCH) {
            // (all sixteen loads in flight before the first logarithm: the dependent load -> log -> store chain per channel was
            // sixteen memory latencies long)
            double v[LCH];
#pragma unroll
            for (int u = 0; u < LCH; ++u) v[u] = src[(size_t)(c0 + u) * N];
#pragma unroll
            for (int u = 0; u < LCH; ++u) {
                L[(size_t)(c0 + u) * span + j] = log(v[u]);
                mn = fmin(mn, v[u]);
                mx = fmax(mx, v[u]);
            }
        } else {
            for (int c = c0; c < c1; ++c) {
                const double v = src[(size_t)c * N];
                L[(size_t)c * span + j] = log(v);
                mn = fmin(mn, v);
                mx = fmax(mx, v);
            }
        }
    }
    pmin[(size_t)group * span + j] = mn;     // minimum / maximum over this group's channels
    pmax[(size_t)group * span + j] = mx;
}

// (ln min, ln max - ln min, flag) of a block of up to 32 windows, once (k_eval_windows used to form them again in each of its R
// workgroups per block of windows: R x groups loads per window and two float64 logarithms, eleven times): stats[4 e .. 4 e + 3];
// flag 1 = all values equal or a non-positive value (rows of zeros; the error flag is raised here). `col` is the column of this
// thread's window's first tap, e its stats slot; every thread of the workgroup comes here (the barrier), live or not
__device__ __forceinline__ void window_stats_body(int64_t col, bool live, int64_t e, int groups, int64_t span, int radius, int step,
                                                  const double* __restrict__ pmin, const double* __restrict__ pmax,
                                                  double* __restrict__ stats, int* __restrict__ flag) {
    // 32 consecutive windows x 8 lanes per window: lane p of a window takes the (tap, group) pairs p, p + 8, ... (a single
    // thread walking all 88 serialises as many L2 latencies); for a fixed pair the 32 windows read one 256-byte run
    const int w = threadIdx.x & 31, p = threadIdx.x >> 5;
    const int R = 2 * radius + 1, pairs = R * groups;
    double mn = INFINITY, mx = -INFINITY;
    if (live) {
#pragma unroll 4
        for (int pq = p; pq < pairs; pq += 8) {
            const int k2 = pq / groups, g = pq - k2 * groups;
            const size_t at = (size_t)g * (size_t)span + (size_t)(col + (int64_t)step * k2);
            mn = fmin(mn, pmin[at]);
            mx = fmax(mx, pmax[at]);
        }
    }
    __shared__ double smn[8][32], smx[8][32];
    smn[p][w] = mn;
    smx[p][w] = mx;
    __syncthreads();
    if (p != 0 || !live) return;
#pragma unroll
    for (int q = 1; q < 8; ++q) {
        mn = fmin(mn, smn[q][w]);
        mx = fmax(mx, smx[q][w]);
    }
    double zero = 0.0;
    if (!(mn > 0.0)) {   // also catches NaN; the reference raises ValueError
        atomicOr(flag, 1);
        zero = 1.0;
    }
    if (mn == mx) zero = 1.0;
    const double lmn = log(mn), range = log(mx) - lmn;
    stats[4 * e] = lmn;
    stats[4 * e + 1] = range;
    stats[4 * e + 2] = zero;
    stats[4 * e + 3] = 1.0 / range;   // (correctly rounded: k_eval_windows divides by `range` through it)
}

// Tap k of the nw <= WB windows with stats slots / output rows e0 .. e0 + nw - 1, window w's first tap at column col0 + w
__device__ __forceinline__ void eval_windows_body(const double* __restrict__ L, const double* __restrict__ stats, int C, int64_t span,
                                                  int64_t e0, int64_t col0, int nw, int k, int radius, int step,
                                                  float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* tile = reinterpret_cast<float*>(smem_raw);            // [WB][C + 1]
    const int tid = threadIdx.x;
    const int R = 2 * radius + 1, CP = C + 1;
    const int w = tid & (WB - 1), cc = tid / WB;                 // 8 channel lanes x 32 windows
    const bool live = w < nw;
    const double* st = stats + 4 * (e0 + (live ? w : 0));
    const double lmn = st[0], range = st[1], rinv = st[3];
    const bool zero = st[2] != 0.0;
    const double* Lk = L + (col0 + w + (int64_t)step * k);       // (read by live threads only)
    // (eight loads in flight per thread; a / range, correctly rounded, in three float64 operations instead of the ~12 + v_rcp_f64
    // of a division: q0 = RN(a rinv) is within an ulp of the quotient, the residual a - q0 range is exact in one fma, and
    // RN(q0 + residual x rinv) is the rounded quotient - Markstein's correction step with rinv = RN(1 / range); bit-identical to
    // the per-window kernel's division in test_every_sample_windows_blocked_and_per_window_kernels_agree)
    constexpr int CL = 256 / WB, UN = 8;
    for (int c0 = cc; c0 < C; c0 += CL * UN) {
        double v[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) v[u] = (live && c0 + CL * u < C) ? Lk[(size_t)(c0 + CL * u) * (size_t)span] : lmn;
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const double a = v[u] - lmn, q0 = a * rinv;
            const float o = (live && !zero) ? (float)fma(fma(-q0, range, a), rinv, q0) : 0.f;
            if (c0 + CL * u < C) tile[w * CP + c0 + CL * u] = o;
        }
    }
    __syncthreads();
    float* orow = out + ((size_t)e0 * R + k) * (size_t)C;
    if ((C & 3) == 0) {
        // 16 bytes per lane: a window's row of C floats is C / 4 consecutive lanes
        const int C4 = C >> 2;
        for (int idx = tid; idx < nw * C4; idx += 256) {
            const int ww = idx / C4, c = (idx - ww * C4) * 4;
            const float* t = tile + ww * CP + c;
            *reinterpret_cast<float4*>(orow + (size_t)ww * R * C + c) = make_float4(t[0], t[1], t[2], t[3]);
        }
    } else {
        for (int idx = tid; idx < nw * C; idx += 256) {
            const int ww = idx / C, c = idx - ww * C;
            orow[(size_t)ww * R * C + c] = tile[ww * CP + c];
        }
    }
}

// column j is sample t0 + j of the utterance
__global__ __launch_bounds__(256) void k_log_columns(const double* __restrict__ env, int C, int64_t N, int64_t t0, int64_t span,
                                                     double* __restrict__ L, double* __restrict__ pmin,
                                                     double* __restrict__ pmax) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= span) return;
    const int64_t t = t0 + j;
    log_columns_body(env + t, (size_t)N, t >= 0 && t < N, (size_t)j, (size_t)span, C, blockIdx.y, L, pmin, pmax);
}

// 32 consecutive windows per workgroup; window e's first tap is column e
__global__ __launch_bounds__(256) void k_window_stats(const double* __restrict__ pmin, const double* __restrict__ pmax, int groups,
                                                      int64_t span, int64_t n_windows, int radius, int step,
                                                      double* __restrict__ stats, int* __restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * 32 + (threadIdx.x & 31);
    window_stats_body(e, e < n_windows, e, groups, span, radius, step, pmin, pmax, stats, flag);
}

// grid (blocks of WB windows, taps); window e has its centre at span index e + step * radius (k_log_columns started `reach`
// samples before the first centre)
__global__ __launch_bounds__(256) void k_eval_windows(const double* __restrict__ L, const double* __restrict__ stats, int C,
                                                      int64_t span, int64_t n_windows, int radius, int step,
                                                      float* __restrict__ out) {
    const int64_t e0 = (int64_t)blockIdx.x * WB;
    const int nw = (int)((n_windows - e0) < WB ? (n_windows - e0) : WB);
    eval_windows_body(L, stats, C, span, e0, e0, nw, blockIdx.y, radius, step, out);
}

// ---- strided windows of a ragged batch (`cnn eval --hop`, f2_eval_batch_strided), hop | step ----
// Window j of an utterance has its centre at radius * step + j * hop, so its tap k reads sample hop * (j + k * step / hop): the
// strided windows are the every-sample windows, with step' = step / hop, of the decimated envelope env'[c][d] = env[c][d * hop].
// A chunk of windows is cut into segments (consecutive windows of one utterance); segment s owns the columns
// [col_s, col_s + count_s + 2 * radius * step') of the compact L / pmin / pmax, which hold env' from its first window's first tap
// on. The three entry points below run the bodies above with the places they read and write taken from host-built tables - one
// entry per 64 columns, one per block of up to WB windows of one segment - so that every utterance of the chunk is served by
// the same three launches. One body: a window's row is bit-identical to the every-sample kernels' and to k_gather_windows'
// (tests/test_gpu_eval_strided.py).
constexpr int CBW = 64;     // columns per table entry of k_log_columns_strided: one wavefront
struct colblock {
    int64_t src;            // element offset of env_b[0][first sample of the entry] in the batch's envelope buffer
    int64_t n;              // samples per channel row of that utterance
    int64_t col;            // first column in L
    int64_t ncols;          // <= CBW
};
struct winblock {
    int64_t row;            // position of the block's first window in the chunk (its output row and stats slot)
    int64_t col;            // column of that window's first tap
    int64_t nw;             // <= WB
    int64_t pad;
};

__global__ __launch_bounds__(256) void k_log_columns_strided(const double* __restrict__ env, int C, int hop, int64_t span,
                                                             const colblock* __restrict__ tab, int nblocks,
                                                             double* __restrict__ L, double* __restrict__ pmin,
                                                             double* __restrict__ pmax) {
    const int blk = blockIdx.x * (256 / CBW) + (threadIdx.x / CBW), lane = threadIdx.x % CBW;
    if (blk >= nblocks) return;
    const colblock cb = tab[blk];
    if (lane >= cb.ncols) return;
    // (neighbouring lanes are hop * 8 bytes apart: from hop = 16 on every load is a 128-byte line of its own)
    log_columns_body(env + (size_t)cb.src + (size_t)lane * (size_t)hop, (size_t)cb.n, true, (size_t)(cb.col + lane), (size_t)span, C,
                     blockIdx.y, L, pmin, pmax);
}

// one workgroup per table entry; `step` is step / hop
__global__ __launch_bounds__(256) void k_window_stats_strided(const double* __restrict__ pmin, const double* __restrict__ pmax,
                                                              int groups, int64_t span, const winblock* __restrict__ tab,
                                                              int radius, int step, double* __restrict__ stats,
                                                              int* __restrict__ flag) {
    const winblock wb = tab[blockIdx.x];
    const int w = threadIdx.x & 31;
    window_stats_body(wb.col + w, w < wb.nw, wb.row + w, groups, span, radius, step, pmin, pmax, stats, flag);
}

// grid (table entries, taps); `step` is step / hop
__global__ __launch_bounds__(256) void k_eval_windows_strided(const double* __restrict__ L, const double* __restrict__ stats, int C,
                                                              int64_t span, const winblock* __restrict__ tab, int radius, int step,
                                                              float* __restrict__ out) {
    const winblock wb = tab[blockIdx.x];
    eval_windows_body(L, stats, C, span, wb.row, wb.col, (int)wb.nw, blockIdx.y, radius, step, out);
}

}  // namespace

// LDS of the blocked kernels' (window, channel) tile, and whether a workgroup can have it: the blocked route serves C channels
static size_t eval_tile_bytes(int C) { return sizeof(float) * WB * ((size_t)C + 1); }
static bool blocked_serves(int C) { return eval_tile_bytes(C) <= 64 * 1024; }

// ctx->gather_log cut up for `span` columns of C channels and n_windows windows: L | pmin | pmax | stats
struct gather_log_parts {
    int groups;
    double *L, *pmin, *pmax, *stats;
};
static int reserve_gather_log(f2_ctx* ctx, int64_t span, int C, int64_t n_windows, gather_log_parts* g) {
    g->groups = (C + LCH - 1) / LCH;
    F2_TRY(f2_reserve(ctx, ctx->gather_log,
                      sizeof(double) * ((size_t)span * ((size_t)C + 2 * (size_t)g->groups) + 4 * (size_t)n_windows)));
    g->L = (double*)ctx->gather_log.ptr;
    g->pmin = g->L + (size_t)span * (size_t)C;
    g->pmax = g->pmin + (size_t)span * (size_t)g->groups;
    g->stats = g->pmax + (size_t)span * (size_t)g->groups;
    return F2_OK;
}

int f2_upload_windows(f2_ctx* ctx, const int64_t* centers, const int* win_utt, int64_t n_windows, const int64_t** d_centers,
                      const int** d_win_utt) {
    const size_t cbytes = sizeof(int64_t) * (size_t)n_windows, ubytes = win_utt ? sizeof(int) * (size_t)n_windows : 0;
    F2_TRY(f2_reserve(ctx, ctx->work2, cbytes + ubytes));
    F2_TRY(f2_upload_async(ctx, ctx->work2.ptr, centers, cbytes));
    if (win_utt) F2_TRY(f2_upload_async(ctx, (char*)ctx->work2.ptr + cbytes, win_utt, ubytes));
    *d_centers = (const int64_t*)ctx->work2.ptr;
    if (d_win_utt) *d_win_utt = win_utt ? (const int*)((char*)ctx->work2.ptr + cbytes) : nullptr;
    return F2_OK;
}

static int launch_eval_windows(f2_ctx* ctx, const double* d_env, int C, int64_t N, int64_t first_center, int64_t n_windows,
                               int radius, int step, float* d_out, int* d_flag) {
    const int64_t reach = (int64_t)step * radius;
    const int64_t span = n_windows + 2 * reach;
    gather_log_parts g;
    F2_TRY(reserve_gather_log(ctx, span, C, n_windows, &g));
    hipLaunchKernelGGL(k_log_columns, dim3((unsigned)((span + 255) / 256), (unsigned)g.groups), dim3(256), 0, ctx->stream, d_env, C,
                       N, first_center - reach, span, g.L, g.pmin, g.pmax);
    F2_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_window_stats, dim3((unsigned)((n_windows + 31) / 32)), dim3(256), 0, ctx->stream, (const double*)g.pmin,
                       (const double*)g.pmax, g.groups, span, n_windows, radius, step, g.stats, d_flag);
    F2_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_eval_windows, dim3((unsigned)((n_windows + WB - 1) / WB), (unsigned)(2 * radius + 1)), dim3(256),
                       eval_tile_bytes(C), ctx->stream, (const double*)g.L, (const double*)g.stats, C, span, n_windows, radius, step,
                       d_out);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

// the limits of one workgroup per window (`kernel`: the k_gather_windows instance), whose LDS holds the window
static int per_window_limits(f2_ctx* ctx, const void* kernel, size_t lds, int radius, int C, int64_t n_windows) {
    F2_CHECK(ctx, lds <= 150 * 1024, F2_ERR_UNSUPPORTED, "window of %d x %d values does not fit in LDS", 2 * radius + 1, C);
    F2_CHECK(ctx, n_windows < (int64_t(1) << 31), F2_ERR_UNSUPPORTED, "too many windows (%lld)", (long long)n_windows);
    if (lds > 64 * 1024) F2_HIP(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return F2_OK;
}

int f2_launch_gather(f2_ctx* ctx, const double* d_env, int C, int64_t N, const int64_t* d_centers,
                     int64_t first_center, int64_t n_windows, int radius, int step, int normalize, float* d_out, int* d_flag) {
    if (n_windows <= 0) return F2_OK;
    const size_t lds = sizeof(double) * (size_t)(2 * radius + 1) * (size_t)C;
    F2_TRY(per_window_limits(ctx, (const void*)k_gather_windows<false>, lds, radius, C, n_windows));
    F2_TRY(f2_prof_begin(ctx, F2_K_GATHER));
    // every-sample normalised windows (`cnn eval`): the two-pass coalesced form; anything else one workgroup per window
    if (!d_centers && normalize && ctx->opt_gather_blocked && n_windows >= 4 * WB && blocked_serves(C)) {
        F2_TRY(launch_eval_windows(ctx, d_env, C, N, first_center, n_windows, radius, step, d_out, d_flag));
        F2_TRY(f2_prof_end(ctx, F2_K_GATHER));
        return F2_OK;
    }
    hipLaunchKernelGGL(k_gather_windows<false>, dim3((unsigned)n_windows), dim3(GT), lds, ctx->stream, d_env, C, N, d_centers,
                       first_center, radius, step, normalize, d_out, d_flag, (const int64_t*)nullptr, (const int*)nullptr);
    F2_HIP(ctx, hipGetLastError());
    F2_TRY(f2_prof_end(ctx, F2_K_GATHER));
    return F2_OK;
}

int f2_launch_gather_ragged(f2_ctx* ctx, const double* d_env, int C, const int64_t* d_offsets, const int64_t* d_centers,
                            const int* d_win_utt, int64_t n_windows, int radius, int step, int normalize, float* d_out,
                            int* d_flag) {
    if (n_windows <= 0) return F2_OK;
    const size_t lds = normalize ? sizeof(double) * (size_t)(2 * radius + 1) * (size_t)C : 0;
    F2_TRY(per_window_limits(ctx, (const void*)k_gather_windows<true>, lds, radius, C, n_windows));
    F2_TRY(f2_prof_begin(ctx, F2_K_GATHER));
    hipLaunchKernelGGL(k_gather_windows<true>, dim3((unsigned)n_windows), dim3(GT), lds, ctx->stream, d_env, C, (int64_t)0,
                       d_centers, (int64_t)0, radius, step, normalize, d_out, d_flag, d_offsets, d_win_utt);
    F2_HIP(ctx, hipGetLastError());
    F2_TRY(f2_prof_end(ctx, F2_K_GATHER));
    return F2_OK;
}

bool f2_gather_strided_blocked(const f2_ctx* ctx, int C, int step, int hop) {
    return ctx->opt_gather_blocked && hop >= 1 && step % hop == 0 && blocked_serves(C);
}

int64_t f2_gather_strided_columns(int64_t count, int radius, int step, int hop) {
    return count + 2 * (int64_t)radius * (step / hop);
}

int f2_launch_gather_strided(f2_ctx* ctx, const double* d_env, int C, const int64_t* d_offsets, const int64_t* h_offsets,
                             const f2_win_seg* segs, int nseg, int radius, int step, int hop, float* d_out, int* d_flag) {
    int64_t n_windows = 0;
    for (int s = 0; s < nseg; ++s) n_windows += segs[s].count;
    if (n_windows <= 0) return F2_OK;
    const int R = 2 * radius + 1;
    F2_CHECK(ctx, n_windows < (int64_t(1) << 31), F2_ERR_UNSUPPORTED, "too many windows (%lld)", (long long)n_windows);
    const int64_t reach = (int64_t)radius * step;

    if (!f2_gather_strided_blocked(ctx, C, step, hop)) {
        // one workgroup per window at the centres radius * step + j * hop (k_gather_windows<true>)
        std::vector<int64_t> centers((size_t)n_windows);
        std::vector<int> win_utt((size_t)n_windows);
        size_t e = 0;
        for (int s = 0; s < nseg; ++s)
            for (int64_t j = 0; j < segs[s].count; ++j, ++e) {
                centers[e] = reach + (segs[s].first + j) * hop;
                win_utt[e] = segs[s].utt;
            }
        const int64_t* d_centers;
        const int* d_win_utt;
        F2_TRY(f2_upload_windows(ctx, centers.data(), win_utt.data(), n_windows, &d_centers, &d_win_utt));
        return f2_launch_gather_ragged(ctx, d_env, C, d_offsets, d_centers, d_win_utt, n_windows, radius, step, 1, d_out, d_flag);
    }

    // the tables: per segment its 64-column entries and its blocks of WB windows
    static_assert(sizeof(colblock) == 32 && sizeof(winblock) == 32, "table entries are four 8-byte words");
    const int stepd = step / hop;
    std::vector<colblock> cols;
    std::vector<winblock> wins;
    int64_t span = 0, row = 0;
    for (int s = 0; s < nseg; ++s) {
        const f2_win_seg& g = segs[s];
        if (g.count <= 0) continue;
        const int64_t o0 = h_offsets[g.utt], N = h_offsets[g.utt + 1] - o0;
        const int64_t ncol = f2_gather_strided_columns(g.count, radius, step, hop);
        // the segment's last column is sample (first + count - 1) * hop + 2 * reach of its utterance
        F2_CHECK(ctx, g.first >= 0 && (g.first + g.count - 1) * hop + 2 * reach < N, F2_ERR_INVALID,
                 "utterance %d: windows %lld .. +%lld at hop %d reach outside its %lld-sample envelope", g.utt, (long long)g.first,
                 (long long)g.count, hop, (long long)N);
        for (int64_t c = 0; c < ncol; c += CBW)
            cols.push_back({(int64_t)C * o0 + (g.first + c) * hop, N, span + c, ncol - c < CBW ? ncol - c : CBW});
        for (int64_t w = 0; w < g.count; w += WB) wins.push_back({row + w, span + w, g.count - w < WB ? g.count - w : WB, 0});
        span += ncol;
        row += g.count;
    }
    gather_log_parts g;
    F2_TRY(reserve_gather_log(ctx, span, C, n_windows, &g));
    const size_t cbytes = sizeof(colblock) * cols.size(), wbytes = sizeof(winblock) * wins.size();
    F2_TRY(f2_reserve(ctx, ctx->work2, cbytes + wbytes));
    F2_TRY(f2_upload_async(ctx, ctx->work2.ptr, cols.data(), cbytes));
    F2_TRY(f2_upload_async(ctx, (char*)ctx->work2.ptr + cbytes, wins.data(), wbytes));
    const colblock* d_cols = (const colblock*)ctx->work2.ptr;
    const winblock* d_wins = (const winblock*)((char*)ctx->work2.ptr + cbytes);
    const int ncb = (int)cols.size();
    F2_TRY(f2_prof_begin(ctx, F2_K_GATHER));
    hipLaunchKernelGGL(k_log_columns_strided, dim3((unsigned)((ncb + 256 / CBW - 1) / (256 / CBW)), (unsigned)g.groups), dim3(256), 0,
                       ctx->stream, d_env, C, hop, span, d_cols, ncb, g.L, g.pmin, g.pmax);
    F2_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_window_stats_strided, dim3((unsigned)wins.size()), dim3(256), 0, ctx->stream, (const double*)g.pmin,
                       (const double*)g.pmax, g.groups, span, d_wins, radius, stepd, g.stats, d_flag);
    F2_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_eval_windows_strided, dim3((unsigned)wins.size(), (unsigned)R), dim3(256), eval_tile_bytes(C), ctx->stream,
                       (const double*)g.L, (const double*)g.stats, C, span, d_wins, radius, stepd, d_out);
    F2_HIP(ctx, hipGetLastError());
    F2_TRY(f2_prof_end(ctx, F2_K_GATHER));
    return F2_OK;
}
