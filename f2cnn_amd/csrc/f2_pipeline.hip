// C-ABI entry points for the window gather (K3), the CNN forward (K4) and the `cnn eval` device pipeline
// (scripts/CNN/Evaluating.py:42-87): host/device pointer handling, chunking, error flags. Host code only.
#include "f2_internal.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int64_t CNN_CHUNK = 16384;  // windows per CNN launch group (activation workspace 1.75 GB, windows 92 MB)
constexpr int64_t DENSE_GROUP = 8 * CNN_CHUNK;   // windows per dense1 / dense2 launch of f2_eval_batch (conv4 + dense1 outputs: 1.3 GB)

int reset_flag(f2_ctx* ctx) {
    F2_HIP(ctx, hipMemsetAsync(ctx->flags.ptr, 0, sizeof(int), ctx->stream));
    return F2_OK;
}

// waits for the stream; the error of a window with a value <= 0 under normalisation (the gather kernels set the flag)
int finish_positive(f2_ctx* ctx) {
    F2_HIP(ctx, hipMemcpyAsync(ctx->host_flags, ctx->flags.ptr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    F2_CHECK(ctx, !ctx->host_flags[0], F2_ERR_NONPOSITIVE, "values must all be positive (normalizeInput)");
    return F2_OK;
}

// Input range of f2_cnn_forward: ctx->flags words RANGE_WORD .. + 2 = bit pattern of max |x| over the finite values, inf / NaN
// seen, complement of the quietest window's max |x| (word 0 is the gather's flag)
constexpr int RANGE_WORD = 4;
// A window whose max |x| lies more than this many binades below the call's bound B loses the low bits of its activations' second
// fp16 pieces (they fall below fp16's normal range: the scales are the call's, set by its loudest window). Calls with B above
// 2^QUIET_BINADES and such a window (a spike among normalised windows) take the float32 kernels; up to there no window is
// served worse than a window whose max is 2^-QUIET_BINADES is at B = 1.
constexpr int QUIET_BINADES = 4;

// The range pass over nwin windows of S floats at d_x with its read-back (waits for the stream): max |x| over the finite values, the
// quietest window's max |x|, and whether an inf / NaN was seen
struct input_range { float max, quiet; bool bad; };
int measure_input_range(f2_ctx* ctx, const float* d_x, int64_t nwin, int S, input_range* r) {
    unsigned* words = (unsigned*)ctx->flags.ptr + RANGE_WORD;
    F2_HIP(ctx, hipMemsetAsync(words, 0, 3 * sizeof(unsigned), ctx->stream));
    F2_TRY(f2_prof_begin(ctx, F2_K_CNN));
    F2_TRY(f2_launch_cnn_input_range(ctx, d_x, nwin, S, words));
    F2_TRY(f2_prof_end(ctx, F2_K_CNN));
    F2_HIP(ctx, hipMemcpyAsync(ctx->host_flags + RANGE_WORD, words, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const unsigned mbits = (unsigned)ctx->host_flags[RANGE_WORD], qbits = ~(unsigned)ctx->host_flags[RANGE_WORD + 2];
    memcpy(&r->max, &mbits, sizeof(float));
    memcpy(&r->quiet, &qbits, sizeof(float));
    r->bad = ctx->host_flags[RANGE_WORD + 1] != 0;
    return F2_OK;
}

// Scale set, route and last_input_bound of f2_cnn_forward (and of f2_cnn_score_windows without normalisation) for the nwin windows
// at d_x. The split path's scales follow the input (f2_cnn_split.h), so the windows are measured - unless the float32 kernels run
// whatever the input: B = 1 for max |x| <= 1, else B = 2^ceil(log2 max |x|), and *bound = B. *S = NULL, the float32 route and
// *bound = -1 without the split path, after inf / NaN, for a B whose scales leave the clamp, or when B > 2^QUIET_BINADES and a
// window's max |x| lies below B / 2^QUIET_BINADES.
int forward_route(f2_ctx* ctx, const f2_cnn* cnn, const float* d_x, int64_t nwin, const f2_scale_set** S, f2_cnn_route* route,
                  double* bound) {
    *S = nullptr;
    *route = f2_cnn_route();
    *bound = -1.0;
    if (!f2_cnn_call_route(ctx, cnn, true).split) return F2_OK;
    input_range r;
    F2_TRY(measure_input_range(ctx, d_x, nwin, cnn->rows * cnn->channels, &r));
    if (r.bad) return F2_OK;
    int e = 0;
    if (r.max > 1.f) {
        int ex;
        const float f = std::frexp(r.max, &ex);   // max = f 2^ex, f in [0.5, 1)
        e = f == 0.5f ? ex - 1 : ex;
        if (e > QUIET_BINADES && (double)r.quiet < std::ldexp(1.0, e - QUIET_BINADES)) return F2_OK;
    }
    F2_TRY(f2_cnn_scale_set(ctx, cnn, e, S));
    if (*S) *bound = std::ldexp(1.0, e);
    *route = f2_cnn_call_route(ctx, cnn, *S != nullptr);
    return F2_OK;
}

// last_input_bound of a host call of several chunks (start at 0): the largest B, -1 once a chunk ran on the float32 kernels
double chunks_bound(double bound, double b) { return b < 0 || bound < 0 ? -1.0 : b > bound ? b : bound; }

int cnn_forward_device(f2_ctx* ctx, const f2_cnn* cnn, const f2_scale_set* S, f2_cnn_route route, const float* d_x, int64_t n,
                       float* d_scores, uint8_t* d_labels) {
    const size_t per = f2_cnn_workspace_floats(cnn);
    const int64_t chunk = n < CNN_CHUNK ? n : CNN_CHUNK;
    F2_TRY(f2_reserve(ctx, ctx->work, sizeof(float) * per * (size_t)chunk));
    const size_t xs = (size_t)cnn->rows * cnn->channels;
    for (int64_t s = 0; s < n; s += chunk) {
        const int64_t m = n - s < chunk ? n - s : chunk;
        F2_TRY(f2_launch_cnn(ctx, cnn, S, route, d_x + (size_t)s * xs, m, (float*)ctx->work.ptr, d_scores ? d_scores + 2 * s : nullptr,
                             d_labels ? d_labels + s : nullptr));
    }
    return F2_OK;
}

}  // namespace

extern "C" {

int f2_gather_windows(f2_ctx* ctx, const double* env, int C, int64_t N, const int64_t* centers, int64_t n_windows,
                      int radius, int step, int normalize, float* out, int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_CHECK(ctx, C >= 0 && N >= 0 && n_windows >= 0 && radius >= 0 && step >= 0, F2_ERR_INVALID, "negative size");
    if (n_windows == 0 || C == 0) return F2_OK;
    F2_CHECK(ctx, env && out, F2_ERR_INVALID, "null data pointer");
    const int R = 2 * radius + 1;
    const int64_t reach = (int64_t)radius * step;
    if (centers) {
        for (int64_t e = 0; e < n_windows; ++e)
            F2_CHECK(ctx, centers[e] - reach >= 0 && centers[e] + reach < N, F2_ERR_INVALID,
                     "window %lld (centre %lld, +-%lld) reaches outside the %lld-sample envelope", (long long)e,
                     (long long)centers[e], (long long)reach, (long long)N);
    } else {
        F2_CHECK(ctx, reach + (n_windows - 1) + reach < N, F2_ERR_INVALID,
                 "%lld every-sample windows do not fit in %lld samples", (long long)n_windows, (long long)N);
    }
    const int64_t* d_centers = nullptr;
    if (centers) F2_TRY(f2_upload_windows(ctx, centers, nullptr, n_windows, &d_centers, nullptr));
    const size_t env_bytes = sizeof(double) * (size_t)C * (size_t)N;
    const size_t out_bytes = sizeof(float) * (size_t)n_windows * R * (size_t)C;
    const double* d_env = env;
    float* d_out = out;
    if (mem_space == F2_MEM_HOST) {
        F2_TRY(f2_reserve(ctx, ctx->stage_in, env_bytes));
        F2_TRY(f2_reserve(ctx, ctx->stage_out, out_bytes));
        F2_HIP(ctx, hipMemcpyAsync(ctx->stage_in.ptr, env, env_bytes, hipMemcpyHostToDevice, ctx->stream));
        d_env = (const double*)ctx->stage_in.ptr;
        d_out = (float*)ctx->stage_out.ptr;
    }
    F2_TRY(reset_flag(ctx));
    F2_TRY(f2_launch_gather(ctx, d_env, C, N, d_centers, reach, n_windows, radius, step, normalize, d_out,
                            (int*)ctx->flags.ptr));
    if (mem_space == F2_MEM_HOST)
        F2_HIP(ctx, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    return normalize || mem_space == F2_MEM_HOST ? finish_positive(ctx) : F2_OK;
}

int f2_cnn_forward(f2_ctx* ctx, const f2_cnn* cnn, const float* x, int64_t n, float* scores, uint8_t* labels,
                   int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_cnn(ctx, cnn, 0, 0));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_CHECK(ctx, n >= 0, F2_ERR_INVALID, "negative window count");
    if (n == 0) return F2_OK;
    F2_CHECK(ctx, x, F2_ERR_INVALID, "x is NULL");
    const size_t xs = (size_t)cnn->rows * cnn->channels;
    const f2_scale_set* S = nullptr;
    f2_cnn_route route;
    if (mem_space == F2_MEM_DEVICE) {
        double bound = -1.0;
        F2_TRY(forward_route(ctx, cnn, x, n, &S, &route, &bound));
        F2_TRY(cnn_forward_device(ctx, cnn, S, route, x, n, scores, labels));
        cnn->last_input_bound = bound;
        return F2_OK;
    }
    const int64_t chunk = n < CNN_CHUNK ? n : CNN_CHUNK;
    F2_TRY(f2_reserve(ctx, ctx->stage_in, sizeof(float) * xs * (size_t)chunk));
    F2_TRY(f2_reserve(ctx, ctx->stage_aux, (sizeof(float) * 2 + 1) * (size_t)chunk + 64));
    float* d_scores = (float*)ctx->stage_aux.ptr;
    uint8_t* d_labels = (uint8_t*)(d_scores + 2 * chunk);
    double bound = 0.0;   // largest B of the chunks, -1 once one of them ran on the float32 kernels
    for (int64_t s = 0; s < n; s += chunk) {
        const int64_t m = n - s < chunk ? n - s : chunk;
        F2_HIP(ctx, hipMemcpyAsync(ctx->stage_in.ptr, x + (size_t)s * xs, sizeof(float) * xs * (size_t)m,
                                   hipMemcpyHostToDevice, ctx->stream));
        double b = -1.0;
        F2_TRY(forward_route(ctx, cnn, (const float*)ctx->stage_in.ptr, m, &S, &route, &b));
        bound = chunks_bound(bound, b);
        F2_TRY(cnn_forward_device(ctx, cnn, S, route, (const float*)ctx->stage_in.ptr, m, d_scores, d_labels));
        if (scores)
            F2_HIP(ctx, hipMemcpyAsync(scores + 2 * s, d_scores, sizeof(float) * 2 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        if (labels) F2_HIP(ctx, hipMemcpyAsync(labels + s, d_labels, (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    cnn->last_input_bound = bound;
    return F2_OK;
}

}  // extern "C"

// ---- `cnn eval` over a ragged batch: what f2_eval_batch / f2_eval_utterance (every sample) and f2_eval_batch_strided share ----
namespace {

struct eval_call {
    bool host = false;
    int R = 0;
    int64_t total = 0;           // samples of the batch
    double* d_env = nullptr;     // envelopes of the batch, (C, n_b) blocks at C * offsets[b]
    // CNN side (eval_cnn_begin)
    int64_t n_total = 0, group_cap = 0;
    size_t flat = 0;
    float *d_a4 = nullptr, *d_a5 = nullptr, *d_scores = nullptr;
    uint8_t* d_labels = nullptr;
    const f2_scale_set* S1 = nullptr;
    f2_cnn_route route;          // of every launch of the call
    int64_t g0 = 0, gn = 0;      // first window and size of the open dense group
};

// the argument errors of the eval calls (include/f2cnn_hip.h: f2_eval_batch); nothing is launched before they pass
int eval_check(f2_ctx* ctx, const f2_cnn* cnn, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C, int lpf,
               double cutoff_hz, int fft_precision, int radius, int step, int mem_space, eval_call* E) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_dsp(ctx, wave_dtype, lpf, cutoff_hz, fft_precision));
    F2_TRY(f2_check_batch(ctx, offsets, B, C, mem_space, true));
    F2_CHECK(ctx, coefs && radius >= 0 && step >= 0, F2_ERR_INVALID, "coefs is NULL, or negative radius or step");
    E->R = 2 * radius + 1;
    F2_TRY(f2_check_cnn(ctx, cnn, E->R, C));
    E->host = mem_space == F2_MEM_HOST;
    E->total = offsets[B];
    return F2_OK;
}

// filterbank + envelope of the whole batch, always by the two kernels: one utterance evaluated alone and inside a batch
// goes through the same envelope kernel. The envelopes stay in stage_out (or the caller's device buffer) for the window loop.
// With no window to evaluate (n_windows == 0) a host call is complete when this returns.
int eval_envelopes(f2_ctx* ctx, eval_call* E, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B,
                   int C, int lpf, double cutoff_hz, int fft_precision, double* env_or_null, int64_t n_windows, int mem_space) {
    F2_CHECK(ctx, wave, F2_ERR_INVALID, "null wave");
    F2_TRY(f2_upload_offsets(ctx, offsets, B));
    F2_TRY(f2_upload_coefs(ctx, coefs, C));
    const size_t env_bytes = sizeof(double) * (size_t)C * (size_t)E->total;
    E->d_env = env_or_null;
    if (E->host || !env_or_null) {
        F2_TRY(f2_reserve(ctx, ctx->stage_out, env_bytes));
        E->d_env = (double*)ctx->stage_out.ptr;
    }
    const void* d_wave;
    F2_TRY(f2_stage_wave(ctx, wave, wave_dtype, E->total, mem_space, &d_wave));
    F2_TRY(f2_envelopes_device(ctx, d_wave, wave_dtype, offsets, B, C, lpf, cutoff_hz, fft_precision, E->d_env, nullptr, false));
    if (E->host && env_or_null) F2_HIP(ctx, hipMemcpyAsync(env_or_null, E->d_env, env_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (n_windows == 0 && E->host) F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return F2_OK;
}

// Buffers of the window loop: xbuf and the convolution workspace for `chunk` windows, conv4 / dense1 outputs of a dense group
// (the dense layers run over the conv4 outputs of up to DENSE_GROUP windows at once: dense1's grid of 64-window workgroups then
// fills whole rounds of the device - launched per 14 240-window utterance its second round was one third full), scores and
// labels of all n_total windows (staged for host calls); nothing leaves HBM. Clears the error flag.
int eval_cnn_begin(f2_ctx* ctx, const f2_cnn* cnn, eval_call* E, int64_t chunk, int64_t n_total, int C, float* scores_or_null,
                   uint8_t* labels_or_null) {
    E->n_total = n_total;
    E->group_cap = n_total < DENSE_GROUP ? n_total : DENSE_GROUP;
    const size_t conv_floats = f2_cnn_workspace_floats(cnn) - f2_cnn_dense_floats(cnn);
    E->flat = f2_cnn_flat_floats(cnn);
    F2_TRY(f2_reserve(ctx, ctx->xbuf, sizeof(float) * (size_t)chunk * E->R * (size_t)C));
    F2_TRY(f2_reserve(ctx, ctx->work, sizeof(float) * conv_floats * (size_t)chunk));
    F2_TRY(f2_reserve(ctx, ctx->dense_in, sizeof(float) * f2_cnn_dense_floats(cnn) * (size_t)E->group_cap));
    E->d_a4 = (float*)ctx->dense_in.ptr;
    E->d_a5 = E->d_a4 + E->flat * (size_t)E->group_cap;
    E->d_scores = scores_or_null;
    E->d_labels = labels_or_null;
    if (E->host) {
        F2_TRY(f2_reserve(ctx, ctx->stage_aux, (sizeof(float) * 2 + 1) * (size_t)n_total + 64));
        E->d_scores = (float*)ctx->stage_aux.ptr;
        E->d_labels = (uint8_t*)(E->d_scores + 2 * n_total);
    }
    F2_TRY(f2_cnn_scale_set(ctx, cnn, 0, &E->S1));   // K3's normalised windows lie in [0, 1] by construction: no range pass
    E->route = f2_cnn_call_route(ctx, cnn, E->S1 != nullptr);
    E->g0 = E->gn = 0;
    return reset_flag(ctx);
}

int eval_dense_flush(f2_ctx* ctx, const f2_cnn* cnn, eval_call* E) {
    if (E->gn > 0)
        F2_TRY(f2_launch_cnn_dense(ctx, cnn, E->S1, E->route, E->d_a4, E->gn, E->d_a5, E->d_scores ? E->d_scores + 2 * E->g0 : nullptr,
                                   E->d_labels ? E->d_labels + E->g0 : nullptr));
    E->g0 += E->gn;
    E->gn = 0;
    return F2_OK;
}

// before the windows of a chunk of m are written to xbuf: room for them in the open dense group
int eval_chunk_room(f2_ctx* ctx, const f2_cnn* cnn, eval_call* E, int64_t m) {
    return E->gn + m > E->group_cap ? eval_dense_flush(ctx, cnn, E) : F2_OK;
}

// conv1 .. conv4 of the m windows in xbuf, appended to the open dense group
int eval_chunk_convs(f2_ctx* ctx, const f2_cnn* cnn, eval_call* E, int64_t m) {
    F2_TRY(f2_launch_cnn_convs(ctx, cnn, E->S1, E->route, (const float*)ctx->xbuf.ptr, m, (float*)ctx->work.ptr, E->d_a4 + E->flat * (size_t)E->gn));
    E->gn += m;
    return F2_OK;
}

// the last dense group, scores / labels to a host caller, and the wait for the stream with the windows' error flag
int eval_cnn_end(f2_ctx* ctx, const f2_cnn* cnn, eval_call* E, float* scores_or_null, uint8_t* labels_or_null) {
    F2_TRY(eval_dense_flush(ctx, cnn, E));
    if (E->host) {
        if (scores_or_null)
            F2_HIP(ctx, hipMemcpyAsync(scores_or_null, E->d_scores, sizeof(float) * 2 * (size_t)E->n_total, hipMemcpyDeviceToHost, ctx->stream));
        if (labels_or_null)
            F2_HIP(ctx, hipMemcpyAsync(labels_or_null, E->d_labels, (size_t)E->n_total, hipMemcpyDeviceToHost, ctx->stream));
    }
    return finish_positive(ctx);
}

}  // namespace

// f2_eval_batch, and f2_eval_utterance as its B = 1 case with the envelope output (env_or_null, in mem_space) and the window
// count (n_windows_out): every-sample windows -> normalise -> conv1 .. conv4, utterance by utterance, chunk by chunk
static int eval_batch_impl(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                           const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step,
                           double* env_or_null, float* scores_or_null, uint8_t* labels_or_null, int64_t* n_windows_out,
                           int mem_space) {
    eval_call E;
    F2_TRY(eval_check(ctx, cnn, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, radius, step, mem_space, &E));
    int64_t nb_total = 0, nb_max = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t nb = offsets[b + 1] - offsets[b] - (int64_t)E.R * step;   // Evaluating.py:73
        if (nb > 0) {
            nb_total += nb;
            nb_max = nb > nb_max ? nb : nb_max;
        }
    }
    if (n_windows_out) *n_windows_out = nb_total;
    if (E.total == 0) return F2_OK;
    F2_TRY(eval_envelopes(ctx, &E, wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, env_or_null, nb_total,
                          mem_space));
    if (nb_total == 0) return F2_OK;
    const int64_t chunk = nb_max < CNN_CHUNK ? nb_max : CNN_CHUNK;
    F2_TRY(eval_cnn_begin(ctx, cnn, &E, chunk, nb_total, C, scores_or_null, labels_or_null));
    const int64_t reach = (int64_t)radius * step;
    for (int b = 0; b < B; ++b) {
        const int64_t N = offsets[b + 1] - offsets[b];
        const int64_t nb = N - (int64_t)E.R * step;
        const double* env_b = E.d_env + (size_t)C * (size_t)offsets[b];
        for (int64_t s = 0; s < nb; s += chunk) {
            const int64_t m = nb - s < chunk ? nb - s : chunk;
            F2_TRY(eval_chunk_room(ctx, cnn, &E, m));
            F2_TRY(f2_launch_gather(ctx, env_b, C, N, nullptr, reach + s, m, radius, step, 1, (float*)ctx->xbuf.ptr,
                                    (int*)ctx->flags.ptr));
            F2_TRY(eval_chunk_convs(ctx, cnn, &E, m));
        }
    }
    return eval_cnn_end(ctx, cnn, &E, scores_or_null, labels_or_null);
}

// windows f2_eval_batch_strided evaluates in an utterance of n samples (R = 2 * radius + 1 rows)
static int64_t strided_windows(int64_t n, int R, int step, int hop) {
    const int64_t nb = n - (int64_t)R * step;
    return nb > 0 ? (nb + hop - 1) / hop : 0;
}

// f2_eval_batch_strided: window j of utterance b is every-sample window j * hop. A chunk is up to CNN_CHUNK windows taken from
// as many utterances as it holds (an utterance may continue in the next chunk): one window-stage launch set and one
// convolution launch set per chunk, whatever B. (On the decimating route a chunk also closes at COLUMN_CAP columns of the
// window stage's scratch - 2 * radius * step / hop columns per segment on top of its windows: 150 MB for 128 channels - which
// only batches of very many very short utterances at a small hop reach.)
static int eval_strided_impl(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                             const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step,
                             int hop, float* scores_or_null, uint8_t* labels_or_null, int64_t* window_offsets_or_null,
                             int mem_space) {
    constexpr int64_t COLUMN_CAP = 8 * CNN_CHUNK;
    eval_call E;
    F2_TRY(eval_check(ctx, cnn, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, radius, step, mem_space, &E));
    F2_CHECK(ctx, hop >= 1, F2_ERR_INVALID, "hop must be at least 1 sample (got %d)", hop);
    std::vector<int64_t> nbh((size_t)B);
    int64_t n_total = 0;
    if (window_offsets_or_null) window_offsets_or_null[0] = 0;
    for (int b = 0; b < B; ++b) {
        nbh[(size_t)b] = strided_windows(offsets[b + 1] - offsets[b], E.R, step, hop);
        n_total += nbh[(size_t)b];
        if (window_offsets_or_null) window_offsets_or_null[b + 1] = n_total;
    }
    if (E.total == 0) return F2_OK;
    F2_TRY(eval_envelopes(ctx, &E, wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, nullptr, n_total, mem_space));
    if (n_total == 0) return F2_OK;
    const int64_t chunk = n_total < CNN_CHUNK ? n_total : CNN_CHUNK;
    F2_TRY(eval_cnn_begin(ctx, cnn, &E, chunk, n_total, C, scores_or_null, labels_or_null));
    const bool columns = f2_gather_strided_blocked(ctx, C, step, hop);
    std::vector<f2_win_seg> segs;
    int64_t m = 0, cols = 0;     // windows and scratch columns of the open chunk
    auto close_chunk = [&]() -> int {
        if (m > 0) {
            F2_TRY(eval_chunk_room(ctx, cnn, &E, m));
            F2_TRY(f2_launch_gather_strided(ctx, E.d_env, C, (const int64_t*)ctx->offsets.ptr, offsets, segs.data(), (int)segs.size(),
                                            radius, step, hop, (float*)ctx->xbuf.ptr, (int*)ctx->flags.ptr));
            F2_TRY(eval_chunk_convs(ctx, cnn, &E, m));
        }
        segs.clear();
        m = cols = 0;
        return F2_OK;
    };
    for (int b = 0; b < B; ++b)
        for (int64_t j = 0; j < nbh[(size_t)b];) {
            int64_t take = nbh[(size_t)b] - j < chunk - m ? nbh[(size_t)b] - j : chunk - m;
            const int64_t c = columns ? f2_gather_strided_columns(take, radius, step, hop) : 0;
            if (m > 0 && cols + c > COLUMN_CAP) {
                F2_TRY(close_chunk());
                continue;
            }
            segs.push_back({b, j, take});
            j += take;
            m += take;
            cols += c;
            if (m == chunk) F2_TRY(close_chunk());
        }
    F2_TRY(close_chunk());
    return eval_cnn_end(ctx, cnn, &E, scores_or_null, labels_or_null);
}

// f2_eval_noise_sweep: the K noisy levels and the clean one of a ragged batch as ONE (K+1) * B-utterance float64 batch in device
// memory (f2_noise.hip), through eval_strided_impl as a device call, then the tally of its labels on the device. Only the clean
// samples go up; sigma, stats and what the caller asked for come back behind one wait.
static int eval_noise_sweep_impl(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                                 const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step,
                                 int hop, const double* snr_db, int K, uint64_t seed, double* noisy_or_null, float* scores_or_null,
                                 uint8_t* labels_or_null, int64_t* window_offsets_or_null, double* sigma_or_null,
                                 int64_t* stats_or_null, int mem_space) {
    eval_call E;
    F2_TRY(eval_check(ctx, cnn, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, radius, step, mem_space, &E));
    F2_CHECK(ctx, hop >= 1, F2_ERR_INVALID, "hop must be at least 1 sample (got %d)", hop);
    F2_CHECK(ctx, K >= 1 && snr_db, F2_ERR_INVALID, "a sweep needs at least one noise level (K=%d) and their snr_db", K);
    for (int k = 0; k < K; ++k) F2_CHECK(ctx, std::isfinite(snr_db[k]), F2_ERR_INVALID, "snr_db[%d] is not finite", k);
    F2_CHECK(ctx, ((int64_t)K + 1) * (B > 0 ? B : 1) <= INT32_MAX / 2, F2_ERR_UNSUPPORTED, "%d levels of %d utterances", K + 1, B);
    F2_CHECK(ctx, wave || E.total == 0, F2_ERR_INVALID, "null wave");
    const int U = (K + 1) * B;
    const int64_t total = E.total;
    // the (K+1) * B batch: the clean offsets tiled, its window offsets, 10^(snr / 10) per level
    std::vector<int64_t> tiled((size_t)U + 1, 0), wo((size_t)U + 1, 0);
    int64_t max_windows = 0;
    for (int l = 0; l <= K; ++l)
        for (int b = 0; b < B; ++b) {
            const size_t u = (size_t)l * B + b;
            const int64_t nw = strided_windows(offsets[b + 1] - offsets[b], E.R, step, hop);
            tiled[u + 1] = (int64_t)l * total + offsets[b + 1];
            wo[u + 1] = wo[u] + nw;
            max_windows = nw > max_windows ? nw : max_windows;
        }
    const int64_t n_total = wo[(size_t)U];
    if (window_offsets_or_null) memcpy(window_offsets_or_null, wo.data(), sizeof(int64_t) * ((size_t)U + 1));
    if (total == 0) {   // nothing to launch: no noise and no window anywhere
        if (sigma_or_null) std::fill(sigma_or_null, sigma_or_null + U, 0.0);
        if (stats_or_null) std::fill(stats_or_null, stats_or_null + 2 * (size_t)U, (int64_t)0);
        return F2_OK;
    }
    std::vector<double> lin((size_t)K);
    for (int k = 0; k < K; ++k) lin[(size_t)k] = std::pow(10.0, snr_db[k] / 10.0);   // Evaluating.py:189 SNRdbToSNRlinear

    // small arrays of the call: [sigma (U) | lin (K) | stats (2 U) | window offsets (U + 1)], all 8-byte words
    F2_TRY(f2_reserve(ctx, ctx->noise_meta, 8 * ((size_t)U + K + 2 * (size_t)U + U + 1)));
    double* d_sigma = (double*)ctx->noise_meta.ptr;
    double* d_lin = d_sigma + U;
    int64_t* d_stats = (int64_t*)(d_lin + K);
    int64_t* d_wo = d_stats + 2 * (size_t)U;
    const size_t noisy_bytes = sizeof(double) * (size_t)(K + 1) * (size_t)total;
    double* d_noisy = noisy_or_null;
    if (E.host || !noisy_or_null) {
        F2_TRY(f2_reserve(ctx, ctx->noise_wave, noisy_bytes));
        d_noisy = (double*)ctx->noise_wave.ptr;
    }
    // scores / labels of the device call below: the caller's device buffers, else staging (the tally always needs the labels)
    float* d_scores = scores_or_null;
    uint8_t* d_labels = labels_or_null;
    if (E.host || !labels_or_null) {
        const bool stage_scores = E.host && scores_or_null;
        F2_TRY(f2_reserve(ctx, ctx->stage_aux, (stage_scores ? sizeof(float) * 2 : 0) * (size_t)n_total + (size_t)n_total + 64));
        if (E.host) d_scores = stage_scores ? (float*)ctx->stage_aux.ptr : nullptr;
        d_labels = (uint8_t*)ctx->stage_aux.ptr + (stage_scores ? sizeof(float) * 2 * (size_t)n_total : 0);
    }
    // the tiled offsets start with the clean ones: one device array serves the noise kernels and the evaluation
    F2_TRY(f2_upload_offsets(ctx, tiled.data(), U));
    F2_TRY(f2_upload_async(ctx, d_lin, lin.data(), sizeof(double) * (size_t)K));
    const void* d_wave;
    F2_TRY(f2_stage_wave(ctx, wave, wave_dtype, total, mem_space, &d_wave));
    const int64_t* d_offsets = (const int64_t*)ctx->offsets.ptr;
    F2_TRY(f2_launch_noise_sigma(ctx, d_wave, wave_dtype, d_offsets, d_lin, B, K, d_sigma));
    F2_TRY(f2_launch_noise_levels(ctx, d_wave, wave_dtype, d_offsets, d_sigma, B, K, total, seed, d_noisy));
    if (E.host && noisy_or_null) F2_HIP(ctx, hipMemcpyAsync(noisy_or_null, d_noisy, noisy_bytes, hipMemcpyDeviceToHost, ctx->stream));
    F2_TRY(eval_strided_impl(ctx, cnn, d_noisy, F2_WAVE_F64, tiled.data(), coefs, U, C, lpf, cutoff_hz, fft_precision, radius, step, hop,
                             d_scores, d_labels, nullptr, F2_MEM_DEVICE));
    F2_HIP(ctx, hipMemsetAsync(d_stats, 0, sizeof(int64_t) * 2 * (size_t)U, ctx->stream));
    if (n_total > 0) {
        F2_TRY(f2_upload_async(ctx, d_wo, wo.data(), sizeof(int64_t) * ((size_t)U + 1)));
        F2_TRY(f2_launch_label_tally(ctx, d_labels, d_wo, B, K, max_windows, d_stats));
        if (E.host && scores_or_null)
            F2_HIP(ctx, hipMemcpyAsync(scores_or_null, d_scores, sizeof(float) * 2 * (size_t)n_total, hipMemcpyDeviceToHost, ctx->stream));
        if (E.host && labels_or_null)
            F2_HIP(ctx, hipMemcpyAsync(labels_or_null, d_labels, (size_t)n_total, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (sigma_or_null) F2_HIP(ctx, hipMemcpyAsync(sigma_or_null, d_sigma, sizeof(double) * (size_t)U, hipMemcpyDeviceToHost, ctx->stream));
    if (stats_or_null)
        F2_HIP(ctx, hipMemcpyAsync(stats_or_null, d_stats, sizeof(int64_t) * 2 * (size_t)U, hipMemcpyDeviceToHost, ctx->stream));
    F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return F2_OK;
}

extern "C" {

int f2_eval_utterance(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, int64_t N, const double* coefs,
                      int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step, double* env_or_null,
                      float* scores_or_null, uint8_t* labels_or_null, int64_t* n_windows_out, int mem_space) {
    if (ctx && !wave) return f2_fail(ctx, F2_ERR_INVALID, "null wave");   // (also for N == 0, unlike f2_eval_batch)
    const int64_t offsets[2] = {0, N};
    return eval_batch_impl(ctx, cnn, wave, wave_dtype, offsets, coefs, 1, C, lpf, cutoff_hz, fft_precision, radius, step,
                           env_or_null, scores_or_null, labels_or_null, n_windows_out, mem_space);
}

int f2_eval_batch(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                  const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step,
                  float* scores_or_null, uint8_t* labels_or_null, int mem_space) {
    return eval_batch_impl(ctx, cnn, wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, radius, step, nullptr,
                           scores_or_null, labels_or_null, nullptr, mem_space);
}

int f2_eval_batch_strided(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                          const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step,
                          int hop, float* scores_or_null, uint8_t* labels_or_null, int64_t* window_offsets_or_null, int mem_space) {
    return eval_strided_impl(ctx, cnn, wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, radius, step, hop,
                             scores_or_null, labels_or_null, window_offsets_or_null, mem_space);
}

int f2_eval_noise_sweep(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                        const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step,
                        int hop, const double* snr_db, int K, uint64_t seed, double* noisy_or_null, float* scores_or_null,
                        uint8_t* labels_or_null, int64_t* window_offsets_or_null, double* sigma_or_null, int64_t* stats_or_null,
                        int mem_space) {
    return eval_noise_sweep_impl(ctx, cnn, wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, radius, step, hop,
                                 snr_db, K, seed, noisy_or_null, scores_or_null, labels_or_null, window_offsets_or_null,
                                 sigma_or_null, stats_or_null, mem_space);
}

int f2_label_accuracy(f2_ctx* ctx, const uint8_t* labels, const int64_t* window_offsets, int U, const int64_t* ref_offsets,
                      const int64_t* ref_timepoints, const uint8_t* ref_signs, int R, int64_t origin, int hop, int step,
                      int64_t* counts, int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_CHECK(ctx, counts, F2_ERR_INVALID, "counts is NULL");
    F2_CHECK(ctx, U >= 0 && R >= (U > 0 ? 1 : 0) && (U == 0 || U % R == 0), F2_ERR_INVALID,
             "%d utterances cannot be scored against %d reference sets in turn", U, R);
    F2_CHECK(ctx, hop >= 1 && step >= 1 && origin >= 0, F2_ERR_INVALID, "hop (%d) and step (%d) must be at least 1, origin (%lld) at least 0",
             hop, step, (long long)origin);
    F2_TRY(f2_check_offsets(ctx, window_offsets, U, "window_offsets"));
    F2_TRY(f2_check_offsets(ctx, ref_offsets, R, "ref_offsets"));
    const int64_t n_rows = window_offsets[U], M = ref_offsets[R];
    F2_CHECK(ctx, labels || n_rows == 0, F2_ERR_INVALID, "null labels");
    F2_CHECK(ctx, (ref_timepoints && ref_signs) || M == 0, F2_ERR_INVALID, "null ref_timepoints or ref_signs");
    for (int r = 0; r < R; ++r)
        for (int64_t i = ref_offsets[r]; i < ref_offsets[r + 1]; ++i) {
            F2_CHECK(ctx, i == ref_offsets[r] || ref_timepoints[i] > ref_timepoints[i - 1], F2_ERR_INVALID,
                     "reference set %d: timepoints must be strictly increasing (label %lld)", r, (long long)(i - ref_offsets[r]));
            F2_CHECK(ctx, ref_signs[i] <= 1, F2_ERR_INVALID, "reference set %d: sign %d of label %lld is neither 0 nor 1", r,
                     (int)ref_signs[i], (long long)(i - ref_offsets[r]));
        }
    int64_t max_rows = 0;
    for (int u = 0; u < U; ++u) max_rows = std::max(max_rows, window_offsets[u + 1] - window_offsets[u]);
    int64_t t_last = 0;   // the timepoint of the last row of the longest utterance has to be an int64
    F2_CHECK(ctx, max_rows == 0 || (!__builtin_mul_overflow(max_rows - 1, (int64_t)hop, &t_last) && !__builtin_add_overflow(t_last, origin, &t_last)),
             F2_ERR_UNSUPPORTED, "row %lld at hop %d from origin %lld is beyond int64", (long long)(max_rows - 1), hop, (long long)origin);
    std::fill(counts, counts + 4 * (size_t)U, (int64_t)0);
    if (n_rows == 0) return F2_OK;

    // small arrays of the call: [counts (4 U) | window offsets (U + 1) | reference offsets (R + 1) | timepoints (M)] in 8-byte
    // words, then the M signs
    F2_TRY(f2_reserve(ctx, ctx->acc_meta, 8 * (4 * (size_t)U + U + 1 + R + 1 + (size_t)M) + (size_t)M));
    int64_t* d_counts = (int64_t*)ctx->acc_meta.ptr;
    int64_t* d_wo = d_counts + 4 * (size_t)U;
    int64_t* d_ro = d_wo + U + 1;
    int64_t* d_rt = d_ro + R + 1;
    uint8_t* d_rs = (uint8_t*)(d_rt + M);
    const uint8_t* d_labels = labels;
    if (mem_space == F2_MEM_HOST) {
        F2_TRY(f2_reserve(ctx, ctx->stage_in, (size_t)n_rows));
        F2_HIP(ctx, hipMemcpyAsync(ctx->stage_in.ptr, labels, (size_t)n_rows, hipMemcpyHostToDevice, ctx->stream));
        d_labels = (const uint8_t*)ctx->stage_in.ptr;
    }
    F2_HIP(ctx, hipMemsetAsync(d_counts, 0, sizeof(int64_t) * 4 * (size_t)U, ctx->stream));
    F2_TRY(f2_upload_async(ctx, d_wo, window_offsets, sizeof(int64_t) * ((size_t)U + 1)));
    F2_TRY(f2_upload_async(ctx, d_ro, ref_offsets, sizeof(int64_t) * ((size_t)R + 1)));
    F2_TRY(f2_upload_async(ctx, d_rt, ref_timepoints, sizeof(int64_t) * (size_t)M));
    F2_TRY(f2_upload_async(ctx, d_rs, ref_signs, (size_t)M));
    F2_TRY(f2_launch_label_accuracy(ctx, d_labels, d_wo, U, d_ro, d_rt, d_rs, R, origin, hop, step, max_rows, d_counts));
    F2_HIP(ctx, hipMemcpyAsync(counts, d_counts, sizeof(int64_t) * 4 * (size_t)U, hipMemcpyDeviceToHost, ctx->stream));
    F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return F2_OK;
}

// f2_cnn_score_windows: chunk by chunk of CNN_CHUNK windows - (upload,) normalise, forward chain, tally - with the windows of a
// chunk, their scores, labels, signs and groups in context scratch where the caller gave host memory or none
int f2_cnn_score_windows(f2_ctx* ctx, const f2_cnn* cnn, const float* windows, int64_t n, int normalize, const uint8_t* signs,
                         const int32_t* groups_or_null, int G, float* scores_or_null, uint8_t* labels_or_null, int64_t* counts,
                         double* loss_sum, int mem_space) {
    constexpr int SCORE_WORD = 1;   // word of ctx->flags the tally kernel ORs into: 1 = a sign above 1, 2 = a group outside [0, G)
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_cnn(ctx, cnn, 0, 0));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_CHECK(ctx, counts && loss_sum, F2_ERR_INVALID, "counts or loss_sum is NULL");
    F2_CHECK(ctx, n >= 0 && G >= 1, F2_ERR_INVALID, "negative window count (%lld) or no group (G=%d)", (long long)n, G);
    F2_CHECK(ctx, normalize == 0 || normalize == 1, F2_ERR_INVALID, "normalize must be 0 or 1 (got %d)", normalize);
    F2_CHECK(ctx, groups_or_null || G == 1, F2_ERR_INVALID, "%d groups but no group array", G);
    F2_CHECK(ctx, (windows && signs) || n == 0, F2_ERR_INVALID, "null windows or signs");
    F2_CHECK(ctx, G <= 1024, F2_ERR_UNSUPPORTED, "%d groups (at most 1024)", G);
    std::fill(counts, counts + 4 * (size_t)G, (int64_t)0);
    std::fill(loss_sum, loss_sum + (size_t)G, 0.0);
    if (n == 0) return F2_OK;

    const bool host = mem_space == F2_MEM_HOST;
    const size_t xs = (size_t)cnn->rows * cnn->channels;
    const int64_t chunk = n < CNN_CHUNK ? n : CNN_CHUNK;
    // small arrays of the call: [counts (4 G) | loss (G) | loss partials of a chunk], all 8-byte words
    F2_TRY(f2_reserve(ctx, ctx->score_meta, 8 * (5 * (size_t)G + f2_score_partial_doubles(chunk, G))));
    int64_t* d_counts = (int64_t*)ctx->score_meta.ptr;
    double* d_loss = (double*)(d_counts + 4 * (size_t)G);
    double* d_partial = d_loss + G;
    // per chunk in stage_aux: [scores (2 floats) | groups (int32) | labels | signs] for what the caller has not got on the device
    const bool own_scores = host || !scores_or_null, own_labels = host || !labels_or_null;
    F2_TRY(f2_reserve(ctx, ctx->stage_aux, (sizeof(float) * 2 + sizeof(int32_t) + 2) * (size_t)chunk + 64));
    float* s_scores = (float*)ctx->stage_aux.ptr;
    int32_t* s_groups = (int32_t*)(s_scores + 2 * chunk);
    uint8_t* s_labels = (uint8_t*)(s_groups + chunk);
    uint8_t* s_signs = s_labels + chunk;
    if (host) F2_TRY(f2_reserve(ctx, ctx->stage_in, sizeof(float) * xs * (size_t)chunk));
    if (normalize) F2_TRY(f2_reserve(ctx, ctx->xbuf, sizeof(float) * xs * (size_t)chunk));

    // normalised windows lie in [0, 1]: the B = 1 scale set without the range pass, as in f2_eval_*; windows as they are take
    // f2_cnn_forward's route - the range of the whole call for device memory, of each chunk for host memory, as there
    const f2_scale_set* S = nullptr;
    f2_cnn_route route;
    double bound = host ? 0.0 : -1.0;   // normalize = 0: what f2_cnn_forward leaves in last_input_bound (host: largest B of the chunks)
    if (normalize) {
        F2_TRY(f2_cnn_scale_set(ctx, cnn, 0, &S));
        route = f2_cnn_call_route(ctx, cnn, S != nullptr);
    } else if (!host) {
        F2_TRY(forward_route(ctx, cnn, windows, n, &S, &route, &bound));
    }

    F2_HIP(ctx, hipMemsetAsync(d_counts, 0, 8 * 5 * (size_t)G, ctx->stream));
    F2_HIP(ctx, hipMemsetAsync((int*)ctx->flags.ptr + SCORE_WORD, 0, sizeof(int), ctx->stream));
    F2_TRY(reset_flag(ctx));
    for (int64_t s = 0; s < n; s += chunk) {
        const int64_t m = n - s < chunk ? n - s : chunk;
        const float* d_w = windows + (size_t)s * xs;
        const uint8_t* d_signs = signs + s;
        const int32_t* d_groups = groups_or_null ? groups_or_null + s : nullptr;
        if (host) {
            // The windows (up to 92 MB a chunk) go up straight from the caller's memory, as in f2_cnn_forward: the pinned buffers
            // of f2_upload_async would cost a host copy of every chunk first. The caller's memory is only read and outlives the
            // copies (the call waits for the stream before it returns); stage_in / stage_aux are reused in stream order, behind the
            // kernels of the chunk before, so the chunks need no wait of their own. Signs and groups: the pinned ring.
            F2_HIP(ctx, hipMemcpyAsync(ctx->stage_in.ptr, d_w, sizeof(float) * xs * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
            F2_TRY(f2_upload_async(ctx, s_signs, d_signs, (size_t)m));
            if (d_groups) {
                F2_TRY(f2_upload_async(ctx, s_groups, d_groups, sizeof(int32_t) * (size_t)m));
                d_groups = s_groups;
            }
            d_w = (const float*)ctx->stage_in.ptr;
            d_signs = s_signs;
        }
        if (normalize) {
            F2_TRY(f2_launch_normalize_windows(ctx, d_w, m, (int)xs, (float*)ctx->xbuf.ptr, (int*)ctx->flags.ptr));
            d_w = (const float*)ctx->xbuf.ptr;
        } else if (host) {
            double b = -1.0;
            F2_TRY(forward_route(ctx, cnn, d_w, m, &S, &route, &b));
            bound = chunks_bound(bound, b);
        }
        float* d_scores = own_scores ? s_scores : scores_or_null + 2 * s;
        uint8_t* d_labels = own_labels ? s_labels : labels_or_null + s;
        F2_TRY(cnn_forward_device(ctx, cnn, S, route, d_w, m, d_scores, d_labels));
        F2_TRY(f2_launch_score_tally(ctx, d_scores, d_labels, d_signs, d_groups, G, m, d_counts, d_partial, d_loss,
                                     (int*)ctx->flags.ptr + SCORE_WORD));
        if (host && scores_or_null)
            F2_HIP(ctx, hipMemcpyAsync(scores_or_null + 2 * s, d_scores, sizeof(float) * 2 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        if (host && labels_or_null)
            F2_HIP(ctx, hipMemcpyAsync(labels_or_null + s, d_labels, (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (!normalize) cnn->last_input_bound = bound;   // (normalize = 1 measures nothing and leaves it alone, as f2_eval_* do)
    F2_HIP(ctx, hipMemcpyAsync(counts, d_counts, sizeof(int64_t) * 4 * (size_t)G, hipMemcpyDeviceToHost, ctx->stream));
    F2_HIP(ctx, hipMemcpyAsync(loss_sum, d_loss, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost, ctx->stream));
    F2_HIP(ctx, hipMemcpyAsync(ctx->host_flags + SCORE_WORD, (int*)ctx->flags.ptr + SCORE_WORD, sizeof(int), hipMemcpyDeviceToHost,
                               ctx->stream));
    F2_TRY(finish_positive(ctx));
    const int wrong = ctx->host_flags[SCORE_WORD];
    F2_CHECK(ctx, !(wrong & 1), F2_ERR_INVALID, "a sign is neither 0 nor 1");
    F2_CHECK(ctx, !(wrong & 2), F2_ERR_INVALID, "a group lies outside [0, %d)", G);
    return F2_OK;
}

int f2_input_batch(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C,
                   int lpf, double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers,
                   int radius, int step, int normalize, float* windows, int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_TRY(f2_check_dsp(ctx, wave_dtype, lpf, cutoff_hz, fft_precision));
    F2_CHECK(ctx, B >= 0 && C > 0 && radius >= 0 && step >= 0, F2_ERR_INVALID, "bad size");
    if (B == 0) return F2_OK;      // (before the offsets are looked at: they may be NULL then)
    F2_TRY(f2_check_offsets(ctx, offsets, B, "offsets"));
    F2_TRY(f2_check_offsets(ctx, center_offsets, B, "center_offsets"));
    const int64_t n_windows = center_offsets[B];
    if (n_windows == 0) return F2_OK;
    F2_CHECK(ctx, wave && coefs && centers && windows, F2_ERR_INVALID, "null data pointer");
    // InputGenerator.py:73-80 indexes each utterance's own envelope: a window must lie inside it
    const int64_t reach = (int64_t)radius * step;
    std::vector<int> win_utt((size_t)n_windows);
    for (int b = 0; b < B; ++b) {
        const int64_t nb = offsets[b + 1] - offsets[b];
        for (int64_t e = center_offsets[b]; e < center_offsets[b + 1]; ++e) {
            F2_CHECK(ctx, centers[e] - reach >= 0 && centers[e] + reach < nb, F2_ERR_INVALID,
                     "utterance %d: window %lld (centre %lld, +-%lld) reaches outside its %lld-sample envelope", b,
                     (long long)(e - center_offsets[b]), (long long)centers[e], (long long)reach, (long long)nb);
            win_utt[(size_t)e] = b;
        }
    }
    const int64_t total = offsets[B];
    const int R = 2 * radius + 1;

    // envelopes of the whole batch, by the routes of f2_filterbank_envelope_fused (gfb_or_null = NULL), into a scratch buffer
    F2_TRY(f2_upload_offsets(ctx, offsets, B));
    F2_TRY(f2_upload_coefs(ctx, coefs, C));
    F2_TRY(f2_reserve(ctx, ctx->stage_out, sizeof(double) * (size_t)C * (size_t)total));
    double* d_env = (double*)ctx->stage_out.ptr;
    const void* d_wave;
    F2_TRY(f2_stage_wave(ctx, wave, wave_dtype, total, mem_space, &d_wave));
    F2_TRY(f2_envelopes_device(ctx, d_wave, wave_dtype, offsets, B, C, lpf, cutoff_hz, fft_precision, d_env, nullptr, true));

    // all windows of the batch in one gather launch: centres and the utterance of every window in one upload
    const int64_t* d_centers;
    const int* d_win_utt;
    F2_TRY(f2_upload_windows(ctx, centers, win_utt.data(), n_windows, &d_centers, &d_win_utt));
    const size_t out_bytes = sizeof(float) * (size_t)n_windows * R * (size_t)C;
    float* d_out = windows;
    if (mem_space == F2_MEM_HOST) {
        F2_TRY(f2_reserve(ctx, ctx->xbuf, out_bytes));
        d_out = (float*)ctx->xbuf.ptr;
    }
    F2_TRY(reset_flag(ctx));
    F2_TRY(f2_launch_gather_ragged(ctx, d_env, C, (const int64_t*)ctx->offsets.ptr, d_centers, d_win_utt, n_windows, radius, step,
                                   normalize, d_out, (int*)ctx->flags.ptr));
    if (mem_space == F2_MEM_HOST) F2_HIP(ctx, hipMemcpyAsync(windows, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    return normalize || mem_space == F2_MEM_HOST ? finish_positive(ctx) : F2_OK;
}

}  // extern "C"

// ---- gammatonegram pictures: f2_envelope_picture and f2_gammatonegram_batch share everything behind the envelopes ----
namespace {

constexpr int PICTURE_MAX_WIDTH = 65536;

// the argument errors of both calls (include/f2cnn_hip.h: f2_envelope_picture) apart from the data pointers; nothing is launched
// or written before they pass
int picture_check(f2_ctx* ctx, const int64_t* offsets, int B, int C, const int64_t* spans_or_null, int width, int pool, int mem_space) {
    F2_TRY(f2_check_batch(ctx, offsets, B, C, mem_space, true));
    F2_CHECK(ctx, width >= 1, F2_ERR_INVALID, "a picture needs at least one column (width=%d)", width);
    F2_CHECK(ctx, pool == 0 || pool == 1, F2_ERR_INVALID, "pool must be 0 (mean) or 1 (maximum), got %d", pool);
    F2_CHECK(ctx, width <= PICTURE_MAX_WIDTH, F2_ERR_UNSUPPORTED, "width %d (at most %d columns)", width, PICTURE_MAX_WIDTH);
    if (spans_or_null)
        for (int b = 0; b < B; ++b) {
            const int64_t nb = offsets[b + 1] - offsets[b], s = spans_or_null[2 * b], e = spans_or_null[2 * b + 1];
            F2_CHECK(ctx, s >= 0 && e >= s && e <= nb, F2_ERR_INVALID, "utterance %d: span [%lld, %lld) does not lie inside its %lld samples",
                     b, (long long)s, (long long)e, (long long)nb);
        }
    return F2_OK;
}

// Pool, levels and range of the envelopes at d_env (device; offsets already uploaded), results to the caller's buffers in mem_space.
// Pictures a host caller asked for, and the pooled values the levels are made from when nobody asked for them, live in ctx->work /
// ctx->work2. Waits for the stream.
int picture_device(f2_ctx* ctx, const double* d_env, const int64_t* offsets, int B, int C, const int64_t* spans_or_null, int width,
                   int pool, double* pooled_or_null, uint8_t* levels_or_null, double* range_or_null, int mem_space) {
    const bool host = mem_space == F2_MEM_HOST;
    const size_t pixels = (size_t)B * (size_t)C * (size_t)width;
    // small arrays of the call: [span records (4 B) | range words (2 B)], all 8-byte words, in one upload
    std::vector<int64_t> meta(6 * (size_t)B);
    int64_t blocks = 0;   // per utterance: what the one with the shortest bins needs
    const double inf = INFINITY;
    for (int b = 0; b < B; ++b) {
        const int64_t s = spans_or_null ? spans_or_null[2 * b] : 0;
        const int64_t m = (spans_or_null ? spans_or_null[2 * b + 1] : offsets[b + 1] - offsets[b]) - s;
        const int lg = f2_picture_lanes_log2(m, width);
        int64_t* u = &meta[4 * (size_t)b];
        u[0] = s, u[1] = m, u[2] = m / width, u[3] = (m % width) << 8 | lg;
        blocks = std::max(blocks, f2_picture_pool_blocks(C, width, lg));
        memcpy(&meta[4 * (size_t)B + 2 * (size_t)b], &inf, sizeof(double));   // (the maximum's word stays 0)
    }
    F2_TRY(f2_reserve(ctx, ctx->pic_meta, sizeof(int64_t) * meta.size()));
    const int64_t* d_utt = (const int64_t*)ctx->pic_meta.ptr;
    uint64_t* d_range = (uint64_t*)ctx->pic_meta.ptr + 4 * (size_t)B;
    double* d_pooled = pooled_or_null;
    if (host || !pooled_or_null) {
        F2_TRY(f2_reserve(ctx, ctx->work, sizeof(double) * pixels));
        d_pooled = (double*)ctx->work.ptr;
    }
    uint8_t* d_levels = levels_or_null;
    if (host && levels_or_null) {
        F2_TRY(f2_reserve(ctx, ctx->work2, pixels));
        d_levels = (uint8_t*)ctx->work2.ptr;
    }
    F2_TRY(f2_upload_async(ctx, ctx->pic_meta.ptr, meta.data(), sizeof(int64_t) * meta.size()));
    F2_TRY(f2_launch_picture_pool(ctx, d_env, (const int64_t*)ctx->offsets.ptr, d_utt, B, C, width, pool, blocks, d_pooled, d_range));
    if (levels_or_null) F2_TRY(f2_launch_picture_levels(ctx, d_pooled, d_range, B, C, width, d_levels));
    if (host && pooled_or_null) F2_HIP(ctx, hipMemcpyAsync(pooled_or_null, d_pooled, sizeof(double) * pixels, hipMemcpyDeviceToHost, ctx->stream));
    if (host && levels_or_null) F2_HIP(ctx, hipMemcpyAsync(levels_or_null, d_levels, pixels, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<double> r(2 * (size_t)B);
    if (range_or_null) F2_HIP(ctx, hipMemcpyAsync(r.data(), d_range, sizeof(double) * r.size(), hipMemcpyDeviceToHost, ctx->stream));
    F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (range_or_null)
        for (int b = 0; b < B; ++b) {   // no pixel > 0: the maximum's word is still 0, the minimum's still +inf
            const bool any = r[2 * (size_t)b + 1] > 0.0;
            range_or_null[2 * b] = any ? r[2 * (size_t)b] : 0.0;
            range_or_null[2 * b + 1] = any ? r[2 * (size_t)b + 1] : 0.0;
        }
    return F2_OK;
}

}  // namespace

extern "C" {

int f2_envelope_picture(f2_ctx* ctx, const double* env, const int64_t* offsets, int B, int C, const int64_t* spans_or_null, int width,
                        int pool, double* pooled_or_null, uint8_t* levels_or_null, double* range_or_null, int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(picture_check(ctx, offsets, B, C, spans_or_null, width, pool, mem_space));
    const int64_t total = offsets[B];
    F2_CHECK(ctx, env || total == 0, F2_ERR_INVALID, "null env");
    if (B == 0 || !(pooled_or_null || levels_or_null || range_or_null)) return F2_OK;
    F2_TRY(f2_upload_offsets(ctx, offsets, B));
    const double* d_env = env;
    if (mem_space == F2_MEM_HOST && total > 0) {
        const size_t bytes = sizeof(double) * (size_t)C * (size_t)total;
        F2_TRY(f2_reserve(ctx, ctx->stage_aux, bytes));
        F2_HIP(ctx, hipMemcpyAsync(ctx->stage_aux.ptr, env, bytes, hipMemcpyHostToDevice, ctx->stream));
        d_env = (const double*)ctx->stage_aux.ptr;
    }
    return picture_device(ctx, d_env, offsets, B, C, spans_or_null, width, pool, pooled_or_null, levels_or_null, range_or_null, mem_space);
}

int f2_gammatonegram_batch(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C,
                           int lpf, double cutoff_hz, int fft_precision, const int64_t* spans_or_null, int width, int pool,
                           double* pooled_or_null, uint8_t* levels_or_null, double* range_or_null, int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_dsp(ctx, wave_dtype, lpf, cutoff_hz, fft_precision));
    F2_TRY(picture_check(ctx, offsets, B, C, spans_or_null, width, pool, mem_space));
    const int64_t total = offsets[B];
    F2_CHECK(ctx, (wave && coefs) || total == 0, F2_ERR_INVALID, "null wave or coefs");
    if (B == 0 || !(pooled_or_null || levels_or_null || range_or_null)) return F2_OK;
    // envelopes of the whole batch, by the routes of f2_filterbank_envelope_fused (gfb_or_null = NULL), into a scratch buffer
    F2_TRY(f2_upload_offsets(ctx, offsets, B));
    double* d_env = nullptr;
    if (total > 0) {
        F2_TRY(f2_upload_coefs(ctx, coefs, C));
        F2_TRY(f2_reserve(ctx, ctx->stage_out, sizeof(double) * (size_t)C * (size_t)total));
        d_env = (double*)ctx->stage_out.ptr;
        const void* d_wave;
        F2_TRY(f2_stage_wave(ctx, wave, wave_dtype, total, mem_space, &d_wave));
        F2_TRY(f2_envelopes_device(ctx, d_wave, wave_dtype, offsets, B, C, lpf, cutoff_hz, fft_precision, d_env, nullptr, true));
    }
    return picture_device(ctx, d_env, offsets, B, C, spans_or_null, width, pool, pooled_or_null, levels_or_null, range_or_null, mem_space);
}

}  // extern "C"

// ---- f2_resample_batch: recordings of any rate, PCM format and channel count to mono float64 at the model's rate ----
namespace {

constexpr int64_t RESAMPLE_MAX_RATIO_TERM = int64_t(1) << 22;   // up, down
constexpr int64_t RESAMPLE_MAX_TABLE = int64_t(1) << 22;        // values of the polyphase table (32 MB)
constexpr int64_t RESAMPLE_MAX_FRAMES = int64_t(1) << 40;       // per utterance: n * up stays inside int64

int64_t gcd64(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b, b = t;
    }
    return a;
}

// The polyphase table of (up, down, half_len, taps) in ctx->rs_tab (f2_internal.h: f2_launch_resample), rebuilt and uploaded only
// when one of them differs from the previous call's.
int resample_table(f2_ctx* ctx, int64_t up, int64_t down, const double* taps, int64_t half_len, int64_t T) {
    const size_t ntaps = (size_t)(2 * half_len + 1);
    if (ctx->rs_up == up && ctx->rs_down == down && ctx->rs_half_len == half_len && ctx->rs_taps_host.size() == ntaps &&
        memcmp(ctx->rs_taps_host.data(), taps, sizeof(double) * ntaps) == 0)
        return F2_OK;
    ctx->rs_half_len = -1;
    std::vector<double> table((size_t)up * (size_t)T);
    for (int64_t p = 0; p < up; ++p)
        for (int64_t s = 0; s < T; ++s) {
            const int64_t idx = p + (T - 1 - s) * up;
            table[(size_t)(p * T + s)] = idx <= 2 * half_len ? taps[idx] : 0.0;
        }
    F2_TRY(f2_reserve(ctx, ctx->rs_tab, sizeof(double) * table.size()));
    F2_TRY(f2_upload_async(ctx, ctx->rs_tab.ptr, table.data(), sizeof(double) * table.size()));
    ctx->rs_taps_host.assign(taps, taps + ntaps);
    ctx->rs_up = up, ctx->rs_down = down, ctx->rs_half_len = half_len;
    return F2_OK;
}

}  // namespace

extern "C" {

int f2_resample_batch(f2_ctx* ctx, const void* audio, int pcm_format, int channels, int channel, const int64_t* offsets, int B,
                      int64_t up, int64_t down, const double* taps, int64_t half_len, double* out, int64_t* out_offsets,
                      int mem_space) {
    static const size_t elem_bytes[] = {1, 2, 4, 4, 8};
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_batch(ctx, offsets, B, channels, mem_space, true));
    F2_CHECK(ctx, channel >= -1 && channel < channels, F2_ERR_INVALID, "channel %d of %d (-1: the mean of all)", channel, channels);
    F2_CHECK(ctx, pcm_format >= F2_PCM_U8 && pcm_format <= F2_PCM_F64, F2_ERR_INVALID, "bad pcm_format %d", pcm_format);
    F2_CHECK(ctx, up >= 1 && down >= 1 && half_len >= 0, F2_ERR_INVALID, "bad ratio %lld / %lld or filter half length %lld",
             (long long)up, (long long)down, (long long)half_len);
    F2_CHECK(ctx, gcd64(up, down) == 1, F2_ERR_INVALID, "up = %lld and down = %lld are not coprime", (long long)up, (long long)down);
    F2_CHECK(ctx, out_offsets, F2_ERR_INVALID, "out_offsets is NULL");
    const bool identity = up == 1 && down == 1;
    F2_CHECK(ctx, taps || identity, F2_ERR_INVALID, "null taps");
    const int64_t total = offsets[B];
    F2_CHECK(ctx, audio || total == 0, F2_ERR_INVALID, "null audio");
    // what the kernel covers
    int64_t T = 0;
    if (!identity) {
        F2_CHECK(ctx, up <= RESAMPLE_MAX_RATIO_TERM && down <= RESAMPLE_MAX_RATIO_TERM, F2_ERR_UNSUPPORTED,
                 "ratio %lld / %lld: up and down may be at most %lld", (long long)up, (long long)down, (long long)RESAMPLE_MAX_RATIO_TERM);
        F2_CHECK(ctx, half_len <= RESAMPLE_MAX_TABLE, F2_ERR_UNSUPPORTED, "filter of %lld taps: the polyphase table may hold at most %lld values",
                 (long long)half_len, (long long)RESAMPLE_MAX_TABLE);
        T = (2 * half_len + up) / up;       // ceil((2 half_len + 1) / up) taps per phase
        F2_CHECK(ctx, up * T <= RESAMPLE_MAX_TABLE, F2_ERR_UNSUPPORTED, "polyphase table of %lld x %lld values (at most %lld)", (long long)up,
                 (long long)T, (long long)RESAMPLE_MAX_TABLE);
        const int64_t span = f2_resample_span(up, down, T);
        F2_CHECK(ctx, span <= F2_RESAMPLE_SPAN_MAX, F2_ERR_UNSUPPORTED,
                 "ratio %lld / %lld with %lld taps per phase: %d outputs need %lld input frames (at most %d are staged per workgroup)",
                 (long long)up, (long long)down, (long long)T, F2_RESAMPLE_BLOCK, (long long)span, F2_RESAMPLE_SPAN_MAX);
    }
    for (int b = 0; b < B; ++b)
        F2_CHECK(ctx, offsets[b + 1] - offsets[b] < RESAMPLE_MAX_FRAMES, F2_ERR_UNSUPPORTED, "utterance %d has %lld frames (at most 2^40 - 1)",
                 b, (long long)(offsets[b + 1] - offsets[b]));
    // per-utterance records and the workgroup prefix, the output offsets
    std::vector<int64_t> meta(4 * (size_t)B + (size_t)B + 1);
    std::vector<int64_t> oo((size_t)B + 1, 0);
    int64_t* first = &meta[4 * (size_t)B];
    first[0] = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b], n_out = (n * up + down - 1) / down;
        int64_t* u = &meta[4 * (size_t)b];
        u[0] = offsets[b], u[1] = n, u[2] = oo[b], u[3] = n_out;
        oo[b + 1] = oo[b] + n_out;
        first[b + 1] = first[b] + (n_out + F2_RESAMPLE_BLOCK - 1) / F2_RESAMPLE_BLOCK;
    }
    const int64_t total_out = oo[B];
    F2_CHECK(ctx, out || total_out == 0, F2_ERR_INVALID, "null out");
    memcpy(out_offsets, oo.data(), sizeof(int64_t) * ((size_t)B + 1));
    if (B == 0 || total_out == 0) return F2_OK;

    const bool host = mem_space == F2_MEM_HOST;
    const void* d_audio;
    F2_TRY(f2_stage_input(ctx, audio, elem_bytes[pcm_format] * (size_t)channels * (size_t)total, mem_space, &d_audio));
    double* d_out = out;
    if (host) {
        F2_TRY(f2_reserve(ctx, ctx->stage_out, sizeof(double) * (size_t)total_out));
        d_out = (double*)ctx->stage_out.ptr;
    }
    if (identity) {
        F2_TRY(f2_launch_pcm_convert(ctx, d_audio, pcm_format, channels, channel, total, d_out));
    } else {
        F2_TRY(resample_table(ctx, up, down, taps, half_len, T));
        F2_TRY(f2_reserve(ctx, ctx->rs_meta, sizeof(int64_t) * meta.size()));
        F2_TRY(f2_upload_async(ctx, ctx->rs_meta.ptr, meta.data(), sizeof(int64_t) * meta.size()));
        F2_TRY(f2_launch_resample(ctx, d_audio, pcm_format, channels, channel, (const int64_t*)ctx->rs_meta.ptr, B, first[B], up, down,
                                  half_len, (int)T, (const double*)ctx->rs_tab.ptr, d_out));
    }
    if (host) {
        F2_HIP(ctx, hipMemcpyAsync(out, d_out, sizeof(double) * (size_t)total_out, hipMemcpyDeviceToHost, ctx->stream));
        F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return F2_OK;
}

}  // extern "C"
