// C-ABI entry points for the window gather (K3), the CNN forward (K4) and the `cnn eval` device pipeline
// (scripts/CNN/Evaluating.py:42-87): host/device pointer handling, chunking, error flags. Host code only.
#include "f2_internal.h"

#include <algorithm>
#include <cmath>

int f2_reset_flag(f2_ctx* ctx) {
    F2_HIP(ctx, hipMemsetAsync(ctx->flags.ptr, 0, sizeof(int), ctx->stream));
    return F2_OK;
}

int f2_finish_positive(f2_ctx* ctx) {
    F2_HIP(ctx, hipMemcpyAsync(ctx->host_flags, ctx->flags.ptr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    F2_CHECK(ctx, !ctx->host_flags[0], F2_ERR_NONPOSITIVE, "values must all be positive (normalizeInput)");
    return F2_OK;
}

namespace {

constexpr int64_t CNN_CHUNK = 16384;  // windows per CNN launch group (activation workspace 1.75 GB, windows 92 MB)
constexpr int64_t DENSE_GROUP = 8 * CNN_CHUNK;   // windows per dense1 / dense2 launch of f2_eval_batch (conv4 + dense1 outputs: 1.3 GB)

// the end of a call that gathers windows: their copy to a host caller; a host call and a normalising one wait (f2_finish_positive)
int finish_windows(f2_ctx* ctx, const f2_output& win, int normalize) {
    F2_TRY(f2_copy_back(ctx, win));
    return normalize || win.host ? f2_finish_positive(ctx) : F2_OK;
}

// The tail of a window call, behind its checks, stagings and uploads: the n_windows windows of 2 * radius + 1 rows and C channels
// are placed (ctx->xbuf, or the caller's device buffer), the flag is reset, gather(d_windows) enqueues what writes them, and the
// call ends as finish_windows says
template <class Gather>
int window_tail(f2_ctx* ctx, float* windows, int64_t n_windows, int radius, int C, int normalize, int mem_space, Gather gather) {
    f2_output win;
    F2_TRY(f2_place(ctx, ctx->xbuf, windows, sizeof(float) * (size_t)n_windows * (2 * radius + 1) * (size_t)C, mem_space, true, &win));
    F2_TRY(f2_reset_flag(ctx));
    F2_TRY(gather(win.as<float>()));
    return finish_windows(ctx, win, normalize);
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

// The range pass over the nwin windows at d_x and the scale set of its bound: B = 1 for max |x| <= 1, else B = 2^ceil(log2 max |x|),
// and *bound = B. *S = NULL and *bound = -1 after inf / NaN, for a B whose scales leave the clamp (or a network without the split
// path), or when B > 2^QUIET_BINADES and a window's max |x| lies below B / 2^QUIET_BINADES.
int measured_scale_set(f2_ctx* ctx, const f2_cnn* cnn, const float* d_x, int64_t nwin, const f2_scale_set** S, double* bound) {
    *S = nullptr;
    *bound = -1.0;
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
    return F2_OK;
}

// Scale set, route and last_input_bound of f2_cnn_forward (and of f2_cnn_score_windows without normalisation) for the nwin windows
// at d_x. The split path's scales follow the input (f2_cnn_split.h), so the windows are measured (measured_scale_set) - unless the
// float32 kernels run whatever the input. *S = NULL, the float32 route and *bound = -1 without the split path and for the inputs
// measured_scale_set has no set for.
int forward_route(f2_ctx* ctx, const f2_cnn* cnn, const float* d_x, int64_t nwin, const f2_scale_set** S, f2_cnn_route* route,
                  double* bound) {
    *S = nullptr;
    *route = f2_cnn_route();
    *bound = -1.0;
    if (!f2_cnn_call_route(ctx, cnn, true).split) return F2_OK;
    F2_TRY(measured_scale_set(ctx, cnn, d_x, nwin, S, bound));
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
    f2_output win;
    F2_TRY(f2_place(ctx, ctx->stage_out, out, sizeof(float) * (size_t)n_windows * R * (size_t)C, mem_space, true, &win));
    const void* d_env;
    F2_TRY(f2_stage_input(ctx, env, sizeof(double) * (size_t)C * (size_t)N, mem_space, &d_env));
    F2_TRY(f2_reset_flag(ctx));
    F2_TRY(f2_launch_gather(ctx, (const double*)d_env, C, N, d_centers, reach, n_windows, radius, step, normalize, win.as<float>(),
                            (int*)ctx->flags.ptr));
    return finish_windows(ctx, win, normalize);
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
    // Device memory: one range pass and one route for the whole call. Host memory: chunk by chunk through stage_in, each chunk
    // with its own range pass and route, its scores and labels back before the next one goes up.
    const int64_t chunk = mem_space == F2_MEM_DEVICE || n < CNN_CHUNK ? n : CNN_CHUNK;
    f2_score_outputs out;
    F2_TRY(f2_place_scores(ctx, scores, labels, chunk, mem_space, false, false, 0, &out));
    double bound = 0.0;   // largest B of the chunks, -1 once one of them ran on the float32 kernels
    for (int64_t s = 0; s < n; s += chunk) {
        const int64_t m = n - s < chunk ? n - s : chunk;
        const void* d_x;
        F2_TRY(f2_stage_input(ctx, x + (size_t)s * xs, sizeof(float) * xs * (size_t)m, mem_space, &d_x));
        const f2_scale_set* S = nullptr;
        f2_cnn_route route;
        double b = -1.0;
        F2_TRY(forward_route(ctx, cnn, (const float*)d_x, m, &S, &route, &b));
        bound = chunks_bound(bound, b);
        const f2_output sc = out.scores.chunk(sizeof(float) * 2 * (size_t)s, sizeof(float) * 2 * (size_t)m), lb = out.labels.chunk((size_t)s, (size_t)m);
        F2_TRY(cnn_forward_device(ctx, cnn, S, route, (const float*)d_x, m, sc.as<float>(), lb.as<uint8_t>()));
        F2_TRY(f2_copy_back(ctx, sc));
        F2_TRY(f2_copy_back(ctx, lb));
        F2_TRY(f2_host_wait(ctx, mem_space));
    }
    cnn->last_input_bound = bound;
    return F2_OK;
}

// The inspection entry: one launch group of f2_cnn_forward's kernels on a named route, with conv4's pooled output and dense1's
// output copied out of the workspace. Every refusal comes before the first output byte is written.
int f2_cnn_layers(f2_ctx* ctx, const f2_cnn* cnn, const float* x, int64_t n, int route, float* pooled_or_null, float* dense1_or_null,
                  float* scores_or_null, int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_cnn(ctx, cnn, 0, 0));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_CHECK(ctx, n >= 0, F2_ERR_INVALID, "negative window count");
    F2_CHECK(ctx, route >= F2_CNN_ROUTE_CALL && route <= F2_CNN_ROUTE_RECORDED, F2_ERR_INVALID, "bad route %d", route);
    if (n == 0) return F2_OK;
    F2_CHECK(ctx, x, F2_ERR_INVALID, "x is NULL");
    F2_CHECK(ctx, n <= CNN_CHUNK, F2_ERR_UNSUPPORTED, "%lld windows: f2_cnn_layers takes at most %lld", (long long)n, (long long)CNN_CHUNK);
    const bool recorded = route == F2_CNN_ROUTE_RECORDED;
    f2_cnn_route want;   // of a forced route
    want.split = !recorded && route >= F2_CNN_ROUTE_TILE, want.ws = !recorded && route >= F2_CNN_ROUTE_WS, want.ws_dense = route == F2_CNN_ROUTE_WS_DENSE;
    const f2_cnn_route can = f2_cnn_capability(cnn);
    F2_CHECK(ctx, (can.split || !want.split) && (can.ws || !want.ws) && (can.ws_dense || !want.ws_dense), F2_ERR_UNSUPPORTED,
             "this %d x %d network does not run on route %d (split %d, weight-stationary %d, its dense1 %d)", cnn->rows, cnn->channels,
             route, (int)can.split, (int)can.ws, (int)can.ws_dense);
    const size_t xs = (size_t)cnn->rows * cnn->channels, flat = f2_cnn_flat_floats(cnn), d1 = f2_cnn_dense_floats(cnn) - flat;
    F2_CHECK(ctx, !want.ws_dense || f2_dense1_ws_takes((int)flat, n), F2_ERR_UNSUPPORTED, "k_dense1_ws does not take %lld windows of %zu",
             (long long)n, flat);
    const void* d_x;
    F2_TRY(f2_stage_input(ctx, x, sizeof(float) * xs * (size_t)n, mem_space, &d_x));
    const f2_scale_set* S = nullptr;
    f2_cnn_route r;
    double b = -1.0;
    if (route == F2_CNN_ROUTE_CALL) {
        F2_TRY(forward_route(ctx, cnn, (const float*)d_x, n, &S, &r, &b));
    } else if (want.split) {
        F2_TRY(measured_scale_set(ctx, cnn, (const float*)d_x, n, &S, &b));
        F2_CHECK(ctx, S, F2_ERR_UNSUPPORTED, "no scale set of the split path for this input (inf / NaN, or out of its range)");
        r = want;
    }
    f2_output po, do1;
    f2_score_outputs so;
    F2_TRY(f2_place(ctx, ctx->stage_out, pooled_or_null, sizeof(float) * flat * (size_t)n, mem_space, false, &po));
    F2_TRY(f2_place(ctx, ctx->work2, dense1_or_null, sizeof(float) * d1 * (size_t)n, mem_space, false, &do1));
    F2_TRY(f2_place_scores(ctx, scores_or_null, nullptr, n, mem_space, false, false, 0, &so));
    if (recorded) {
        // the gradient chain's forward, chunk by chunk through its own scratch: what it recorded is copied out before the next chunk
        const int64_t chunk = f2_cnn_grad_chunk(cnn);
        for (int64_t s = 0; s < n; s += chunk) {
            const int64_t m = n - s < chunk ? n - s : chunk;
            float* sc = so.scores.dev ? so.scores.as<float>() + 2 * (size_t)s : nullptr;
            F2_TRY(f2_launch_cnn_input_gradient(ctx, cnn, (const float*)d_x + (size_t)s * xs, m, nullptr, nullptr, sc));
            const float *p2, *a5;
            f2_cnn_grad_recorded(ctx, cnn, m, &p2, &a5);
            if (po.dev)
                F2_HIP(ctx, hipMemcpyAsync(po.as<float>() + flat * (size_t)s, p2, sizeof(float) * flat * (size_t)m, hipMemcpyDeviceToDevice, ctx->stream));
            if (do1.dev)
                F2_HIP(ctx, hipMemcpyAsync(do1.as<float>() + d1 * (size_t)s, a5, sizeof(float) * d1 * (size_t)m, hipMemcpyDeviceToDevice, ctx->stream));
        }
    } else {
        const size_t per = f2_cnn_workspace_floats(cnn);
        F2_TRY(f2_reserve(ctx, ctx->work, sizeof(float) * per * (size_t)n));
        float* d_ws = (float*)ctx->work.ptr;
        float* a4 = d_ws + (size_t)n * (per - flat - d1);   // the workspace as f2_launch_cnn lays it out: [conv2 | conv3 | conv4 | dense1]
        float* a5 = a4 + (size_t)n * flat;
        F2_TRY(f2_launch_cnn_convs(ctx, cnn, S, r, (const float*)d_x, n, d_ws, a4));
        F2_TRY(f2_launch_cnn_dense(ctx, cnn, S, r, a4, n, a5, so.scores.as<float>(), nullptr));
        if (po.dev) F2_TRY(f2_launch_scale_copy(ctx, a4, po.as<float>(), (int64_t)(flat * (size_t)n), 1.f / f2_cnn_a4_scale(cnn, S, r)));
        if (do1.dev) F2_HIP(ctx, hipMemcpyAsync(do1.dev, a5, do1.bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    F2_TRY(f2_copy_back(ctx, po));
    F2_TRY(f2_copy_back(ctx, do1));
    F2_TRY(f2_copy_back(ctx, so.scores));
    return f2_host_wait(ctx, mem_space);
}

}  // extern "C"

// ---- `cnn eval` over a ragged batch: what f2_eval_batch / f2_eval_utterance (every sample) and f2_eval_batch_strided share ----
namespace {

struct eval_call {
    int R = 0;
    double* d_env = nullptr;     // envelopes of the batch, (C, n_b) blocks at C * offsets[b]
    // CNN side (eval_cnn_begin)
    int64_t group_cap = 0;
    size_t flat = 0;
    float *d_a4 = nullptr, *d_a5 = nullptr;
    f2_score_outputs out;        // scores and labels of all windows of the call
    const f2_scale_set* S1 = nullptr;
    f2_cnn_route route;          // of every launch of the call
    int64_t g0 = 0, gn = 0;      // first window and size of the open dense group
};

// the argument errors of the eval calls (include/f2cnn_hip.h: f2_eval_batch); nothing is launched before they pass
int eval_check(f2_ctx* ctx, const f2_cnn* cnn, const f2_batch& X, int radius, int step, eval_call* E) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_dsp(ctx, X.wave_dtype, X.lpf, X.cutoff_hz, X.fft_precision));
    F2_TRY(f2_check_batch(ctx, X.offsets, X.B, X.C, X.mem_space, true));
    F2_CHECK(ctx, X.coefs && radius >= 0 && step >= 0, F2_ERR_INVALID, "coefs is NULL, or negative radius or step");
    E->R = 2 * radius + 1;
    return f2_check_cnn(ctx, cnn, E->R, X.C);
}

// filterbank + envelope of the whole batch, always by the two kernels: one utterance evaluated alone and inside a batch
// goes through the same envelope kernel. The envelopes stay in stage_out (or the caller's device buffer) for the window loop.
// With no window to evaluate (n_windows == 0) a host call is complete when this returns.
int eval_envelopes(f2_ctx* ctx, eval_call* E, const f2_batch& X, double* env_or_null, int64_t n_windows) {
    F2_CHECK(ctx, X.wave, F2_ERR_INVALID, "null wave");
    F2_TRY(f2_batch_envelopes(ctx, X, env_or_null, nullptr, false, &E->d_env));
    return n_windows == 0 ? f2_host_wait(ctx, X.mem_space) : F2_OK;
}

// Buffers of the window loop: xbuf and the convolution workspace for `chunk` windows, conv4 / dense1 outputs of a dense group
// (the dense layers run over the conv4 outputs of up to DENSE_GROUP windows at once: dense1's grid of 64-window workgroups then
// fills whole rounds of the device - launched per 14 240-window utterance its second round was one third full), scores and
// labels of all n_total windows (staged for host calls); nothing leaves HBM. Clears the error flag. on_device: a kernel of the
// call reads scores and labels (they get scratch when the caller gave no device buffer); tail_bytes: E->out.tail for the caller.
int eval_cnn_begin(f2_ctx* ctx, const f2_cnn* cnn, eval_call* E, int64_t chunk, int64_t n_total, int C, float* scores_or_null,
                   uint8_t* labels_or_null, int mem_space, bool on_device = false, size_t tail_bytes = 0) {
    E->group_cap = n_total < DENSE_GROUP ? n_total : DENSE_GROUP;
    const size_t conv_floats = f2_cnn_workspace_floats(cnn) - f2_cnn_dense_floats(cnn);
    E->flat = f2_cnn_flat_floats(cnn);
    F2_TRY(f2_reserve(ctx, ctx->xbuf, sizeof(float) * (size_t)chunk * E->R * (size_t)C));
    F2_TRY(f2_reserve(ctx, ctx->work, sizeof(float) * conv_floats * (size_t)chunk));
    F2_TRY(f2_reserve(ctx, ctx->dense_in, sizeof(float) * f2_cnn_dense_floats(cnn) * (size_t)E->group_cap));
    E->d_a4 = (float*)ctx->dense_in.ptr;
    E->d_a5 = E->d_a4 + E->flat * (size_t)E->group_cap;
    F2_TRY(f2_place_scores(ctx, scores_or_null, labels_or_null, n_total, mem_space, on_device, on_device, tail_bytes, &E->out));
    F2_TRY(f2_cnn_scale_set(ctx, cnn, 0, &E->S1));   // K3's normalised windows lie in [0, 1] by construction: no range pass
    E->route = f2_cnn_call_route(ctx, cnn, E->S1 != nullptr);
    E->g0 = E->gn = 0;
    return f2_reset_flag(ctx);
}

int eval_dense_flush(f2_ctx* ctx, const f2_cnn* cnn, eval_call* E) {
    float* d_scores = E->out.scores.as<float>();
    uint8_t* d_labels = E->out.labels.as<uint8_t>();
    if (E->gn > 0)
        F2_TRY(f2_launch_cnn_dense(ctx, cnn, E->S1, E->route, E->d_a4, E->gn, E->d_a5, d_scores ? d_scores + 2 * E->g0 : nullptr,
                                   d_labels ? d_labels + E->g0 : nullptr));
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
int eval_cnn_end(f2_ctx* ctx, const f2_cnn* cnn, eval_call* E) {
    F2_TRY(eval_dense_flush(ctx, cnn, E));
    F2_TRY(f2_copy_back(ctx, E->out.scores));
    F2_TRY(f2_copy_back(ctx, E->out.labels));
    return f2_finish_positive(ctx);
}

}  // namespace

// f2_eval_batch, and f2_eval_utterance as its B = 1 case with the envelope output (env_or_null, in mem_space) and the window
// count (n_windows_out): every-sample windows -> normalise -> conv1 .. conv4, utterance by utterance, chunk by chunk
static int eval_batch_impl(f2_ctx* ctx, const f2_cnn* cnn, const f2_batch& X, int radius, int step, double* env_or_null,
                           float* scores_or_null, uint8_t* labels_or_null, int64_t* n_windows_out) {
    eval_call E;
    F2_TRY(eval_check(ctx, cnn, X, radius, step, &E));
    const int64_t* offsets = X.offsets;
    const int B = X.B, C = X.C;
    int64_t nb_total = 0, nb_max = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t nb = offsets[b + 1] - offsets[b] - (int64_t)E.R * step;   // Evaluating.py:73
        if (nb > 0) {
            nb_total += nb;
            nb_max = nb > nb_max ? nb : nb_max;
        }
    }
    if (n_windows_out) *n_windows_out = nb_total;
    if (X.total() == 0) return F2_OK;
    F2_TRY(eval_envelopes(ctx, &E, X, env_or_null, nb_total));
    if (nb_total == 0) return F2_OK;
    const int64_t chunk = nb_max < CNN_CHUNK ? nb_max : CNN_CHUNK;
    F2_TRY(eval_cnn_begin(ctx, cnn, &E, chunk, nb_total, C, scores_or_null, labels_or_null, X.mem_space));
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
    return eval_cnn_end(ctx, cnn, &E);
}

// windows f2_eval_batch_strided evaluates in an utterance of n samples (R = 2 * radius + 1 rows)
static int64_t strided_windows(int64_t n, int R, int step, int hop) {
    const int64_t nb = n - (int64_t)R * step;
    return nb > 0 ? (nb + hop - 1) / hop : 0;
}

// The window loop of f2_eval_batch_strided (and f2_eval_figure_batch) between eval_cnn_begin and eval_cnn_end: utterance b has
// nbh[b] windows. A chunk is up to `chunk` windows taken from as many utterances as it holds (an utterance may continue in the next
// chunk): one window-stage launch set and one convolution launch set per chunk, whatever B. (On the decimating route a chunk also
// closes at COLUMN_CAP columns of the window stage's scratch - 2 * radius * step / hop columns per segment on top of its windows:
// 150 MB for 128 channels - which only batches of very many very short utterances at a small hop reach.)
// d_windows: where the window stage writes a chunk (the eval calls: ctx->xbuf). occ (f2_eval_occlusion_batch): the chunk's windows
// are then expanded into xbuf as (m, occ->K + 1, R, C) and the network sees m * (occ->K + 1) windows.
struct occlusion_stage {
    const int32_t* d_patches;
    int K;
    float fill;
};
// sal (f2_eval_saliency_batch): the chunk's windows are differentiated while they are in d_windows (f2_cnn_grad.hip: recorded
// forward + backward-data chain through ctx->grad_ws) and only their profile rows are kept, at d_profile + 2 C * (windows so far).
struct saliency_stage {
    double* d_profile;
    int64_t done;
};
static int strided_window_loop(f2_ctx* ctx, const f2_cnn* cnn, eval_call* E, const f2_batch& X, const std::vector<int64_t>& nbh,
                               int64_t chunk, int radius, int step, int hop, float* d_windows, const occlusion_stage* occ = nullptr,
                               saliency_stage* sal = nullptr) {
    constexpr int64_t COLUMN_CAP = 8 * CNN_CHUNK;
    const int64_t* offsets = X.offsets;
    const int B = X.B, C = X.C;
    const bool columns = f2_gather_strided_blocked(ctx, C, step, hop);
    std::vector<f2_win_seg> segs;
    int64_t m = 0, cols = 0;     // windows and scratch columns of the open chunk
    auto close_chunk = [&]() -> int {
        if (m > 0) {
            const int64_t seen = occ ? m * (occ->K + 1) : m;   // windows the network sees
            F2_TRY(eval_chunk_room(ctx, cnn, E, seen));
            F2_TRY(f2_launch_gather_strided(ctx, E->d_env, C, (const int64_t*)ctx->offsets.ptr, offsets, segs.data(), (int)segs.size(),
                                            radius, step, hop, d_windows, (int*)ctx->flags.ptr));
            if (occ) F2_TRY(f2_launch_occlude_windows(ctx, d_windows, m, E->R, C, occ->d_patches, occ->K, occ->fill, (float*)ctx->xbuf.ptr));
            F2_TRY(eval_chunk_convs(ctx, cnn, E, seen));
            if (sal) {
                F2_TRY(f2_launch_cnn_input_gradient(ctx, cnn, d_windows, m, nullptr, sal->d_profile + 2 * (size_t)C * (size_t)sal->done, nullptr));
                sal->done += m;
            }
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
    return close_chunk();
}

extern "C" {

int f2_eval_utterance(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, int64_t N, const double* coefs,
                      int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step, double* env_or_null,
                      float* scores_or_null, uint8_t* labels_or_null, int64_t* n_windows_out, int mem_space) {
    if (ctx && !wave) return f2_fail(ctx, F2_ERR_INVALID, "null wave");   // (also for N == 0, unlike f2_eval_batch)
    const int64_t offsets[2] = {0, N};
    const f2_batch X = {wave, wave_dtype, offsets, coefs, 1, C, lpf, cutoff_hz, fft_precision, mem_space};
    return eval_batch_impl(ctx, cnn, X, radius, step, env_or_null, scores_or_null, labels_or_null, n_windows_out);
}

int f2_eval_batch(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                  const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step,
                  float* scores_or_null, uint8_t* labels_or_null, int mem_space) {
    const f2_batch X = {wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, mem_space};
    return eval_batch_impl(ctx, cnn, X, radius, step, nullptr, scores_or_null, labels_or_null, nullptr);
}

// f2_eval_batch_strided: window j of utterance b is every-sample window j * hop, in chunks of up to CNN_CHUNK windows
// (strided_window_loop).
int f2_eval_batch_strided(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                          const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step,
                          int hop, float* scores_or_null, uint8_t* labels_or_null, int64_t* window_offsets_or_null, int mem_space) {
    const f2_batch X = {wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, mem_space};
    eval_call E;
    F2_TRY(eval_check(ctx, cnn, X, radius, step, &E));
    F2_CHECK(ctx, hop >= 1, F2_ERR_INVALID, "hop must be at least 1 sample (got %d)", hop);
    std::vector<int64_t> nbh((size_t)B);
    int64_t n_total = 0;
    if (window_offsets_or_null) window_offsets_or_null[0] = 0;
    for (int b = 0; b < B; ++b) {
        nbh[(size_t)b] = strided_windows(offsets[b + 1] - offsets[b], E.R, step, hop);
        n_total += nbh[(size_t)b];
        if (window_offsets_or_null) window_offsets_or_null[b + 1] = n_total;
    }
    if (X.total() == 0) return F2_OK;
    F2_TRY(eval_envelopes(ctx, &E, X, nullptr, n_total));
    if (n_total == 0) return F2_OK;
    const int64_t chunk = n_total < CNN_CHUNK ? n_total : CNN_CHUNK;
    F2_TRY(eval_cnn_begin(ctx, cnn, &E, chunk, n_total, C, scores_or_null, labels_or_null, mem_space));
    F2_TRY(strided_window_loop(ctx, cnn, &E, X, nbh, chunk, radius, step, hop, (float*)ctx->xbuf.ptr));
    return eval_cnn_end(ctx, cnn, &E);
}

// f2_eval_segments_batch: the strided call with its scores and labels kept on the device, then the launches of f2_decision_path,
// f2_decision_runs and f2_interval_tally (f2_segments.hip) on them. One block of ctx->seg_ws for everything the stages keep, placed
// before the first launch; the small results (value, run_offsets) come down in front of the wait of eval_cnn_end.
int f2_eval_segments_batch(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs,
                           int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step, int hop, double logit_scale,
                           int64_t penalty, const int64_t* iv_offsets_or_null, const int64_t* iv_bounds, int R, float* scores_or_null,
                           uint8_t* labels_or_null, int64_t* window_offsets_or_null, uint8_t* path_or_null, int32_t* emissions_or_null,
                           int64_t* value_or_null, int64_t* run_offsets_or_null, int64_t* runs_or_null, int64_t* tally_or_null,
                           int mem_space) {
    const f2_batch X = {wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, mem_space};
    eval_call E;
    F2_TRY(eval_check(ctx, cnn, X, radius, step, &E));
    F2_CHECK(ctx, hop >= 1, F2_ERR_INVALID, "hop must be at least 1 sample (got %d)", hop);
    F2_CHECK(ctx, X.wave || X.total() == 0, F2_ERR_INVALID, "null wave");
    std::vector<int64_t> nbh((size_t)B), wo((size_t)B + 1, 0);
    for (int b = 0; b < B; ++b) {
        nbh[(size_t)b] = strided_windows(offsets[b + 1] - offsets[b], E.R, step, hop);
        wo[(size_t)b + 1] = wo[(size_t)b] + nbh[(size_t)b];
    }
    const int64_t n_total = wo[(size_t)B];
    f2_seg_plan S;
    S.set(wo.data(), B);
    const bool want_runs = run_offsets_or_null || runs_or_null, want_tally = tally_or_null != nullptr;
    const bool want_path = path_or_null || emissions_or_null || value_or_null || want_runs || want_tally;
    int64_t tally_rows = 0;
    F2_TRY(f2_check_decision_path(ctx, logit_scale, penalty));
    F2_TRY(f2_check_segment_rows(ctx, n_total));
    F2_CHECK(ctx, !want_tally || iv_offsets_or_null, F2_ERR_INVALID, "a tally needs iv_offsets");
    if (want_tally) F2_TRY(f2_check_intervals(ctx, B, iv_offsets_or_null, iv_bounds, R, (int64_t)radius * step, hop, S.max_rows, &tally_rows));
    if (window_offsets_or_null) memcpy(window_offsets_or_null, wo.data(), sizeof(int64_t) * wo.size());
    if (X.total() == 0 || n_total == 0) {
        if (value_or_null) std::fill(value_or_null, value_or_null + B, (int64_t)0);
        if (run_offsets_or_null) std::fill(run_offsets_or_null, run_offsets_or_null + B + 1, (int64_t)0);
    }
    if (X.total() == 0) return F2_OK;

    const bool host = mem_space != F2_MEM_DEVICE;
    const size_t n = (size_t)n_total, tally_bytes = sizeof(int64_t) * 4 * (size_t)tally_rows;
    char *s_path = nullptr, *s_q = nullptr, *s_runs = nullptr, *s_tally = nullptr;
    if (n_total > 0 && want_path) {
        S.name_arrays(true, want_runs, want_tally ? iv_offsets_or_null[R] : 0, want_tally ? R : 0);
        if (host || !path_or_null) S.name_bytes(&s_path, n);
        if (host || !emissions_or_null) S.name_bytes(&s_q, sizeof(int32_t) * n);
        if (runs_or_null && host) S.name_bytes(&s_runs, sizeof(int64_t) * 4 * n);
        if (want_tally && host) S.name_bytes(&s_tally, tally_bytes);
        F2_TRY(S.reserve(ctx));
    }
    F2_TRY(eval_envelopes(ctx, &E, X, nullptr, n_total));
    if (n_total == 0) {
        // (intervals of utterances without rows own no row)
        if (want_tally && tally_rows > 0) {
            if (host) memset(tally_or_null, 0, tally_bytes);
            else F2_HIP(ctx, hipMemsetAsync(tally_or_null, 0, tally_bytes, ctx->stream));
        }
        return F2_OK;
    }
    const int64_t chunk = n_total < CNN_CHUNK ? n_total : CNN_CHUNK;
    F2_TRY(eval_cnn_begin(ctx, cnn, &E, chunk, n_total, C, scores_or_null, labels_or_null, mem_space, want_path));
    F2_TRY(strided_window_loop(ctx, cnn, &E, X, nbh, chunk, radius, step, hop, (float*)ctx->xbuf.ptr));
    std::vector<int64_t> ro((size_t)B + 1, 0);
    uint8_t* d_runs_src = nullptr;
    if (want_path) {
        F2_TRY(eval_dense_flush(ctx, cnn, &E));
        uint8_t* d_path = host || !path_or_null ? (uint8_t*)s_path : path_or_null;
        int32_t* d_q = host || !emissions_or_null ? (int32_t*)s_q : emissions_or_null;
        const uint8_t* d_labels = E.out.labels.as<uint8_t>();
        F2_TRY(S.upload_tables(ctx));
        F2_TRY(f2_launch_decision_path(ctx, S, E.out.scores.as<float>(), logit_scale, penalty, d_path, d_q));
        if (host && path_or_null) F2_HIP(ctx, hipMemcpyAsync(path_or_null, d_path, n, hipMemcpyDeviceToHost, ctx->stream));
        if (host && emissions_or_null)
            F2_HIP(ctx, hipMemcpyAsync(emissions_or_null, d_q, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
        if (value_or_null)
            F2_HIP(ctx, hipMemcpyAsync(value_or_null, S.d_value, sizeof(int64_t) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
        if (want_runs) {
            F2_TRY(f2_launch_runs_count(ctx, S, d_path, d_q));
            F2_HIP(ctx, hipMemcpyAsync(ro.data(), S.d_ro, sizeof(int64_t) * ro.size(), hipMemcpyDeviceToHost, ctx->stream));
            if (runs_or_null) {
                d_runs_src = host ? (uint8_t*)s_runs : (uint8_t*)runs_or_null;
                F2_TRY(f2_launch_runs_scatter(ctx, S, d_path, d_q, n_total, (int64_t*)d_runs_src));
            }
        }
        if (want_tally && tally_rows > 0) {
            int64_t* d_tally = host ? (int64_t*)s_tally : tally_or_null;
            F2_TRY(f2_launch_interval_tally(ctx, S, d_labels, d_path, d_q, iv_offsets_or_null, iv_bounds, R, (int64_t)radius * step, hop,
                                            tally_rows, d_tally));
            if (host) F2_HIP(ctx, hipMemcpyAsync(tally_or_null, d_tally, tally_bytes, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    const int rc = eval_cnn_end(ctx, cnn, &E);   // (waits for the stream)
    if (rc != F2_OK && rc != F2_ERR_NONPOSITIVE) return rc;
    if (run_offsets_or_null) memcpy(run_offsets_or_null, ro.data(), sizeof(int64_t) * ro.size());
    if (host && runs_or_null && ro[(size_t)B] > 0) {
        F2_HIP(ctx, hipMemcpyAsync(runs_or_null, d_runs_src, sizeof(int64_t) * 4 * (size_t)ro[(size_t)B], hipMemcpyDeviceToHost, ctx->stream));
        F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return rc;
}

}  // extern "C"

// ---- the robustness sweeps: K levels of one axis (noise, room, envelope cutoff, spectral resolution) and the unchanged level of a ragged batch as ONE
// (K+1) * B-utterance batch in device memory - utterance l * B + b is utterance b at level l, the unchanged level last - evaluated
// like f2_eval_batch_strided, its labels tallied against the unchanged level's on the device ----
namespace {

// The (K+1) * B batch on the host, and the tally's two small arrays. The empty cases, for every sweep: nothing is launched when
// total == 0, and sigma is zeros then; stats are zeros whenever n_total == 0 (sweep_begin fills them; a wave sweep with samples but
// no window still runs tally() and stats_back(), which bring the same zeros).
struct sweep_plan {
    int B = 0, K = 0, U = 0;
    int64_t total = 0, n_total = 0, max_windows = 0;   // samples of a level; windows of all levels, of the utterance with the most
    std::vector<int64_t> tiled, wo, nbh;               // the caller's offsets tiled (U + 1), window offsets (U + 1), windows (U)
    int64_t *d_stats = nullptr, *d_wo = nullptr;
    // after the axis's own arrays, before meta->reserve()
    void carve(f2_meta_carve* meta) { meta->add(&d_stats, 2 * (size_t)U), meta->add(&d_wo, (size_t)U + 1); }
    // stats of the U utterances from their labels (all written: behind the last dense launch)
    int tally(f2_ctx* ctx, const uint8_t* d_labels) const {
        F2_HIP(ctx, hipMemsetAsync(d_stats, 0, sizeof(int64_t) * 2 * (size_t)U, ctx->stream));
        if (n_total == 0) return F2_OK;
        F2_TRY(f2_upload_async(ctx, d_wo, wo.data(), sizeof(int64_t) * ((size_t)U + 1)));
        return f2_launch_label_tally(ctx, d_labels, d_wo, B, K, max_windows, d_stats);
    }
    int stats_back(f2_ctx* ctx, int64_t* stats_or_null) const {
        if (stats_or_null)
            F2_HIP(ctx, hipMemcpyAsync(stats_or_null, d_stats, sizeof(int64_t) * 2 * (size_t)U, hipMemcpyDeviceToHost, ctx->stream));
        return F2_OK;
    }
};

// The argument errors of a sweep in their order - f2_eval_batch_strided's, the axis's own (level_check), the size of the (K+1) * B
// batch (per_channel: of its B * C rows too, for levels that are envelopes), null wave - then the plan, window_offsets_or_null and
// the zero stats of a call without windows.
template <class LevelCheck>
int sweep_begin(f2_ctx* ctx, const f2_cnn* cnn, const f2_batch& X, int radius, int step, int hop, int K, LevelCheck level_check,
                bool per_channel, int64_t* window_offsets_or_null, int64_t* stats_or_null, eval_call* E, sweep_plan* P) {
    F2_TRY(eval_check(ctx, cnn, X, radius, step, E));
    F2_CHECK(ctx, hop >= 1, F2_ERR_INVALID, "hop must be at least 1 sample (got %d)", hop);
    F2_TRY(level_check());
    const int B = X.B;
    F2_CHECK(ctx, ((int64_t)K + 1) * (B > 0 ? B : 1) <= INT32_MAX / 2, F2_ERR_UNSUPPORTED, "%d levels of %d utterances", K + 1, B);
    F2_CHECK(ctx, !per_channel || (int64_t)B * X.C <= INT32_MAX, F2_ERR_UNSUPPORTED, "%d utterances of %d channels", B, X.C);
    const int64_t total = X.total();
    F2_CHECK(ctx, X.wave || total == 0, F2_ERR_INVALID, "null wave");
    const int U = (K + 1) * B;
    P->B = B, P->K = K, P->U = U, P->total = total;
    P->tiled.assign((size_t)U + 1, 0), P->wo.assign((size_t)U + 1, 0), P->nbh.assign((size_t)U, 0);
    for (int l = 0; l <= K; ++l)
        for (int b = 0; b < B; ++b) {
            const size_t u = (size_t)l * B + b;
            P->nbh[u] = strided_windows(X.offsets[b + 1] - X.offsets[b], E->R, step, hop);
            P->tiled[u + 1] = (int64_t)l * total + X.offsets[b + 1];
            P->wo[u + 1] = P->wo[u] + P->nbh[u];
            P->max_windows = std::max(P->max_windows, P->nbh[u]);
        }
    P->n_total = P->wo[(size_t)U];
    if (window_offsets_or_null) memcpy(window_offsets_or_null, P->wo.data(), sizeof(int64_t) * ((size_t)U + 1));
    if (stats_or_null && P->n_total == 0) std::fill(stats_or_null, stats_or_null + 2 * (size_t)U, (int64_t)0);
    return F2_OK;
}

// A sweep whose levels are waveforms (noise, room): the levels as float64 in ctx->levels or the caller's device buffer, through
// f2_eval_batch_strided as a device call on the tiled offsets, the tally, and what the caller asked for behind one wait. Of the axis:
// level_check (sweep_begin); carve(meta, U) names its small arrays; fill(d_offsets, total, d_levels) stages the wave and queues the
// launches that fill the levels (the tiled offsets on the device start with the caller's: one array serves them and the
// evaluation); *d_sigma, if the axis has one: U doubles for sigma_or_null.
template <class LevelCheck, class Carve, class Fill>
int wave_sweep(f2_ctx* ctx, const f2_cnn* cnn, const f2_batch& X, int radius, int step, int hop, int K, LevelCheck level_check,
               Carve carve, Fill fill, double* levels_or_null, float* scores_or_null, uint8_t* labels_or_null,
               int64_t* window_offsets_or_null, int64_t* stats_or_null, double* sigma_or_null = nullptr, double** d_sigma = nullptr) {
    eval_call E;
    sweep_plan P;
    F2_TRY(sweep_begin(ctx, cnn, X, radius, step, hop, K, level_check, false, window_offsets_or_null, stats_or_null, &E, &P));
    if (P.total == 0) {
        if (sigma_or_null) std::fill(sigma_or_null, sigma_or_null + P.U, 0.0);
        return F2_OK;
    }
    // small arrays of the call, held across the nested evaluation (which does not touch ctx->meta)
    f2_meta_carve meta;
    carve(&meta, (size_t)P.U);
    P.carve(&meta);
    F2_TRY(meta.reserve(ctx));
    f2_output levels;
    F2_TRY(f2_place(ctx, ctx->levels, levels_or_null, sizeof(double) * (size_t)(K + 1) * (size_t)P.total, X.mem_space, true, &levels));
    // scores / labels of the device call below (the tally always needs the labels). They stay in stage_aux: the nested call, a
    // device call with both pointers given, uses stage_out, xbuf, work and dense_in
    f2_score_outputs out;
    F2_TRY(f2_place_scores(ctx, scores_or_null, labels_or_null, P.n_total, X.mem_space, false, true, 0, &out));
    F2_TRY(f2_upload_offsets(ctx, P.tiled.data(), P.U));
    F2_TRY(fill((const int64_t*)ctx->offsets.ptr, P.total, levels.as<double>()));
    F2_TRY(f2_copy_back(ctx, levels));
    F2_TRY(f2_eval_batch_strided(ctx, cnn, levels.dev, F2_WAVE_F64, P.tiled.data(), X.coefs, P.U, X.C, X.lpf, X.cutoff_hz, X.fft_precision,
                                 radius, step, hop, out.scores.as<float>(), out.labels.as<uint8_t>(), nullptr, F2_MEM_DEVICE));
    F2_TRY(P.tally(ctx, out.labels.as<uint8_t>()));
    if (P.n_total > 0) {
        F2_TRY(f2_copy_back(ctx, out.scores));
        F2_TRY(f2_copy_back(ctx, out.labels));
    }
    if (sigma_or_null) F2_HIP(ctx, hipMemcpyAsync(sigma_or_null, *d_sigma, sizeof(double) * (size_t)P.U, hipMemcpyDeviceToHost, ctx->stream));
    F2_TRY(P.stats_back(ctx, stats_or_null));
    F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return F2_OK;
}

// A sweep whose levels are envelopes (envelope cutoff, spectral resolution): filterbank + envelope of the batch once (eval_envelopes,
// as X asks for them); the K levels and the copy as ONE (K+1) * B-utterance batch of envelopes in ctx->levels or the caller's device
// buffer; the window loop of f2_eval_batch_strided over that batch with the tiled offsets; the tally of its labels against level K.
// One wait at the end (eval_cnn_end). Of the axis: level_check (sweep_begin); carve(meta) names its small arrays; ready() reserves
// and uploads what its kernel needs beside the envelopes, before anything is launched; fill(d_env, d_offsets, total, d_levels)
// queues the launch that fills the levels (the tiled offsets on the device start with the caller's).
template <class LevelCheck, class Carve, class Ready, class Fill>
int envelope_sweep(f2_ctx* ctx, const f2_cnn* cnn, const f2_batch& X, int radius, int step, int hop, int K, LevelCheck level_check,
                   Carve carve, Ready ready, Fill fill, double* env_levels_or_null, float* scores_or_null, uint8_t* labels_or_null,
                   int64_t* window_offsets_or_null, int64_t* stats_or_null) {
    const int C = X.C, mem_space = X.mem_space;
    eval_call E;
    sweep_plan P;
    F2_TRY(sweep_begin(ctx, cnn, X, radius, step, hop, K, level_check, true, window_offsets_or_null, stats_or_null, &E, &P));
    if (P.total == 0) return F2_OK;

    // small arrays and the levels first: nothing below reallocates what a queued kernel uses (eval_envelopes does not touch
    // ctx->meta, ctx->levels or ctx->mix)
    f2_meta_carve meta;
    carve(&meta);
    P.carve(&meta);
    F2_TRY(meta.reserve(ctx));
    f2_output levels;
    F2_TRY(f2_place(ctx, ctx->levels, env_levels_or_null, sizeof(double) * ((size_t)K + 1) * (size_t)C * (size_t)P.total, mem_space, true,
                    &levels));
    F2_TRY(ready());
    F2_TRY(eval_envelopes(ctx, &E, X, nullptr, P.n_total));
    // the tiled offsets start with the clean ones: one device array serves the level kernel and the window stage
    F2_TRY(f2_upload_offsets(ctx, P.tiled.data(), P.U));
    F2_TRY(fill(E.d_env, (const int64_t*)ctx->offsets.ptr, P.total, levels.as<double>()));
    F2_TRY(f2_copy_back(ctx, levels));
    if (P.n_total == 0) {
        F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return F2_OK;
    }
    E.d_env = levels.as<double>();
    const f2_batch XU = {nullptr, F2_WAVE_F64, P.tiled.data(), X.coefs, P.U, C, 0, 0.0, X.fft_precision, mem_space};
    const int64_t chunk = P.n_total < CNN_CHUNK ? P.n_total : CNN_CHUNK;
    F2_TRY(eval_cnn_begin(ctx, cnn, &E, chunk, P.n_total, C, scores_or_null, labels_or_null, mem_space, true));
    F2_TRY(strided_window_loop(ctx, cnn, &E, XU, P.nbh, chunk, radius, step, hop, (float*)ctx->xbuf.ptr));
    F2_TRY(eval_dense_flush(ctx, cnn, &E));   // the tally reads every label
    F2_TRY(P.tally(ctx, E.out.labels.as<uint8_t>()));
    F2_TRY(P.stats_back(ctx, stats_or_null));
    return eval_cnn_end(ctx, cnn, &E);   // (waits for the stream)
}

}  // namespace

extern "C" {

// f2_eval_noise_sweep: a wave sweep whose levels come from the two noise kernels (f2_noise.hip). Only the clean samples go up;
// sigma, stats and what the caller asked for come back behind one wait.
int f2_eval_noise_sweep(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                        const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step,
                        int hop, const double* snr_db, int K, uint64_t seed, double* noisy_or_null, float* scores_or_null,
                        uint8_t* labels_or_null, int64_t* window_offsets_or_null, double* sigma_or_null, int64_t* stats_or_null,
                        int mem_space) {
    const f2_batch X = {wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, mem_space};
    std::vector<double> lin;   // 10^(snr / 10) per level (Evaluating.py:189 SNRdbToSNRlinear)
    double *d_sigma, *d_lin;
    return wave_sweep(
        ctx, cnn, X, radius, step, hop, K,
        [&]() -> int {
            F2_CHECK(ctx, K >= 1 && snr_db, F2_ERR_INVALID, "a sweep needs at least one noise level (K=%d) and their snr_db", K);
            for (int k = 0; k < K; ++k) F2_CHECK(ctx, std::isfinite(snr_db[k]), F2_ERR_INVALID, "snr_db[%d] is not finite", k);
            return F2_OK;
        },
        [&](f2_meta_carve* meta, size_t U) { meta->add(&d_sigma, U), meta->add(&d_lin, (size_t)K); },
        [&](const int64_t* d_offsets, int64_t total, double* d_noisy) -> int {
            for (int k = 0; k < K; ++k) lin.push_back(std::pow(10.0, snr_db[k] / 10.0));
            F2_TRY(f2_upload_async(ctx, d_lin, lin.data(), sizeof(double) * (size_t)K));
            const void* d_wave;
            F2_TRY(f2_stage_wave(ctx, wave, wave_dtype, total, mem_space, &d_wave));
            F2_TRY(f2_launch_noise_sigma(ctx, d_wave, wave_dtype, d_offsets, d_lin, B, K, d_sigma));
            return f2_launch_noise_levels(ctx, d_wave, wave_dtype, d_offsets, d_sigma, B, K, total, seed, d_noisy);
        },
        noisy_or_null, scores_or_null, labels_or_null, window_offsets_or_null, stats_or_null, sigma_or_null, &d_sigma);
}

// f2_eval_reverb_sweep: a wave sweep whose levels come from k_reverb_levels (f2_reverb.hip). Only the dry samples and the taps go
// up; one wait at the end.
int f2_eval_reverb_sweep(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                         const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step,
                         int hop, const double* rir, const int64_t* rir_offsets, int K, double* wet_or_null, float* scores_or_null,
                         uint8_t* labels_or_null, int64_t* window_offsets_or_null, int64_t* stats_or_null, int mem_space) {
    const f2_batch X = {wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, mem_space};
    f2_reverb_arrays A;
    return wave_sweep(
        ctx, cnn, X, radius, step, hop, K, [&] { return f2_check_rir(ctx, rir, rir_offsets, K); },
        [&](f2_meta_carve* meta, size_t) { f2_reverb_meta(meta, B, rir_offsets, K, &A); },
        [&](const int64_t* d_offsets, int64_t total, double* d_wet) -> int {
            const void* d_wave;
            F2_TRY(f2_stage_wave(ctx, wave, wave_dtype, total, mem_space, &d_wave));
            return f2_launch_reverb_levels(ctx, d_wave, wave_dtype, d_offsets, offsets, B, rir, rir_offsets, K, A, d_wet);
        },
        wet_or_null, scores_or_null, labels_or_null, window_offsets_or_null, stats_or_null);
}

// f2_eval_shaped_noise_sweep: a wave sweep whose levels come from k_noise_sigma and k_shaped_noise_levels (f2_noise_shaped.hip). Only
// the clean samples and the taps go up; sigma, stats and what the caller asked for come back behind one wait.
int f2_eval_shaped_noise_sweep(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                               const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step,
                               int hop, const double* snr_db, const double* fir, const int64_t* fir_offsets, int K, uint64_t seed,
                               double* noisy_or_null, float* scores_or_null, uint8_t* labels_or_null, int64_t* window_offsets_or_null,
                               double* sigma_or_null, int64_t* stats_or_null, int mem_space) {
    const f2_batch X = {wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, mem_space};
    f2_shaped_arrays A;
    return wave_sweep(
        ctx, cnn, X, radius, step, hop, K, [&] { return f2_check_fir(ctx, snr_db, fir, fir_offsets, K); },
        [&](f2_meta_carve* meta, size_t) { f2_shaped_meta(meta, B, fir_offsets, K, &A); },
        [&](const int64_t* d_offsets, int64_t total, double* d_noisy) -> int {
            const void* d_wave;
            F2_TRY(f2_stage_wave(ctx, wave, wave_dtype, total, mem_space, &d_wave));
            return f2_launch_shaped_noise_levels(ctx, d_wave, wave_dtype, d_offsets, offsets, B, snr_db, fir, fir_offsets, K, seed, A,
                                                 d_noisy);
        },
        noisy_or_null, scores_or_null, labels_or_null, window_offsets_or_null, stats_or_null, sigma_or_null, &A.d_sigma);
}

// f2_eval_masker_sweep: a wave sweep whose levels come from k_noise_sigma and the two masker kernels (f2_masker.hip). Only the clean
// samples and the recordings go up; sigma, gain, start, stats and what the caller asked for come back behind one wait.
int f2_eval_masker_sweep(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs,
                         int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step, int hop, const double* snr_db,
                         const double* masker, const int64_t* masker_offsets, int R, const int32_t* masker_of, int K, uint64_t seed,
                         double* noisy_or_null, float* scores_or_null, uint8_t* labels_or_null, int64_t* window_offsets_or_null,
                         double* sigma_or_null, double* gain_or_null, int64_t* start_or_null, int64_t* stats_or_null, int mem_space) {
    const f2_batch X = {wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, mem_space};
    f2_masker_arrays A;
    bool ran = false;
    const int rc = wave_sweep(
        ctx, cnn, X, radius, step, hop, K, [&] { return f2_check_masker_levels(ctx, snr_db, masker, masker_offsets, R, masker_of, K); },
        [&](f2_meta_carve* meta, size_t) { f2_masker_meta(meta, B, K, &A); },
        [&](const int64_t* d_offsets, int64_t, double* d_noisy) -> int {
            const void* d_wave;
            F2_TRY(f2_stage_wave(ctx, wave, wave_dtype, offsets[B], mem_space, &d_wave));
            F2_TRY(f2_launch_masker_levels(ctx, d_wave, wave_dtype, d_offsets, offsets, B, snr_db, masker, masker_offsets, R, masker_of, K, seed,
                                           A, d_noisy));
            const size_t bytes = sizeof(double) * ((size_t)K + 1) * (size_t)B;   // (read behind the sweep's one wait)
            if (gain_or_null) F2_HIP(ctx, hipMemcpyAsync(gain_or_null, A.d_gain, bytes, hipMemcpyDeviceToHost, ctx->stream));
            if (start_or_null) F2_HIP(ctx, hipMemcpyAsync(start_or_null, A.d_start, bytes, hipMemcpyDeviceToHost, ctx->stream));
            ran = true;
            return F2_OK;
        },
        noisy_or_null, scores_or_null, labels_or_null, window_offsets_or_null, stats_or_null, sigma_or_null, &A.d_sigma);
    if (rc == F2_OK && !ran) {   // a batch without samples: nothing was launched
        const size_t U = ((size_t)K + 1) * (size_t)(B > 0 ? B : 0);
        if (gain_or_null) std::fill(gain_or_null, gain_or_null + U, 0.0);
        if (start_or_null) std::fill(start_or_null, start_or_null + U, (int64_t)0);
    }
    return rc;
}

// f2_eval_cutoff_sweep: an envelope sweep whose levels come from k_lowpass_levels (f2_lowpass.hip), on the unfiltered envelopes. Only
// the samples and the K coefficient pairs go up; one wait at the end.
int f2_eval_cutoff_sweep(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                         const double* coefs, int B, int C, int fft_precision, int radius, int step, int hop,
                         const double* cutoff_hz, int K, double* env_levels_or_null, float* scores_or_null, uint8_t* labels_or_null,
                         int64_t* window_offsets_or_null, int64_t* stats_or_null, int mem_space) {
    const f2_batch X = {wave, wave_dtype, offsets, coefs, B, C, 0, 0.0, fft_precision, mem_space};
    double* d_coef;
    return envelope_sweep(
        ctx, cnn, X, radius, step, hop, K, [&] { return f2_check_cutoffs(ctx, cutoff_hz, K); },
        [&](f2_meta_carve* meta) { meta->add(&d_coef, 2 * (size_t)K); }, [&] { return f2_upload_lowpass_coefs(ctx, cutoff_hz, K, d_coef); },
        [&](const double* d_env, const int64_t* d_offsets, int64_t total, double* d_levels) {
            return f2_launch_lowpass_levels(ctx, d_env, d_offsets, B, C, total, d_coef, K, d_levels);
        },
        env_levels_or_null, scores_or_null, labels_or_null, window_offsets_or_null, stats_or_null);
}

// f2_eval_smear_sweep: an envelope sweep whose levels come from k_channel_mix_levels (f2_smear.hip), on the envelopes as the strided
// call makes them (low-passed if lpf). Only the samples and the matrices go up; one wait at the end.
int f2_eval_smear_sweep(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                        const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step, int hop,
                        const double* mix, int K, double* env_levels_or_null, float* scores_or_null, uint8_t* labels_or_null,
                        int64_t* window_offsets_or_null, int64_t* stats_or_null, int mem_space) {
    const f2_batch X = {wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, mem_space};
    f2_smear_plan M;
    return envelope_sweep(
        ctx, cnn, X, radius, step, hop, K, [&] { return f2_check_mix(ctx, mix, K, C, &M); }, [](f2_meta_carve*) {},
        [&] { return f2_smear_reserve(ctx, M, B); },
        [&](const double* d_env, const int64_t* d_offsets, int64_t, double* d_levels) {
            return f2_launch_channel_mix_levels(ctx, d_env, d_offsets, offsets, B, M, d_levels);
        },
        env_levels_or_null, scores_or_null, labels_or_null, window_offsets_or_null, stats_or_null);
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

    int64_t *d_counts, *d_wo, *d_ro, *d_rt;
    uint8_t* d_rs;
    f2_meta_carve meta;
    meta.add(&d_counts, 4 * (size_t)U), meta.add(&d_wo, (size_t)U + 1), meta.add(&d_ro, (size_t)R + 1), meta.add(&d_rt, (size_t)M);
    meta.add(&d_rs, (size_t)M);
    F2_TRY(meta.reserve(ctx));
    const void* d_labels;
    F2_TRY(f2_stage_input(ctx, labels, (size_t)n_rows, mem_space, &d_labels));
    F2_HIP(ctx, hipMemsetAsync(d_counts, 0, sizeof(int64_t) * 4 * (size_t)U, ctx->stream));
    F2_TRY(f2_upload_async(ctx, d_wo, window_offsets, sizeof(int64_t) * ((size_t)U + 1)));
    F2_TRY(f2_upload_async(ctx, d_ro, ref_offsets, sizeof(int64_t) * ((size_t)R + 1)));
    F2_TRY(f2_upload_async(ctx, d_rt, ref_timepoints, sizeof(int64_t) * (size_t)M));
    F2_TRY(f2_upload_async(ctx, d_rs, ref_signs, (size_t)M));
    F2_TRY(f2_launch_label_accuracy(ctx, (const uint8_t*)d_labels, d_wo, U, d_ro, d_rt, d_rs, R, origin, hop, step, max_rows, d_counts));
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

    // host memory: windows, signs and groups go up chunk by chunk, and (normalize = 0) every chunk has its own range pass and route
    const bool per_chunk = mem_space != F2_MEM_DEVICE;
    const size_t xs = (size_t)cnn->rows * cnn->channels;
    const int64_t chunk = n < CNN_CHUNK ? n : CNN_CHUNK;
    // small arrays of the call: counts and loss (one memset clears both), the loss partials of a chunk
    int64_t* d_counts;
    double *d_loss, *d_partial;
    f2_meta_carve meta;
    meta.add(&d_counts, 4 * (size_t)G), meta.add(&d_loss, (size_t)G), meta.add(&d_partial, f2_score_partial_doubles(chunk, G));
    F2_TRY(meta.reserve(ctx));
    // per chunk in stage_aux: scores and labels the caller has not got on the device (the tally reads both), behind them the
    // groups and signs of a host caller
    f2_score_outputs out;
    F2_TRY(f2_place_scores(ctx, scores_or_null, labels_or_null, chunk, mem_space, true, true, (sizeof(int32_t) + 1) * (size_t)chunk, &out));
    int32_t* s_groups = (int32_t*)out.tail;
    uint8_t* s_signs = (uint8_t*)(s_groups + chunk);
    if (normalize) F2_TRY(f2_reserve(ctx, ctx->xbuf, sizeof(float) * xs * (size_t)chunk));

    // normalised windows lie in [0, 1]: the B = 1 scale set without the range pass, as in f2_eval_*; windows as they are take
    // f2_cnn_forward's route - the range of the whole call for device memory, of each chunk for host memory, as there
    const f2_scale_set* S = nullptr;
    f2_cnn_route route;
    double bound = per_chunk ? 0.0 : -1.0;   // normalize = 0: what f2_cnn_forward leaves in last_input_bound (host: largest B of the chunks)
    if (normalize) {
        F2_TRY(f2_cnn_scale_set(ctx, cnn, 0, &S));
        route = f2_cnn_call_route(ctx, cnn, S != nullptr);
    } else if (!per_chunk) {
        F2_TRY(forward_route(ctx, cnn, windows, n, &S, &route, &bound));
    }

    F2_HIP(ctx, hipMemsetAsync(d_counts, 0, 8 * 5 * (size_t)G, ctx->stream));
    F2_HIP(ctx, hipMemsetAsync((int*)ctx->flags.ptr + SCORE_WORD, 0, sizeof(int), ctx->stream));
    F2_TRY(f2_reset_flag(ctx));
    for (int64_t s = 0; s < n; s += chunk) {
        const int64_t m = n - s < chunk ? n - s : chunk;
        // The windows (up to 92 MB a chunk) go up straight from the caller's memory, as in f2_cnn_forward: the pinned buffers
        // of f2_upload_async would cost a host copy of every chunk first. The caller's memory is only read and outlives the
        // copies (the call waits for the stream before it returns); stage_in / stage_aux are reused in stream order, behind the
        // kernels of the chunk before, so the chunks need no wait of their own. Signs and groups: the pinned ring.
        const void* d_w;
        F2_TRY(f2_stage_input(ctx, windows + (size_t)s * xs, sizeof(float) * xs * (size_t)m, mem_space, &d_w));
        const uint8_t* d_signs = signs + s;
        const int32_t* d_groups = groups_or_null ? groups_or_null + s : nullptr;
        if (per_chunk) {
            F2_TRY(f2_upload_async(ctx, s_signs, d_signs, (size_t)m));
            if (d_groups) {
                F2_TRY(f2_upload_async(ctx, s_groups, d_groups, sizeof(int32_t) * (size_t)m));
                d_groups = s_groups;
            }
            d_signs = s_signs;
        }
        if (normalize) {
            F2_TRY(f2_launch_normalize_windows(ctx, (const float*)d_w, m, (int)xs, (float*)ctx->xbuf.ptr, (int*)ctx->flags.ptr));
            d_w = ctx->xbuf.ptr;
        } else if (per_chunk) {
            double b = -1.0;
            F2_TRY(forward_route(ctx, cnn, (const float*)d_w, m, &S, &route, &b));
            bound = chunks_bound(bound, b);
        }
        const f2_output sc = out.scores.chunk(sizeof(float) * 2 * (size_t)s, sizeof(float) * 2 * (size_t)m), lb = out.labels.chunk((size_t)s, (size_t)m);
        F2_TRY(cnn_forward_device(ctx, cnn, S, route, (const float*)d_w, m, sc.as<float>(), lb.as<uint8_t>()));
        F2_TRY(f2_launch_score_tally(ctx, sc.as<float>(), lb.as<uint8_t>(), d_signs, d_groups, G, m, d_counts, d_partial, d_loss,
                                     (int*)ctx->flags.ptr + SCORE_WORD));
        F2_TRY(f2_copy_back(ctx, sc));
        F2_TRY(f2_copy_back(ctx, lb));
    }
    if (!normalize) cnn->last_input_bound = bound;   // (normalize = 1 measures nothing and leaves it alone, as f2_eval_* do)
    F2_HIP(ctx, hipMemcpyAsync(counts, d_counts, sizeof(int64_t) * 4 * (size_t)G, hipMemcpyDeviceToHost, ctx->stream));
    F2_HIP(ctx, hipMemcpyAsync(loss_sum, d_loss, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost, ctx->stream));
    F2_HIP(ctx, hipMemcpyAsync(ctx->host_flags + SCORE_WORD, (int*)ctx->flags.ptr + SCORE_WORD, sizeof(int), hipMemcpyDeviceToHost,
                               ctx->stream));
    F2_TRY(f2_finish_positive(ctx));
    const int wrong = ctx->host_flags[SCORE_WORD];
    F2_CHECK(ctx, !(wrong & 1), F2_ERR_INVALID, "a sign is neither 0 nor 1");
    F2_CHECK(ctx, !(wrong & 2), F2_ERR_INVALID, "a group lies outside [0, %d)", G);
    return F2_OK;
}

}  // extern "C"

namespace {

// The small arrays of a noise stage in ctx->meta and its two launches. A clean stage (N.clean()) has none and converts alone.
// A coloured stage (N.coloured()) also names the arrays of k_shaped_noise_pick, which then takes the place of k_noise_pick behind
// the same sigma kernel. h_offsets: the batch's offsets on the host.
struct noise_pick_meta {
    double *d_sigma = nullptr, *d_lin = nullptr;
    int64_t* d_level = nullptr;   // B int32 values in 8-byte slots
    f2_shaped_pick_arrays S;
    void carve(f2_meta_carve* meta, int B, const int64_t* h_offsets, const f2_noise_pick_args& N) {
        if (N.clean()) return;
        meta->add(&d_sigma, (size_t)B), meta->add(&d_lin, (size_t)N.K), meta->add(&d_level, ((size_t)B + 1) / 2);
        if (N.coloured()) f2_shaped_pick_meta(meta, B, h_offsets, N, &S);
    }
    int launch(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const int64_t* h_offsets, int B, int64_t total,
               const f2_noise_pick_args& N, double* d_noisy) const {
        if (!N.clean()) {
            std::vector<double> lin;   // 10^(snr / 10) per level (Evaluating.py:189 SNRdbToSNRlinear)
            for (int k = 0; k < N.K; ++k) lin.push_back(std::pow(10.0, N.snr_db[k] / 10.0));
            F2_TRY(f2_upload_async(ctx, d_lin, lin.data(), sizeof(double) * (size_t)N.K));
            F2_TRY(f2_upload_async(ctx, d_level, N.level_of, sizeof(int32_t) * (size_t)B));
        }
        if (N.coloured()) {
            F2_TRY(f2_launch_noise_pick_sigma(ctx, d_wave, wave_dtype, d_offsets, d_lin, (const int32_t*)d_level, B, N.K, d_sigma));
            return f2_launch_shaped_noise_pick(ctx, d_wave, wave_dtype, d_offsets, h_offsets, B, N, S, (const int32_t*)d_level, d_sigma,
                                               d_noisy);
        }
        return f2_launch_noise_pick(ctx, d_wave, wave_dtype, d_offsets, d_lin, (const int32_t*)d_level, B, N.K, total, N.first_utterance,
                                    N.seed, d_sigma, d_noisy);
    }
};

// The gather that ends a window call with a smear stage (sharp or all_sharp: the plain ragged gather and nothing else). carve
// names the levels of the utterances in the call's f2_meta_carve; reserve sizes ctx->mix for the image unless it is up already
// (before the call's first launch); launch uploads what is not up and gathers from d_env with the offsets in ctx->offsets, ORing into
// word 0 of ctx->flags.
struct mix_gather_meta {
    const f2_mix_gather_args* S = nullptr;
    int64_t* d_mix_of = nullptr;   // B int32 values in 8-byte slots
    void carve(f2_meta_carve* meta, int B, const f2_mix_gather_args& smear) {
        if (smear.sharp() || smear.all_sharp) return;
        S = &smear;
        meta->add(&d_mix_of, ((size_t)B + 1) / 2);
    }
    int reserve(f2_ctx* ctx) const { return S && !S->d_wT ? f2_reserve(ctx, ctx->mix, f2_mix_image_bytes(*S->plan)) : F2_OK; }
    int launch(f2_ctx* ctx, const double* d_env, int B, int C, const f2_window_list& W, float* d_windows) const {   // (W on the device)
        const int64_t* d_offsets = (const int64_t*)ctx->offsets.ptr;
        if (!S)
            return f2_launch_gather_ragged(ctx, d_env, C, d_offsets, W.centers, W.win_utt, W.n_windows, W.radius, W.step, W.normalize, d_windows,
                                           (int*)ctx->flags.ptr);
        const int64_t* d_spans = S->d_spans;
        const double* d_wT = S->d_wT;
        if (!d_wT) F2_TRY(f2_upload_mix_image(ctx, *S->plan, ctx->mix.ptr, &d_spans, &d_wT));
        F2_TRY(f2_upload_async(ctx, d_mix_of, S->mix_of, sizeof(int32_t) * (size_t)B));
        return f2_launch_gather_mixed(ctx, d_env, C, d_offsets, W.centers, W.win_utt, W.n_windows, W.radius, W.step, W.normalize, *S->plan,
                                      d_spans, d_wT, (const int32_t*)d_mix_of, d_windows, (int*)ctx->flags.ptr);
    }
};

}  // namespace

// The argument checks of f2_input_batch, and behind them those of the noise stage when the call has one (noise != NULL), all before
// anything is launched. *n_windows == 0 on F2_OK: an empty call. win_utt: the utterance of every window.
int f2_check_input_batch(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C, int lpf,
                      double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers, int radius, int step,
                      const void* windows, int mem_space, const f2_noise_pick_args* noise, int64_t* n_windows, std::vector<int>* win_utt) {
    *n_windows = 0;
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_TRY(f2_check_dsp(ctx, wave_dtype, lpf, cutoff_hz, fft_precision));
    F2_CHECK(ctx, B >= 0 && C > 0 && radius >= 0 && step >= 0, F2_ERR_INVALID, "bad size");
    if (noise) F2_TRY(f2_check_noise_pick(ctx, B, *noise));
    return f2_check_window_lists(ctx, offsets, B, center_offsets, centers, radius, step, wave && coefs && centers && windows, n_windows, win_utt);
}

int f2_check_window_lists(f2_ctx* ctx, const int64_t* offsets, int B, const int64_t* center_offsets, const int64_t* centers, int radius,
                          int step, bool data_given, int64_t* n_windows, std::vector<int>* win_utt) {
    *n_windows = 0;
    if (B == 0) return F2_OK;      // (before the offsets are looked at: they may be NULL then)
    F2_TRY(f2_check_offsets(ctx, offsets, B, "offsets"));
    F2_TRY(f2_check_offsets(ctx, center_offsets, B, "center_offsets"));
    const int64_t n = center_offsets[B];
    if (n == 0) return F2_OK;
    F2_CHECK(ctx, data_given, F2_ERR_INVALID, "null data pointer");
    // InputGenerator.py:73-80 indexes each utterance's own envelope: a window must lie inside it
    const int64_t reach = (int64_t)radius * step;
    win_utt->resize((size_t)n);
    for (int b = 0; b < B; ++b) {
        const int64_t nb = offsets[b + 1] - offsets[b];
        for (int64_t e = center_offsets[b]; e < center_offsets[b + 1]; ++e) {
            F2_CHECK(ctx, centers[e] - reach >= 0 && centers[e] + reach < nb, F2_ERR_INVALID,
                     "utterance %d: window %lld (centre %lld, +-%lld) reaches outside its %lld-sample envelope", b,
                     (long long)(e - center_offsets[b]), (long long)centers[e], (long long)reach, (long long)nb);
            (*win_utt)[(size_t)e] = b;
        }
    }
    *n_windows = n;
    return F2_OK;
}

int f2_check_noise_pick(f2_ctx* ctx, int B, const f2_noise_pick_args& N) {
    F2_CHECK(ctx, N.K >= 0, F2_ERR_INVALID, "negative number of noise levels (K=%d)", N.K);
    F2_CHECK(ctx, ((int64_t)N.K + 1) * (B > 0 ? B : 1) <= INT32_MAX / 2, F2_ERR_UNSUPPORTED, "%d levels of %d utterances", N.K + 1, B);
    F2_CHECK(ctx, (uint64_t)N.first_utterance + (uint64_t)(B > 0 ? B : 0) <= (uint64_t(1) << 32), F2_ERR_UNSUPPORTED,
             "utterances %u .. %u + %d do not fit the generator's 32-bit utterance number", N.first_utterance, N.first_utterance, B);
    if (N.clean()) return F2_OK;
    F2_CHECK(ctx, N.snr_db, F2_ERR_INVALID, "level_of is given for K=%d levels, but snr_db is NULL", N.K);
    for (int k = 0; k < N.K; ++k) F2_CHECK(ctx, std::isfinite(N.snr_db[k]), F2_ERR_INVALID, "snr_db[%d] is not finite", k);
    for (int b = 0; b < B; ++b)
        F2_CHECK(ctx, N.level_of[b] >= 0 && N.level_of[b] <= N.K, F2_ERR_INVALID, "utterance %d: level %d is outside [0, %d]", b,
                 (int)N.level_of[b], N.K);
    return F2_OK;
}

int f2_launch_noisy_windows(f2_ctx* ctx, const f2_batch& X, const f2_window_list& W, const f2_augment_args& A, float* d_windows) {
    const int B = X.B;
    const int64_t* offsets = X.offsets;
    const int64_t total = X.total();
    const bool wet = !A.rooms.dry(), masked = !A.maskers.silent(), filtered = !A.cutoffs.unfiltered();
    mix_gather_meta G;
    // the small arrays and the waveforms first: nothing the envelopes reserve is one of these areas
    noise_pick_meta M;
    f2_reverb_pick_arrays R;
    f2_masker_pick_arrays K;
    f2_lowpass_pick_arrays L;
    f2_meta_carve meta;
    M.carve(&meta, B, offsets, A.noise);
    if (wet) f2_reverb_pick_meta(&meta, B, offsets, A.rooms, &R);
    if (masked) f2_masker_pick_meta(&meta, B, A.maskers, &K);
    if (filtered) f2_lowpass_pick_meta(&meta, B, A.cutoffs, &L);
    G.carve(&meta, B, A.smear);
    F2_TRY(meta.reserve(ctx));
    F2_TRY(G.reserve(ctx));
    F2_TRY(f2_reserve(ctx, ctx->levels, sizeof(double) * (size_t)total));
    if (wet) F2_TRY(f2_reserve(ctx, ctx->wet, sizeof(double) * (size_t)total));
    if (masked) F2_TRY(f2_reserve(ctx, ctx->masked, sizeof(double) * (size_t)total));
    F2_TRY(f2_upload_offsets(ctx, offsets, B));
    const void* d_wave = X.wave;
    int wave_dtype = X.wave_dtype;
    if (wet) {   // f2_reverb_pick into ctx->wet, then f2_noise_pick(F2_WAVE_F64) from there: sigma is the reverberant signal's
        F2_TRY(f2_launch_reverb_pick(ctx, d_wave, wave_dtype, (const int64_t*)ctx->offsets.ptr, offsets, B, A.rooms, R, (double*)ctx->wet.ptr));
        d_wave = ctx->wet.ptr, wave_dtype = F2_WAVE_F64;
    }
    if (masked) {   // f2_masker_pick into ctx->masked, then the noise from there: its sigma is the masked signal's
        F2_TRY(f2_launch_masker_pick(ctx, d_wave, wave_dtype, (const int64_t*)ctx->offsets.ptr, B, total, A.maskers, K, (double*)ctx->masked.ptr));
        d_wave = ctx->masked.ptr, wave_dtype = F2_WAVE_F64;
    }
    F2_TRY(M.launch(ctx, d_wave, wave_dtype, (const int64_t*)ctx->offsets.ptr, offsets, B, total, A.noise, (double*)ctx->levels.ptr));
    // f2_input_batch from here on, as a device call on the float64 buffer
    f2_batch E = X;
    E.wave = ctx->levels.ptr, E.wave_dtype = F2_WAVE_F64, E.mem_space = F2_MEM_DEVICE;
    if (filtered) E.lpf = 0;   // the stage filters unfiltered envelopes (A.check refused lpf = 1 beside it)
    double* d_env;
    F2_TRY(f2_batch_envelopes(ctx, E, nullptr, nullptr, true, &d_env));
    // f2_lowpass_pick on the envelope scratch, in place: the rows of an unfiltered utterance are neither read nor written
    if (filtered) F2_TRY(f2_launch_lowpass_pick(ctx, d_env, (const int64_t*)ctx->offsets.ptr, B, X.C, total, A.cutoffs, L, d_env));
    f2_window_list D = W;
    if (!W.on_device) F2_TRY(f2_upload_windows(ctx, W.centers, W.win_utt, W.n_windows, &D.centers, &D.win_utt));
    return G.launch(ctx, d_env, B, X.C, D, d_windows);
}

extern "C" {

int f2_input_batch(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C,
                   int lpf, double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers,
                   int radius, int step, int normalize, float* windows, int mem_space) {
    int64_t n_windows;
    std::vector<int> win_utt;
    F2_TRY(f2_check_input_batch(ctx, wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, center_offsets, centers, radius,
                             step, windows, mem_space, nullptr, &n_windows, &win_utt));
    if (n_windows == 0) return F2_OK;

    // envelopes of the whole batch, by the routes of f2_filterbank_envelope_fused (gfb_or_null = NULL), into a scratch buffer
    const f2_batch X = {wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, mem_space};
    double* d_env;
    F2_TRY(f2_batch_envelopes(ctx, X, nullptr, nullptr, true, &d_env));

    // all windows of the batch in one gather launch: centres and the utterance of every window in one upload
    const int64_t* d_centers;
    const int* d_win_utt;
    F2_TRY(f2_upload_windows(ctx, centers, win_utt.data(), n_windows, &d_centers, &d_win_utt));
    return window_tail(ctx, windows, n_windows, radius, C, normalize, mem_space, [&](float* d_windows) {
        return f2_launch_gather_ragged(ctx, d_env, C, (const int64_t*)ctx->offsets.ptr, d_centers, d_win_utt, n_windows, radius, step, normalize,
                                       d_windows, (int*)ctx->flags.ptr);
    });
}

// f2_noise_pick / f2_shaped_noise_pick: the clean samples go up (host calls), the sigma kernel and k_noise_pick or k_shaped_noise_pick
// run, the float64 samples and sigma come back. A device call waits only for sigma. colours: the call is f2_shaped_noise_pick,
// which needs its taps unless every utterance is clean.
static int noise_pick_call(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, int B, f2_noise_pick_args N, bool colours,
                           double* noisy, double* sigma_or_null, int mem_space) {
    noise_pick_meta M;
    return f2_stage_call(
        ctx, offsets, B, mem_space,
        [&]() -> int {   // (the dtype before B, and the offsets last and only where there is an utterance: they may be NULL without)
            F2_TRY(f2_check_wave_dtype(ctx, wave_dtype));
            F2_CHECK(ctx, B >= 0, F2_ERR_INVALID, "bad batch size (B=%d)", B);
            F2_TRY(f2_check_mem_space(ctx, mem_space, false));
            F2_TRY(f2_check_noise_pick(ctx, B, N));
            if (B > 0) F2_TRY(f2_check_offsets(ctx, offsets, B, "offsets"));
            return colours ? f2_check_noise_colours(ctx, B, &N, true) : F2_OK;
        },
        [&](f2_meta_carve* meta) {
            M.carve(meta, B, offsets, N);
            return F2_OK;
        },
        wave, [&](int64_t total, const void** d_wave) { return f2_stage_wave(ctx, wave, wave_dtype, total, mem_space, d_wave); },
        &f2_ctx::levels, noisy, sizeof(double),
        [&](const void* d_wave, const int64_t* d_offsets, int64_t total, double* d_out) {
            return M.launch(ctx, d_wave, wave_dtype, d_offsets, offsets, B, total, N, d_out);
        },
        sigma_or_null, (size_t)(B > 0 ? B : 0), &M.d_sigma);
}

int f2_noise_pick(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, int B, const double* snr_db, int K,
                  const int32_t* level_of, uint32_t first_utterance, uint64_t seed, double* noisy, double* sigma_or_null, int mem_space) {
    return noise_pick_call(ctx, wave, wave_dtype, offsets, B, {snr_db, K, level_of, first_utterance, seed}, false, noisy, sigma_or_null,
                           mem_space);
}

int f2_shaped_noise_pick(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, int B, const double* snr_db,
                         const double* fir, const int64_t* fir_offsets, int K, const int32_t* level_of, uint32_t first_utterance,
                         uint64_t seed, double* noisy, double* sigma_or_null, int mem_space) {
    return noise_pick_call(ctx, wave, wave_dtype, offsets, B, {snr_db, K, level_of, first_utterance, seed, fir, fir_offsets}, true, noisy,
                           sigma_or_null, mem_space);
}

// f2_gather_windows_mixed: the envelopes go up (host calls), the windows are gathered through the matrices of their utterances' levels
// and come back; the end of the call is f2_input_batch's.
int f2_gather_windows_mixed(f2_ctx* ctx, const double* env, const int64_t* offsets, int B, int C, const int64_t* center_offsets,
                            const int64_t* centers, int radius, int step, int normalize, const double* mix, int K, const int32_t* mix_of,
                            float* windows, int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_CHECK(ctx, B >= 0 && C > 0 && radius >= 0 && step >= 0, F2_ERR_INVALID, "bad size");
    f2_mix_gather_args S;
    S.mix = mix, S.K = K, S.mix_of = mix_of;
    F2_TRY(f2_check_mix_gather(ctx, B, C, radius, &S));
    int64_t n_windows;
    std::vector<int> win_utt;
    F2_TRY(f2_check_window_lists(ctx, offsets, B, center_offsets, centers, radius, step, env && centers && windows, &n_windows, &win_utt));
    if (n_windows == 0) return F2_OK;
    mix_gather_meta G;
    f2_meta_carve meta;
    G.carve(&meta, B, S);
    F2_TRY(meta.reserve(ctx));
    F2_TRY(G.reserve(ctx));
    const void* d_env;
    F2_TRY(f2_stage_input(ctx, env, sizeof(double) * (size_t)C * (size_t)offsets[B], mem_space, &d_env));
    F2_TRY(f2_upload_offsets(ctx, offsets, B));
    f2_window_list W = {nullptr, nullptr, true, n_windows, radius, step, normalize};
    F2_TRY(f2_upload_windows(ctx, centers, win_utt.data(), n_windows, &W.centers, &W.win_utt));
    return window_tail(ctx, windows, n_windows, radius, C, normalize, mem_space,
                       [&](float* d_windows) { return G.launch(ctx, (const double*)d_env, B, C, W, d_windows); });
}

// The one window path behind a noise stage: f2_input_batch_filtered, and without cutoffs f2_input_batch_masked, and without maskers
// f2_input_batch_smeared, and without matrices f2_input_batch_coloured, and with fir == NULL f2_input_batch_wet, and without rooms
// f2_input_batch_noisy.
int f2_input_batch_filtered(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C, int lpf,
                          double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers, int radius, int step,
                          int normalize, const double* rir, const int64_t* rir_offsets, int Kr, const int32_t* room_of, const double* snr_db,
                          const double* fir, const int64_t* fir_offsets, int K, const int32_t* level_of, uint32_t first_utterance,
                          uint64_t seed, const double* mix, int Km, const int32_t* mix_of, const double* masker_snr_db, const double* masker,
                          const int64_t* masker_offsets, int R, const int32_t* masker_of, int Kk, const int32_t* masker_level_of,
                          const double* cutoff_levels_hz, int Kc, const int32_t* cutoff_of, float* windows, int mem_space) {
    f2_augment_args A = f2_augment_args::of(rir, rir_offsets, Kr, room_of, snr_db, fir, fir_offsets, K, level_of, first_utterance, seed, mix, Km,
                                            mix_of)
                            .with_maskers(masker_snr_db, masker, masker_offsets, R, masker_of, Kk, masker_level_of)
                            .with_cutoffs(cutoff_levels_hz, Kc, cutoff_of);
    int64_t n_windows;
    std::vector<int> win_utt;
    F2_TRY(f2_check_input_batch(ctx, wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, center_offsets, centers, radius,
                             step, windows, mem_space, &A.noise, &n_windows, &win_utt));
    F2_TRY(A.check(ctx, B, C, radius, lpf));
    if (n_windows == 0) return F2_OK;
    f2_batch X = {nullptr, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, F2_MEM_DEVICE};
    F2_TRY(f2_stage_wave(ctx, wave, wave_dtype, offsets[B], mem_space, &X.wave));
    const f2_window_list W = {centers, win_utt.data(), false, n_windows, radius, step, normalize};
    return window_tail(ctx, windows, n_windows, radius, C, normalize, mem_space,
                       [&](float* d_windows) { return f2_launch_noisy_windows(ctx, X, W, A, d_windows); });
}

int f2_input_batch_masked(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C, int lpf,
                          double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers, int radius, int step,
                          int normalize, const double* rir, const int64_t* rir_offsets, int Kr, const int32_t* room_of, const double* snr_db,
                          const double* fir, const int64_t* fir_offsets, int K, const int32_t* level_of, uint32_t first_utterance,
                          uint64_t seed, const double* mix, int Km, const int32_t* mix_of, const double* masker_snr_db, const double* masker,
                          const int64_t* masker_offsets, int R, const int32_t* masker_of, int Kk, const int32_t* masker_level_of,
                          float* windows, int mem_space) {
    return f2_input_batch_filtered(ctx, wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, center_offsets, centers, radius,
                                   step, normalize, rir, rir_offsets, Kr, room_of, snr_db, fir, fir_offsets, K, level_of, first_utterance, seed,
                                   mix, Km, mix_of, masker_snr_db, masker, masker_offsets, R, masker_of, Kk, masker_level_of, nullptr, 0,
                                   nullptr, windows, mem_space);
}

int f2_input_batch_smeared(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C, int lpf,
                           double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers, int radius, int step,
                           int normalize, const double* rir, const int64_t* rir_offsets, int Kr, const int32_t* room_of, const double* snr_db,
                           const double* fir, const int64_t* fir_offsets, int K, const int32_t* level_of, uint32_t first_utterance,
                           uint64_t seed, const double* mix, int Km, const int32_t* mix_of, float* windows, int mem_space) {
    return f2_input_batch_masked(ctx, wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, center_offsets, centers, radius,
                                 step, normalize, rir, rir_offsets, Kr, room_of, snr_db, fir, fir_offsets, K, level_of, first_utterance, seed,
                                 mix, Km, mix_of, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, windows, mem_space);
}

int f2_input_batch_coloured(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C, int lpf,
                            double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers, int radius, int step,
                            int normalize, const double* rir, const int64_t* rir_offsets, int Kr, const int32_t* room_of, const double* snr_db,
                            const double* fir, const int64_t* fir_offsets, int K, const int32_t* level_of, uint32_t first_utterance,
                            uint64_t seed, float* windows, int mem_space) {
    return f2_input_batch_smeared(ctx, wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, center_offsets, centers, radius,
                                  step, normalize, rir, rir_offsets, Kr, room_of, snr_db, fir, fir_offsets, K, level_of, first_utterance, seed,
                                  nullptr, 0, nullptr, windows, mem_space);
}

int f2_input_batch_wet(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C, int lpf,
                       double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers, int radius, int step,
                       int normalize, const double* rir, const int64_t* rir_offsets, int Kr, const int32_t* room_of, const double* snr_db,
                       int K, const int32_t* level_of, uint32_t first_utterance, uint64_t seed, float* windows, int mem_space) {
    return f2_input_batch_coloured(ctx, wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, center_offsets, centers, radius,
                                   step, normalize, rir, rir_offsets, Kr, room_of, snr_db, nullptr, nullptr, K, level_of, first_utterance,
                                   seed, windows, mem_space);
}

int f2_input_batch_noisy(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C,
                         int lpf, double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers,
                         int radius, int step, int normalize, const double* snr_db, int K, const int32_t* level_of,
                         uint32_t first_utterance, uint64_t seed, float* windows, int mem_space) {
    return f2_input_batch_coloured(ctx, wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, center_offsets, centers, radius,
                                   step, normalize, nullptr, nullptr, 0, nullptr, snr_db, nullptr, nullptr, K, level_of, first_utterance,
                                   seed, windows, mem_space);
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

// The small arrays of a picture call: [span records (4 B) | range words (2 B)], all 8-byte words, in one upload
struct picture_meta {
    int64_t* d_utt = nullptr;
    uint64_t* d_range = nullptr;
    std::vector<double> range;   // the range words as they come back (picture_range reads them after the wait)
    void add(f2_meta_carve* carve, int B) { carve->add(&d_utt, 4 * (size_t)B), carve->add(&d_range, 2 * (size_t)B); }
};

// Pool, levels and range of the envelopes at d_env (device; offsets already uploaded; P carved), results to the caller's buffers in
// mem_space. Pictures a host caller asked for, and the pooled values the levels are made from when nobody asked for them, live in
// ctx->work / ctx->work2. Enqueues everything, the copies to the caller included, and does not wait.
int picture_enqueue(f2_ctx* ctx, const double* d_env, const int64_t* offsets, int B, int C, const int64_t* spans_or_null, int width,
                    int pool, picture_meta* P, double* pooled_or_null, uint8_t* levels_or_null, bool want_range, int mem_space) {
    const size_t pixels = (size_t)B * (size_t)C * (size_t)width;
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
    f2_output pooled, levels;   // (the levels are made from the pooled values: those are needed whoever asked)
    F2_TRY(f2_place(ctx, ctx->work, pooled_or_null, sizeof(double) * pixels, mem_space, true, &pooled));
    F2_TRY(f2_place(ctx, ctx->work2, levels_or_null, pixels, mem_space, false, &levels));
    F2_TRY(f2_upload_async(ctx, P->d_utt, meta.data(), sizeof(int64_t) * meta.size()));
    F2_TRY(f2_launch_picture_pool(ctx, d_env, (const int64_t*)ctx->offsets.ptr, P->d_utt, B, C, width, pool, blocks, pooled.as<double>(), P->d_range));
    if (levels.dev) F2_TRY(f2_launch_picture_levels(ctx, pooled.as<double>(), P->d_range, B, C, width, levels.as<uint8_t>()));
    F2_TRY(f2_copy_back(ctx, pooled));
    F2_TRY(f2_copy_back(ctx, levels));
    P->range.assign(want_range ? 2 * (size_t)B : 0, 0.0);
    if (want_range)
        F2_HIP(ctx, hipMemcpyAsync(P->range.data(), P->d_range, sizeof(double) * P->range.size(), hipMemcpyDeviceToHost, ctx->stream));
    return F2_OK;
}

// after the wait for the stream: the range words of picture_enqueue as the caller gets them
void picture_range(const picture_meta& P, int B, double* range_or_null) {
    if (range_or_null)
        for (int b = 0; b < B; ++b) {   // no pixel > 0: the maximum's word is still 0, the minimum's still +inf
            const bool any = P.range[2 * (size_t)b + 1] > 0.0;
            range_or_null[2 * b] = any ? P.range[2 * (size_t)b] : 0.0;
            range_or_null[2 * b + 1] = any ? P.range[2 * (size_t)b + 1] : 0.0;
        }
}

// both, for a call that makes pictures only. Waits for the stream.
int picture_device(f2_ctx* ctx, const double* d_env, const int64_t* offsets, int B, int C, const int64_t* spans_or_null, int width,
                   int pool, double* pooled_or_null, uint8_t* levels_or_null, double* range_or_null, int mem_space) {
    picture_meta P;
    f2_meta_carve carve;
    P.add(&carve, B);
    F2_TRY(carve.reserve(ctx));
    F2_TRY(picture_enqueue(ctx, d_env, offsets, B, C, spans_or_null, width, pool, &P, pooled_or_null, levels_or_null, range_or_null != nullptr,
                           mem_space));
    F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    picture_range(P, B, range_or_null);
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
    const void* d_env;
    F2_TRY(f2_stage_into(ctx, ctx->stage_aux, env, sizeof(double) * (size_t)C * (size_t)total, mem_space, &d_env));
    return picture_device(ctx, (const double*)d_env, offsets, B, C, spans_or_null, width, pool, pooled_or_null, levels_or_null, range_or_null, mem_space);
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
    F2_TRY(f2_upload_offsets(ctx, offsets, B));   // (a batch without a sample still gets its pictures: picture_device reads them)
    const f2_batch X = {wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, mem_space};
    double* d_env = nullptr;
    if (total > 0) F2_TRY(f2_batch_envelopes(ctx, X, nullptr, nullptr, true, &d_env));
    return picture_device(ctx, d_env, offsets, B, C, spans_or_null, width, pool, pooled_or_null, levels_or_null, range_or_null, mem_space);
}

}  // extern "C"

// ---- `cnn eval --figure`, `--occlusion`, `--saliency`: the reductions f2_score_track, f2_occlusion_map and f2_saliency_map share their
// argument checks and their records; the fused calls f2_eval_figure_batch, f2_eval_occlusion_batch and f2_eval_saliency_batch are one
// body (figure_call) = strided evaluation + picture + reductions over one set of envelopes ----
namespace {

// The records of k_score_track (f2_internal.h) of one reduction: made for U utterances with the spans given and named among the
// call's small arrays (add; `blocks`: the workgroups every utterance gets), uploaded right before the launch (upload)
struct track_meta {
    std::vector<int64_t> rec;
    int64_t* d_rec = nullptr;
    int64_t blocks = 0;
    void add(f2_meta_carve* carve, const int64_t* window_offsets, int U, const int64_t* spans, int hop, int width) {
        rec.resize(5 * (size_t)U);
        for (int u = 0; u < U; ++u) {
            const int64_t s = spans[2 * u], m = spans[2 * u + 1] - s;
            const int lg = f2_track_lanes_log2(m, width, hop);
            int64_t* r = &rec[5 * (size_t)u];
            r[0] = window_offsets[u], r[1] = window_offsets[u + 1] - window_offsets[u], r[2] = s, r[3] = m, r[4] = lg;
            blocks = std::max(blocks, f2_track_blocks(width, lg));
        }
        carve->add(&d_rec, rec.size());
    }
    int upload(f2_ctx* ctx) const { return f2_upload_async(ctx, d_rec, rec.data(), sizeof(int64_t) * rec.size()); }
};

// The argument errors of the three reductions, in their order; nothing is launched or written before they pass. Of the call: own()
// - the checks of its own size argument; have_data - its input pointers are there (asked for once there is a row) - and what to say
// when they or `out` are not.
template <class Own>
int reduction_check(f2_ctx* ctx, int U, int hop, int64_t origin, int width, const int64_t* window_offsets, const int64_t* spans,
                    int mem_space, Own own, bool have_data, const char* no_data, const void* out, const char* no_out) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_CHECK(ctx, U >= 0 && hop >= 1 && origin >= 0 && width >= 1, F2_ERR_INVALID,
             "U (%d) and origin (%lld) must be at least 0, hop (%d) and width (%d) at least 1", U, (long long)origin, hop, width);
    F2_TRY(own());
    F2_TRY(f2_check_offsets(ctx, window_offsets, U, "window_offsets"));
    F2_CHECK(ctx, spans, F2_ERR_INVALID, "spans is NULL");
    F2_CHECK(ctx, have_data || window_offsets[U] == 0, F2_ERR_INVALID, "%s", no_data);
    F2_CHECK(ctx, out || U == 0, F2_ERR_INVALID, "%s", no_out);
    int64_t max_rows = 0;
    for (int u = 0; u < U; ++u) {
        F2_CHECK(ctx, spans[2 * u] >= 0 && spans[2 * u + 1] >= spans[2 * u], F2_ERR_INVALID, "utterance %d: [%lld, %lld) is not a span", u,
                 (long long)spans[2 * u], (long long)spans[2 * u + 1]);
        max_rows = std::max(max_rows, window_offsets[u + 1] - window_offsets[u]);
    }
    F2_CHECK(ctx, width <= PICTURE_MAX_WIDTH, F2_ERR_UNSUPPORTED, "width %d (at most %d columns)", width, PICTURE_MAX_WIDTH);
    int64_t t_last = 0;   // the sample of the last row of the longest utterance has to be an int64
    F2_CHECK(ctx, max_rows == 0 || (!__builtin_mul_overflow(max_rows - 1, (int64_t)hop, &t_last) && !__builtin_add_overflow(t_last, origin, &t_last)),
             F2_ERR_UNSUPPORTED, "row %lld at hop %d from origin %lld is beyond int64", (long long)(max_rows - 1), hop, (long long)origin);
    return F2_OK;
}

// One output a fused call reduces its windows to: over the caller's spans in `width` columns (the track, a map), or - summary - over
// the whole utterances [0, n_b) in one column
struct figure_reduction {
    double* callers;   // NULL: not asked for (its records are still named)
    size_t bytes;
    bool summary;
};

// The body of the three fused calls. The envelopes are made once (eval_envelopes) and stay in ctx->stage_out for the picture and the
// window loop. Order on the stream: envelopes, picture (pooled values in ctx->work, a host caller's levels in ctx->work2, both copied
// out before anything else is queued), window loop (which takes ctx->work as the convolution workspace and ctx->work2 for its window
// lists: behind the picture's last reader on the stream, and f2_reserve waits for the stream before it moves a block), the reductions
// in the order of `red`, each with its copy to a host caller, whose outputs lie in that order behind the scores in ctx->stage_aux.
// One carve of ctx->meta for all. Of the call:
//   check(R, n_total)   its own argument errors, behind the shared ones (the tables between them cannot fail) and before
//                       window_offsets_or_null, the first thing written
//   carve(meta)         names its small arrays behind the picture's and the records
//   windows(E, nbh, n_total, tail_bytes)   for n_total > 0: its scratch, eval_cnn_begin and strided_window_loop
//   launch(E, d_rec, width, blocks, out)   the kernel of its reductions (also over no rows, when there is no window)
template <class Check, class Carve, class Windows, class Launch>
int figure_call(f2_ctx* ctx, const f2_cnn* cnn, const f2_batch& X, int radius, int step, int hop, const int64_t* spans_or_null, int width,
                int pool, uint8_t* levels_or_null, double* range_or_null, int64_t* window_offsets_or_null, Check check, Carve carve,
                Windows windows, const figure_reduction* red, int n_red, Launch launch) {
    const int64_t* offsets = X.offsets;
    const int B = X.B, C = X.C, mem_space = X.mem_space;
    eval_call E;
    F2_TRY(eval_check(ctx, cnn, X, radius, step, &E));
    F2_CHECK(ctx, hop >= 1, F2_ERR_INVALID, "hop must be at least 1 sample (got %d)", hop);
    F2_TRY(picture_check(ctx, offsets, B, C, spans_or_null, width, pool, mem_space));
    const int64_t total = X.total();
    F2_CHECK(ctx, X.wave || total == 0, F2_ERR_INVALID, "null wave");
    std::vector<int64_t> nbh((size_t)B), wo((size_t)B + 1, 0), spans(2 * (size_t)B), whole(2 * (size_t)B);
    for (int b = 0; b < B; ++b) {
        const int64_t nb = offsets[b + 1] - offsets[b];
        nbh[(size_t)b] = strided_windows(nb, E.R, step, hop);
        wo[(size_t)b + 1] = wo[(size_t)b] + nbh[(size_t)b];
        spans[2 * (size_t)b] = spans_or_null ? spans_or_null[2 * b] : 0;
        spans[2 * (size_t)b + 1] = spans_or_null ? spans_or_null[2 * b + 1] : nb;
        whole[2 * (size_t)b] = 0, whole[2 * (size_t)b + 1] = nb;
    }
    const int64_t n_total = wo[(size_t)B];
    F2_TRY(check(E.R, n_total));
    if (window_offsets_or_null) memcpy(window_offsets_or_null, wo.data(), sizeof(int64_t) * wo.size());
    if (B == 0) return F2_OK;

    const bool want_picture = levels_or_null || range_or_null, host = mem_space != F2_MEM_DEVICE;
    size_t tail_bytes = 0;   // a host caller's reductions: behind the scores
    picture_meta P;
    track_meta T[2];
    f2_meta_carve meta;
    P.add(&meta, B);
    for (int i = 0; i < n_red; ++i) {
        T[i].add(&meta, wo.data(), B, red[i].summary ? whole.data() : spans.data(), hop, red[i].summary ? 1 : width);
        if (host && red[i].callers) tail_bytes += red[i].bytes;
    }
    carve(&meta);
    F2_TRY(meta.reserve(ctx));
    F2_TRY(f2_upload_offsets(ctx, offsets, B));   // (a batch without a sample still gets its pictures)
    if (total > 0) F2_TRY(eval_envelopes(ctx, &E, X, nullptr, n_total));
    if (want_picture)
        F2_TRY(picture_enqueue(ctx, E.d_env, offsets, B, C, spans_or_null, width, pool, &P, nullptr, levels_or_null, range_or_null != nullptr,
                               mem_space));
    if (n_total > 0) {
        F2_TRY(windows(&E, nbh, n_total, tail_bytes));
        F2_TRY(eval_dense_flush(ctx, cnn, &E));
    } else {
        F2_TRY(f2_place_scores(ctx, nullptr, nullptr, 0, mem_space, false, false, tail_bytes, &E.out));
    }
    char* tail = E.out.tail;
    for (int i = 0; i < n_red; ++i) {
        if (!red[i].callers) continue;
        f2_output o;
        o.dev = host ? tail : (char*)red[i].callers, o.host = host ? (char*)red[i].callers : nullptr;
        o.bytes = red[i].bytes, o.callers = !host;
        if (host) tail += red[i].bytes;
        F2_TRY(T[i].upload(ctx));
        F2_TRY(launch(E, T[i].d_rec, red[i].summary ? 1 : width, T[i].blocks, o.as<double>()));
        F2_TRY(f2_copy_back(ctx, o));
    }
    int rc = F2_OK;
    if (n_total > 0)
        rc = eval_cnn_end(ctx, cnn, &E);   // (waits for the stream)
    else
        F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (rc == F2_OK || rc == F2_ERR_NONPOSITIVE) picture_range(P, B, range_or_null);
    return rc;
}

}  // namespace

extern "C" {

int f2_score_track(f2_ctx* ctx, const float* scores, const uint8_t* labels, const int64_t* window_offsets, int U, const int64_t* spans,
                   int64_t origin, int hop, int width, double* track, int mem_space) {
    F2_TRY(reduction_check(ctx, U, hop, origin, width, window_offsets, spans, mem_space, [] { return F2_OK; }, scores && labels,
                           "null scores or labels", track, "track is NULL"));
    if (U == 0) return F2_OK;
    const size_t n_rows = (size_t)window_offsets[U];
    track_meta T;
    f2_meta_carve meta;
    T.add(&meta, window_offsets, U, spans, hop, width);
    F2_TRY(meta.reserve(ctx));
    const void *d_scores, *d_labels;
    F2_TRY(f2_stage_input(ctx, scores, sizeof(float) * 2 * n_rows, mem_space, &d_scores));
    F2_TRY(f2_stage_into(ctx, ctx->stage_aux, labels, n_rows, mem_space, &d_labels));
    f2_output out;
    F2_TRY(f2_place(ctx, ctx->stage_out, track, sizeof(double) * 5 * (size_t)U * (size_t)width, mem_space, false, &out));
    F2_TRY(T.upload(ctx));
    F2_TRY(f2_launch_score_track(ctx, (const float*)d_scores, (const uint8_t*)d_labels, T.d_rec, U, origin, hop, width, T.blocks, out.as<double>()));
    F2_TRY(f2_copy_back(ctx, out));
    return f2_host_wait(ctx, mem_space);
}

// figure_call with the network's own windows and one reduction, the track
int f2_eval_figure_batch(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs,
                         int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step, int hop,
                         const int64_t* spans_or_null, int width, int pool, uint8_t* levels_or_null, double* range_or_null,
                         double* track_or_null, float* scores_or_null, uint8_t* labels_or_null, int64_t* window_offsets_or_null,
                         int mem_space) {
    const f2_batch X = {wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, mem_space};
    auto windows = [&](eval_call* E, const std::vector<int64_t>& nbh, int64_t n_total, size_t tail_bytes) -> int {
        const int64_t chunk = n_total < CNN_CHUNK ? n_total : CNN_CHUNK;
        F2_TRY(eval_cnn_begin(ctx, cnn, E, chunk, n_total, C, scores_or_null, labels_or_null, mem_space, track_or_null != nullptr, tail_bytes));
        return strided_window_loop(ctx, cnn, E, X, nbh, chunk, radius, step, hop, (float*)ctx->xbuf.ptr);
    };
    auto launch = [&](const eval_call& E, const int64_t* d_rec, int w, int64_t blocks, double* out) {
        return f2_launch_score_track(ctx, E.out.scores.as<float>(), E.out.labels.as<uint8_t>(), d_rec, B, (int64_t)radius * step, hop, w, blocks, out);
    };
    const figure_reduction track = {track_or_null, sizeof(double) * 5 * (size_t)B * (size_t)width, false};
    return figure_call(ctx, cnn, X, radius, step, hop, spans_or_null, width, pool, levels_or_null, range_or_null, window_offsets_or_null,
                       [](int, int64_t) { return F2_OK; }, [](f2_meta_carve*) {}, windows, &track, 1, launch);
}

}  // extern "C"

// ---- `cnn eval --occlusion`: f2_occlude_windows, f2_occlusion_map, and f2_eval_occlusion_batch = the figure call with every window
// evaluated at K + 1 occlusion levels and the map of their differences instead of the track ----
namespace {

constexpr int OCCLUSION_MAX_PATCHES = 1024;

// the argument errors the occlusion calls share: K patches inside an (R, C) window, n windows at K + 1 levels
int occlusion_check(f2_ctx* ctx, const int32_t* patches, int K, int min_K, int R, int C, int64_t n) {
    F2_CHECK(ctx, K >= min_K, F2_ERR_INVALID, "K (%d) must be at least %d", K, min_K);
    F2_CHECK(ctx, patches || K == 0, F2_ERR_INVALID, "patches is NULL");
    F2_CHECK(ctx, K <= OCCLUSION_MAX_PATCHES, F2_ERR_UNSUPPORTED, "%d patches (at most %d)", K, OCCLUSION_MAX_PATCHES);
    for (int k = 0; k < K; ++k) {
        const int32_t* p = patches + 4 * (size_t)k;
        F2_CHECK(ctx, p[0] >= 0 && p[1] <= R && p[0] < p[1] && p[2] >= 0 && p[3] <= C && p[2] < p[3], F2_ERR_INVALID,
                 "patch %d: rows [%d, %d) x channels [%d, %d) is empty or leaves the %d x %d window", k, p[0], p[1], p[2], p[3], R, C);
    }
    int64_t levels = 0;
    F2_CHECK(ctx, !__builtin_mul_overflow(n, (int64_t)K + 1, &levels) && levels < (int64_t(1) << 31), F2_ERR_UNSUPPORTED,
             "%lld windows at %d levels (fewer than 2^31 in all)", (long long)n, K + 1);
    return F2_OK;
}

// the patch table as it goes up: K x 4 int32 in 2 K 8-byte words of the call's metadata
void occlusion_patch_words(const int32_t* patches, int K, std::vector<int64_t>* words) {
    words->assign(2 * (size_t)K, 0);
    if (K > 0) memcpy(words->data(), patches, sizeof(int32_t) * 4 * (size_t)K);
}

}  // namespace

extern "C" {

int f2_occlude_windows(f2_ctx* ctx, const float* x, int64_t n, int R, int C, const int32_t* patches, int K, float fill, float* out,
                       int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_CHECK(ctx, n >= 0 && R >= 0 && C >= 0 && K >= 0, F2_ERR_INVALID, "negative size (n=%lld, R=%d, C=%d, K=%d)", (long long)n, R, C, K);
    F2_CHECK(ctx, (x && out) || n == 0, F2_ERR_INVALID, "null data pointer");
    F2_TRY(occlusion_check(ctx, patches, K, 0, R, C, n));
    F2_CHECK(ctx, (int64_t)R * C < (int64_t(1) << 31), F2_ERR_UNSUPPORTED, "windows of %d x %d values", R, C);
    if (n == 0 || R == 0 || C == 0) return F2_OK;
    const int64_t L = (int64_t)K + 1;
    const size_t xs = (size_t)R * (size_t)C;

    std::vector<int64_t> words;
    occlusion_patch_words(patches, K, &words);
    int64_t* d_words = nullptr;
    f2_meta_carve meta;
    meta.add(&d_words, words.size());
    F2_TRY(meta.reserve(ctx));
    if (K > 0) F2_TRY(f2_upload_async(ctx, d_words, words.data(), sizeof(int64_t) * words.size()));
    // Device memory: one launch. Host memory: chunks of at most CNN_CHUNK output windows through stage_in / stage_out, each chunk's
    // windows back before the next one goes up.
    const int64_t per = CNN_CHUNK / L > 0 ? CNN_CHUNK / L : 1;
    const int64_t chunk = mem_space == F2_MEM_DEVICE || n < per ? n : per;
    f2_output win;
    F2_TRY(f2_place(ctx, ctx->stage_out, out, sizeof(float) * xs * (size_t)(chunk * L), mem_space, true, &win));
    win.bytes = sizeof(float) * xs * (size_t)(n * L);   // (of the whole output: chunk() cuts it)
    for (int64_t s = 0; s < n; s += chunk) {
        const int64_t m = n - s < chunk ? n - s : chunk;
        const void* d_x;
        F2_TRY(f2_stage_input(ctx, x + (size_t)s * xs, sizeof(float) * xs * (size_t)m, mem_space, &d_x));
        const f2_output o = win.chunk(sizeof(float) * xs * (size_t)(s * L), sizeof(float) * xs * (size_t)(m * L));
        F2_TRY(f2_launch_occlude_windows(ctx, (const float*)d_x, m, R, C, (const int32_t*)d_words, K, fill, o.as<float>()));
        F2_TRY(f2_copy_back(ctx, o));
        F2_TRY(f2_host_wait(ctx, mem_space));
    }
    return F2_OK;
}

int f2_occlusion_map(f2_ctx* ctx, const float* scores, const uint8_t* labels, const int64_t* window_offsets, int U, int K,
                     const int64_t* spans, int64_t origin, int hop, int width, double* map, int mem_space) {
    auto own = [&]() -> int {
        F2_CHECK(ctx, K >= 1, F2_ERR_INVALID, "K (%d) must be at least 1", K);
        F2_CHECK(ctx, K <= OCCLUSION_MAX_PATCHES, F2_ERR_UNSUPPORTED, "%d patches (at most %d)", K, OCCLUSION_MAX_PATCHES);
        return F2_OK;
    };
    F2_TRY(reduction_check(ctx, U, hop, origin, width, window_offsets, spans, mem_space, own, scores && labels, "null scores or labels", map,
                           "map is NULL"));
    if (U == 0) return F2_OK;
    const size_t level_rows = ((size_t)K + 1) * (size_t)window_offsets[U];
    track_meta T;
    f2_meta_carve meta;
    T.add(&meta, window_offsets, U, spans, hop, width);
    F2_TRY(meta.reserve(ctx));
    const void *d_scores, *d_labels;
    F2_TRY(f2_stage_input(ctx, scores, sizeof(float) * 2 * level_rows, mem_space, &d_scores));
    F2_TRY(f2_stage_into(ctx, ctx->stage_aux, labels, level_rows, mem_space, &d_labels));
    f2_output out;
    F2_TRY(f2_place(ctx, ctx->stage_out, map, sizeof(double) * 4 * (size_t)U * (size_t)K * (size_t)width, mem_space, false, &out));
    F2_TRY(T.upload(ctx));
    F2_TRY(f2_launch_occlusion_map(ctx, (const float*)d_scores, (const uint8_t*)d_labels, T.d_rec, U, K, origin, hop, width, T.blocks, out.as<double>()));
    F2_TRY(f2_copy_back(ctx, out));
    return f2_host_wait(ctx, mem_space);
}

// figure_call with two changes: the window stage writes a chunk of m = chunk / (K + 1) windows to ctx->occ_src and k_occlude_windows
// expands them into ctx->xbuf, window-major, so that the convolutions and the dense groups see m (K + 1) windows and write contiguous
// score rows; the map and the summary take the track's place.
int f2_eval_occlusion_batch(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs,
                            int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step, int hop,
                            const int32_t* patches, int K, float fill, const int64_t* spans_or_null, int width, int pool,
                            uint8_t* levels_or_null, double* range_or_null, double* map_or_null, double* summary_or_null,
                            float* scores_or_null, uint8_t* labels_or_null, int64_t* window_offsets_or_null, int mem_space) {
    const f2_batch X = {wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, mem_space};
    const int64_t L = (int64_t)K + 1;
    std::vector<int64_t> words;
    int64_t* d_words = nullptr;
    auto check = [&](int R, int64_t n_total) -> int {
        F2_CHECK(ctx, fill >= 0.f && fill <= 1.f, F2_ERR_INVALID, "fill (%g) must lie in [0, 1], the range of a normalised window", (double)fill);
        return occlusion_check(ctx, patches, K, 1, R, C, n_total);
    };
    auto windows = [&](eval_call* E, const std::vector<int64_t>& nbh, int64_t n_total, size_t tail_bytes) -> int {
        const int64_t per = CNN_CHUNK / L > 0 ? CNN_CHUNK / L : 1;   // source windows of a chunk
        const int64_t chunk = n_total < per ? n_total : per;
        F2_TRY(f2_reserve(ctx, ctx->occ_src, sizeof(float) * (size_t)chunk * E->R * (size_t)C));
        F2_TRY(eval_cnn_begin(ctx, cnn, E, chunk * L, n_total * L, C, scores_or_null, labels_or_null, mem_space, map_or_null || summary_or_null,
                              tail_bytes));
        F2_TRY(f2_upload_async(ctx, d_words, words.data(), sizeof(int64_t) * words.size()));
        const occlusion_stage occ = {(const int32_t*)d_words, K, fill};
        return strided_window_loop(ctx, cnn, E, X, nbh, chunk, radius, step, hop, (float*)ctx->occ_src.ptr, &occ);
    };
    auto launch = [&](const eval_call& E, const int64_t* d_rec, int w, int64_t blocks, double* out) {
        return f2_launch_occlusion_map(ctx, E.out.scores.as<float>(), E.out.labels.as<uint8_t>(), d_rec, B, K, (int64_t)radius * step, hop, w, blocks, out);
    };
    const size_t summary_bytes = sizeof(double) * 4 * (size_t)B * (size_t)K;
    const figure_reduction red[2] = {{map_or_null, summary_bytes * (size_t)width, false}, {summary_or_null, summary_bytes, true}};
    auto carve = [&](f2_meta_carve* meta) { occlusion_patch_words(patches, K, &words), meta->add(&d_words, words.size()); };
    return figure_call(ctx, cnn, X, radius, step, hop, spans_or_null, width, pool, levels_or_null, range_or_null, window_offsets_or_null, check,
                       carve, windows, red, 2, launch);
}

}  // extern "C"

// ---- `cnn eval --saliency`: f2_saliency_map, and f2_eval_saliency_batch = the figure call with every window differentiated while it
// is in scratch (f2_cnn_grad.hip) and the map of the per-channel profiles instead of the track ----
extern "C" {

int f2_saliency_map(f2_ctx* ctx, const double* profile, const int64_t* window_offsets, int U, int C, const int64_t* spans, int64_t origin,
                    int hop, int width, double* map, int mem_space) {
    auto own = [&]() -> int {
        F2_CHECK(ctx, C >= 1, F2_ERR_INVALID, "C (%d) must be at least 1", C);
        F2_CHECK(ctx, C <= 65535, F2_ERR_UNSUPPORTED, "%d channels (at most 65535)", C);
        return F2_OK;
    };
    F2_TRY(reduction_check(ctx, U, hop, origin, width, window_offsets, spans, mem_space, own, profile != nullptr, "profile is NULL", map,
                           "map is NULL"));
    if (U == 0) return F2_OK;
    track_meta T;
    f2_meta_carve meta;
    T.add(&meta, window_offsets, U, spans, hop, width);
    F2_TRY(meta.reserve(ctx));
    const void* d_profile;
    F2_TRY(f2_stage_input(ctx, profile, sizeof(double) * 2 * (size_t)C * (size_t)window_offsets[U], mem_space, &d_profile));
    f2_output out;
    F2_TRY(f2_place(ctx, ctx->stage_out, map, sizeof(double) * 3 * (size_t)U * (size_t)C * (size_t)width, mem_space, false, &out));
    F2_TRY(T.upload(ctx));
    F2_TRY(f2_launch_saliency_map(ctx, (const double*)d_profile, T.d_rec, U, C, origin, hop, width, T.blocks, out.as<double>()));
    F2_TRY(f2_copy_back(ctx, out));
    return f2_host_wait(ctx, mem_space);
}

// figure_call with two changes: after the normal route's convolutions a chunk's windows (still in ctx->xbuf) go through
// f2_launch_cnn_input_gradient, which keeps 16 C bytes of profile per window in ctx->sal_profile; the map and the summary, reduced
// from those rows, take the track's place.
int f2_eval_saliency_batch(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs,
                           int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step, int hop,
                           const int64_t* spans_or_null, int width, int pool, uint8_t* levels_or_null, double* range_or_null,
                           double* map_or_null, double* summary_or_null, float* scores_or_null, uint8_t* labels_or_null,
                           int64_t* window_offsets_or_null, int mem_space) {
    const f2_batch X = {wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, mem_space};
    auto check = [&](int, int64_t) -> int {
        F2_CHECK(ctx, C <= 65535, F2_ERR_UNSUPPORTED, "%d channels (at most 65535)", C);
        return F2_OK;
    };
    auto windows = [&](eval_call* E, const std::vector<int64_t>& nbh, int64_t n_total, size_t tail_bytes) -> int {
        const int64_t chunk = n_total < CNN_CHUNK ? n_total : CNN_CHUNK;
        const bool differentiate = map_or_null || summary_or_null;
        if (differentiate) F2_TRY(f2_reserve(ctx, ctx->sal_profile, sizeof(double) * 2 * (size_t)C * (size_t)n_total));
        F2_TRY(eval_cnn_begin(ctx, cnn, E, chunk, n_total, C, scores_or_null, labels_or_null, mem_space, false, tail_bytes));
        saliency_stage sal = {(double*)ctx->sal_profile.ptr, 0};
        return strided_window_loop(ctx, cnn, E, X, nbh, chunk, radius, step, hop, (float*)ctx->xbuf.ptr, nullptr, differentiate ? &sal : nullptr);
    };
    auto launch = [&](const eval_call&, const int64_t* d_rec, int w, int64_t blocks, double* out) {
        return f2_launch_saliency_map(ctx, (const double*)ctx->sal_profile.ptr, d_rec, B, C, (int64_t)radius * step, hop, w, blocks, out);
    };
    const size_t summary_bytes = sizeof(double) * 3 * (size_t)B * (size_t)C;
    const figure_reduction red[2] = {{map_or_null, summary_bytes * (size_t)width, false}, {summary_or_null, summary_bytes, true}};
    return figure_call(ctx, cnn, X, radius, step, hop, spans_or_null, width, pool, levels_or_null, range_or_null, window_offsets_or_null, check,
                       [](f2_meta_carve*) {}, windows, red, 2, launch);
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

    int64_t* d_meta;
    f2_meta_carve carve;
    carve.add(&d_meta, meta.size());
    F2_TRY(carve.reserve(ctx));
    const void* d_audio;
    F2_TRY(f2_stage_input(ctx, audio, elem_bytes[pcm_format] * (size_t)channels * (size_t)total, mem_space, &d_audio));
    f2_output res;
    F2_TRY(f2_place(ctx, ctx->stage_out, out, sizeof(double) * (size_t)total_out, mem_space, true, &res));
    if (identity) {
        F2_TRY(f2_launch_pcm_convert(ctx, d_audio, pcm_format, channels, channel, total, res.as<double>()));
    } else {
        F2_TRY(resample_table(ctx, up, down, taps, half_len, T));
        F2_TRY(f2_upload_async(ctx, d_meta, meta.data(), sizeof(int64_t) * meta.size()));
        F2_TRY(f2_launch_resample(ctx, d_audio, pcm_format, channels, channel, d_meta, B, first[B], up, down, half_len, (int)T,
                                  (const double*)ctx->rs_tab.ptr, res.as<double>()));
    }
    F2_TRY(f2_copy_back(ctx, res));
    return f2_host_wait(ctx, mem_space);
}

}  // extern "C"
