/*
 * f2cnn_hip.h -- C ABI of libf2cnn_hip.so: the MI355X (gfx950) implementation of the F2CNN hot path.
 *
 * The reference (tictacmenthe/F2CNN) is pure Python and has no FFI; its boundary for this path is a
 * set of NumPy-in / NumPy-out functions. Each entry point below replaces the body of one of them
 * (file:line relative to the reference tree) and is what a ctypes binding in the reference would
 * call (see INTEGRATION.md for the stub). Plain pointers and sizes only; no torch / HIP types.
 *
 * Conventions
 *   - every function returns F2_OK (0) or a negative f2_status; f2_last_error() gives the text.
 *   - `mem_space` says whether DATA pointers (wave, gfb, env, x, scores, ...) are host or device
 *     pointers. Small metadata arrays (offsets, coefs, centers) are ALWAYS host pointers.
 *   - F2_MEM_HOST calls stage through device memory and return when the result is in the host
 *     buffer. F2_MEM_DEVICE calls enqueue on the context's stream and return immediately
 *     (f2_ctx_synchronize() or a stream-ordered consumer to wait): the small per-batch arrays they
 *     upload (offsets, utterance lists, ...) are staged through page-locked memory owned by the
 *     context, so a new batch shape does not wait for the stream either. What does wait: a scratch
 *     buffer that has to grow (the first call of a size), and the calls that hand an error flag of
 *     the device back (f2_gather_windows with normalisation, f2_eval_*: F2_ERR_NONPOSITIVE;
 *     f2_eval_noise_sweep also waits to hand back sigma and stats, f2_label_accuracy and
 *     f2_cnn_score_windows their counts, f2_envelope_picture and f2_gammatonegram_batch the range
 *     of every picture).
 *   - ragged batches: utterance b has n_b = offsets[b+1]-offsets[b] samples; its wave starts at
 *     wave + offsets[b]; its (C, n_b) C-order float64 matrix starts at out + C*offsets[b]. For a
 *     uniform batch this is the plain [B][C][N] layout, and each utterance's block is bit-for-bit the
 *     payload of the reference's .GFB.npy / .ENV1.npy file (row 0 = highest centre frequency).
 *   - one host thread per context; a context owns one device, one stream and its scratch memory.
 */
#ifndef F2CNN_HIP_H
#define F2CNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct f2_ctx f2_ctx;
typedef struct f2_cnn f2_cnn;

typedef enum {
    F2_OK = 0,
    F2_ERR_INVALID = -1,      /* bad argument (null pointer, negative size, ...)              */
    F2_ERR_HIP = -2,          /* a HIP runtime call failed (no device, launch failure, ...)    */
    F2_ERR_UNSUPPORTED = -3,  /* valid request this build cannot serve (e.g. row too long)     */
    F2_ERR_NOMEM = -4,        /* device or host allocation failed                              */
    F2_ERR_NONPOSITIVE = -5   /* normalizeInput met a value <= 0 (reference: ValueError)       */
} f2_status;

/* F2_MEM_HOST_ASYNC: host pointers like F2_MEM_HOST, but the call returns as soon as the copies and kernels are
 * queued on the context's stream; the host buffers must stay valid (and should be page-locked: f2_host_alloc, so
 * that the copies really are asynchronous) until f2_ctx_synchronize() returns. The file drivers use it with two
 * contexts so that batch k's device-to-host copy runs beside batch k+1's host-to-device copy and kernels.
 * Accepted by f2_erb_filterbank_batch, f2_envelope_batch and f2_filterbank_envelope_fused. */
enum { F2_MEM_HOST = 0, F2_MEM_DEVICE = 1, F2_MEM_HOST_ASYNC = 2 };
/* Alignment: device buffers need the natural alignment of their element type only (hipMalloc gives far more).
 * Utterance lengths are arbitrary: rows of the (C, n) matrices start wherever C-order puts them, and the kernels keep
 * their stores on whole 128-byte lines and their loads wide for any n (no padding of n, no pitch parameter). */
enum { F2_WAVE_I16 = 0, F2_WAVE_F64 = 1 };
/* arithmetic of the Hilbert FFT: F2_FFT_F32 (default; 3.6e-7 max-norm error) or
 * F2_FFT_F64 (reference-grade, slower). The IIR recurrences are float64 in both. */
enum { F2_FFT_F32 = 0, F2_FFT_F64 = 1 };

/* ---- library / context -------------------------------------------------------------------- */
int f2_version(void);   /* 100 * major + minor; 101 added f2_eval_batch, 102 f2_host_alloc + F2_MEM_HOST_ASYNC, 103 f2_ctx_set_option, 105 f2_spectral_guard_read + f2_cnn_get_info,
                           106 f2_cnn_forward accepts any finite input on the split path (scales from the input's range; the
                           f2_cnn_get_info keys "f16x3_ok", "f16x3_check_diff", "last_input_bound"), 107 f2_input_batch,
                           108 f2_eval_batch_strided, 109 f2_eval_noise_sweep, 110 f2_label_accuracy, 111 f2_cnn_score_windows,
                           112 f2_envelope_picture + f2_gammatonegram_batch, 113 f2_resample_batch,
                           114 f2_score_track + f2_eval_figure_batch, 115 f2_cnn_layers */
int f2_device_count(int* count);
int f2_ctx_create(int device, f2_ctx** ctx);
int f2_ctx_destroy(f2_ctx* ctx);
int f2_ctx_synchronize(f2_ctx* ctx);
/* adopt an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream */
int f2_ctx_set_stream(f2_ctx* ctx, void* hip_stream);
void* f2_ctx_get_stream(f2_ctx* ctx);
/* text of the last error on this context (ctx == NULL: last context-less error) */
const char* f2_last_error(f2_ctx* ctx);
/* Per-context tuning switches (the reference has none: its only knobs are the CLI arguments). Unknown key:
 * F2_ERR_INVALID. Keys (value -1 = decide from the batch, where stated):
 *   "spectral"       1 (default) / 0   f2_filterbank_envelope_fused serves eligible utterances with the one-kernel
 *                                      spectral path; 0 = always filterbank kernel + envelope kernel
 *   "spectral_min_rows"  rows (utterances x channels) a call needs before that path is used (default 4096: below,
 *                        the serial filter-state kernel is not hidden and the time-split filterbank kernel is faster)
 *   "spectral_tol"   accuracy guard of that path (default 4e-6): padding-region residual, relative to the maximum of the row as
 *                    delivered (the low-passed row when lpf != 0), that sends an utterance back
 *   "spectral_min_pad"  zero-padding samples (2^k - n) a row needs for that path: -1 (default) = what the slowest channel's
 *                    ringing needs to reach its peak, from the coefficient table (256 for the reference's 100 Hz .. 8 kHz
 *                    bank), so that the guard sees the error it has to judge; an explicit value >= 64 for experiments
 *   "spectral_guard_dump"  1 / 0 (default)   keep the guard's per-row values (f2_spectral_guard_read)
 *   "k1_split"       -1 / 0 / K >= 2   time-split filterbank for small batches: auto / never / K segments
 *   "k1_queue"       -1 / 0 / 1        unit queue of the filterbank for ragged batches
 *   "k1_qwaves"      0 / n             waves of the queue launch (0 = from the batch)
 *   "env_pair"       1 / 0             on-chip envelope kernel for rows of 32769..65536 samples
 *   "env_plan4"      0 / 1             four-pass transform plan for every 8193..16384-sample row
 *   "cnn_f16x3"      1 (default) / 0   (old alias "cnn_bf16x3") conv2..conv4 + dense1 of f2_cnn_* / f2_eval_* on the fp16 matrix
 *                                      cores with both operands split in two fp16 pieces, each layer's operands scaled by powers
 *                                      of two (three MFMAs per product, float32 accumulation: scores at the float32 rounding
 *                                      level, within 1e-6 of the float32 matrix path, several times its speed; the scales follow
 *                                      the input's range, see f2_cnn_forward); 0 = v_mfma_f32_32x32x2_f32 throughout
 *   "cnn_ws"         1 (default) / 0   with "cnn_f16x3", windows of 10 / 11 rows (the reference's 11 x C): persistent weight-
 *                                      stationary kernels (each wave keeps the weights of its role in registers, conv1 on the
 *                                      matrix cores too, one barrier per tile); 0 = one workgroup per tile, weights re-read
 *   "cnn_ws_dense"   1 (default) / 0   with "cnn_ws": dense1 on 96-window tiles (a weight fragment feeds nine MFMAs), its loads
 *                                      issued and waited for by hand; 0 = the 64-window kernel of "cnn_f16x3"
 *   "gather_blocked" 1 (default) / 0   every-sample normalised windows (f2_gather_windows without centres, f2_eval_*): logarithm
 *                                      once per envelope sample and blocks of 32 consecutive windows, bit-identical to 0 = one
 *                                      workgroup per window
 * Read-only (f2_ctx_get_option): "spectral_routed" = utterances of the last fused call that went through the spectral
 * kernel, "spectral_flagged" = those of them its accuracy guard handed back to the two-kernel route (waits for the
 * stream); "spectral_routed_samples" / "spectral_flagged_samples" = the same in samples.
 * Two contexts on two host threads choose independently. */
int f2_ctx_set_option(f2_ctx* ctx, const char* key, double value);
int f2_ctx_get_option(f2_ctx* ctx, const char* key, double* value);
/* Diagnostic of the spectral path's accuracy guard (no reference counterpart; used by tests/diag/guard_search.py). With
 * option "spectral_guard_dump" = 1 the last f2_filterbank_envelope_fused call that took the spectral route keeps, per
 * (utterance b, channel c) row in batch order, four floats {maximum of |analytic signal| inside the row, maximum of the
 * padding-region residual, maximum of the low-passed row (0 without low-pass), 1 if this row tripped the guard}; rows the
 * spectral kernel did not serve read as NaN. Copies min(rows, available) rows to `out` (host) and waits for the stream. */
int f2_spectral_guard_read(f2_ctx* ctx, float* out, int64_t rows, int64_t* rows_available);

/* ---- device memory + timing helpers (so a host language needs no HIP binding of its own) ---- */
int f2_dev_malloc(f2_ctx* ctx, size_t bytes, void** dptr);
int f2_dev_free(f2_ctx* ctx, void* dptr);
int f2_dev_memset(f2_ctx* ctx, void* dptr, int value, size_t bytes);
/* page-locked host memory for the staging buffers of F2_MEM_HOST / F2_MEM_HOST_ASYNC calls (the reference's
 * numpy.save / numpy.load buffers, GammatoneFiltering.py:61-62, EnvelopeExtraction.py:80,94-95) */
int f2_host_alloc(f2_ctx* ctx, size_t bytes, void** hptr);
int f2_host_free(f2_ctx* ctx, void* hptr);
int f2_memcpy_h2d(f2_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int f2_memcpy_d2h(f2_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int f2_event_create(f2_ctx* ctx, void** event);
int f2_event_destroy(f2_ctx* ctx, void* event);
int f2_event_record(f2_ctx* ctx, void* event);                 /* on the context's stream */
int f2_event_elapsed_ms(f2_ctx* ctx, void* start, void* stop, float* ms); /* waits for `stop` */
int f2_event_query(f2_ctx* ctx, void* event, int* done);       /* does not wait: *done = 1 once the stream has passed it */

/* ---- per-kernel timing (HIP events recorded around every kernel launch on the context's stream) ----
 * Kernel ids: F2_K_* below. f2_prof_get waits for the stream, returns the number of launches of that
 * kernel since the last f2_prof_enable(ctx, 1) / f2_prof_reset and their summed device time. */
enum {
    F2_K_FILTERBANK = 0,   /* k_erb_filterbank                                                       */
    F2_K_ENVELOPE = 1,     /* k_envelope and its long-row variants                                   */
    F2_K_GATHER = 2,
    F2_K_CNN = 3,
    F2_K_FUSED = 4,        /* k_spectral_envelope: filterbank + envelope of a row in ONE kernel      */
    F2_K_SPECTRUM = 5,     /* k_utterance_spectrum: float64 transform of each utterance, once        */
    F2_K_TAIL = 6,         /* k_tail_state: filter state at the end of each row                      */
    F2_K_COUNT = 7
};
int f2_prof_enable(f2_ctx* ctx, int on);
int f2_prof_reset(f2_ctx* ctx);
int f2_prof_get(f2_ctx* ctx, int kernel_id, int* launches, float* total_ms);
const char* f2_prof_kernel_name(int kernel_id);

/* ---- K1: ERB gammatone filterbank ------------------------------------------------------------
 * Replaces gammatone/filters.py:195-239 erb_filterbank (called from
 * scripts/processing/GammatoneFiltering.py:42-47 GetFilteredOutputFromArray and
 * scripts/CNN/Evaluating.py:52), batched over utterances.
 *   wave     int16 (F2_WAVE_I16) or float64 (F2_WAVE_F64) samples, ragged by `offsets`
 *   offsets  host, B+1 entries, offsets[0] == 0, non-decreasing
 *   coefs    host, (C,10) float64 rows [A0,A11,A12,A13,A14,A2,B0,B1,B2,gain] (make_erb_filters)
 *   gfb      out, float64, C*offsets[B] elements
 */
int f2_erb_filterbank_batch(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets,
                            const double* coefs, int B, int C, double* gfb, int mem_space);

/* ---- K2: Hilbert-magnitude envelope + optional 1st-order Butterworth low-pass ----------------
 * Replaces scripts/processing/EnvelopeExtraction.py:51-67 ExtractEnvelopeFromMatrix (with
 * paddedHilbert :20-36 and lowPassFilter :39-48), batched. lpf == 0: magnitude only; otherwise
 * butter(1, cutoff_hz/8000) (8000 hard-coded as in the reference) applied from zero state.
 *   gfb / env  float64, ragged (C, n_b) blocks as above (env may alias gfb)
 */
int f2_envelope_batch(f2_ctx* ctx, const double* gfb, const int64_t* offsets, int B, int C, int lpf,
                      double cutoff_hz, int fft_precision, double* env, int mem_space);

/* ---- K1+K2 without the float64 GFB round trip through HBM -------------------------------------
 * `prepare filter` + `prepare envelope` in one call (GammatoneFiltering.py:69-78 followed by
 * EnvelopeExtraction.py:101-117). gfb_or_null != NULL additionally emits the filterbank output
 * (needed when .GFB.npy files must be written). */
int f2_filterbank_envelope_fused(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets,
                                 const double* coefs, int B, int C, int lpf, double cutoff_hz,
                                 int fft_precision, double* env, double* gfb_or_null, int mem_space);

/* ---- K3: window gather (+ per-window log min-max normalisation) ------------------------------
 * Replaces the Python gathers of scripts/processing/InputGenerator.py:73-80 (centers given,
 * normalize = 0, output cast to float32 as at :83) and scripts/CNN/Evaluating.py:76-80
 * (centers == NULL: centre_i = radius*step + i for i < n_windows; normalize = 1 applies
 * scripts/CNN/Training.py:13-28 normalizeInput in float64 before the float32 cast).
 *   env      (C, N) float64 C-order
 *   out      (n_windows, 2*radius+1, C) float32
 * Returns F2_ERR_NONPOSITIVE if normalize != 0 and a window holds a value <= 0 (reference raises
 * ValueError), F2_ERR_INVALID if a window reaches outside [0, N).
 */
int f2_gather_windows(f2_ctx* ctx, const double* env, int C, int64_t N, const int64_t* centers,
                      int64_t n_windows, int radius, int step, int normalize, float* out, int mem_space);

/* ---- K1+K2+K3: training windows straight from the waves ------------------------------------------
 * Replaces scripts/processing/InputGenerator.py:73-83 (windows at the labelled timepoints, cast to float32) together
 * with the `prepare filter` + `prepare envelope` runs whose .ENV1.npy files it reads: the envelopes of the ragged batch
 * stay in device scratch memory and only the windows leave it.
 *   wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision   as for f2_filterbank_envelope_fused; the
 *                     envelopes are what that call computes for the same batch and options with gfb_or_null = NULL
 *   center_offsets    host, B+1 entries, center_offsets[0] == 0, non-decreasing: utterance b owns the centres
 *                     centers[center_offsets[b] .. center_offsets[b+1])
 *   centers           host, center_offsets[B] timepoints, each relative to the first sample of its own utterance
 *   windows           out, (center_offsets[B], 2*radius+1, C) float32; window e is what f2_gather_windows gives for
 *                     centers[e] on its utterance's (C, n_b) envelope (bit for bit), all windows in one launch
 *   normalize         as for f2_gather_windows (0: `prepare input`; 1: scripts/CNN/Training.py:13-28 normalizeInput)
 * wave and windows are in mem_space (F2_MEM_HOST or F2_MEM_DEVICE). Returns F2_ERR_INVALID if a window reaches outside
 * [0, n_b) of its utterance (the message names the utterance, the centre and n_b), F2_ERR_NONPOSITIVE if normalize != 0
 * and a window holds a value <= 0. B == 0, no centres at all, or utterances without centres (which may be shorter than
 * a window): F2_OK, nothing written for them.
 */
int f2_input_batch(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B,
                   int C, int lpf, double cutoff_hz, int fft_precision, const int64_t* center_offsets,
                   const int64_t* centers, int radius, int step, int normalize, float* windows, int mem_space);

/* ---- K4: CNN forward ---------------------------------------------------------------------------
 * Replaces keras model.predict + the label rule of scripts/CNN/Evaluating.py:85-87 for the
 * architecture built at scripts/CNN/Training.py:93-114.
 * f2_cnn_create copies 12 host tensors in Keras layouts, in this order:
 *   conv1 kernel (3,3,1,32) bias (32) | conv2 (3,3,32,32),(32) | conv3 (3,3,32,64),(64) |
 *   conv4 (3,3,64,64),(64) | dense1 (F,516),(516) | dense2 (516,2),(2),  F = flatten size for (rows, channels)
 * f2_cnn_forward: x (n, rows, channels) float32 -> scores (n,2) softmax float32 and
 * labels[i] = scores[i][1] > scores[i][0] (ties -> 0). scores or labels may be NULL.
 * Any finite input is accepted, as keras model.predict accepts it. With option "cnn_f16x3" (the default) a pass over x
 * finds max |x|; the split path then runs with the scales of the input bound B = 1 when max |x| <= 1 (the scales of every
 * normalised window: f2_eval_* use them without the pass) and B = 2^ceil(log2 max |x|) above that. An input holding inf /
 * NaN, or one whose B would need a scale outside [2^-20, 2^20], runs on the float32 kernels (option "cnn_f16x3" = 0), and
 * its scores are what those give. x in device memory: the call synchronises the stream once (to read the range back);
 * x in host memory: per chunk of 16384 windows, as before.
 */
int f2_cnn_create(f2_ctx* ctx, const float* const* tensors, int rows, int channels, f2_cnn** cnn);
int f2_cnn_destroy(f2_ctx* ctx, f2_cnn* cnn);
/* What f2_cnn_create found out about this network (no reference counterpart). Keys: "flat" (flatten size); "ws_ok" /
 * "ws_dense_ok" = 1 if the weight-stationary convolution / dense1 kernels (option "cnn_ws" / "cnn_ws_dense") serve this
 * network: its shape qualifies AND they reproduced the per-tile kernels' scores on f2_cnn_create's self-check batch (their
 * hand-placed memory waits are only valid for the register allocation of the compiler they were validated with; a library
 * built by another hipcc that fails the check falls back to the per-tile kernels and says so on stderr);
 * "ws_check_diff" / "ws_dense_check_diff" = the score differences measured (-1: not applicable);
 * "f16x3_ok" = 1 if the split-fp16 path serves this network: f2_cnn_create held it against the float32 kernels on its
 * self-check batch (inputs in [0, 1), and the same x 2^10 with the scales of B = 2^10) and it agreed to 5e-6, else 0 (the
 * network runs on the float32 kernels, said on stderr); "f16x3_check_diff" = the larger of the two score differences
 * measured (-1: no split path); "last_input_bound" = B of the last f2_cnn_forward (or f2_cnn_score_windows with normalize = 0) on
 * this network (a host call of several chunks: the largest), -1 if the float32 kernels ran, 0 before the first call. */
int f2_cnn_get_info(f2_ctx* ctx, const f2_cnn* cnn, const char* key, double* value);
int f2_cnn_forward(f2_ctx* ctx, const f2_cnn* cnn, const float* x, int64_t n, float* scores,
                   uint8_t* labels, int mem_space);

/* An inspection entry, for tests and diagnosis (no reference counterpart; nothing in the product calls it): the activations behind the
 * two scores of f2_cnn_forward, on a route the caller names. x (n, R, C) float32 in mem_space. Every output is optional (NULL), all
 * in mem_space:
 *   pooled (n, flat) float32   conv4 + ReLU + max-pool in true units, flattened in the order (pooled row, pooled column, channel) -
 *                              the row order of dense1's kernel. The split routes keep it multiplied by a power of two between
 *                              the kernels; that is undone here, exactly
 *   dense1 (n, 516) float32    dense1 + ReLU as the dense kernels of the route wrote it
 *   scores (n, 2) float32      the softmax
 * route = F2_CNN_ROUTE_CALL: the kernels and scales f2_cnn_forward takes for this x on this context (its options, its range pass);
 * the scores are f2_cnn_forward's bit for bit. The forced routes ignore the context's options: F32 the float32 kernels, TILE the
 * per-tile split-fp16 kernels (float32 conv3 / conv4 for windows whose conv2 output does not pool to four rows), WS the
 * weight-stationary convolutions with the per-tile dense1, WS_DENSE those with k_dense1_ws. A forced split route runs with the scale
 * set f2_cnn_forward would take for the measured input bound. RECORDED is the float32 forward pass that f2_cnn_input_gradient
 * records its masks from (its own convolution kernels, in chunks of at most 1024 windows), with that call's scores.
 * F2_ERR_UNSUPPORTED, with nothing written: a forced route this network or this input cannot take - f2_cnn_get_info's "f16x3_ok" /
 * "ws_ok" / "ws_dense_ok" is 0 for it, x holds inf / NaN or has no scale set (the cases in which f2_cnn_forward takes the float32
 * kernels) on a split route -, so that a forced route never runs other kernels than the ones it names; and n > 16384 (the entry does
 * not chunk). F2_ERR_INVALID, with nothing written: f2_cnn_forward's argument errors, and a route outside the enumerators. n == 0:
 * F2_OK. The call leaves "last_input_bound" alone. F2_MEM_HOST calls return with the outputs filled; F2_MEM_DEVICE calls wait for the
 * stream once where the input is measured, and enqueue the rest. */
enum { F2_CNN_ROUTE_CALL = 0, F2_CNN_ROUTE_F32 = 1, F2_CNN_ROUTE_TILE = 2, F2_CNN_ROUTE_WS = 3, F2_CNN_ROUTE_WS_DENSE = 4,
       F2_CNN_ROUTE_RECORDED = 5 };
int f2_cnn_layers(f2_ctx* ctx, const f2_cnn* cnn, const float* x /* (n, R, C), mem_space */, int64_t n, int route,
                  float* pooled_or_null /* (n, flat), mem_space */, float* dense1_or_null /* (n, 516), mem_space */,
                  float* scores_or_null /* (n, 2), mem_space */, int mem_space);

/* ---- `cnn eval` device pipeline -----------------------------------------------------------------
 * scripts/CNN/Evaluating.py:42-87 for one utterance with every intermediate kept in HBM:
 * filterbank -> envelope -> every-sample window gather + normalise -> CNN -> labels.
 * f2_eval_utterance is f2_eval_batch (below) with the one utterance offsets = {0, N}: the same kernels in the same
 * order, scores and labels bit-identical, and the same argument errors (see there). On top of it, n_windows_out
 * receives max(0, N - (2*radius+1)*step) (Evaluating.py:73), env_or_null (C,N) float64 the envelopes (in `mem_space`;
 * a device buffer serves as the call's envelope buffer itself), and a NULL wave is an error even for N = 0.
 */
int f2_eval_utterance(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, int64_t N,
                      const double* coefs, int C, int lpf, double cutoff_hz, int fft_precision,
                      int radius, int step, double* env_or_null, float* scores_or_null,
                      uint8_t* labels_or_null, int64_t* n_windows_out, int mem_space);

/* The same pipeline for a ragged batch of utterances (scripts/CNN/Evaluating.py:138-177 EvaluateRandom evaluates a
 * list of files with one model): filterbank and envelope run once for the whole batch - a single utterance only
 * fills two wavefronts of the filterbank kernel - then windows + CNN utterance by utterance. Utterance b has
 * nb_b = max(0, n_b - (2*radius+1)*step) windows; scores / labels are the concatenation over b in batch order
 * (sum nb_b rows), both optional, in `mem_space`.
 * F2_ERR_INVALID (nothing is launched): NULL ctx, cnn, coefs or offsets; mem_space other than F2_MEM_HOST / F2_MEM_DEVICE;
 * wave_dtype or fft_precision not one of the enumerators; lpf with cutoff_hz outside (0, 8000); B < 0, C <= 0, radius < 0,
 * step < 0; offsets[0] != 0 or decreasing offsets; a network on another device or built for other than (2*radius+1) x C
 * windows; a NULL wave with offsets[B] > 0. F2_ERR_NONPOSITIVE: a window holds a value <= 0 (normalizeInput).
 */
int f2_eval_batch(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                  const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius,
                  int step, float* scores_or_null, uint8_t* labels_or_null, int mem_space);

/* f2_eval_batch with a decision every `hop` samples instead of every sample (the reference's loop, Evaluating.py:71-87, takes
 * every sample; the labelled quantity, a slope over 11 frames 10 ms apart, does not change at that rate). Utterance b with
 * nb_b = max(0, n_b - (2*radius+1)*step) every-sample windows gets nbh_b = ceil(nb_b / hop) windows; window j of this call IS
 * window j*hop of f2_eval_batch - centre sample radius*step + j*hop, the same envelope (the two-kernel route), the same window
 * arithmetic, the same network: scores and labels are bit-identical to those rows, and hop = 1 reproduces f2_eval_batch.
 * scores (sum nbh_b, 2) / labels (sum nbh_b) are the concatenation over b in `mem_space`, both optional;
 * window_offsets_or_null, always a HOST array of B+1 like `offsets`, receives the prefix sums of nbh_b (also when the call then
 * has nothing to launch).
 * The window stage and the convolutions work on chunks of up to 16 384 windows taken across utterance boundaries, so the
 * number of kernel launches follows the number of windows, not B. When hop divides step the windows are the every-sample
 * windows of the decimated envelope env[c][j*hop]: one logarithm per sample that an evaluated window uses, for all utterances
 * of a chunk in three launches; any other hop takes one workgroup per window (f2_input_batch's kernel, normalising).
 * Errors: those of f2_eval_batch, checked the same way, plus hop < 1 -> F2_ERR_INVALID (nothing is launched).
 * F2_ERR_NONPOSITIVE is raised only by windows that are evaluated: a sample <= 0 that no evaluated window reads does not fail
 * the call (the reference raises from normalizeInput of a window, not from the envelope).
 */
int f2_eval_batch_strided(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                          const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius,
                          int step, int hop, float* scores_or_null, uint8_t* labels_or_null,
                          int64_t* window_offsets_or_null /* host, B+1 */, int mem_space);

/* ---- `cnn noisesweep`: one ragged batch at K noise levels and clean, in one device pass -----------------------------------
 * scripts/CNN/Evaluating.py:193-221 (EvaluateWithNoise) adds Gaussian noise to one file at one SNR with NumPy on the host and
 * evaluates the float64 result. This call forms K+1 "levels" of the clean batch on the device - level k < K is every utterance
 * plus its own noise at snr_db[k], level K the clean batch converted to float64 (exact for int16) - evaluates them as ONE
 * (K+1)*B-utterance float64 batch and counts, on the device, how the labels of every level compare with the clean level's.
 * Only the clean samples are uploaded. Level l, utterance b is utterance u = l*B + b of that batch; its offsets are the clean
 * offsets tiled: tiled[u] = l*offsets[B] + offsets[b].
 *   sigma   sigma[u] = RMS(clean_b) / 10^(snr_db[l] / 10): the reference's scaling (Evaluating.py:199), a power ratio where an
 *           amplitude ratio belongs, reproduced and not corrected. 0 for level K and for an empty utterance. F2_WAVE_I16: the
 *           squares are summed in int64 (exact), RMS = sqrt((double)sum / n) - the bits of numpy.sqrt(numpy.mean(numpy.square(
 *           float64 samples))). F2_WAVE_F64: a float64 sum in a fixed order (no floating-point atomics): the same bits on every
 *           call. 10^(snr_db / 10) is the host's pow().
 *   noise   sample i (counted from the utterance's first sample) of utterance u becomes clean + sigma[u] * z (product and sum
 *           rounded separately) with z = sqrt(-2 ln u1) * cos(2 pi u2),
 *             (w0, w1, w2, w3) = Philox4x32-10(counter = (i & 0xffffffff, i >> 32, l, b), key = (seed & 0xffffffff, seed >> 32))
 *             u1 = ((w0 >> 5) * 2^26 + (w1 >> 6) + 1) * 2^-53   in (0, 1]
 *             u2 = ((w2 >> 5) * 2^26 + (w3 >> 6)) * 2^-53       in [0, 1)
 *           Philox with the standard constants (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85);
 *           everything after the 32-bit words in float64; 2 pi = 6.283185307179586. One Philox call serves one sample and the
 *           sine twin is discarded, so a sample depends on (seed, level, utterance, i) alone - not on the launch shape, the
 *           batch around it or the machine (up to the device's log / sqrt / cos, a few ulp). A level whose sigma is 0 is the
 *           clean samples exactly.
 *   noisy_or_null   (K+1) * offsets[B] float64, level-major, in mem_space: the waveforms that were evaluated (a device buffer
 *                   serves as the call's own buffer; otherwise they live in context scratch)
 *   scores_or_null, labels_or_null, window_offsets_or_null (host, (K+1)*B + 1)
 *           bit for bit what f2_eval_batch_strided(F2_WAVE_F64) returns for the (K+1)*B batch `noisy` with the tiled offsets
 *           and the same coefs ... hop: it is that call's code on that buffer. window_offsets is filled whenever the arguments
 *           pass.
 *   sigma_or_null   host, (K+1)*B
 *   stats_or_null   host, (K+1)*B*2: stats[2u] = windows of u labelled rising, stats[2u+1] = windows of u whose label equals
 *           the clean level's label for the same window of the same utterance (for level K: its window count). Counted by a
 *           kernel over the device's label array (workgroup sums, then vector integer atomics on a zeroed buffer), also when
 *           labels_or_null is NULL.
 * Errors: everything f2_eval_batch_strided rejects, by the same checks and before anything is launched or written; K < 1, a
 * NULL snr_db or a non-finite snr_db[k]: F2_ERR_INVALID. F2_ERR_NONPOSITIVE as in the strided call (only evaluated windows).
 * B == 0, or no utterance long enough for a window: F2_OK with window_offsets / sigma / stats filled. The call waits for the
 * stream before it returns (it hands back sigma, stats and the error flag), whatever mem_space is.
 */
int f2_eval_noise_sweep(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                        const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius,
                        int step, int hop, const double* snr_db /* host, K */, int K, uint64_t seed,
                        double* noisy_or_null, float* scores_or_null, uint8_t* labels_or_null,
                        int64_t* window_offsets_or_null /* host, (K+1)*B + 1 */, double* sigma_or_null /* host, (K+1)*B */,
                        int64_t* stats_or_null /* host, (K+1)*B*2 */, int mem_space);

/* ---- `cnn eval|evalnoise|evalrand|noisesweep --accuracy`: the labels of an evaluation against the VTR-derived labels --------
 * scripts/CNN/Evaluating.py:38-40, 92-108 (the end of EvaluateOneWavArray) holds every decision of a file against the labels
 * LabelDataGenerator.ExtractLabel derives from the file's .FB / .PHN, in a double loop of interpreted Python over decisions and
 * label pairs. Here: one kernel over the label array of a strided evaluation, for a whole batch.
 *   labels          (window_offsets[U]) uint8 in mem_space, 0 = falling, anything else = rising: utterance u owns rows
 *                   window_offsets[u] .. window_offsets[u+1] - 1 (what f2_eval_batch_strided / f2_eval_noise_sweep return)
 *   ref_offsets, ref_timepoints, ref_signs   R reference sets, set r being entries ref_offsets[r] .. ref_offsets[r+1] - 1:
 *                   the label timepoints T[0..n) of a file in samples, strictly increasing, and their signs s[0..n), 0 falling,
 *                   1 rising. Utterance u is scored against set u % R (a sweep passes U = (K+1)*B and R = B).
 *   The rule. Row j of an utterance has the timepoint t = origin + j*hop (int64).
 *     - the row is COUNTED if there is a k with T[k] < t < T[k+1] and (t - T[k] < step or T[k+1] - t < step);
 *     - its reference sign is s[k] if t - T[k] <= T[k+1] - t, else s[k+1] (a tie goes to the earlier label); the row is correct
 *       if its label equals that sign;
 *     - never counted: a row with t equal to a label timepoint, a row before the first label or after the last, every row of
 *       an utterance whose set has fewer than two labels.
 *   origin          0 reproduces the reference, which compares the ROW INDEX with the label timepoint (Evaluating.py:96
 *                   enumerates the decisions; its own TODO) although row j is centred on sample radius*step + j - reproduced,
 *                   not corrected, like the noise scaling of f2_eval_noise_sweep. origin = radius*step gives every row its
 *                   true centre sample (f2_eval_batch_strided: radius*step + j*hop).
 *   counts          host, U*4: counts[4u + 2*ref + pred] = counted rows of utterance u with reference sign `ref` and label
 *                   `pred`. Accuracy = (counts[4u] + counts[4u+3]) / (sum of the four); the reference divides by zero when
 *                   nothing is counted. Workgroup sums, then 64-bit vector integer atomics on a zeroed buffer: the same bits
 *                   on every call.
 * The small arrays are uploaded through the context's page-locked staging; the call waits for the stream before it returns
 * (it hands back counts), whatever mem_space is.
 * F2_ERR_INVALID, with nothing launched and counts untouched: a NULL ctx / window_offsets / ref_offsets / counts; NULL labels
 * with window_offsets[U] > 0; NULL ref_timepoints or ref_signs with ref_offsets[R] > 0; U < 0; R < 1 or U % R != 0 when U > 0
 * (R < 0 always); hop < 1, step < 1 or origin < 0; offsets that do not start at 0 or decrease; timepoints not strictly increasing
 * inside a set; a sign above 1; a mem_space other than F2_MEM_HOST / F2_MEM_DEVICE. F2_ERR_UNSUPPORTED: the timepoint of an
 * utterance's last row does not fit int64. U == 0, or no rows at all: F2_OK with counts zeroed.
 */
int f2_label_accuracy(f2_ctx* ctx, const uint8_t* labels /* mem_space */,
                      const int64_t* window_offsets /* host, U+1 */, int U,
                      const int64_t* ref_offsets /* host, R+1 */, const int64_t* ref_timepoints /* host */,
                      const uint8_t* ref_signs /* host */, int R,
                      int64_t origin, int hop, int step,
                      int64_t* counts /* host, U*4: counts[4u + 2*ref + pred] */, int mem_space);

/* ---- `cnn test`: a model scored on stored, labelled windows in one device pass ---------------------------------------------
 * scripts/CNN/Training.py:136 (model.evaluate(x_test, y_test), and validation_data in every epoch) answers "how good is this
 * model on the labelled windows" - the rows of input_data.npy (`prepare input`) with the signs of label_data.csv (`prepare
 * label`) - after normalising every window on the host (:71-75). Here: the stored float32 windows go up once, are normalised on
 * the device, run through the forward chain of f2_cnn_forward and are tallied by a kernel, broken down by a caller-given group.
 *   windows   (n, rows, C) float32 in mem_space, rows x C being the window shape of `cnn`
 *   normalize 1: raw envelope windows. Each is normalised with the arithmetic of f2_gather_windows (normalize = 1): values
 *             widened to float64, min / max over the window, (ln v - ln min) / (ln max - ln min) in float64, rounded once to
 *             float32; an all-equal window gives zeros; a value <= 0 or a NaN anywhere: F2_ERR_NONPOSITIVE. Bit for bit what
 *             f2_gather_windows returns for the same window held in an envelope (the convention this package trains under: not
 *             the reference's float32 logarithms of Training.py:71-75). The network then runs with the scales of the input bound
 *             B = 1, without the range pass, as in f2_eval_*.
 *             0: the windows go to the network as they are, by f2_cnn_forward's route (range pass, scale set or float32 kernels;
 *             the range is that of the whole call for device memory and of each chunk of 16384 windows for host memory, as there).
 *             Like f2_cnn_forward it then sets "last_input_bound" of f2_cnn_get_info; a call with normalize = 1 measures no
 *             range and leaves that value as it was.
 *   scores_or_null (n, 2), labels_or_null (n), in mem_space: bit for bit what f2_cnn_forward returns for the same (normalised)
 *             windows in the same mem_space; without them the scores and labels of a chunk live in context scratch.
 *   signs     n uint8 in mem_space: 0 falling, 1 rising (the last column of label_data.csv)
 *   groups_or_null  n int32 in mem_space, the group of every window, in [0, G); NULL requires G == 1: everything is group 0
 *   counts    host, G*4: counts[4g + 2*sign + pred] = windows of group g with that sign and label. Workgroup counts in LDS, then
 *             64-bit vector integer atomics on a zeroed buffer: the same bits on every call. Accuracy of a group =
 *             (counts[4g] + counts[4g+3]) / (sum of the four).
 *   loss_sum  host, G: sum over the group's windows of -ln(min(max((double)scores[i][signs[i]], 1e-7), 1.0)) in float64, the
 *             categorical cross-entropy as Keras clips it. Mean loss = loss_sum[g] / windows of g, formed by the caller. No
 *             floating-point atomics: a workgroup of 256 windows adds the terms of each group in window order, the workgroups'
 *             partial sums are added in workgroup order, chunk after chunk - the same bits on every call and in both memory
 *             spaces (up to the device's logarithm, a few ulp, against another machine's).
 * The call works in chunks of 16384 windows (host memory: one chunk staged at a time) and waits for the stream before it returns
 * (it hands back counts, loss_sum and the error flags), whatever mem_space is.
 * F2_ERR_INVALID, with nothing launched and counts / loss_sum untouched: NULL ctx, cnn, counts or loss_sum; NULL windows or signs
 * with n > 0; n < 0; G < 1; NULL groups with G != 1; normalize other than 0 / 1; a network on another device; a mem_space other
 * than F2_MEM_HOST / F2_MEM_DEVICE. F2_ERR_UNSUPPORTED, likewise: G > 1024. Found by the kernels, so after the pass and with
 * counts / loss_sum unspecified: a sign above 1 or a group outside [0, G) -> F2_ERR_INVALID (the message names the sign if both
 * occurred); F2_ERR_NONPOSITIVE as above. n == 0: F2_OK with counts and loss_sum zeroed.
 */
int f2_cnn_score_windows(f2_ctx* ctx, const f2_cnn* cnn,
                         const float* windows /* (n, rows, C) float32, mem_space */, int64_t n, int normalize,
                         const uint8_t* signs /* n, mem_space: 0 falling, 1 rising */,
                         const int32_t* groups_or_null /* n, mem_space: group of every window, in [0, G) */, int G,
                         float* scores_or_null /* (n, 2), mem_space */, uint8_t* labels_or_null /* n, mem_space */,
                         int64_t* counts /* host, G*4: counts[4g + 2*sign + pred] */,
                         double* loss_sum /* host, G */, int mem_space);

/* ---- `plot gtg`: gammatonegram pictures of a ragged batch, reduced on the device ---------------------------------------------
 * scripts/plotting/PlottingProcessing.py:81-133 (PlotEnvelopesAndFormantsFromFile) runs filterbank and envelope on the CPU,
 * replicates every channel row by its ERB ratio (:27-60) and hands a 941 x n float64 image to imshow(norm=LogNorm()). Here the
 * envelopes are pooled over time columns and normalised on the device: a picture is C x width values, whatever n is. Row
 * replication, colours and formant tracks are display work on C x width bytes and stay with the caller.
 *   The picture of utterance b. Its envelope is the (C, n_b) block of the ragged batch; its span is [s_b, e_b) =
 *   spans[2b], spans[2b+1] with 0 <= s_b <= e_b <= n_b (spans_or_null == NULL: [0, n_b)); m = e_b - s_b, W = width. Column x in
 *   [0, W) covers the samples [lo_x, hi_x), lo_x = s_b + floor(x*m / W), hi_x = s_b + floor((x+1)*m / W), and hi_x = lo_x + 1
 *   where that bin would be empty (m < W: the nearest sample is repeated). m == 0: every pixel of the utterance is 0.0 / level 0
 *   and its range is (0, 0).
 *   pooled  (B, C, W) float64: pool = 0 the mean of the bin (a float64 sum divided by the count), pool = 1 its maximum. A NaN
 *           sample makes the pixel NaN in both modes. The sum has a fixed order (each lane of a wave adds its own samples of the
 *           bin in index order, then a fixed shuffle tree) and uses no floating-point atomics: the same bits on every call and
 *           in both memory spaces. Consecutive lanes read consecutive samples of a row for every bin size; rows may start at
 *           any 8-byte alignment.
 *   range   host, 2B: vmin_b = smallest pixel > 0 of picture b, vmax_b = largest (wave and workgroup minima / maxima, then
 *           64-bit vector integer atomics on the bit patterns, which order as positive doubles do). Pixels <= 0 and NaN do not
 *           enter; a picture without a positive pixel has the range (0, 0).
 *   levels  (B, C, W) uint8: matplotlib's LogNorm() autoscaled over the picture. A pixel v > 0 gets the level
 *           1 + (int)(254*t + 0.5), t = (ln v - ln vmin) / (ln vmax - ln vmin) in float64 (t = 0 when vmax == vmin); a pixel <= 0
 *           or NaN gets level 0 (LogNorm masks it; a masked pixel is drawn as background).
 * f2_envelope_picture is PlotEnvelopeSpectrogram's data side (:45-78) for envelopes that already exist; env, pooled and levels
 * are in mem_space (host envelopes are staged like the input of f2_envelope_batch). f2_gammatonegram_batch is
 * PlotEnvelopesAndFormantsFromFile's data side (:97-106): the envelopes are what f2_filterbank_envelope_fused computes for the
 * same batch and options with gfb_or_null = NULL; they stay in device scratch memory as in f2_input_batch, and the code of
 * f2_envelope_picture runs on that buffer - for host memory only the wave goes up and only pooled / levels come down.
 * All three outputs are optional. Both calls wait for the stream before they return (they hand back the range), whatever
 * mem_space is.
 * F2_ERR_INVALID, with nothing launched and nothing written: a NULL ctx or NULL offsets; NULL env / wave / coefs with
 * offsets[B] > 0; a mem_space other than F2_MEM_HOST / F2_MEM_DEVICE; B < 0, C <= 0, width < 1, pool not 0 / 1; offsets that do
 * not start at 0 or that decrease; a span with s_b < 0, e_b < s_b or e_b > n_b (the message names the utterance); for the wave
 * call, a wave_dtype or fft_precision that is not an enumerator and lpf with cutoff_hz outside (0, 8000).
 * F2_ERR_UNSUPPORTED, likewise: width > 65536. B == 0: F2_OK.
 */
int f2_envelope_picture(f2_ctx* ctx, const double* env /* ragged (C, n_b) blocks, mem_space */,
                        const int64_t* offsets /* host, B+1 */, int B, int C,
                        const int64_t* spans_or_null /* host, 2B: s_b, e_b */, int width, int pool,
                        double* pooled_or_null /* (B, C, width), mem_space */,
                        uint8_t* levels_or_null /* (B, C, width), mem_space */,
                        double* range_or_null /* host, 2B: vmin, vmax */, int mem_space);
int f2_gammatonegram_batch(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs,
                           int B, int C, int lpf, double cutoff_hz, int fft_precision,
                           const int64_t* spans_or_null, int width, int pool, double* pooled_or_null,
                           uint8_t* levels_or_null, double* range_or_null, int mem_space);

/* ---- `cnn eval|evalnoise|evalrand|noisesweep --resample`: recordings of any rate and PCM format brought to the model's rate --
 * The reference evaluates whatever scipy.io.wavfile.read returns at the file's own rate (scripts/CNN/Evaluating.py:116-135 hands
 * it to the filterbank designed for that rate); a network trained at 16 kHz then sees another filterbank and another frame step.
 * This call turns a ragged batch of interleaved PCM frames into mono float64 samples in int16 units at up/down times the rate:
 * scipy.signal.resample_poly with zero padding, for the whole batch in one launch.
 *   audio     interleaved frames (offsets[B], channels) of pcm_format, in mem_space; utterance b owns the frames offsets[b] ..
 *             offsets[b+1] - 1 (offsets count FRAMES). Natural alignment of the element type is all that is needed: int16 data
 *             may start at any even byte, uint8 data at any byte.
 *   step 1    every element becomes a float64 in int16 units, exactly (all scalings are powers of two):
 *               F2_PCM_U8 (v - 128) * 256 | F2_PCM_I16 v | F2_PCM_I32 v / 65536 (also 24-bit files read left-justified into
 *               int32) | F2_PCM_F32, F2_PCM_F64 v * 32768
 *             channel >= 0 picks that channel of every frame; channel == -1 is the mean (((c0 + c1) + c2) + ...) / channels, added
 *             in float64 in channel order.
 *   step 2    x = the mono signal of utterance b, n = its frames, n_out = ceil(n * up / down):
 *               y[k] = sum over i of x[i] * taps[k*down + half_len - i*up],  0 <= i < n, 0 <= k*down + half_len - i*up <= 2*half_len,
 *             the terms added in ascending i, for 0 <= k < n_out. With taps = firwin(2*half_len + 1, 1 / max(up, down),
 *             window=('kaiser', 5.0)) * up and half_len = 10 * max(up, down) this is resample_poly(x, up, down) - bit for bit
 *             when product and sum are rounded separately; the device may fuse them, which stays inside the rounding bound of a
 *             dot product of ceil((2*half_len + 1) / up) terms. The order of the sum is fixed (one lane per output sample, no
 *             atomics): the same bits on every call and in both memory spaces.
 *             up == down == 1: step 1 only - out is the converted input bit for bit, taps may be NULL and is not read.
 *   out       float64, out_offsets[B] samples in mem_space, utterance b at out + out_offsets[b]
 *   out_offsets  host, B+1: the running sums of n_out, written whenever the arguments pass
 * F2_MEM_DEVICE: the call enqueues on the context's stream and returns (out_offsets is computed on the host); F2_MEM_HOST: it
 * returns when `out` is filled. The polyphase table of (up, down, half_len, taps) stays in the context for the next call.
 * F2_ERR_INVALID, with nothing launched or written: a NULL ctx, offsets or out_offsets; NULL audio with offsets[B] > 0; NULL out
 * with out_offsets[B] > 0; NULL taps unless up == down == 1; B < 0; channels < 1; channel outside [-1, channels); an unknown
 * pcm_format; up < 1, down < 1 or half_len < 0; up and down not coprime; offsets that do not start at 0 or that decrease; a
 * mem_space other than F2_MEM_HOST / F2_MEM_DEVICE.
 * F2_ERR_UNSUPPORTED, likewise (the message names the limit): a workgroup of 256 outputs needs more than 4096 input frames
 * (floor((up - 1 + 255*down) / up) + ceil((2*half_len + 1) / up): every ratio with max(up, down) <= 1024, 1/8 <= down/up <= 8 and
 * half_len = 10 * max(up, down) fits), up or down above 2^22, a polyphase table above 2^22 values, an utterance of 2^40 frames or
 * more. B == 0 or only empty utterances: F2_OK.
 */
enum { F2_PCM_U8 = 0, F2_PCM_I16 = 1, F2_PCM_I32 = 2, F2_PCM_F32 = 3, F2_PCM_F64 = 4 };
int f2_resample_batch(f2_ctx* ctx, const void* audio /* (offsets[B], channels) interleaved, mem_space */, int pcm_format,
                      int channels, int channel /* -1: mean */, const int64_t* offsets /* host, B+1, in FRAMES */, int B,
                      int64_t up, int64_t down, const double* taps /* host, 2*half_len+1 */, int64_t half_len,
                      double* out /* mem_space */, int64_t* out_offsets /* host, B+1, written by the call */, int mem_space);

/* ---- `cnn eval|evalnoise|evalrand --figure`: the decisions of an evaluation over its gammatonegram, one device pass ------------
 * scripts/plotting/PlottingCNN.py (called from EvaluateOneWavArray, scripts/CNN/Evaluating.py:109-113) draws the gammatonegram with
 * a rising / falling tick per decision and, below it, the network's probability of "rising" over time - from every score, on the
 * host, after a second filterbank + envelope pass for the picture. Here the scores are reduced on the device to the time columns
 * of the picture, and one call makes the picture from the envelopes the evaluation uses.
 *
 * f2_score_track: scores (window_offsets[U], 2) float32 and labels (window_offsets[U]) uint8 in mem_space, as
 * f2_eval_batch_strided returns them. Utterance u owns rows j = 0 .. n_u - 1, n_u = window_offsets[u+1] - window_offsets[u]; row j
 * stands at sample t_j = origin + j*hop. Its span is [s_u, e_u) = spans[2u], spans[2u+1] (required), m = e_u - s_u, W = width;
 * the columns are those of f2_envelope_picture: lo_x = s_u + floor(x*m / W), hi_x = s_u + floor((x+1)*m / W), and hi_x = lo_x + 1
 * where that bin is empty. Column x owns the rows with lo_x <= t_j < hi_x, a contiguous range of j (for m < W neighbouring columns
 * repeat a sample and each of them owns its rows); m == 0: no column owns a row.
 *   track   (U, W, 5) float64 in mem_space, track[u][x] =
 *             [0] rows    the count of owned rows, exact
 *             [1] rising  the count of owned rows with labels[j] != 0, exact
 *             [2] mean    the float64 sum of (double)scores[j][1] over the owned rows, divided by rows
 *             [3] min     the smallest scores[j][1] of the owned rows, the float32 value widened
 *             [4] max     the largest
 *           A column without rows is {0, 0, NaN, NaN, NaN}; a NaN score makes mean, min and max of its column NaN.
 *           The sum has a fixed order (2^lg lanes per column, lg from the most rows a column of the utterance can own, at most 64
 *           lanes; each lane adds its own rows in index order, then a fixed shuffle tree) and uses no floating-point atomics: the
 *           same bits on every call and in both memory spaces. A column may own any number of rows (width 1 over a long file).
 * F2_MEM_DEVICE: the call enqueues on the context's stream and returns; F2_MEM_HOST: it returns when track is filled.
 * F2_ERR_INVALID, with nothing launched and track untouched: a NULL ctx, window_offsets or spans; NULL scores or labels with
 * window_offsets[U] > 0; NULL track with U > 0; U < 0, hop < 1, origin < 0 or width < 1; window offsets that do not start at 0 or
 * that decrease; a span with s < 0 or e < s; a mem_space other than F2_MEM_HOST / F2_MEM_DEVICE. F2_ERR_UNSUPPORTED, likewise:
 * width > 65536; an utterance whose last row's t_j does not fit int64. U == 0: F2_OK.
 *
 * f2_eval_figure_batch: filterbank, envelope, picture, strided evaluation and track of a ragged batch in one pass. The envelopes
 * are computed once and never leave the device. Every output is optional and defined by the calls above, bit for bit:
 *   scores, labels, window_offsets   what f2_eval_batch_strided returns for the same wave ... hop and mem_space
 *   levels (B, C, W), range (host, 2B)   what f2_envelope_picture returns (spans, width, pool as there) for the envelopes the
 *           evaluation uses: those of the two-kernel route, i.e. what f2_eval_utterance hands out in env_or_null for each
 *           utterance, laid out as the ragged batch. They are NOT the envelopes f2_gammatonegram_batch may take from the spectral
 *           route (equal to a few ulp only), so a `plot gtg` picture of the same file may differ from this one in a level here
 *           and there.
 *   track (B, W, 5)   what f2_score_track returns for those scores, labels and window_offsets, the same spans (NULL: [0, n_b)),
 *           origin = radius*step, hop and width. An utterance too short for a window still gets its picture; its track is all
 *           empty columns.
 * hop == 1 evaluates every sample: scores and labels are then those of f2_eval_batch.
 * Errors: everything f2_eval_batch_strided rejects and everything f2_envelope_picture rejects (width, pool, spans), by the same
 * checks and before anything is launched or written. F2_ERR_NONPOSITIVE as in the strided call. B == 0: F2_OK. The call waits for
 * the stream before it returns (it hands back the range and the error flag), whatever mem_space is.
 */
int f2_score_track(f2_ctx* ctx, const float* scores /* (window_offsets[U], 2), mem_space */,
                   const uint8_t* labels /* (window_offsets[U]), mem_space */,
                   const int64_t* window_offsets /* host, U+1 */, int U,
                   const int64_t* spans /* host, 2U: s_u, e_u in samples, required */,
                   int64_t origin, int hop, int width,
                   double* track /* (U, width, 5), mem_space */, int mem_space);
int f2_eval_figure_batch(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                         const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision,
                         int radius, int step, int hop,
                         const int64_t* spans_or_null /* host, 2B */, int width, int pool,
                         uint8_t* levels_or_null /* (B, C, width), mem_space */, double* range_or_null /* host, 2B */,
                         double* track_or_null /* (B, width, 5), mem_space */,
                         float* scores_or_null, uint8_t* labels_or_null, int64_t* window_offsets_or_null /* host, B+1 */,
                         int mem_space);

/* ---- `cnn eval|evalnoise|evalrand --occlusion`: which channel bands the decisions rest on, one device pass ----------------------
 * An occlusion map: blank a band of channels in the network's input, run the network again, record how far P(rising) moves and how
 * often the label flips. The windows are expanded, evaluated and reduced on the device; no window crosses the link.
 * (f2_version stays 114 with these three entries: look the symbols up to find out whether a build has them.)
 *
 * f2_occlude_windows: x (n, R, C) float32 -> out (n, K+1, R, C) float32, both in mem_space, window-major. Level 0 of a window is
 * the window; level k+1 is the window with patch k, the half-open rectangle [r0, r1) x [c0, c1) = patches[4k .. 4k+3] (host,
 * int32), replaced by `fill`. Every element moves as its bit pattern: a NaN payload in x or in fill survives. K == 0: out is a copy
 * of x. Patches may repeat and overlap (each level holds one patch). Device pointers need element alignment only. F2_MEM_DEVICE:
 * the call enqueues and returns; F2_MEM_HOST: it works through device scratch in chunks of at most 16384 output windows and
 * returns when out is filled.
 * F2_ERR_INVALID, with nothing launched and out untouched: a NULL ctx; NULL x or out with n > 0; NULL patches with K > 0; n, R, C
 * or K negative; a patch with r0 < 0, r1 > R or r0 >= r1, or the same on columns; a mem_space other than F2_MEM_HOST /
 * F2_MEM_DEVICE. F2_ERR_UNSUPPORTED, likewise: K > 1024; n*(K+1) >= 2^31; R*C >= 2^31.
 *
 * f2_occlusion_map: scores (window_offsets[U], K+1, 2) float32 and labels (window_offsets[U], K+1) uint8 in mem_space, the
 * network's outputs for such windows. Rows, spans and columns are those of f2_score_track (same origin, hop, spans, width rule).
 * With d_j = (double)scores[j][k+1][1] - (double)scores[j][0][1]:
 *   map   (U, K, W, 4) float64 in mem_space, map[u][k][x] =
 *           [0] rows      the count of owned rows, exact
 *           [1] flips     the count of owned rows with (labels[j][k+1] != 0) != (labels[j][0] != 0), exact
 *           [2] mean d    the float64 sum of d_j over the owned rows, divided by rows
 *           [3] mean |d|  the float64 sum of |d_j|, divided by rows
 *         A column without rows is {0, 0, NaN, NaN}; a NaN score makes [2] and [3] of its column and patch NaN. The sums have
 *         f2_score_track's fixed order: the same bits on every call and in both memory spaces.
 * Argument errors: those of f2_score_track, and K < 1 (F2_ERR_INVALID), K > 1024 (F2_ERR_UNSUPPORTED). U == 0: F2_OK.
 *
 * f2_eval_occlusion_batch: f2_eval_figure_batch with every window evaluated at K+1 occlusion levels, and the map in the track's
 * place. Every output is optional and defined by calls that exist, bit for bit:
 *   scores (n, K+1, 2), labels (n, K+1), window_offsets   [:, 0] is what f2_eval_batch_strided returns for the same arguments;
 *           [w][k+1] is what f2_cnn_forward returns for level k+1 of f2_occlude_windows applied to normalised window w - the one
 *           f2_input_batch (normalize = 1) gives at centre radius*step + j*hop. The input stays in [0, 1] for 0 <= fill <= 1, so
 *           the scale set is the one every eval call uses.
 *   levels (B, C, W), range (host, 2B)   what f2_eval_figure_batch returns
 *   map (B, K, W, 4)   f2_occlusion_map of those scores and labels, origin = radius*step, the same hop, spans (NULL: [0, n_b)), width
 *   summary (B, K, 4)  f2_occlusion_map with spans [0, n_b) and width 1: every row of the utterance
 * Errors, before anything is launched or written: everything f2_eval_figure_batch rejects; everything f2_occlude_windows rejects
 * for R = 2*radius+1 and C, and K < 1; fill outside [0, 1] or NaN (F2_ERR_INVALID); total windows * (K+1) >= 2^31
 * (F2_ERR_UNSUPPORTED). F2_ERR_NONPOSITIVE as in the strided call. B == 0: F2_OK. The call waits for the stream before it returns.
 */
int f2_occlude_windows(f2_ctx* ctx, const float* x /* (n, R, C), mem_space */, int64_t n, int R, int C,
                       const int32_t* patches /* host, (K, 4): r0 r1 c0 c1 */, int K, float fill,
                       float* out /* (n, K+1, R, C), mem_space */, int mem_space);
int f2_occlusion_map(f2_ctx* ctx, const float* scores /* (window_offsets[U], K+1, 2), mem_space */,
                     const uint8_t* labels /* (window_offsets[U], K+1), mem_space */,
                     const int64_t* window_offsets /* host, U+1 */, int U, int K,
                     const int64_t* spans /* host, 2U, required */, int64_t origin, int hop, int width,
                     double* map /* (U, K, width, 4), mem_space */, int mem_space);
int f2_eval_occlusion_batch(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                            const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision,
                            int radius, int step, int hop,
                            const int32_t* patches /* host, (K, 4) */, int K, float fill,
                            const int64_t* spans_or_null /* host, 2B */, int width, int pool,
                            uint8_t* levels_or_null /* (B, C, width), mem_space */, double* range_or_null /* host, 2B */,
                            double* map_or_null /* (B, K, width, 4), mem_space */, double* summary_or_null /* (B, K, 4), mem_space */,
                            float* scores_or_null /* (n, K+1, 2) */, uint8_t* labels_or_null /* (n, K+1) */,
                            int64_t* window_offsets_or_null /* host, B+1 */, int mem_space);

/* ---- `cnn eval|evalnoise|evalrand --saliency`: the input gradient of the decisions, one backward pass on the device -----------
 * The complement of the occlusion map: G = dP(rising)/dx for every cell of every normalised window comes from one backward-data
 * pass through the network (f2_cnn.hip's head comment), at a cost that does not depend on the resolution asked for. sum G x over a
 * band of channels is the first-order prediction of what the occlusion map measures for that band with fill 0, sign reversed.
 * (f2_version stays 114 with these three entries: look the symbols up to find out whether a build has them.)
 *
 * f2_cnn_input_gradient: x (n, R, C) float32 in mem_space, R = rows and C = channels of the f2_cnn. With P = softmax(z)[1]:
 *   grad    (n, R, C) float32   G[w][r][c] = dP_w/dx[w][r][c] = P (1 - P) d(z1 - z0)/dx
 *   profile (n, C, 2) float64   [w][c][0] = sum over r (ascending) of (double)G[w][r][c] * (double)x[w][r][c]
 *                               [w][c][1] = sum over r of |(double)G[w][r][c]|
 *   scores  (n, 2) float32      the scores of the recorded forward
 * Every output is optional (NULL), all in mem_space. All arithmetic is float32 with float32 accumulation. The masks come from the
 * "recorded forward", a pass of the float32 kernels' arithmetic (fmaf chains; not the split-fp16 route), so its scores are not
 * promised bit-equal to f2_cnn_forward's: they lie within the 2e-5 of the oracle that f2_cnn_forward's lie within.
 *   ReLU       passes gradient where its pre-activation is > 0; at exactly 0 the gradient is 0
 *   max-pool   sends the gradient to the maximal element of its 2 x 2 block, among equal elements to the first in (row, column)
 *              order; rows and columns of conv2's and conv4's output that the pool drops (odd height or width) get gradient 0
 * Behaviour is defined for finite x: a window with a non-finite value may get any G and any scores, without a fault and without
 * changing another window's bits. Sums have a fixed order and there are no floating-point atomics: the same bits on every call, in
 * both memory spaces and wherever a window stands in the batch. The chain works in chunks of at most 1024 windows whose
 * activations and gradients stay within 1 GiB of context scratch whatever n is; F2_MEM_HOST calls stage 4096 windows at a time and
 * return when the outputs are filled, F2_MEM_DEVICE calls enqueue and return (the first gradient call of an f2_cnn builds its
 * rotated, transposed weights and waits for that). Device pointers need element alignment only.
 * F2_ERR_INVALID, with nothing launched or written: a NULL ctx or cnn, a cnn of another device, n < 0, NULL x with n > 0, a
 * mem_space other than F2_MEM_HOST / F2_MEM_DEVICE. n == 0: F2_OK.
 *
 * f2_saliency_map: profile (window_offsets[U], C, 2) float64 in mem_space, rows as f2_cnn_input_gradient writes them. Rows, spans
 * and columns are those of f2_score_track (same origin, hop, spans, width rule).
 *   map   (U, C, W, 3) float64 in mem_space, map[u][c][x] =
 *           [0] rows        the count of owned rows, exact
 *           [1] mean G x    the float64 sum of profile[j][c][0] over the owned rows, divided by rows
 *           [2] mean |G|    the float64 sum of profile[j][c][1], divided by rows
 *         A column without rows is {0, NaN, NaN}. The sums have f2_score_track's fixed order: the same bits on every call and in
 *         both memory spaces.
 * Argument errors: those of f2_score_track (profile in the place of scores and labels), and C < 1 (F2_ERR_INVALID), C > 65535
 * (F2_ERR_UNSUPPORTED). U == 0: F2_OK.
 *
 * f2_eval_saliency_batch: f2_eval_figure_batch with every window differentiated while it is in scratch, and the map in the track's
 * place. Every output is optional and defined by calls that exist, bit for bit:
 *   scores (n, 2), labels (n), window_offsets, levels (B, C, W), range (host, 2B)   what f2_eval_figure_batch returns: the normal
 *           route still makes the decisions
 *   map (B, C, W, 3)   f2_saliency_map of the profile f2_cnn_input_gradient gives for the normalised windows of f2_input_batch
 *           (normalize = 1) at the same centres; origin = radius*step, the same hop, spans (NULL: [0, n_b)), width
 *   summary (B, C, 3)  f2_saliency_map with spans [0, n_b) and width 1: every row of the utterance
 * Only the profile is kept for all windows (16 C bytes per window). Errors, before anything is launched or written: everything
 * f2_eval_figure_batch rejects, and C > 65535 (F2_ERR_UNSUPPORTED). F2_ERR_NONPOSITIVE as in the strided call. B == 0: F2_OK. The
 * call waits for the stream before it returns.
 */
int f2_cnn_input_gradient(f2_ctx* ctx, const f2_cnn* cnn, const float* x /* (n, R, C), mem_space */, int64_t n,
                          float* grad_or_null /* (n, R, C), mem_space */, double* profile_or_null /* (n, C, 2), mem_space */,
                          float* scores_or_null /* (n, 2), mem_space */, int mem_space);
int f2_saliency_map(f2_ctx* ctx, const double* profile /* (window_offsets[U], C, 2), mem_space */,
                    const int64_t* window_offsets /* host, U+1 */, int U, int C,
                    const int64_t* spans /* host, 2U, required */, int64_t origin, int hop, int width,
                    double* map /* (U, C, width, 3), mem_space */, int mem_space);
int f2_eval_saliency_batch(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                           const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision,
                           int radius, int step, int hop,
                           const int64_t* spans_or_null /* host, 2B */, int width, int pool,
                           uint8_t* levels_or_null /* (B, C, width), mem_space */, double* range_or_null /* host, 2B */,
                           double* map_or_null /* (B, C, width, 3), mem_space */, double* summary_or_null /* (B, C, 3), mem_space */,
                           float* scores_or_null /* (n, 2) */, uint8_t* labels_or_null /* (n) */,
                           int64_t* window_offsets_or_null /* host, B+1 */, int mem_space);

/* ---- `cnn lpfsweep`: one ragged batch at K envelope cutoffs and unfiltered, in one device pass ------------------------------
 * The reference low-passes the envelope after the magnitude (EnvelopeExtraction.py:39-67), so the filterbank and the Hilbert
 * transform do not depend on the cutoff: a sweep needs them once, and one low-pass of envelopes that are already in memory.
 * (f2_version stays 114 with these two entries: look the symbols up to find out whether a build has them.)
 *
 * f2_lowpass_levels: env holds the ragged float64 envelopes of a batch as f2_envelope_batch delivers them - (C, n_b) blocks,
 * utterance b at C * offsets[b]. levels receives K+1 "levels" of it, level-major, (K+1) * C * offsets[B] doubles: level l < K is
 * every row filtered with butter(1, cutoff_hz[l] / 8000), level K the input copied bit for bit (the reference's "NOLPF"). Level
 * l, utterance b is utterance u = l*B + b of a (K+1)*B batch whose offsets are the clean offsets tiled:
 * tiled[u] = l*offsets[B] + offsets[b] (the convention of f2_eval_noise_sweep).
 *   coefficients   k = tan(pi * cutoff / 16000), b0 = k / (1 + k), a1 = (k - 1) / (k + 1): the host's tan(), float64. 8000 is
 *                  hard-coded as in the reference and in f2_envelope_batch, whatever the framerate.
 *   recurrence     y[n] = b0 * (x[n] + x[n-1]) - a1 * y[n-1], every row from zero state, everything in float64. A row is one
 *                  (utterance, channel) pair; state never crosses a row or an utterance boundary. The input is any finite
 *                  float64: the filter is linear and nothing assumes positive data.
 *   formulation    s[n] = q * s[n-1] + x[n] with q = -a1, y[n] = b0 * (s[n] + s[n-1]). One workgroup walks a row in segments of
 *                  4096 samples; inside a segment a lane folds its pairs of samples, a weighted scan (powers of q formed in
 *                  float64) runs across the wave, the wave totals are chained through LDS, and s at the end of the segment
 *                  enters the next one. The segmentation is a function of the row length alone and every sum has a fixed order
 *                  (no floating-point atomics): the bits of a filtered row depend on its samples and its cutoff only - not on
 *                  B, on the row's place in the batch, on K or on the other cutoffs. Rows of any length, 0 and 1 included.
 *   memory         every input sample is read once for all K cutoffs; the K filters and the copy are produced from the same
 *                  registers. Loads and stores are 16 bytes wide whatever the parity of the row start (dword-aligned wide
 *                  accesses); only the last sample of an odd tail moves alone.
 * F2_ERR_INVALID, with nothing launched and levels untouched: a NULL ctx or offsets; offsets that do not start at 0 or that
 * decrease; B < 0; C <= 0; K < 1; a NULL cutoff_hz; a cutoff that is not finite or outside (0, 8000); NULL env or levels with
 * offsets[B] > 0; a mem_space other than F2_MEM_HOST / F2_MEM_DEVICE. F2_ERR_UNSUPPORTED, likewise: K > 64. B == 0 or
 * offsets[B] == 0: F2_OK.
 *
 * f2_eval_cutoff_sweep: filterbank + envelope of the batch once (unfiltered, the two kernels of the eval calls), f2_lowpass_levels'
 * kernel on the result, then the window stage and the network of f2_eval_batch_strided over the (K+1)*B batch of envelopes,
 * and the tally of f2_eval_noise_sweep. Only the int16 / float64 samples go up; one wait at the end. Every output is optional.
 *   env_levels_or_null   (K+1) * C * offsets[B] float64, level-major, in mem_space (a device buffer serves as the call's own
 *           buffer; otherwise the levels live in context scratch). Bit for bit f2_lowpass_levels of its own level K block.
 *   scores_or_null, labels_or_null, window_offsets_or_null (host, (K+1)*B + 1)
 *           Level K: bit for bit what f2_eval_batch_strided(lpf = 0) returns for the batch. Level l: bit for bit f2_cnn_forward
 *           of the windows f2_gather_windows(normalize = 1) takes from level l's envelopes at centres radius*step + j*hop.
 *   stats_or_null   host, (K+1)*B*2: stats[2u] = windows of u labelled rising, stats[2u+1] = windows of u whose label equals
 *           the unfiltered level's label for the same window of the same utterance (for level K: its window count).
 * Errors, all before anything is launched or written: everything f2_eval_batch_strided rejects; K < 1, a NULL cutoff_hz, a
 * cutoff that is not finite or outside (0, 8000): F2_ERR_INVALID; K > 64, or (K+1)*B beyond what f2_eval_noise_sweep accepts:
 * F2_ERR_UNSUPPORTED. F2_ERR_NONPOSITIVE as in the strided call: a cutoff above 4 kHz has q < 0 and can produce values <= 0,
 * exactly as lpf = 1 does there. B == 0, or no utterance long enough for a window: F2_OK with window_offsets / stats filled.
 */
int f2_lowpass_levels(f2_ctx* ctx, const double* env /* ragged (C, n_b) blocks, mem_space */, const int64_t* offsets /* host, B+1 */,
                      int B, int C, const double* cutoff_hz /* host, K */, int K,
                      double* levels /* (K+1) * C * offsets[B], level-major, mem_space */, int mem_space);
int f2_eval_cutoff_sweep(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                         const double* coefs, int B, int C, int fft_precision, int radius, int step, int hop,
                         const double* cutoff_hz /* host, K */, int K,
                         double* env_levels_or_null /* (K+1) * C * offsets[B], mem_space */,
                         float* scores_or_null, uint8_t* labels_or_null,
                         int64_t* window_offsets_or_null /* host, (K+1)*B + 1 */,
                         int64_t* stats_or_null /* host, (K+1)*B*2 */, int mem_space);

/* ---- `cnn reverbsweep`: one ragged batch at K impulse responses and dry, in one device pass ---------------------------------
 * Reverberation acts on the waveform, before the filterbank. (f2_version stays 114 with these two entries: look the symbols up
 * to find out whether a build has them.)
 *
 * f2_reverb_levels: for utterance b (n_b samples, int16 or float64) and level l < K with impulse response h_l (T_l =
 * rir_offsets[l+1] - rir_offsets[l] float64 taps at rir + rir_offsets[l])
 *     wet[l][b][k] = sum_{t = 0 .. min(k, T_l - 1)} h_l[t] * x_b[k - t],   k = 0 .. n_b - 1
 * the causal convolution truncated to the utterance's own length (numpy.convolve(x, h)[:n]): a level has the offsets, the window
 * count and the time axis of the dry one. Level K is the dry batch converted to float64 (exact for int16), as level K of
 * f2_eval_noise_sweep. levels is level-major, (K+1) * offsets[B] float64; level l, utterance b is utterance u = l*B + b of a
 * (K+1)*B batch whose offsets are the dry offsets tiled: tiled[u] = l*offsets[B] + offsets[b].
 *   arithmetic     one float64 accumulator per output sample, starting from 0; taps in ascending t; each step is
 *                  acc = fma(h[t], x[k-t], acc), the samples converted to float64 first. No atomics, and the sum of one output
 *                  is never split across lanes or workgroups. A sample of a level therefore depends on (x_b, h_l, k) alone - not
 *                  on the launch shape, the batch around it, K or the other responses, the memory space or the input dtype of
 *                  equal values - and the same bits come out on every call. (A workgroup walks the taps in chunks and also adds
 *                  the terms fma(h[t], 0, acc) of the taps k < t < T_l that its chunk holds; they leave acc as it is, except that
 *                  a sum that has underflowed to -0 can come out as +0.)
 *   kernel         direct form; one workgroup per (tile of 1024 outputs, level), the input span of a chunk of 1024 taps staged
 *                  in LDS as float64 (zero before the utterance's start), the taps read through the scalar path, four
 *                  consecutive outputs per lane on a sliding register window. The cost grows with n_b * T_l; an FFT route is
 *                  not part of this call.
 * rir and rir_offsets are always host pointers, like coefs. wave and levels are in mem_space; device pointers need element
 * alignment only. F2_MEM_DEVICE: the call enqueues on the context's stream and returns; F2_MEM_HOST: it returns when levels is
 * filled.
 * F2_ERR_INVALID, with nothing launched and levels untouched: a NULL ctx or offsets; offsets that do not start at 0 or that
 * decrease; B < 0; a bad wave_dtype; K < 1; a NULL rir or rir_offsets; rir_offsets that do not start at 0 or that decrease; a
 * response of 0 taps; a tap that is not finite; NULL wave or levels with offsets[B] > 0; a mem_space other than F2_MEM_HOST /
 * F2_MEM_DEVICE. F2_ERR_UNSUPPORTED, likewise: K > 64; a response of more than 32768 taps (F2_REVERB_MAX_TAPS, 2.05 s at 16 kHz);
 * (K+1)*B beyond what f2_eval_noise_sweep accepts. B == 0 or offsets[B] == 0: F2_OK.
 *
 * f2_eval_reverb_sweep: f2_eval_noise_sweep with the two noise kernels replaced by f2_reverb_levels' kernel. Only the dry samples
 * and the taps go up; the levels are evaluated as ONE (K+1)*B-utterance float64 batch; one wait at the end. Every output is
 * optional.
 *   wet_or_null   (K+1) * offsets[B] float64, level-major, in mem_space: the waveforms that were evaluated (a device buffer
 *           serves as the call's own buffer; otherwise they live in context scratch). Bit for bit f2_reverb_levels.
 *   scores_or_null, labels_or_null, window_offsets_or_null (host, (K+1)*B + 1)
 *           bit for bit what f2_eval_batch_strided(F2_WAVE_F64) returns for the (K+1)*B batch `wet` with the tiled offsets and
 *           the same coefs ... hop: it is that call's code on that buffer. window_offsets is filled whenever the arguments pass.
 *   stats_or_null   host, (K+1)*B*2: stats[2u] = windows of u labelled rising, stats[2u+1] = windows of u whose label equals
 *           the dry level's label for the same window of the same utterance (for level K: its window count), counted on the
 *           device as in f2_eval_noise_sweep, also when labels_or_null is NULL.
 * Errors, all before anything is launched or written: everything f2_eval_batch_strided rejects, by the same checks; what
 * f2_reverb_levels rejects of K, rir and rir_offsets, with the same status. F2_ERR_NONPOSITIVE as in the strided call. B == 0, or
 * no utterance long enough for a window: F2_OK with window_offsets / stats filled. The call waits for the stream before it
 * returns, whatever mem_space is.
 */
int f2_reverb_levels(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets /* host, B+1 */, int B,
                     const double* rir /* host, rir_offsets[K] taps */, const int64_t* rir_offsets /* host, K+1 */, int K,
                     double* levels /* (K+1) * offsets[B], level-major, mem_space */, int mem_space);
int f2_eval_reverb_sweep(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                         const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius,
                         int step, int hop, const double* rir /* host, rir_offsets[K] taps */,
                         const int64_t* rir_offsets /* host, K+1 */, int K,
                         double* wet_or_null /* (K+1) * offsets[B], mem_space */, float* scores_or_null,
                         uint8_t* labels_or_null, int64_t* window_offsets_or_null /* host, (K+1)*B + 1 */,
                         int64_t* stats_or_null /* host, (K+1)*B*2 */, int mem_space);

/* ---- `cnn smearsweep`: one ragged batch at K spectral resolutions and sharp, in one device pass ------------------------------
 * The front end is a bank of C channels plus envelopes - the signal of a channel vocoder. Its two standard degradations, channel
 * interaction (envelopes leak into neighbouring channels) and a reduced number of bands, are linear maps across the channels of
 * envelopes that are already in device memory: one kernel, and the rest is the cutoff sweep's middle. (f2_version stays 114 with
 * these two entries: look the symbols up to find out whether a build has them.)
 *
 * f2_channel_mix_levels: env holds the ragged float64 envelopes of a batch as f2_envelope_batch delivers them - (C, n_b) blocks,
 * utterance b at C * offsets[b]. mix holds K matrices (C, C), row-major: mix[l][c][c'] is the weight of input channel c' in output
 * channel c. levels receives K+1 "levels", level-major, (K+1) * C * offsets[B] doubles: level l < K is mix[l] applied to every
 * sample column, level K the input copied bit for bit. Level l, utterance b is utterance u = l*B + b of a (K+1)*B batch whose
 * offsets are the caller's tiled: tiled[u] = l*offsets[B] + offsets[b] (the convention of f2_lowpass_levels).
 *   arithmetic     for level l < K, row c, sample i: lo the first and hi one past the last c' with mix[l][c][c'] != 0 (the row's
 *                  support, found on the host during the argument check); acc = +0.0; for c' = lo .. hi-1 ascending
 *                  acc = fma(mix[l][c][c'], env[b][c'][i], acc); store acc. One float64 accumulator per output, no atomics, no
 *                  sum split across lanes; zeros inside the support are walked; a row of zeros stores +0.0. The bits of a sample
 *                  therefore depend on its envelope column and its matrix row alone - not on B, on the utterance's place in the
 *                  batch, on K, on the other levels or rows, or on the memory space. The one liberty: a result that is a zero is
 *                  stored as +0.0 (a -0.0 under an identity row comes out +0.0, and so does a sum that has underflowed to -0).
 *                  The input is any finite float64; nothing assumes positive data. Rows of any length, 0 and 1 included; any
 *                  C from 1 to 512 (F2_SMEAR_MAX_CHANNELS); K <= 64.
 *   kernel         lanes run along time; one workgroup per (tile of 512 samples of one utterance, level, tile of 16 output
 *                  channels), a lane owning 2 samples x 16 accumulators. It walks the union of the supports of its 16 rows (outside
 *                  its own support a row's weights are zeros, which leave its accumulator alone): per input channel two 8-byte
 *                  loads per lane - consecutive lanes, consecutive doubles, so a row may start at any 8-byte boundary - feed 32
 *                  FMAs, whose weights are wave-uniform, come through the scalar load path from a transposed, zero-padded image of
 *                  the matrices (built in the argument check, uploaded once per call) and enter the FMA as its scalar operand.
 * mix is always a host pointer, like coefs. env and levels are in mem_space; device pointers need element alignment only.
 * F2_MEM_DEVICE: the call enqueues on the context's stream and returns; F2_MEM_HOST: it returns when levels is filled.
 * F2_ERR_INVALID, with nothing launched and levels untouched: a NULL ctx or offsets; offsets that do not start at 0 or that
 * decrease; B < 0; C <= 0; K < 1; a NULL mix; a weight that is not finite (the message names level, row and column); NULL env or
 * levels with offsets[B] > 0; a mem_space other than F2_MEM_HOST / F2_MEM_DEVICE. F2_ERR_UNSUPPORTED, likewise: K > 64; C > 512.
 * B == 0 or offsets[B] == 0: F2_OK.
 *
 * f2_eval_smear_sweep: filterbank + envelope of the batch once (the two kernels of the eval calls; low-passed at cutoff_hz if lpf,
 * so that a model trained on low-passed envelopes can be asked), f2_channel_mix_levels' kernel on the result, then the window stage
 * and the network of f2_eval_batch_strided over the (K+1)*B batch of envelopes, and the tally of f2_eval_noise_sweep. Only the int16
 * / float64 samples and the matrices go up; one wait at the end. Every output is optional.
 *   env_levels_or_null   (K+1) * C * offsets[B] float64, level-major, in mem_space (a device buffer serves as the call's own
 *           buffer; otherwise the levels live in context scratch). Bit for bit f2_channel_mix_levels of its own level K block.
 *   scores_or_null, labels_or_null, window_offsets_or_null (host, (K+1)*B + 1)
 *           Level K: bit for bit what f2_eval_batch_strided returns for the batch with the same lpf and cutoff_hz. Level l: bit
 *           for bit f2_cnn_forward of the windows f2_gather_windows(normalize = 1) takes from level l's envelopes at centres
 *           radius*step + j*hop.
 *   stats_or_null   host, (K+1)*B*2: stats[2u] = windows of u labelled rising, stats[2u+1] = windows of u whose label equals
 *           the sharp level's label for the same window of the same utterance (for level K: its window count).
 * Errors, all before anything is launched or written: everything f2_eval_batch_strided rejects, by the same checks; then what
 * f2_channel_mix_levels rejects of K, mix and C, with the same status; then (K+1)*B beyond what f2_eval_noise_sweep accepts:
 * F2_ERR_UNSUPPORTED. F2_ERR_NONPOSITIVE as in the strided call: a matrix with a zero row, or with negative weights, can produce
 * values <= 0. B == 0, or no utterance long enough for a window: F2_OK with window_offsets / stats filled. The call waits for the
 * stream before it returns, whatever mem_space is.
 */
int f2_channel_mix_levels(f2_ctx* ctx, const double* env /* ragged (C, n_b) blocks, mem_space */, const int64_t* offsets /* host, B+1 */,
                          int B, int C, const double* mix /* host, (K, C, C) */, int K,
                          double* levels /* (K+1) * C * offsets[B], level-major, mem_space */, int mem_space);
int f2_eval_smear_sweep(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                        const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step, int hop,
                        const double* mix /* host, (K, C, C) */, int K,
                        double* env_levels_or_null, float* scores_or_null, uint8_t* labels_or_null,
                        int64_t* window_offsets_or_null /* host, (K+1)*B + 1 */, int64_t* stats_or_null /* host, (K+1)*B*2 */, int mem_space);

/* ---- `cnn train --engine hip`: a training step on the device ------------------------------------------------------------------
 * The reference trains with Keras (Training.py:117-135): categorical cross-entropy, RMSprop(lr 1e-4, decay 1e-6), three Dropout
 * layers. These entries run that step on the recorded float32 forward and the backward-data chain of f2_cnn_input_gradient, with
 * weight-gradient kernels, dropout and the optimiser beside them. (f2_version stays 115 with these entries: look the symbols up.)
 *
 * f2_cnn_loss_gradient (stateless): x (n_all, R, C) float32 and y (n_all) uint8 labels (0 falling, anything else rising) in
 * mem_space; the m windows of the call are x[index[j]] (index (m) int64 in mem_space), or the first m without an index. Window j
 * is window b = j of the call's batch. Outputs, every one optional (NULL) and none changing another:
 *   grads      host array of 12 pointers, each to a tensor in mem_space in f2_cnn_create's order and Keras layouts: the gradient of
 *              L = sum over the m windows of -ln softmax(z)[y] (the sum, not the mean; the probabilities are not clipped)
 *   loss_sum   host, one double: L, float64 from the float32 logits
 *   correct    host, one int64: the windows whose training-mode decision (scores[1] > scores[0], ties falling) equals the label
 * The forward is the recorded float32 pass in training mode: Keras' three Dropout layers, after the two pools and after dense1's
 * ReLU, with the rates drop[0..2] and inverted scaling. With the element's index e in the library's order of the tensor -
 * (Hp1, Wp1, 32), (Hp2, Wp2, 64), (516) - and l = 0 / 1 / 2 for the layer:
 *             (w0, w1, w2, w3) = Philox4x32-10(counter = (e >> 2, b, l, step & 0xffffffff), key = (seed & 0xffffffff, seed >> 32))
 *             the element uses word e & 3; it is kept iff word * 2^-32 >= rate, and a kept value is multiplied by the float32
 *             nearest 1 / (1 - rate). Philox with the standard constants, as in f2_eval_noise_sweep. A rate of 0 draws nothing:
 *             drop = {0, 0, 0} is the chain without dropout, whatever seed and step are.
 * The gradient at the logits is dz = softmax(z) - onehot(y); ReLU and max-pool pass gradient by f2_cnn_input_gradient's rules; a
 * dropped cell passes none, a kept one 1 / (1 - rate) times it. Weight gradients: dW[tap][ci][co] = sum over windows and output
 * pixels of in[pixel + tap][ci] g[pixel][co], biases the sums of g, dense layers a^T g. Summation: no float32 chain is longer than
 * 1024 terms (conv2 .. conv4: at most 1024 pixels of one window per partial sum on the f32 matrix cores, the window cut the same
 * way wherever it stands); partial sums are added in float64, in an order that depends on the window shape and on m alone, on a
 * float64 gradient that also carries the sum over the chain's chunks of at most 1024 windows and is rounded to float32 once.
 * conv1, dense1 (on the float64 matrix cores), dense2 and the dense biases are float64 sums of exact products of float32 values. No
 * floating-point atomics: the same bits on every call and in both memory spaces.
 * F2_MEM_HOST calls stage only the m windows of the call (4096 at a time) and return when the outputs are filled; F2_MEM_DEVICE
 * calls enqueue, and wait for the stream only when loss_sum or correct is asked for. The call shares ctx's gradient scratch with
 * f2_cnn_input_gradient. F2_ERR_INVALID, with nothing launched or written: a NULL ctx, cnn or drop; a cnn of another device; m < 0;
 * NULL x or y with m > 0; a rate outside [0, 1); a NULL entry of grads; a negative index in host memory; a mem_space other than
 * F2_MEM_HOST / F2_MEM_DEVICE. The call is not told n_all: that every index is below it is the caller's duty, as is an index in
 * device memory being non-negative. m == 0: F2_OK, zero gradients, loss 0, 0 correct.
 *
 * f2_trainer_*: the weights, RMSprop's accumulators and the training set stay on the device between steps.
 *   create     12 host tensors (f2_cnn_create's order and checks), the window shape, RMSprop's constants, the three rates and the
 *              seed of the masks. Accumulators start at 0, "iterations" at 0.
 *   set_data   x (n, R, C) float32 normalised windows and y (n) uint8 labels, host memory, copied to the device once
 *   steps      order (count) int64, host, indices into the training set: ceil(count / batch) steps, step s on the windows
 *              order[s batch .. min((s + 1) batch, count)), the last one partial, enqueued back to back with one wait at the end.
 *              Each step: the gradient g of f2_cnn_loss_gradient with those indices, the trainer's rates and seed and step =
 *              "iterations" (same launch, same bits), then with m the step's window count, in float32 per element,
 *                  gm = g / m;  a = rho a + (1 - rho) gm^2;  p = p - lr_t gm / (sqrt(a) + eps),
 *              lr_t = lr / (1 + decay iterations) formed in double and rounded to float32 - RMSprop as Keras 2.2 runs it -, then
 *              the layouts the kernels read are rebuilt from the new weights on the device and "iterations" goes up by one.
 *              loss_sum / correct (host, optional): the sums of the steps' L and hits, each step with the weights it started from.
 *   get        what = F2_TRAINER_WEIGHTS, F2_TRAINER_ACCUMULATORS or F2_TRAINER_GRADIENT (the last step's g): 12 host tensors
 *   get_info   "iterations": steps taken so far
 * F2_ERR_INVALID, with nothing launched: NULL arguments, a trainer of another device, non-finite or negative constants, rho outside
 * [0, 1], a rate outside [0, 1), batch < 1, count < 0, an order entry outside [0, n), an unknown `what` or key.
 */
typedef struct f2_trainer f2_trainer;
enum { F2_TRAINER_WEIGHTS = 0, F2_TRAINER_ACCUMULATORS = 1, F2_TRAINER_GRADIENT = 2 };
int f2_cnn_loss_gradient(f2_ctx* ctx, const f2_cnn* cnn, const float* x /* (n_all, R, C), mem_space */, const uint8_t* y /* (n_all), mem_space */,
                         const int64_t* index_or_null /* (m), mem_space */, int64_t m, const double* drop /* host, 3 */, uint64_t seed,
                         uint64_t step, float* const* grads_or_null /* host, 12 pointers into mem_space */, double* loss_sum_or_null /* host */,
                         int64_t* correct_or_null /* host */, int mem_space);
int f2_trainer_create(f2_ctx* ctx, const float* const* tensors, int rows, int channels, double lr, double rho, double eps, double decay,
                      const double* drop /* host, 3 */, uint64_t seed, f2_trainer** trainer);
int f2_trainer_destroy(f2_ctx* ctx, f2_trainer* trainer);
int f2_trainer_set_data(f2_ctx* ctx, f2_trainer* trainer, const float* x /* host, (n, R, C) */, const uint8_t* y /* host, (n) */, int64_t n);
int f2_trainer_steps(f2_ctx* ctx, f2_trainer* trainer, const int64_t* order /* host, count */, int64_t count, int batch,
                     double* loss_sum_or_null /* host */, int64_t* correct_or_null /* host */);
int f2_trainer_get(f2_ctx* ctx, const f2_trainer* trainer, int what, float* const* tensors /* host, 12 pointers to host tensors */);
int f2_trainer_get_info(f2_ctx* ctx, const f2_trainer* trainer, const char* key, double* value);

/* ---- Training from the waves: windows re-rendered under fresh noise --------------------------------
 * The reference adds noise to a waveform before the filterbank (scripts/CNN/Evaluating.py:193-221) and trains on a fixed tensor of
 * stored windows, an epoch being one pass over it (scripts/CNN/Training.py:129-134). These entries rebuild the training windows from
 * the audio under a new noise condition per utterance, so that an epoch can see the corpus as no earlier epoch did. (f2_version
 * stays 115 with these entries: look the symbols up.)
 *
 * f2_noise_pick (stateless): f2_eval_noise_sweep's noise with one level per utterance. Utterance b runs at level l = level_of[b]:
 *   l < K    sample i becomes clean + sigma_b * z, product and sum rounded separately, sigma_b = RMS(clean_b) / 10^(snr_db[l] / 10)
 *            by the sweep's rule (int64 sums for int16, its fixed-order float64 sum otherwise) and z the sweep's deviate for
 *            (seed, level l, utterance first_utterance + b, i)
 *   l == K   the sample converted to float64, exactly
 *   level_of == NULL or K == 0: every utterance is clean.
 * With first_utterance == 0, utterance b of `noisy` is bit for bit utterance b of level level_of[b] of the sweep's noisy_or_null for
 * the same snr_db and seed, and sigma[b] its sigma[level_of[b] * B + b]. A sample depends on (seed, level, utterance number, i)
 * alone: not on B, the launch shape, the memory space or the input dtype of equal values. One workgroup per utterance for sigma,
 * one thread per sample for the noise, plain vector stores.
 *   wave, noisy      in mem_space (F2_MEM_HOST or F2_MEM_DEVICE); noisy: offsets[B] float64
 *   offsets, snr_db (K), level_of (B, each in [0, K]), sigma_or_null (B)    host
 * Errors, before anything is launched or written: what f2_eval_noise_sweep rejects of offsets, wave_dtype, mem_space and snr_db
 * (non-finite), and its limit on (K + 1) * B (F2_ERR_UNSUPPORTED); K < 0, level_of given with K > 0 and a NULL snr_db, a level_of
 * entry outside [0, K] (the message names the utterance): F2_ERR_INVALID; first_utterance + B beyond 2^32: F2_ERR_UNSUPPORTED.
 * B == 0 or no samples: F2_OK. F2_MEM_DEVICE calls enqueue and return; they wait only when sigma_or_null is asked for.
 *
 * f2_input_batch_noisy: bit for bit f2_input_batch(F2_WAVE_F64, ...) on f2_noise_pick's output for the same arguments - that call's
 * code on that buffer, which lives in context scratch and never leaves the device. Always the float64 route, also when every
 * utterance is clean. f2_input_batch's checks and statuses plus those of f2_noise_pick.
 *
 * f2_trainer_set_waves / render / get_windows: a trainer that owns the waves.
 *   set_waves    copies the waves, coefficients, centres and signs (host memory) to the device once. The training set becomes the
 *                n = center_offsets[B] windows with labels `signs`; x is reserved and undefined until the first render. It
 *                replaces what set_data put there, and set_data replaces it.
 *   render       utterances in groups [g group, min((g + 1) group, B)): group g is bit for bit f2_input_batch_noisy on those
 *                utterances with first_utterance = g group, normalize = 1 and the stored options, written straight to row
 *                center_offsets[g group] of x. The envelope scratch is bounded by the group, not by the corpus. Everything is
 *                enqueued on the context's stream; one wait at the end, for the error flag. level_of: host, B, or NULL.
 *   get_windows  rows first .. first + count - 1 of x and of the labels to host memory (either pointer may be NULL)
 *   get_info     "windows": n; "utterances": B of set_waves (0 after set_data)
 * f2_trainer_steps is unchanged and trains on what was rendered last.
 * F2_ERR_INVALID, with nothing changed: C or 2 radius + 1 other than the trainer's window shape, group < 1, a sign above 1, a window
 * that leaves its utterance (found in set_waves; the message names utterance, centre and length as f2_input_batch's does), what
 * f2_input_batch and f2_noise_pick reject, render without waves, rows outside [0, n) in get_windows. Utterances without centres,
 * empty utterances, B == 0: F2_OK. F2_ERR_NONPOSITIVE from the normaliser comes back from render, with x unspecified.
 */
int f2_noise_pick(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets /* host, B+1 */, int B,
                  const double* snr_db /* host, K */, int K, const int32_t* level_of /* host, B, each in [0, K] */,
                  uint32_t first_utterance, uint64_t seed, double* noisy /* offsets[B] float64, mem_space */,
                  double* sigma_or_null /* host, B */, int mem_space);
int f2_input_batch_noisy(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C,
                         int lpf, double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers,
                         int radius, int step, int normalize, const double* snr_db, int K, const int32_t* level_of,
                         uint32_t first_utterance, uint64_t seed, float* windows, int mem_space);
int f2_trainer_set_waves(f2_ctx* ctx, f2_trainer* trainer, const void* wave /* host */, int wave_dtype, const int64_t* offsets,
                         const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision,
                         const int64_t* center_offsets, const int64_t* centers, const uint8_t* signs /* host, center_offsets[B] */,
                         int radius, int step, int group);
int f2_trainer_render(f2_ctx* ctx, f2_trainer* trainer, const double* snr_db, int K, const int32_t* level_of /* host, B, or NULL */,
                      uint64_t seed);
int f2_trainer_get_windows(f2_ctx* ctx, const f2_trainer* trainer, int64_t first, int64_t count, float* x /* host */,
                           uint8_t* y /* host */);

/* ---- Training in rooms: one impulse response per utterance, new every epoch -------------------------------------------------
 * Reverberation acts on the waveform, before the filterbank, as noise does; a tensor of stored windows cannot be reverberated.
 * f2_reverb_levels makes every one of K rooms for every utterance, level-major - what a sweep wants. A training render wants one
 * room per utterance, in the layout of the waves, and these entries make that and nothing else. They compose with the noise
 * entries above: room first, then noise at an SNR of the reverberant signal. (f2_version stays 115 with these entries: look the
 * symbols up.)
 *
 * f2_reverb_pick (stateless): utterance b of `wet` (offsets[B] float64, the layout of `wave`) at room l = room_of[b]:
 *   l < K    wet[b][k] = sum_{t = 0 .. min(k, T_l - 1)} h_l[t] * x_b[k - t], numpy.convolve(x_b, h_l)[:n_b], by f2_reverb_levels'
 *            arithmetic word for word: one float64 accumulator per output, taps in ascending t, acc = fma(h[t], x[k-t], acc), no
 *            atomics, no sum split across lanes. Bit for bit utterance b of level l of f2_reverb_levels for the same rir - the
 *            tile of 1024 outputs and the chunk of 1024 taps are walked by the same code, so that this holds for a sum that
 *            underflowed to a signed zero as well (that call's one liberty).
 *   l == K   the samples converted to float64, exactly
 *   room_of == NULL or K == 0: every utterance is dry, and rir / rir_offsets may be NULL.
 * A sample depends on (x_b, h_l, k) alone: not on B, the utterance's place in the batch, the rooms of the other utterances, the
 * memory space or the input dtype of equal values.
 *   kernel   one workgroup per tile of 1024 outputs and nothing else (the sweep's grid is tiles x levels); the tap walk of a tile
 *            is the sweep's own function. A tile costs min(T_l, k0 + 1024) taps and nothing when dry, so the host, which knows every
 *            cost, uploads the list of (utterance, tile) most taps first, ties in (utterance, tile) order, and a workgroup reads
 *            its entry: the long tiles do not start last, and no workgroup searches the offsets. The results do not depend on
 *            the order (context option "reverb_pick_sort" = 0: utterance by utterance).
 *   wave, wet   in mem_space (F2_MEM_HOST or F2_MEM_DEVICE); device pointers need element alignment only; plain vector stores
 *   offsets, rir, rir_offsets (K+1), room_of (B)   host
 * F2_MEM_DEVICE: the call enqueues on the context's stream and returns; F2_MEM_HOST: it returns when wet is filled.
 * Errors, before anything is launched or written: what f2_reverb_levels rejects of ctx, offsets, B, wave_dtype and mem_space; K < 0;
 * unless every utterance is dry: a NULL rir (room_of given with K > 0), what f2_reverb_levels rejects of rir and rir_offsets with its
 * statuses (K > 64 and more than F2_REVERB_MAX_TAPS = 32768 taps: F2_ERR_UNSUPPORTED), a room_of entry outside [0, K] (the message
 * names the utterance): F2_ERR_INVALID. NULL wave or wet with samples: F2_ERR_INVALID. B == 0 or no samples: F2_OK.
 *
 * f2_input_batch_wet: f2_input_batch_noisy's arguments plus rir, rir_offsets, Kr, room_of. Bit for bit
 * f2_input_batch(F2_WAVE_F64, ...) on f2_noise_pick(F2_WAVE_F64, ...) on f2_reverb_pick(...): the same code on two buffers in
 * context scratch that never leave the device (the noise kernels read one and write the other). Sigma of an utterance is
 * therefore the RMS of its reverberant signal by the sweep's fixed-order float64 rule, for a dry utterance among rooms too. With
 * Kr == 0 or room_of == NULL there is no reverberant stage and the result is bit for bit f2_input_batch_noisy (whose sigma of
 * int16 samples is the int64 one). Errors: those of f2_input_batch_noisy, then those of f2_reverb_pick, all before a launch.
 *
 * f2_trainer_render_wet: f2_trainer_render with a room per utterance. Group g is bit for bit f2_input_batch_wet on its utterances
 * with first_utterance = g group, normalize = 1 and the stored options, written straight to its rows of x; the scratch is bounded
 * by the group; the taps go up once per call, not once per group; one wait at the end. room_of, level_of: host, B, or NULL.
 * f2_trainer_render is this call without rooms, bit for bit. Errors: f2_trainer_render's and f2_reverb_pick's, nothing launched.
 */
int f2_reverb_pick(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets /* host, B+1 */, int B,
                   const double* rir /* host, rir_offsets[K] taps */, const int64_t* rir_offsets /* host, K+1 */, int K,
                   const int32_t* room_of /* host, B, each in [0, K], or NULL */,
                   double* wet /* offsets[B] float64, mem_space, layout of `wave` */, int mem_space);
int f2_input_batch_wet(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C,
                       int lpf, double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers,
                       int radius, int step, int normalize, const double* rir, const int64_t* rir_offsets, int Kr,
                       const int32_t* room_of, const double* snr_db, int K, const int32_t* level_of, uint32_t first_utterance,
                       uint64_t seed, float* windows, int mem_space);
int f2_trainer_render_wet(f2_ctx* ctx, f2_trainer* trainer, const double* rir, const int64_t* rir_offsets, int Kr,
                          const int32_t* room_of /* host, B, or NULL */, const double* snr_db, int K,
                          const int32_t* level_of /* host, B, or NULL */, uint64_t seed);

/* ---- `cnn noisesweep --colours`: one ragged batch under K coloured noises and clean, in one device pass ---------------------
 * The white sweep (f2_eval_noise_sweep) with a filter per level between the generator and the sum: pink, speech-shaped or
 * matched noise instead of white. (f2_version stays 114 with these two entries: look the symbols up to find out whether a
 * build has them.)
 *
 * f2_shaped_noise_levels: level l < K has an SNR snr_db[l] and a filter h_l of T_l = fir_offsets[l+1] - fir_offsets[l] float64
 * taps at fir + fir_offsets[l]. Sample i (counted from the utterance's first sample) of utterance b becomes
 *     c     = sum over t = 0 .. T_l - 1 of h_l[t] * z(seed, l, b, (i - t) mod 2^64)
 *     noisy = clean + sigma * c
 *     sigma = RMS(clean_b) / 10^(snr_db[l] / 10)
 *   deviate      z(seed, l, b, i) is the deviate of f2_eval_noise_sweep - Philox4x32-10 with counter (i & 0xffffffff, i >> 32, l,
 *                b) and key (seed & 0xffffffff, seed >> 32), two 53-bit uniforms, the cosine branch of Box-Muller - made by the
 *                same device function.
 *   before the utterance   the index i - t wraps as an unsigned 64-bit counter, so the samples before the utterance's first are
 *                deviates like any others, with counter words (low, 0xffffffff, l, b): the noise is stationary from sample 0 on;
 *                there is no zero lead-in and no transient.
 *   arithmetic   one float64 accumulator per output sample, starting from 0.0; taps in ascending t; each step is
 *                acc = fma(h[t], z[i-t], acc). Then noisy = clean + sigma * c, product and sum rounded separately; where sigma
 *                is 0 (level K, an all-zero or empty utterance) the clean sample exactly. No atomics, and the sum of one
 *                output is never split across lanes or workgroups. A sample therefore depends on (seed, l, b, i, h_l) and its
 *                clean utterance alone - not on B, the utterances around it, the launch shape, the tile size, the memory space
 *                or the input dtype of equal values.
 *   sigma        the white sweep's rule and its kernel: the same bits as f2_eval_noise_sweep's sigma for the same snr_db.
 *   filter gain  the library does not normalise the filters. With sum h^2 = 1 the expected noise power is sigma^2, so that "SNR"
 *                means what it means for the white sweep; f2cnn_amd/noise.py normalises every filter it hands out.
 *   white        T_l = 1, h_l = [1.0] reproduces level l of f2_eval_noise_sweep bit for bit: fma(1.0, z, 0.0) is z.
 *   level K      the clean batch converted to float64 (exact for int16).
 *   kernel       direct form; one workgroup per (tile of 1024 outputs, level); the deviates of the tile's span [k0 - (T_l - 1),
 *                k0 + 1024) generated once into LDS as float64 (24 KB at 2048 taps), the taps read through the scalar path, four
 *                consecutive outputs per lane on a sliding register window: the walk of f2_reverb_levels.
 * noisy is level-major, (K+1) * offsets[B] float64; level l, utterance b is utterance u = l*B + b of a (K+1)*B batch whose
 * offsets are the clean offsets tiled, as in f2_eval_noise_sweep. snr_db, fir and fir_offsets are always host pointers, and so
 * is sigma_or_null ((K+1)*B, level-major, 0 for level K). wave and noisy are in mem_space; device pointers need element
 * alignment only. F2_MEM_DEVICE: the call enqueues on the context's stream and returns (it waits only to hand back sigma);
 * F2_MEM_HOST: it returns when noisy is filled.
 * Limits: T_l <= 2048 (F2_SHAPED_MAX_TAPS, 128 ms at 16 kHz), K <= 64.
 * F2_ERR_INVALID, with nothing launched and no output written: a NULL ctx or offsets; offsets that do not start at 0 or that
 * decrease; B < 0; a bad wave_dtype or mem_space; K < 1, a NULL snr_db or a snr_db[k] that is not finite (f2_eval_noise_sweep's
 * checks); a NULL fir or fir_offsets; fir_offsets[0] != 0 or decreasing fir_offsets; a level with no taps; a tap that is not
 * finite (the messages name the level); NULL wave or noisy with offsets[B] > 0. F2_ERR_UNSUPPORTED, likewise: K > 64; a filter of
 * more than 2048 taps; (K+1)*B beyond what f2_eval_noise_sweep accepts. B == 0 or offsets[B] == 0: F2_OK, sigma filled with zeros.
 *
 * f2_eval_shaped_noise_sweep: f2_eval_noise_sweep with k_noise_levels replaced by f2_shaped_noise_levels' kernel. Only the
 * clean samples and the taps go up; the levels are evaluated as ONE (K+1)*B-utterance float64 batch; one wait at the end. Every
 * output is optional.
 *   noisy_or_null   (K+1) * offsets[B] float64, level-major, in mem_space. Bit for bit f2_shaped_noise_levels.
 *   scores_or_null, labels_or_null, window_offsets_or_null (host, (K+1)*B + 1)
 *           bit for bit what f2_eval_batch_strided(F2_WAVE_F64) returns for the (K+1)*B batch `noisy` with the tiled offsets and
 *           the same coefs ... hop: it is that call's code on that buffer. window_offsets is filled whenever the arguments pass.
 *   sigma_or_null, stats_or_null   as in f2_eval_noise_sweep, the tally by the same kernel.
 * Errors, all before anything is launched or written, in the sweeps' order: everything f2_eval_batch_strided rejects, by the same
 * checks; hop < 1; then what f2_shaped_noise_levels rejects of K, snr_db, fir and fir_offsets, with the same status.
 * F2_ERR_NONPOSITIVE as in the strided call. B == 0, or no utterance long enough for a window: F2_OK with window_offsets / sigma /
 * stats filled as f2_eval_noise_sweep fills them. The call waits for the stream before it returns, whatever mem_space is.
 */
int f2_shaped_noise_levels(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets /* host, B+1 */, int B,
                           const double* snr_db /* host, K */, const double* fir /* host, fir_offsets[K] taps */,
                           const int64_t* fir_offsets /* host, K+1 */, int K, uint64_t seed,
                           double* noisy /* (K+1) * offsets[B], level-major, mem_space */,
                           double* sigma_or_null /* host, (K+1)*B */, int mem_space);
int f2_eval_shaped_noise_sweep(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                               const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius,
                               int step, int hop, const double* snr_db /* host, K */,
                               const double* fir /* host, fir_offsets[K] taps */, const int64_t* fir_offsets /* host, K+1 */,
                               int K, uint64_t seed, double* noisy_or_null /* (K+1) * offsets[B], mem_space */,
                               float* scores_or_null, uint8_t* labels_or_null,
                               int64_t* window_offsets_or_null /* host, (K+1)*B + 1 */, double* sigma_or_null /* host, (K+1)*B */,
                               int64_t* stats_or_null /* host, (K+1)*B*2 */, int mem_space);

/* ---- Training against colours: one coloured-noise level per utterance, new every epoch --------------------------------------
 * f2_shaped_noise_levels makes every one of K levels for every utterance, level-major - what a sweep wants. A training render wants
 * one level per utterance, in the layout of the waves, and these entries make that and nothing else. A level is a pair (filter,
 * SNR), as in the sweep. They compose with the entries of "Training in rooms": room first, then coloured noise at an SNR of the
 * reverberant signal. (f2_version stays 115 with these entries: look the symbols up.)
 *
 * f2_shaped_noise_pick (stateless): utterance b of `noisy` (offsets[B] float64, the layout of `wave`) at level l = level_of[b]:
 *   l < K    sample i becomes clean + sigma_b * c, product and sum rounded separately, with
 *                c = sum over t = 0 .. T_l - 1 of h_l[t] * z(seed, l, first_utterance + b, (i - t) mod 2^64)
 *            by f2_shaped_noise_levels' arithmetic word for word: one float64 accumulator per output, starting from 0.0; taps in
 *            ascending t; acc = fma(h[t], z[i-t], acc); no atomics; the sum of one output never split across lanes; the index
 *            wraps below zero as a 64-bit counter. sigma_b = RMS(clean_b) / 10^(snr_db[l] / 10) by f2_noise_pick's kernel: the
 *            same bits as f2_noise_pick's sigma.
 *   l == K, or sigma_b == 0 (an all-zero or empty utterance)    the sample converted to float64, exactly
 *   level_of == NULL or K == 0: every utterance is clean, and fir / fir_offsets may be NULL.
 * Identity with the sweep: with first_utterance == 0, utterance b is bit for bit utterance b of level level_of[b] of
 * f2_shaped_noise_levels for the same snr_db, fir and seed - the tile of 1024 outputs and the epilogue are the same device
 * functions - and sigma[b] is that call's sigma[level_of[b] * B + b]. Identity with white: with every filter one tap of 1.0 the
 * result is bit for bit f2_noise_pick, for any first_utterance. A sample depends on (seed, l, utterance number, i, h_l) and its
 * clean utterance alone: not on B, the utterance's place in the batch, the levels of the other utterances, the memory space or the
 * input dtype of equal values.
 *   kernel   one workgroup of 256 threads per tile of 1024 outputs and nothing else (the sweep's grid is tiles x levels). A tile
 *            costs T_l taps and nothing when clean, so the host uploads the list of (utterance, tile) most taps first, ties in
 *            (utterance, tile) order - the list builder of f2_reverb_pick - and a workgroup reads its entry: no workgroup
 *            searches the offsets. The results do not depend on the order (context option "noise_pick_sort" = 0: utterance by
 *            utterance). LDS as the sweep's (24 KB at 2048 taps), taps through the scalar path, plain vector stores.
 *   wave, noisy   in mem_space (F2_MEM_HOST or F2_MEM_DEVICE); device pointers need element alignment only
 *   offsets, snr_db (K), fir, fir_offsets (K+1), level_of (B), sigma_or_null (B)   host
 * F2_MEM_DEVICE: the call enqueues on the context's stream and returns; it waits only when sigma_or_null is asked for.
 * F2_MEM_HOST: it returns when noisy is filled.
 * Errors, before anything is launched or written: those of f2_noise_pick; then, unless every utterance is clean (level_of NULL,
 * K == 0, or every entry equal to K): a NULL fir or fir_offsets (F2_ERR_INVALID) and what f2_shaped_noise_levels rejects of them,
 * with its statuses - K > 64 and more than F2_SHAPED_MAX_TAPS = 2048 taps: F2_ERR_UNSUPPORTED; fir_offsets[0] != 0, decreasing
 * fir_offsets, a level with no taps, a tap that is not finite: F2_ERR_INVALID (the messages name the level). NULL wave or noisy
 * with samples: F2_ERR_INVALID. B == 0 or no samples: F2_OK, sigma filled with zeros.
 *
 * f2_input_batch_coloured: f2_input_batch_wet's arguments plus fir, fir_offsets after snr_db. Bit for bit
 * f2_input_batch(F2_WAVE_F64, ...) on f2_shaped_noise_pick(F2_WAVE_F64, ...) on f2_reverb_pick(...): the same code on two buffers
 * in context scratch that never leave the device. fir == NULL: bit for bit f2_input_batch_wet (it is that call). With Kr == 0 or
 * room_of == NULL there is no reverberant stage and the noise stage reads the waves themselves (the sigma of int16 samples is then
 * the int64 one, as in f2_input_batch_noisy). Errors: those of f2_input_batch_noisy, then those of f2_shaped_noise_pick's taps
 * (with a non-NULL fir), then those of f2_reverb_pick, all before a launch.
 *
 * f2_trainer_render_coloured: f2_trainer_render_wet's arguments plus fir, fir_offsets after snr_db. Group g is bit for bit
 * f2_input_batch_coloured on its utterances with first_utterance = g group, normalize = 1 and the stored options, written straight
 * to its rows of x; the taps of rooms and filters go up once per call into buffers the trainer owns, not once per group; one wait
 * at the end. f2_trainer_render_wet is this call with fir == NULL, bit for bit. Errors: f2_trainer_render_wet's and those of the
 * taps, nothing launched.
 */
int f2_shaped_noise_pick(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets /* host, B+1 */, int B,
                         const double* snr_db /* host, K */, const double* fir /* host, fir_offsets[K] taps */,
                         const int64_t* fir_offsets /* host, K+1 */, int K,
                         const int32_t* level_of /* host, B, each in [0, K], or NULL */, uint32_t first_utterance, uint64_t seed,
                         double* noisy /* offsets[B] float64, mem_space, layout of `wave` */, double* sigma_or_null /* host, B */,
                         int mem_space);
int f2_input_batch_coloured(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C,
                            int lpf, double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers,
                            int radius, int step, int normalize, const double* rir, const int64_t* rir_offsets, int Kr,
                            const int32_t* room_of, const double* snr_db, const double* fir /* or NULL: white */,
                            const int64_t* fir_offsets, int K, const int32_t* level_of, uint32_t first_utterance, uint64_t seed,
                            float* windows, int mem_space);
int f2_trainer_render_coloured(f2_ctx* ctx, f2_trainer* trainer, const double* rir, const int64_t* rir_offsets, int Kr,
                               const int32_t* room_of /* host, B, or NULL */, const double* snr_db,
                               const double* fir /* or NULL: white */, const int64_t* fir_offsets, int K,
                               const int32_t* level_of /* host, B, or NULL */, uint64_t seed);

/* ---- Training at reduced resolution: one spectral resolution per utterance, new every epoch ---------------------------------
 * f2_channel_mix_levels mixes every sample of every envelope at every one of K levels - what a sweep wants. A training render
 * wants the windows of its labelled timepoints, one level per utterance: 3.8 % of the sample columns of a corpus of 3 s files with
 * 164 windows each. These entries mix those columns and no others, inside the gather: no second envelope buffer. The degradation
 * acts on the envelopes, so it comes last: room, noise, envelopes, mixing gather. (f2_version stays 115 with these entries: look
 * the symbols up.)
 *
 * f2_gather_windows_mixed (stateless): the ragged gather of f2_input_batch on envelopes that are already in memory, with a mixing
 * matrix per utterance. Window e of utterance b, at level l = mix_of[b]:
 *   l < K    v[k][c] = sum over c' of mix[l][c][c'] * env_b[c'][centers[e] + step * (k - radius)], by f2_channel_mix_levels'
 *            arithmetic word for word: one float64 accumulator per output, starting from +0.0; c' ascending over a span that
 *            holds the row's support (first to one past the last non-zero weight, found on the host; zeros inside it are walked);
 *            acc = fma(w, x, acc); the sum of one output never split across lanes; no atomics; a closing acc + 0.0. Then
 *            f2_input_batch's normaliser on v: (ln v - ln min) / (ln max - ln min) over the window in float64, then float32; an
 *            all-equal window is zeros; with normalize == 0 the window is (float) v.
 *   l == K   sharp: f2_input_batch's gather, with no mixing pass. An identity matrix is mixed like any other.
 *   mix_of == NULL or K == 0: every utterance is sharp, and mix may be NULL.
 * Identity with the sweep: the bits of a mixed value depend on its envelope column and its matrix row alone, so window e is bit
 * for bit the plain ragged gather on utterance b's block of level mix_of[b] of f2_channel_mix_levels(env, mix, K). A window does
 * not depend on B, the utterance's place in the batch, the levels of the other utterances, K, or the memory space.
 *   kernel   one workgroup of 256 threads per window. The window's R x C values are read once into LDS, the mixed window is
 *            formed into a second LDS array, and the reduction, the flag rule and the epilogue are the device function the plain
 *            gather calls. The weights are uploaded once per call as the transposed, zero-padded image of f2_channel_mix_levels
 *            with the span of every tile of 16 rows beside it. Plain vector stores.
 *   env      ragged (C, n_b) float64 blocks, utterance b at C * offsets[b], in mem_space (F2_MEM_HOST or F2_MEM_DEVICE)
 *   windows  (center_offsets[B], 2 * radius + 1, C) float32, in mem_space; device pointers need element alignment only
 *   offsets (B+1), center_offsets (B+1), centers (relative to their utterance), mix (K, C, C), mix_of (B)   host
 * F2_MEM_DEVICE: the call enqueues on the context's stream and waits only for the flag, that is with normalize != 0, as
 * f2_input_batch. F2_MEM_HOST: it returns when windows is filled.
 * Errors, before anything is launched or written: what f2_input_batch rejects of B, C, radius, step, offsets, center_offsets,
 * NULL data pointers and windows that leave their utterance (F2_ERR_INVALID); K < 0 (F2_ERR_INVALID); unless every utterance is
 * sharp by mix_of == NULL or K == 0: what f2_channel_mix_levels rejects of mix, K and C, with its statuses - a NULL mix or a
 * weight that is not finite: F2_ERR_INVALID, K > F2_SMEAR_MAX_LEVELS = 64 or C > F2_SMEAR_MAX_CHANNELS = 512:
 * F2_ERR_UNSUPPORTED - a mix_of entry outside [0, K] (F2_ERR_INVALID, the message names the utterance), and a window whose two
 * arrays, (2 * radius + 1) * (2 C + 1) float64 values, do not fit the 150 KiB of LDS of a workgroup (F2_ERR_UNSUPPORTED).
 * A value <= 0 in a window under normalisation (a matrix row of zeros, for one): F2_ERR_NONPOSITIVE after the run, that window
 * zeros, as f2_input_batch.
 *
 * f2_input_batch_smeared: f2_input_batch_coloured's arguments plus mix, Km, mix_of behind seed. Bit for bit
 * f2_gather_windows_mixed on the envelopes f2_input_batch_coloured gathers from; nothing leaves the device in between. Km == 0 or
 * mix_of == NULL: bit for bit f2_input_batch_coloured (it is that call). Errors: those of f2_input_batch_coloured, then those of
 * f2_gather_windows_mixed's matrices and levels, all before a launch.
 *
 * f2_trainer_render_smeared: f2_trainer_render_coloured's arguments plus mix, Km, mix_of behind seed. Group g is bit for bit
 * f2_input_batch_smeared on its utterances with first_utterance = g group, normalize = 1 and the stored options; the image of the
 * matrices goes up once per call into a buffer the trainer owns, not once per group. f2_trainer_render_coloured is this call
 * without matrices, bit for bit. Errors: f2_trainer_render_coloured's and those of the matrices and levels, nothing launched.
 */
int f2_gather_windows_mixed(f2_ctx* ctx, const double* env /* ragged (C, n_b) blocks, mem_space */, const int64_t* offsets /* host, B+1 */,
                            int B, int C, const int64_t* center_offsets /* host, B+1 */, const int64_t* centers /* host */, int radius,
                            int step, int normalize, const double* mix /* host, (K, C, C), or NULL */, int K,
                            const int32_t* mix_of /* host, B, each in [0, K], or NULL */,
                            float* windows /* (center_offsets[B], 2 radius + 1, C), mem_space */, int mem_space);
int f2_input_batch_smeared(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C,
                           int lpf, double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers,
                           int radius, int step, int normalize, const double* rir, const int64_t* rir_offsets, int Kr,
                           const int32_t* room_of, const double* snr_db, const double* fir /* or NULL: white */,
                           const int64_t* fir_offsets, int K, const int32_t* level_of, uint32_t first_utterance, uint64_t seed,
                           const double* mix /* host, (Km, C, C), or NULL: sharp */, int Km,
                           const int32_t* mix_of /* host, B, each in [0, Km], or NULL */, float* windows, int mem_space);
int f2_trainer_render_smeared(f2_ctx* ctx, f2_trainer* trainer, const double* rir, const int64_t* rir_offsets, int Kr,
                              const int32_t* room_of /* host, B, or NULL */, const double* snr_db,
                              const double* fir /* or NULL: white */, const int64_t* fir_offsets, int K,
                              const int32_t* level_of /* host, B, or NULL */, uint64_t seed,
                              const double* mix /* host, (Km, C, C), or NULL: sharp */, int Km,
                              const int32_t* mix_of /* host, B, or NULL */);

/* ---- Recorded maskers: `cnn noisesweep --maskers` and `cnn train --augment-maskers` ----------------------------------------------
 * Every other noise of this library is Gaussian. A recorded masker (babble, a cafeteria, music) keeps the envelope modulations of
 * its own that `like:` removes: the recording itself is mixed in, not a noise with its spectrum. (f2_version stays 115 with these
 * entries: look the symbols up to find out whether a build has them.)
 *
 * The maskers are R recordings of float64 samples, packed in `masker` with R + 1 `masker_offsets`; recording r has
 * M_r = masker_offsets[r+1] - masker_offsets[r] samples. A level l < K is a pair (recording r = masker_of[l], snr_db[l]); level K
 * is clean. For utterance number utt (b in f2_masker_levels and the sweep, first_utterance + b in f2_masker_pick, a window call or
 * a render) of n samples at level l:
 *   segment   start = ((w1 << 32) | w0) mod M_r as unsigned 64-bit integers, (w0, w1, w2, w3) = Philox4x32-10 with counter
 *             (r, 0x4D41534B, 0, utt) and key (seed & 0xffffffff, seed >> 32), by the generator's own device function. No deviate
 *             has 0x4D41534B as its second counter word (theirs is 0 or 0xffffffff for rows of at most 2^22 samples): the streams
 *             are disjoint. The start depends on (seed, r, utt) alone, so two levels of one recording mix the same segment and
 *             differ in their SNR only. The segment is cyclic, m[i] = masker_r[(start + i) mod M_r], i < n: a recording shorter
 *             than the utterance wraps.
 *   sigma     RMS(clean) / 10^(snr_db[l] / 10), the white sweep's rule and its kernels: the same bits as f2_eval_noise_sweep /
 *             f2_noise_pick return for that SNR, so that "10 dB" means the same on the white, coloured and masker axes.
 *   gain      P = sum over i < n of m[i]^2 in float64 in a fixed order: one workgroup of 1024 threads per (utterance, level),
 *             thread t adds i = t, t + 1024, ... in that order, then the tree of the sigma kernel (lanes by shuffles, waves in
 *             order). No atomics: the same bits on every call. gain = sigma / sqrt(P / n), and 0 where n = 0, sigma = 0 or P = 0
 *             (a silent segment); no infinity or NaN is formed.
 *   mix       noisy[i] = clean[i] + gain * m[i], product and sum rounded separately. Where gain is 0, and at level K, the clean
 *             sample converted to float64 exactly.
 * A sample depends on (seed, r, snr, utt, i), its clean utterance and the recording - not on B, K, the other utterances or levels,
 * the launch shape, the memory space or the input dtype of equal values.
 *   kernels   the mix is one thread per sample, consecutive lanes on consecutive float64 values of the wave, the recording (up to
 *             the wrap) and the output, as k_noise_levels; the index is reduced once per thread and corrected by compare and
 *             subtract. One device function for the start and the sum in both gain kernels, one for the segment and the mix in both
 *             mix kernels. Plain vector stores.
 * Limits: 1 <= R <= 64, 1 <= K <= 64 (K = 0 allowed where a level per utterance is picked), every recording 1 .. 2^26 samples.
 * Beyond them: F2_ERR_UNSUPPORTED. F2_ERR_INVALID: a NULL masker, masker_offsets or masker_of; masker_offsets that do not start at 0
 * or that decrease; an empty recording; a sample that is not finite; a masker_of entry outside [0, R); and what the white sweep
 * rejects of K and snr_db. All before anything is launched or written; the messages name the level or the recording.
 * masker, masker_offsets, masker_of and snr_db are always host pointers; the recordings go up once per call (once per render, into
 * a buffer the trainer owns).
 *
 * f2_masker_levels: the (K+1) * offsets[B] float64 samples of all levels, level-major, utterance u = l*B + b of a (K+1)*B batch
 * whose offsets are the clean ones tiled, as f2_shaped_noise_levels. sigma_or_null, gain_or_null (float64) and start_or_null
 * (int64) are host arrays of (K+1)*B, level-major; the clean level holds 0 in all three. wave and noisy are in mem_space (device
 * pointers need element alignment only). F2_MEM_DEVICE: the call enqueues and waits only to hand back sigma / gain / start.
 * Errors: f2_shaped_noise_levels' of the batch, then the maskers'. B == 0 or offsets[B] == 0: F2_OK, the three filled with zeros.
 *
 * f2_eval_masker_sweep: f2_eval_shaped_noise_sweep with the levels made by f2_masker_levels' kernels. Only the clean samples and
 * the recordings go up; one wait at the end; every output is optional. noisy is bit for bit f2_masker_levels; scores, labels and
 * window_offsets are bit for bit what f2_eval_batch_strided(F2_WAVE_F64) returns on it; stats come from the white sweep's tally
 * kernel. Errors in the sweeps' order, the maskers' last.
 *
 * f2_masker_pick: utterance b at level level_of[b] in [0, K] as utterance number first_utterance + b, the output in the layout of
 * the waves; sigma / gain / start of B. With first_utterance == 0 bit for bit that level of that utterance of f2_masker_levels.
 * level_of == NULL or K == 0, or every entry K: the conversion to float64 alone, and masker may be NULL. Errors: f2_noise_pick's of
 * the batch, K, snr_db, level_of and first_utterance, then the maskers'.
 *
 * f2_input_batch_masked: f2_input_batch_smeared's arguments plus the masker stage behind mix_of (its SNRs, the recordings, the
 * levels and a level per utterance); the stage draws with the call's seed and first_utterance. The stages run in the order room,
 * masker, noise, envelopes, mixing gather: the Gaussian noise is added to the masked signal, and its sigma is that float64
 * signal's. Bit for bit f2_input_batch_smeared(F2_WAVE_F64, no rooms) on f2_masker_pick(F2_WAVE_F64) on f2_reverb_pick; nothing
 * leaves the device in between. Kk == 0 or masker_level_of == NULL: bit for bit f2_input_batch_smeared (it is that call). Errors:
 * those of f2_input_batch_smeared, then the masker stage's, all before a launch.
 *
 * f2_trainer_render_masked: f2_trainer_render_smeared's arguments plus the same stage. Group g is bit for bit f2_input_batch_masked
 * on its utterances with first_utterance = g group; the recordings go up once per call. f2_trainer_render_smeared is this call
 * without maskers, bit for bit.
 */
int f2_masker_levels(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets /* host, B+1 */, int B,
                     const double* snr_db /* host, K */, const double* masker /* host, masker_offsets[R] samples */,
                     const int64_t* masker_offsets /* host, R+1 */, int R, const int32_t* masker_of /* host, K, each in [0, R) */,
                     int K, uint64_t seed, double* noisy /* (K+1) * offsets[B], level-major, mem_space */,
                     double* sigma_or_null /* host, (K+1)*B */, double* gain_or_null /* host, (K+1)*B */,
                     int64_t* start_or_null /* host, (K+1)*B */, int mem_space);
int f2_eval_masker_sweep(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                         const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step,
                         int hop, const double* snr_db /* host, K */, const double* masker, const int64_t* masker_offsets /* host, R+1 */,
                         int R, const int32_t* masker_of /* host, K */, int K, uint64_t seed,
                         double* noisy_or_null /* (K+1) * offsets[B], mem_space */, float* scores_or_null, uint8_t* labels_or_null,
                         int64_t* window_offsets_or_null /* host, (K+1)*B + 1 */, double* sigma_or_null /* host, (K+1)*B */,
                         double* gain_or_null /* host, (K+1)*B */, int64_t* start_or_null /* host, (K+1)*B */,
                         int64_t* stats_or_null /* host, (K+1)*B*2 */, int mem_space);
int f2_masker_pick(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets /* host, B+1 */, int B,
                   const double* snr_db /* host, K */, const double* masker, const int64_t* masker_offsets /* host, R+1 */, int R,
                   const int32_t* masker_of /* host, K */, int K, const int32_t* level_of /* host, B, each in [0, K], or NULL */,
                   uint32_t first_utterance, uint64_t seed, double* noisy /* offsets[B], mem_space */,
                   double* sigma_or_null /* host, B */, double* gain_or_null /* host, B */, int64_t* start_or_null /* host, B */,
                   int mem_space);
int f2_input_batch_masked(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C,
                          int lpf, double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers,
                          int radius, int step, int normalize, const double* rir, const int64_t* rir_offsets, int Kr,
                          const int32_t* room_of, const double* snr_db, const double* fir /* or NULL: white */,
                          const int64_t* fir_offsets, int K, const int32_t* level_of, uint32_t first_utterance, uint64_t seed,
                          const double* mix /* host, (Km, C, C), or NULL: sharp */, int Km,
                          const int32_t* mix_of /* host, B, each in [0, Km], or NULL */, const double* masker_snr_db /* host, Kk */,
                          const double* masker /* host, or NULL: no maskers */, const int64_t* masker_offsets /* host, R+1 */, int R,
                          const int32_t* masker_of /* host, Kk */, int Kk,
                          const int32_t* masker_level_of /* host, B, each in [0, Kk], or NULL */, float* windows, int mem_space);
int f2_trainer_render_masked(f2_ctx* ctx, f2_trainer* trainer, const double* rir, const int64_t* rir_offsets, int Kr,
                             const int32_t* room_of /* host, B, or NULL */, const double* snr_db,
                             const double* fir /* or NULL: white */, const int64_t* fir_offsets, int K,
                             const int32_t* level_of /* host, B, or NULL */, uint64_t seed,
                             const double* mix /* host, (Km, C, C), or NULL: sharp */, int Km,
                             const int32_t* mix_of /* host, B, or NULL */, const double* masker_snr_db /* host, Kk */,
                             const double* masker /* host, or NULL: no maskers */, const int64_t* masker_offsets /* host, R+1 */,
                             int R, const int32_t* masker_of /* host, Kk */, int Kk,
                             const int32_t* masker_level_of /* host, B, or NULL */);

/* ---- `cnn train --augment-cutoffs`: an envelope cutoff per utterance ------------------------------------------------------------
 * f2_lowpass_levels makes every utterance at every cutoff; training needs one cutoff per utterance, new every epoch. (f2_version
 * stays 115 with these three entries: look the symbols up to find out whether a build has them.)
 * A cutoff level l < K is cutoff_hz[l] in Hz; level K is unfiltered, as in f2_lowpass_levels. cutoff_hz and cutoff_of are always
 * host pointers. Limits and errors of cutoff_hz and K are f2_lowpass_levels' (K <= 64: beyond, F2_ERR_UNSUPPORTED; every cutoff
 * finite and inside (0, 8000): F2_ERR_INVALID, the message names the cutoff) except that K == 0 is allowed; a cutoff_of entry
 * outside [0, K]: F2_ERR_INVALID, the message names the utterance. All before anything is launched or written.
 *   kernel    k_lowpass_pick: one workgroup per row (utterance, channel) walks the segments of k_lowpass_levels with the same loads,
 *             the same filter call and the same carried state, through one device function the two kernels share, with the pair
 *             {b0, a1} of the row's level. Plain vector stores.
 *
 * f2_lowpass_pick: utterance b of env at level cutoff_of[b], in the layout of env (C * offsets[B] doubles). Bit for bit block
 * cutoff_of[b] of f2_lowpass_levels for that utterance - whatever the batch around it, K or the other cutoffs - and at level K bit
 * for bit the input. filtered == env is allowed for F2_MEM_DEVICE and filters in place: nothing of an unfiltered utterance is then
 * read or written. cutoff_of == NULL or K == 0: a copy (nothing at all in place), and cutoff_hz may be NULL. Errors:
 * f2_lowpass_levels' of the batch, then the stage's. B == 0 or offsets[B] == 0: F2_OK.
 *
 * f2_input_batch_filtered: f2_input_batch_masked's arguments plus the cutoff stage behind masker_level_of. The stages run in the
 * order room, masker, noise, envelopes, cutoff, (mixing) gather. With the stage (Kc > 0 and cutoff_of != NULL) the envelopes of
 * the call are computed with lpf = 0 and filtered in place by k_lowpass_pick before the gather: the windows of utterance b are bit
 * for bit f2_gather_windows / f2_gather_windows_mixed on f2_lowpass_pick on the unfiltered envelopes of the stages before. A call
 * with the stage and lpf = 1 is F2_ERR_INVALID (the message names both). Without the stage: bit for bit f2_input_batch_masked (it
 * is that call), lpf = 1 included. Errors: those of f2_input_batch_masked, then the cutoff stage's, all before a launch.
 *
 * f2_trainer_render_filtered: f2_trainer_render_masked's arguments plus the same stage. Group g is bit for bit
 * f2_input_batch_filtered on its utterances; the filter coefficients go up once per call. A trainer whose waves were set with
 * lpf = 1 refuses the stage (F2_ERR_INVALID). f2_trainer_render_masked is this call without cutoffs, bit for bit.
 */
int f2_lowpass_pick(f2_ctx* ctx, const double* env /* C * offsets[B], mem_space */, const int64_t* offsets /* host, B+1 */, int B,
                    int C, const double* cutoff_hz /* host, K */, int K,
                    const int32_t* cutoff_of /* host, B, each in [0, K], or NULL */,
                    double* filtered /* C * offsets[B], mem_space; may be env in device memory */, int mem_space);
int f2_input_batch_filtered(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C,
                            int lpf, double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers,
                            int radius, int step, int normalize, const double* rir, const int64_t* rir_offsets, int Kr,
                            const int32_t* room_of, const double* snr_db, const double* fir /* or NULL: white */,
                            const int64_t* fir_offsets, int K, const int32_t* level_of, uint32_t first_utterance, uint64_t seed,
                            const double* mix /* host, (Km, C, C), or NULL: sharp */, int Km,
                            const int32_t* mix_of /* host, B, each in [0, Km], or NULL */, const double* masker_snr_db /* host, Kk */,
                            const double* masker /* host, or NULL: no maskers */, const int64_t* masker_offsets /* host, R+1 */, int R,
                            const int32_t* masker_of /* host, Kk */, int Kk,
                            const int32_t* masker_level_of /* host, B, each in [0, Kk], or NULL */,
                            const double* cutoff_levels_hz /* host, Kc, or NULL: no cutoffs */, int Kc,
                            const int32_t* cutoff_of /* host, B, each in [0, Kc], or NULL */, float* windows, int mem_space);
int f2_trainer_render_filtered(f2_ctx* ctx, f2_trainer* trainer, const double* rir, const int64_t* rir_offsets, int Kr,
                               const int32_t* room_of /* host, B, or NULL */, const double* snr_db,
                               const double* fir /* or NULL: white */, const int64_t* fir_offsets, int K,
                               const int32_t* level_of /* host, B, or NULL */, uint64_t seed,
                               const double* mix /* host, (Km, C, C), or NULL: sharp */, int Km,
                               const int32_t* mix_of /* host, B, or NULL */, const double* masker_snr_db /* host, Kk */,
                               const double* masker /* host, or NULL: no maskers */, const int64_t* masker_offsets /* host, R+1 */,
                               int R, const int32_t* masker_of /* host, Kk */, int Kk,
                               const int32_t* masker_level_of /* host, B, or NULL */,
                               const double* cutoff_levels_hz /* host, Kc, or NULL: no cutoffs */, int Kc,
                               const int32_t* cutoff_of /* host, B, or NULL */);

/* ---- `cnn eval --segments`: decisions smoothed into transitions ---------------------------------------------------------------
 * The reference stops at a rising / falling label per row (Evaluating.py:73-90); where the network is unsure the labels flicker,
 * and a run-length reading of them is mostly noise. Here: the most probable two-state sequence under a switching penalty, its
 * maximal runs, and the rows of every labelled interval (a phoneme) counted, all on the device. (f2_version stays 115 with these
 * four entries: look the symbols up to find out whether a build has them.)
 * Rows are those of f2_score_track / f2_label_accuracy: utterance u owns rows window_offsets[u] .. window_offsets[u+1] - 1, row j
 * stands at sample t = origin + j*hop, scores[j][1] is P(rising). mem_space is F2_MEM_HOST or F2_MEM_DEVICE; device pointers need
 * element alignment only; the small host arrays go up through the context's page-locked staging.
 *
 * f2_decision_path: the smoothed decision per row.
 *   emission    q_j = (int32) rint(logit_scale * (ln c(scores[j][1]) - ln c(scores[j][0]))), c(p) = min(max((double)p, 1e-7), 1.0)
 *               (f2_cnn_score_windows' clip), float64 throughout, rint to nearest with ties to even; a NaN in either score: q_j = 0.
 *   objective   over x in {0,1}^n: maximise sum_j x_j q_j - penalty * #{j >= 1 : x_j != x_{j-1}}, in int64.
 *   path        the one the sequential definition gives, ties included: V_0 = (0, q_0); V_j(s) = max(V_{j-1}(s), V_{j-1}(1-s) -
 *               penalty) + (s ? q_j : 0); bp_j(s) = s if V_{j-1}(s) >= V_{j-1}(1-s) - penalty (a tie stays), else 1-s;
 *               x_{n-1} = 1 iff V_{n-1}(1) > V_{n-1}(0) (a tie is falling); x_{j-1} = bp_j(x_j). With penalty = 0: x_j = (q_j > 0)
 *               wherever q_j != 0, a row with q_j = 0 takes the state of the row after it, and the last row is falling.
 *   outputs     path (window_offsets[U]) uint8 in mem_space; emissions_or_null int32, same shape and memory space;
 *               value_or_null (host, U) int64, the optimum. An utterance without rows has value 0 and writes nothing.
 *   kernels     the recurrence is a product of 2 x 2 matrices over (max, +) on int64, which is exactly associative: a product per
 *               tile of F2_PATH_TILE rows, a scan of the tile products per utterance (F2_PATH_SCAN_CHUNK tiles per step), each
 *               tile redone from the vector that enters it; then the same three steps from the right for the back pointers, which
 *               are maps {0,1} -> {0,1} under composition. Any order of an exact associative product gives the same V, hence the
 *               same path: the same bytes on every call, in both memory spaces, alone or inside a batch. No kernel waits for
 *               another workgroup.
 *   The call waits for the stream when it hands back value (whatever mem_space is) or serves host memory.
 *   F2_ERR_INVALID, before anything is launched or written: a NULL ctx / window_offsets; NULL scores or path with rows; U < 0;
 *   offsets that do not start at 0 or decrease; logit_scale not finite or <= 0; penalty < 0; a bad mem_space. F2_ERR_UNSUPPORTED,
 *   likewise: logit_scale > 2^20, penalty > 2^40, 2^31 rows or more (inside these limits |V| < 2^62).
 *
 * f2_decision_runs: maximal runs of equal decisions. labels: a path or raw labels, nonzero = rising.
 *   run_offsets (host, U+1)   utterance u owns runs run_offsets[u] .. run_offsets[u+1] - 1; always filled when the arguments pass.
 *   runs (capacity, 4) int64 in mem_space, or NULL to count only: {first row j0 within the utterance, rows, label 0 / 1,
 *               sum of q_j over the run (0 without emissions)}, utterance-major, ascending j0; a run never crosses an utterance
 *               boundary. capacity = window_offsets[U] always suffices.
 *   Boundary flags, integer prefix sums of the flags and of q, scatter: exact, the same bytes on every call and in both memory
 *   spaces. The call waits for the stream once to hand back run_offsets (and a second time behind the runs of a host caller).
 *   F2_ERR_INVALID: a NULL ctx / window_offsets / run_offsets; NULL labels with rows; U < 0; bad offsets; capacity < 0 with runs;
 *   a bad mem_space. F2_ERR_UNSUPPORTED: 2^31 rows or more; a non-NULL runs with capacity < run_offsets[U] - then run_offsets is
 *   filled and runs untouched.
 *
 * f2_interval_tally: decisions per labelled interval, the device side of a per-phoneme table.
 *   iv_offsets (host, R+1), iv_bounds (host, 2 * iv_offsets[R]) int64 pairs [a_k, b_k)   R interval sets, utterance u uses set
 *               u % R (a sweep passes U = (K+1)*B and R = B); within a set 0 <= a_k <= b_k <= a_{k+1}. Interval k owns the rows
 *               with a_k <= t_j < b_k.
 *   tally       (sum over u of the intervals of set u % R, 4) int64 in mem_space, utterance-major: {rows, rows with labels != 0,
 *               rows with path != 0 (0 if path is NULL), sum of q (0 if emissions is NULL)}.
 *   F2_ERR_INVALID, before anything is launched or written: a NULL ctx / tally / window_offsets / iv_offsets; NULL labels with
 *   rows; NULL iv_bounds with intervals; U < 0; R < 1 or U % R != 0 when U > 0 (R < 0 always); hop < 1 or origin < 0; bad offsets;
 *   bounds that are negative, reversed or overlap the interval before; a bad mem_space. F2_ERR_UNSUPPORTED: 2^31 rows or tally rows
 *   or more; the timepoint of an utterance's last row does not fit int64.
 *
 * f2_eval_segments_batch: f2_eval_batch_strided, then the three stages on the device's scores; nothing comes down in between.
 *   scores, labels, window_offsets   bit for bit what f2_eval_batch_strided returns for the same wave ... hop and mem_space
 *   path, emissions, value           f2_decision_path of those scores
 *   run_offsets, runs                f2_decision_runs of that path and those emissions; runs has room for window_offsets[B]
 *                                    rows (f2_eval_batch_strided's window count)
 *   tally                            f2_interval_tally of labels, path, emissions with origin = radius*step; NULL iv_offsets: none
 *   Every output is optional (NULL) and bit for bit what the separate call gives on those scores; path and emissions are made
 *   whenever runs or tally need them. One wait at the end (a host caller's runs come down behind it, once their number is known).
 *   Errors: everything f2_eval_batch_strided rejects, by the same checks and first; then those of the three stages in their order,
 *   all before anything is launched or written.
 */
#define F2_PATH_TILE 1024       /* rows per workgroup of the decoding kernels */
#define F2_PATH_SCAN_CHUNK 256  /* tiles per step of the per-utterance scans of the tile products */
int f2_decision_path(f2_ctx* ctx, const float* scores /* (window_offsets[U], 2), mem_space */,
                     const int64_t* window_offsets /* host, U+1 */, int U, double logit_scale, int64_t penalty,
                     uint8_t* path /* (window_offsets[U]), mem_space */, int32_t* emissions_or_null /* likewise */,
                     int64_t* value_or_null /* host, U */, int mem_space);
int f2_decision_runs(f2_ctx* ctx, const uint8_t* labels /* (window_offsets[U]), mem_space */,
                     const int32_t* emissions_or_null /* likewise */, const int64_t* window_offsets /* host, U+1 */, int U,
                     int64_t* run_offsets /* host, U+1 */, int64_t* runs_or_null /* (capacity, 4), mem_space */, int64_t capacity,
                     int mem_space);
int f2_interval_tally(f2_ctx* ctx, const uint8_t* labels /* mem_space */, const uint8_t* path_or_null /* mem_space */,
                      const int32_t* emissions_or_null /* mem_space */, const int64_t* window_offsets /* host, U+1 */, int U,
                      const int64_t* iv_offsets /* host, R+1 */, const int64_t* iv_bounds /* host, 2 * iv_offsets[R] */, int R,
                      int64_t origin, int hop, int64_t* tally /* (rows, 4), mem_space */, int mem_space);
int f2_eval_segments_batch(f2_ctx* ctx, const f2_cnn* cnn, const void* wave, int wave_dtype, const int64_t* offsets,
                           const double* coefs, int B, int C, int lpf, double cutoff_hz, int fft_precision, int radius, int step,
                           int hop, double logit_scale, int64_t penalty, const int64_t* iv_offsets_or_null /* host, R+1 */,
                           const int64_t* iv_bounds /* host */, int R, float* scores_or_null, uint8_t* labels_or_null,
                           int64_t* window_offsets_or_null /* host, B+1 */, uint8_t* path_or_null, int32_t* emissions_or_null,
                           int64_t* value_or_null /* host, B */, int64_t* run_offsets_or_null /* host, B+1 */,
                           int64_t* runs_or_null /* (window_offsets[B], 4), mem_space */, int64_t* tally_or_null /* mem_space */,
                           int mem_space);

#ifdef __cplusplus
}
#endif
#endif /* F2CNN_HIP_H */
