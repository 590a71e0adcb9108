// Internal declarations shared by the translation units of libf2cnn_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/f2cnn_hip.h"

// A grow-only device allocation (f2_reserve) that frees itself. Move-only: a copy would free the block twice.
struct f2_scratch {
    void* ptr = nullptr;
    size_t bytes = 0;
    f2_scratch() = default;
    f2_scratch(f2_scratch&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr, o.bytes = 0; }
    f2_scratch& operator=(f2_scratch&& o) noexcept {
        std::swap(ptr, o.ptr);     // (o frees the old block when it goes)
        std::swap(bytes, o.bytes);
        return *this;
    }
    ~f2_scratch() {
        if (ptr) (void)hipFree(ptr);
    }
};

// tables of the spectral filterbank + envelope kernel (f2_spectral.hip) for one (coefficient table, length class)
struct f2_spec_tables {
    int log2h = 0, C = 0;
    std::vector<double> coefs;
    int64_t tpitch = 0;
    f2_scratch hu, e, lgroup, e64;
};
#define F2_SPECTRAL_MIN_LOG2H 12   // rows of 4097 ... 65536 samples
#define F2_SPECTRAL_MAX_LOG2H 15

struct f2_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    int num_cus = 0;
    char err[512] = {0};
    // grow-only device scratch areas (freed by `delete ctx`, never before; stream-ordered reuse only)
    f2_scratch coefs;      // filter coefficients of the current call
    f2_scratch offsets;    // ragged offsets of the current call
    f2_scratch stage_in;   // F2_MEM_HOST staging
    f2_scratch stage_out;
    f2_scratch stage_aux;
    f2_scratch work;       // intermediates (GFB between K1 and K2, activations, ...)
    f2_scratch work2;
    f2_scratch xbuf;       // window tensor chunk between K3 and K4
    f2_scratch occ_src;    // f2_eval_occlusion_batch: the source windows of a chunk, which k_occlude_windows expands into xbuf
    f2_scratch grad_ws;    // f2_cnn_input_gradient: activations and gradients of a chunk of windows (f2_cnn_grad.hip), at most 1 GiB
    f2_scratch train_ws;   // f2_cnn_loss_gradient / f2_trainer_steps: partial sums, float64 gradient and the small per-window arrays (f2_cnn_train.hip)
    f2_scratch sal_profile;  // f2_eval_saliency_batch: the (C, 2) float64 profile rows of all windows of the call
    f2_scratch dense_in;   // conv4 outputs (+ dense1 outputs) of the windows of several utterances: one dense launch for all
    // the four sweeps, f2_lowpass_levels, f2_reverb_levels, f2_channel_mix_levels: the (K+1) x batch levels (float64 waveforms or envelopes) when the caller
    // gives no device buffer. One area: each of these calls places one set of levels, and nothing they nest (f2_eval_batch_strided,
    // with or without lpf; eval_envelopes) places another. f2_noise_pick / f2_launch_noisy_windows: the noisy float64 batch, by the same rule
    // (f2_batch_envelopes, which they nest, places nothing here).
    f2_scratch levels;
    // f2_reverb_pick / f2_launch_noisy_windows with rooms: the reverberant float64 batch, which the noise kernels read while they
    // write `levels` (a span of its own: k_noise_pick's pointers are __restrict__)
    f2_scratch wet;
    // f2_masker_levels, f2_masker_pick, f2_eval_masker_sweep, f2_launch_noisy_windows with maskers: [masker_offsets | samples] of the
    // recordings of the call in flight (up to 64 x 2^26 float64 samples: too much for `meta`), uploaded once per call
    f2_scratch masker;
    // f2_launch_noisy_windows with maskers: the masked float64 batch, which the noise kernels read while they write `levels`
    f2_scratch masked;
    // f2_channel_mix_levels, f2_eval_smear_sweep: tile sums, tile spans and the transposed mixing matrices of the call in flight (up to
    // 134 MB at 64 levels of 512 channels: too much for `meta`). Reserved once per call, before its first launch.
    f2_scratch mix;
    // The small arrays of the call in flight (f2_meta_carve): sigma / stats / window offsets of the noise sweep, filter coefficients /
    // stats / window offsets of the cutoff sweep, taps / tile sums / stats / window offsets of the reverberation sweep, counts and reference
    // labels of f2_label_accuracy, counts / loss sums / loss partials of f2_cnn_score_windows, span records and range words of the
    // pictures, utterance records of f2_resample_batch, sigma / level factors / levels of f2_noise_pick. One area for all of them, which holds while
    //  - nothing cached lives here: what a later call may find unchanged (spec_meta, rs_tab, offsets, coefs) has its own area;
    //  - a call carves it once, before its first launch and before any nested entry point runs (f2_reserve frees and reallocates
    //    on growth, and the noise sweep holds its pointers across the nested f2_eval_batch_strided), and no code reached from a
    //    nested call reserves it;
    //  - every reader and every upload goes through ctx->stream, so the next call's reuse is ordered behind them.
    f2_scratch meta;
    // f2_decision_path, f2_decision_runs, f2_interval_tally, f2_eval_segments_batch: every device array of the call in flight that is
    // not the caller's (f2_seg_plan, f2_segments.hip), reserved once per call before its first launch
    f2_scratch seg_ws;
    f2_scratch rs_tab;     // f2_resample_batch: the polyphase table of the last (up, down, half_len, taps)
    int64_t rs_up = 0, rs_down = 0, rs_half_len = -1;
    std::vector<double> rs_taps_host;   // the taps rs_tab was built from (skip the rebuild and the upload when equal)
    f2_scratch gather_log; // ln of the envelope samples a chunk of every-sample windows touches + column min / max (f2_gather.hip)
    // FFT twiddle tables (ensure_twiddles, f2_fft_lds.h), [precision][log2 H], built on first use: one per context for the
    // row launch, the flagged launch and the spectral kernels
    f2_scratch tw[2][16];
    f2_scratch tw_p3[2];   // the same for the three-pass plan of H = 8192 (k_envelope<F, 13, 3>), [precision]
    f2_scratch tw_large[2][24];   // same for the global-memory transform of long rows
    f2_scratch tw_split[24];      // tables of the four-step transform (f2_envelope_split.hip), by log2 H
    std::vector<int> pair_list_host[2];   // what pair_list currently holds (skip the upload when equal)
    f2_scratch tw_pair[2], pair_list[2];   // two-sub-row transform of 16385..65536-sample rows (f2_envelope_pair.hip): tables, utterance lists
    f2_scratch work3;             // utterance lists of the four-step launches
    f2_scratch handoff, handoff_off;   // float32 hand-off of long rows (f2_plan_handoff)
    std::vector<int64_t> handoff_off_host;
    f2_scratch k1_states, k1_mtab;     // time-split filterbank (small batches): segment end states, T^L per channel
    f2_scratch k1_order;               // ragged batches: unit order (longest first) + the queue counter
    int k1_mtab_L = 0;                 // segment length k1_mtab was built for ...
    std::vector<double> k1_mtab_coefs; // ... and the coefficient rows
    std::vector<int64_t> offsets_host;  // what ctx->offsets currently holds (skip re-upload when equal)
    std::vector<double> coefs_host;     // what ctx->coefs currently holds
    bool prof_on = false;
    struct prof_span {
        hipEvent_t first, second;   // start, stop
        bool closed;                // stop has been recorded (false when the launch in between failed)
    };
    std::vector<prof_span> prof[F2_K_COUNT];                         // one span per launch group
    std::vector<hipEvent_t> prof_pool;                               // recycled events
    // spectral path (f2_spectral.hip)
    std::vector<f2_spec_tables> spec_tabs;
    f2_scratch spec_x, spec_rho;          // utterance spectra, per-row digits of the launch in flight
    f2_scratch spec_xpart;                // float64 partial spectra of decimated (long) utterances
    f2_scratch spec_meta, spec_uflag;     // [initial flags (B) | utterance lists]; the flags the kernels update
    f2_scratch spec_gdump;                // [B][C][4] floats, option "spectral_guard_dump"
    size_t spec_gdump_rows = 0;           // B x C of the call that filled it
    std::vector<int> spec_meta_host;      // what spec_meta currently holds
    int spec_coefs_ok = -1;               // coefs_host eligible for the spectral kernel: -1 not decided, 0, 1
    int spec_min_pad = 64;                // ... and the padding samples its accuracy guard needs (ringing peak of the slowest channel)
    size_t spec_last_B = 0;               // batch size of the last fused call that used the spectral kernel (0: none)
    f2_scratch spec_lptab;                // low-pass powers per thread (lowpass_pairs_store_tab) ...
    double spec_lptab_a1 = 0.0;           // ... for this a1 (one table for every workgroup size: tests/test_gpu_call_history.py)
    // options (f2_ctx_set_option); -1 = decide from the batch
    int opt_spectral = 1;                 // route eligible utterances of the fused call through the spectral kernel
    int opt_spectral_min_rows = 4096;     // ... when the call has at least this many eligible rows (utterances x channels)
    float opt_spectral_tol = 4e-6f;       // accuracy guard: padding residual / maximum of the delivered row that flags an utterance
    int opt_spectral_min_pad = -1;        // padding samples a row needs for that route: -1 = from the coefficient table, else >= 64
    int opt_spectral_guard_dump = 0;      // diagnostic: keep the guard's per-row values of the last fused call (f2_spectral_guard_read)
    int opt_k1_split = -1;                // segments of the time-split filterbank (0 = never, >= 2 = force)
    int opt_k1_queue = -1;                // unit queue of the filterbank for ragged batches (0 / 1)
    int opt_k1_qwaves = 0;                // waves of the queue launch (0 = from the batch)
    int opt_env_pair = 1;                 // on-chip kernel for rows of 32769..65536 samples
    int opt_cnn_f16x3 = 1;               // conv2 .. conv4 + dense1 on the fp16 matrix cores, operands split in two pieces (3 MFMAs per product; "cnn_f16x3")
    int opt_cnn_ws = 1;                   // ... with the weights of each wave's role held in registers (f2_cnn_ws.hip; windows of 10 / 11 rows)
    int opt_cnn_ws_dense = 1;             // ... and dense1 with 96 windows per weight fragment, loads waited for by hand (k_dense1_ws)
    int opt_reverb_pick_sort = 1;         // k_reverb_pick's tile list: most taps first (0: utterance by utterance; the same results)
    int opt_noise_pick_sort = 1;          // k_shaped_noise_pick's tile list: most taps first (0: utterance by utterance; the same results)
    int opt_gather_blocked = 1;          // every-sample windows: logarithm once per sample, blocks of 32 windows (0: one workgroup per window)
    int opt_env_plan4 = 0;                // four-pass plan for every 1 s row (default: three passes where measured faster)
    // pinned staging of small host -> device uploads (f2_upload_async): a ring of page-locked memory the copies read from,
    // so that a call with device pointers only enqueues (the caller's / a local's array is copied on the host at once)
    char* up_ring = nullptr;
    size_t up_cap = 0, up_head = 0;
    struct up_span {
        size_t begin, end;
        hipEvent_t done;
    };
    std::vector<up_span> up_inflight;                  // oldest first
    struct up_side {
        void* ptr;
        size_t cap;
        hipEvent_t done;   // recorded behind the last copy that read from the buffer
        bool busy;         // `done` not yet seen reached
    };
    std::vector<up_side> up_big;   // grow-only page-locked side buffers of uploads too large for the ring, reused once copied
    f2_scratch flags;      // small device words (error flags)
    int* host_flags = nullptr;  // pinned mirror
    f2_scratch stamps;     // per-workgroup phase stamps, diagnostic build only (-DF2_STAMPS: f2_stamps_buffer)
};

#include "f2_cnn_split.h"
// offsets (floats) into f2_scale_set::sbias: conv2's biases x sa_3; conv3's x sa_3 sb_3 (accumulator-initial form) and x sa_4
// (epilogue form); conv4's x sa_dense1
enum { F2_SB_B2 = 0, F2_SB_B3I = 64, F2_SB_B3F = 128, F2_SB_B4 = 192, F2_SB_FLOATS = 256 };

// One set of the split path's power-of-two scales (f2_cnn_split.h), for network inputs bounded by |x| <= B = 2^e
struct f2_scale_set {
    f2_split_scales sc = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
    float c2_true = 1.f, sa_d1 = 1.f;   // 1 / (sa_2 sb_2): conv2's epilogue multiplier for outputs in true units; dense1's input scale
    float* sbias = nullptr;             // biases in the scaled units the split kernels' epilogues use (F2_SB_* offsets), device
    bool ok = false;                    // every scale inside the clamp [2^-20, 2^20] (always true for B = 1: the inputs the
                                        // scales were first designed for, kept as they were whatever the weights)
};
#define F2_BOUND_EXP_MAX 128            // finite float32 inputs: |x| < 2^128

// What f2_cnn_create keeps of the weights to run the L1 cascade of the scales for any input bound (f2_cnn.hip)
struct f2_cnn_cascade {
    std::vector<double> l1[5], absb[5];   // conv1 .. conv4, dense1: per output column, L1 norm of its weights and |bias|
    double sb[4] = {1.0, 1.0, 1.0, 1.0};  // weight scales of conv2 .. conv4, dense1 (independent of the input bound)
    std::vector<float> b2, b3, b4;        // biases of conv2 .. conv4 (the sbias forms)
};

struct f2_cnn {
    int rows = 0, channels = 0, flat = 0;
    int dev = 0;
    float* blob = nullptr;       // all tensors, device
    size_t off[12] = {0};        // element offsets of the 12 tensors in `blob`
    const float* t(int i) const { return blob + off[i]; }
    uint16_t* blob16 = nullptr;  // conv2 .. conv4 and dense1 kernels, scaled and split into two fp16 pieces (f2_cnn_split.h, k_*_h16x3)
    size_t off16[4] = {0};       // element offsets of the four layers in `blob16`
    const void* zeros = nullptr; // 256 zero bytes behind them (source of the padding pixels of f2_cnn_ws.hip's LDS-DMA loads)
    f2_cnn_cascade cascade;
    // scale sets by input-bound exponent e (B = 2^e): [0] built by f2_cnn_create, the others on first use by f2_cnn_forward
    // (f2_cnn_scale_set); each owns its sbias buffer, freed by f2_cnn_destroy
    mutable std::mutex sets_mu;
    mutable f2_scale_set* sets[F2_BOUND_EXP_MAX + 1] = {nullptr};
    // rotated, transposed kernels of conv2 .. conv4 and W1T for the backward-data pass (f2_cnn_grad.hip), built under sets_mu on the
    // first gradient call, freed by f2_cnn_destroy
    mutable float* grad_blob = nullptr;
    mutable double last_input_bound = 0.0;   // B of the last f2_cnn_forward / unnormalised f2_cnn_score_windows, -1: the float32 kernels ran, 0: none yet
    // f2_cnn_create's self-check of the weight-stationary kernels (hand-placed s_waitcnt around inline-asm loads: correct only
    // while the register allocator of the hipcc that built the library leaves those registers alone) against the per-tile
    // split-fp16 kernels on a fixed batch; a kernel that disagrees is not used with this network
    bool ws_ok = true, ws_dense_ok = true;
    float ws_check_diff = -1.f, ws_dense_check_diff = -1.f;   // max |score difference| measured (-1: not applicable)
    // ... and of the split path as a whole against the float32 kernels, at B = 1 and B = 2^10: off for this network if it disagrees
    bool f16x3_ok = true;
    float f16x3_check_diff = -1.f;
};

// The scale set for inputs bounded by 2^e, built (and its biases uploaded) on first use. *out = NULL: the split path cannot take
// such inputs (a scale would leave the clamp) or is off for this network - run the float32 kernels.
int f2_cnn_scale_set(f2_ctx* ctx, const f2_cnn* cnn, int e, const f2_scale_set** out);

// activation workspace (floats) the CNN needs per window
size_t f2_cnn_workspace_floats(const f2_cnn* cnn);

extern char g_f2_err[512];

int f2_fail(f2_ctx* ctx, int code, const char* fmt, ...);
int f2_reserve(f2_ctx* ctx, f2_scratch& s, size_t bytes);
// host -> device copy on the context's stream that does not wait for it: the bytes are copied into page-locked staging
// memory first (ring for small arrays, a one-off buffer for large tables), `src` may be reused at once
int f2_upload_async(f2_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int f2_upload_offsets(f2_ctx* ctx, const int64_t* offsets, int B);
int f2_upload_coefs(f2_ctx* ctx, const double* coefs, int C);

struct f2_cnn;
// ---- argument checks of the entry points that take caller data (f2_api.hip): every one of these conditions is tested here
// and nowhere else; all fail with F2_ERR_INVALID ----
int f2_check_ctx(f2_ctx* ctx);    // non-NULL, and makes its device current
int f2_check_wave_dtype(f2_ctx* ctx, int wave_dtype);
int f2_check_envelope_args(f2_ctx* ctx, int lpf, double cutoff_hz, int fft_precision);
int f2_check_dsp(f2_ctx* ctx, int wave_dtype, int lpf, double cutoff_hz, int fft_precision);   // the two above
int f2_check_mem_space(f2_ctx* ctx, int mem_space, bool allow_async);
int f2_check_offsets(f2_ctx* ctx, const int64_t* offsets, int B, const char* name);   // non-NULL, [0] == 0, non-decreasing
// B, C, mem_space and offsets of a ragged batch. `pipeline` (the calls of f2_pipeline.hip): C == 0 and F2_MEM_HOST_ASYNC are
// errors; without it C == 0 is an empty call and the third memory space is accepted
int f2_check_batch(f2_ctx* ctx, const int64_t* offsets, int B, int C, int mem_space, bool pipeline);
// B, wave_dtype, mem_space and offsets of a ragged batch of waves, in that order (the stage calls of waves)
int f2_check_wave_batch(f2_ctx* ctx, int wave_dtype, const int64_t* offsets, int B, int mem_space);
// A packed table of K runs of taps (taps, offsets: K + 1 entries) behind the caller's own checks of K and the two pointers:
// K <= max_levels (F2_ERR_UNSUPPORTED), offsets from 0 and non-decreasing, every run of 1 .. max_taps (above: F2_ERR_UNSUPPORTED)
// finite taps (F2_ERR_INVALID), tested in that order. The caller's words make the messages: "<K> <many> (at most ..)",
// "<offsets>[0] must be 0<at_zero>", "<offsets> must be non-decreasing (<index><l>)", "<one> <l> has no taps" and so on.
struct f2_tap_words {
    const char *many, *offsets, *at_zero, *index, *one;
};
int f2_check_taps(f2_ctx* ctx, const double* taps, const int64_t* offsets, int K, int max_levels, int max_taps, const f2_tap_words& W);
// The tile table of a ragged batch: the total of ceil(n_b / block) over the B utterances of h_offsets, and with `first` the B + 1
// running sums (what tile_owner of f2_tile_owner.h searches). f2_check_workgroups: a grid dimension of `count` workgroups exists
// (F2_ERR_UNSUPPORTED from 2^31 on: "<what> needs <count> workgroups<per> (at most 2^31 - 1)").
int64_t f2_tile_table(const int64_t* h_offsets, int B, int block, std::vector<int64_t>* first = nullptr);
int f2_check_workgroups(f2_ctx* ctx, int64_t count, const char* what, const char* per);
// The tile list of a kernel whose grid is the tiles alone (k_reverb_pick, k_shaped_noise_pick): one entry utterance << 32 | tile
// per tile of `block` outputs, in (utterance, tile) order; with `sorted`, most expensive first by cost(b, n_b, tile), ties in that
// order (a stable sort), so that the tiles that run longest do not start last. What the kernels compute does not depend on the order.
template <class Cost>
void f2_tile_list(const int64_t* h_offsets, int B, int block, bool sorted, std::vector<int64_t>* tiles, Cost cost) {
    tiles->clear();
    std::vector<int32_t> costs;
    for (int b = 0; b < B; ++b) {
        const int64_t n = h_offsets[b + 1] - h_offsets[b], nt = (n + block - 1) / block;
        for (int64_t i = 0; i < nt; ++i) {
            tiles->push_back((int64_t)b << 32 | i);
            if (sorted) costs.push_back(cost(b, n, i));
        }
    }
    if (!sorted) return;
    std::vector<int32_t> idx(tiles->size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int32_t)i;
    std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t c) { return costs[(size_t)a] > costs[(size_t)c]; });
    std::vector<int64_t> out(tiles->size());
    for (size_t i = 0; i < idx.size(); ++i) out[i] = (*tiles)[(size_t)idx[i]];
    tiles->swap(out);
}
// non-NULL, weights on the context's device, built for rows x C windows (rows == 0: the call has no window shape of its own)
int f2_check_cnn(f2_ctx* ctx, const f2_cnn* cnn, int rows, int C);
// *d_wave = the caller's pointer for F2_MEM_DEVICE, else ctx->stage_in after an asynchronous copy of `total` samples into it
int f2_stage_wave(f2_ctx* ctx, const void* wave, int wave_dtype, int64_t total, int mem_space, const void** d_wave);
// the same for `bytes` bytes of any input (f2_stage_wave is this with the sample size of wave_dtype), and into another area
int f2_stage_input(f2_ctx* ctx, const void* src, size_t bytes, int mem_space, const void** d_src);
int f2_stage_into(f2_ctx* ctx, f2_scratch& area, const void* src, size_t bytes, int mem_space, const void** d_src);
// the wait for the stream that ends an F2_MEM_HOST call (F2_MEM_DEVICE and F2_MEM_HOST_ASYNC calls only enqueue)
int f2_host_wait(f2_ctx* ctx, int mem_space);

// ---- where an output lives (f2_api.hip). The one rule of every entry point:
//   device memory, pointer given   the caller's pointer
//   device memory, NULL            `area` if a later kernel needs the data, else nowhere (dev == NULL)
//   host memory, pointer given     `area`, and f2_copy_back enqueues the copy to the caller
//   host memory, NULL              `area` without a copy back if a later kernel needs the data, else nowhere
// (F2_MEM_HOST_ASYNC is host memory here.) ----
struct f2_output {
    char* dev = nullptr;    // what the kernels write
    char* host = nullptr;   // where f2_copy_back sends it, or NULL
    size_t bytes = 0;
    bool callers = false;   // dev is the caller's buffer (all of it), not scratch
    template <class T>
    T* as() const { return (T*)dev; }
    // bytes [first, first + n) of an output made chunk by chunk: scratch holds one chunk at a time, a caller's buffer all of them
    f2_output chunk(size_t first, size_t n) const {
        f2_output c;
        c.dev = dev && callers ? dev + first : dev, c.host = host ? host + first : nullptr, c.bytes = n, c.callers = callers;
        return c;
    }
};
int f2_place(f2_ctx* ctx, f2_scratch& area, void* caller_or_null, size_t bytes, int mem_space, bool needed_on_device, f2_output* out);
int f2_copy_back(f2_ctx* ctx, const f2_output& o);   // enqueued on the stream, not waited for; nothing without a host destination
// Scores (2 floats) and labels (1 byte) of n windows by that rule, sharing ctx->stage_aux as [scores | labels | tail] + 64 bytes of
// slack: only the parts that need scratch are there; `tail` (8-byte aligned, NULL for tail_bytes == 0) is the caller's to use.
struct f2_score_outputs {
    f2_output scores, labels;
    char* tail = nullptr;
};
int f2_place_scores(f2_ctx* ctx, float* scores_or_null, uint8_t* labels_or_null, int64_t n, int mem_space, bool need_scores,
                    bool need_labels, size_t tail_bytes, f2_score_outputs* out);

// The small arrays of a call, carved from ctx->meta (see the three conditions there): name every array once with add(), then
// reserve() sizes the area and sets the pointers - 8-byte elements first, byte arrays behind them, each kind in the order named
// and without gaps (so arrays named in a row can go up in one upload).
struct f2_meta_carve {
    struct item {
        void* slot;      // the T* to set
        size_t bytes;
        bool wide;
    } items[20];   // (a window call with every stage names 17)
    int n = 0;
    template <class T>
    void add(T** p, size_t count) {
        static_assert(sizeof(T) == 8 || sizeof(T) == 1, "8-byte or byte elements");
        items[n++] = {(void*)p, sizeof(T) * count, sizeof(T) == 8};
    }
    int reserve(f2_ctx* ctx);
};

// A ragged batch of waves and how its envelopes are made: the arguments the envelope calls share, filled once by the entry point
struct f2_batch {
    const void* wave;
    int wave_dtype;
    const int64_t* offsets;
    const double* coefs;
    int B, C, lpf;
    double cutoff_hz;
    int fft_precision, mem_space;
    int64_t total() const { return offsets[B]; }
};
// Envelopes of the batch on the device: uploads offsets and coefficients, places the envelopes (stage_out, or the caller's device
// buffer) and the filterbank rows if wanted (stage_aux), stages the wave, runs f2_envelopes_device and enqueues the copies to a host
// caller. *d_env: where the envelopes are. Does not wait.
int f2_batch_envelopes(f2_ctx* ctx, const f2_batch& X, double* env_or_null, double* gfb_or_null, bool spectral, double** d_env);

#define F2_HIP(ctx, call)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return f2_fail((ctx), F2_ERR_HIP, "%s -> %s (%s:%d)", #call, hipGetErrorString(e_), \
                           __FILE__, __LINE__);                                                \
    } while (0)

#define F2_CHECK(ctx, cond, code, ...)                        \
    do {                                                      \
        if (!(cond)) return f2_fail((ctx), (code), __VA_ARGS__); \
    } while (0)

#define F2_TRY(expr)              \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != F2_OK) return rc_; \
    } while (0)

// One body for the calls that turn a ragged batch into levels, or into one level per utterance (f2_reverb_levels, f2_reverb_pick,
// f2_shaped_noise_levels, f2_noise_pick, f2_lowpass_levels, f2_channel_mix_levels). Of the call:
//   check()                 every argument check behind the context's, in the call's own order (the tests pin the precedence); after
//                           it offsets is valid wherever B > 0
//   carve(meta)             names its small arrays (and reserves what it keeps elsewhere)
//   in, stage(total, &d_in) its input and how that reaches the device (f2_stage_wave, f2_stage_input)
//   area, out, bytes_per_sample   where its output goes by the rule of f2_place, and how large it is per sample of the batch
//   launch(d_in, d_offsets, total, d_out)   its uploads and launches
//   sigma_or_null, n_sigma, d_sigma   a call with a sigma: n_sigma values from *d_sigma (which the carve sets, or leaves NULL: zeros)
//                           come back; zeros on an empty batch
// A host call waits for the stream; a device call only with a sigma to bring back.
template <class Check, class Carve, class Stage, class Launch>
int f2_stage_call(f2_ctx* ctx, const int64_t* offsets, int B, int mem_space, Check check, Carve carve, const void* in, Stage stage,
                  f2_scratch f2_ctx::*area, double* out, size_t bytes_per_sample, Launch launch, double* sigma_or_null = nullptr,
                  size_t n_sigma = 0, double* const* d_sigma = nullptr) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(check());
    const int64_t total = B > 0 ? offsets[B] : 0;
    if (total == 0) {
        if (sigma_or_null) std::fill(sigma_or_null, sigma_or_null + n_sigma, 0.0);
        return F2_OK;
    }
    F2_CHECK(ctx, in && out, F2_ERR_INVALID, "null data pointer");
    f2_meta_carve meta;
    F2_TRY(carve(&meta));
    F2_TRY(meta.reserve(ctx));
    f2_output o;
    F2_TRY(f2_place(ctx, ctx->*area, out, bytes_per_sample * (size_t)total, mem_space, true, &o));
    const void* d_in;
    F2_TRY(stage(total, &d_in));
    F2_TRY(f2_upload_offsets(ctx, offsets, B));
    F2_TRY(launch(d_in, (const int64_t*)ctx->offsets.ptr, total, o.as<double>()));
    F2_TRY(f2_copy_back(ctx, o));
    if (!sigma_or_null) return f2_host_wait(ctx, mem_space);
    if (*d_sigma) F2_HIP(ctx, hipMemcpyAsync(sigma_or_null, *d_sigma, sizeof(double) * n_sigma, hipMemcpyDeviceToHost, ctx->stream));
    else std::fill(sigma_or_null, sigma_or_null + n_sigma, 0.0);
    F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return F2_OK;
}

// ---- per-workgroup phase stamps, diagnostic build only (-DF2_STAMPS; tools/k2_stamps.py, tools/pair_stamps.py) ----
// F2_STAMP_ARRAY(st, N) declares N stamps in registers; F2_STAMP(st, k) records s_memrealtime (100 MHz, 10 ns ticks) into
// st[k] with nothing scheduled across it; F2_STAMP_STORE(st, N, out) has thread 0 write them to out[blockIdx.x * N + k]
// (out == NULL: nothing). The default build compiles all three to nothing.
#ifdef F2_STAMPS
#define F2_STAMP_ARRAY(st, N) unsigned long long st[N] = {0}
#define F2_STAMP(st, k)                            \
    do {                                           \
        __builtin_amdgcn_sched_barrier(0);         \
        (st)[k] = __builtin_amdgcn_s_memrealtime(); \
        __builtin_amdgcn_sched_barrier(0);         \
    } while (0)
#define F2_STAMP_STORE(st, N, out)                                                                       \
    do {                                                                                                 \
        if (threadIdx.x == 0 && (out))                                                                   \
            for (int k_ = 0; k_ < (N); ++k_) (out)[(size_t)blockIdx.x * (N) + k_] = (st)[k_];            \
    } while (0)
// Host side. f2_stamps_buffer: the device array for `rows` workgroups of `phases` (<= 10) stamps each, zeroed on the
// stream, or NULL beyond 128 x 2048 rows (one buffer of the context, reused by every launch: take it after the previous
// report). f2_stamps_report: waits for the stream, reads the
// stamps back and prints the mean ticks of each phase k >= 1 (stamp k - stamp k-1) as "<tag> <what> <name>=<ticks> ...";
// with `residency`, also the mean workgroup lifetime (first to last stamp) and how many workgroups were alive at once.
int f2_stamps_buffer(f2_ctx* ctx, size_t rows, int phases, unsigned long long** out);
int f2_stamps_report(f2_ctx* ctx, const unsigned long long* d_stamps, size_t rows, int phases, const char* const* names,
                     const char* tag, const char* what, bool residency);
#else
#define F2_STAMP_ARRAY(st, N) \
    do {                      \
    } while (0)
#define F2_STAMP(st, k) \
    do {                \
    } while (0)
#define F2_STAMP_STORE(st, N, out) \
    do {                           \
    } while (0)
#endif

// Profiling bracket: f2_prof_begin before the launch(es) of one kernel id, f2_prof_end after. A span whose launch
// failed in between is never closed: it is recycled by the next f2_prof_begin / f2_prof_reset and skipped by f2_prof_get.
int f2_prof_begin(f2_ctx* ctx, int kernel_id);
int f2_prof_end(f2_ctx* ctx, int kernel_id);

// kernel arguments shared by the envelope kernels
struct f2_env_params {
    const double* gfb;
    double* env;
    const int64_t* offsets;
    const int* ulist;  // utterances served by this launch (NULL: identity)
    const int* uflag;  // per utterance of the batch, or NULL: rows of utterances whose flag is 0 are left alone
    int C;
    int lpf;
    int f32_in;        // input rows are float32 at the start of their float64 slot (hand-off from K1)
    unsigned long long* stamps;   // diagnostic build only
    double b0, a1;     // y[n] = b0 (e[n] + e[n-1]) - a1 y[n-1]
};
// f2_envelope_flagged.hip: the utterances P.ulist[0..nutt) of length class log2h whose P.uflag entry is set (float FFT)
int f2_launch_envelope_flagged(f2_ctx* ctx, const f2_env_params& P, int log2h, unsigned nutt);

// longest row (2^22 samples = 262 s at 16 kHz) the global-memory envelope path accepts
// rows between the LDS limit and 262144 samples: four-step transform with LDS-resident 4096-point parts
bool f2_envelope_split_supports(int log2h, int precision);
int f2_launch_envelope_split(f2_ctx* ctx, const double* d_gfb, double* d_env, const int64_t* d_offsets, const int* utts,
                             int nutt, int log2h, int C, int lpf, double b0, double a1, const float* d_x32,
                             const int64_t* d_x32_off, const int* d_uflag = nullptr);
// rows of 32769..65536 samples, float transforms, input not aliased with the output: two LDS-resident sub-rows per workgroup
bool f2_envelope_pair_supports(int log2h, int precision);
int f2_launch_envelope_pair(f2_ctx* ctx, const double* d_gfb, double* d_env, const int64_t* d_offsets,
                            const int64_t* h_offsets, const int* utts, int nutt, int log2h, int C, int lpf, double b0,
                            double a1, const float* d_x32, const int64_t* d_x32_off, const int64_t* h_x32_off,
                            const int* d_uflag = nullptr);
#define F2_MAX_LOG2M_LARGE 22
int f2_launch_envelope_large(f2_ctx* ctx, const double* d_x, double* d_y, int64_t n, int C, int lpf, double b0,
                             double a1, int precision);

static inline int f2_log2_ceil(int64_t n) {
    int k = 0;
    while ((int64_t(1) << k) < n) ++k;
    return k;
}

// ---- launchers implemented in the kernel translation units (device pointers only) ----
// How the filterbank hands its rows to the envelope kernels inside one call (decided from the utterance lengths):
// float64 rows in the output buffer, or float32 - at the start of each row's float64 slot for rows the LDS-resident
// kernel takes (<= 32768 samples), compact (C, n) float rows in a scratch buffer for the four-step path (whose last
// pass writes float64 results over the slot while other workgroups still read their inputs).
struct f2_handoff {
    bool f32 = false;
    float* d_x32 = nullptr;                 // scratch of the long rows, or NULL when there are none
    const int64_t* d_x32_off = nullptr;     // device, per utterance: float offset into d_x32, -1 = in the row's own slot
    const int64_t* h_x32_off = nullptr;     // the same on the host (owned by the context, valid until the next plan)
};
int f2_plan_handoff(f2_ctx* ctx, const int64_t* h_offsets, int B, int C, int precision, bool want_gfb, f2_handoff* plan);
// d_uflag (device, B ints) != NULL: only utterances whose flag is non-zero are processed (the rest were served by the
// spectral kernel); the flags may be written by earlier launches on the stream.
// h_flag0 (host, B ints, with d_uflag): the flags as they are before the spectral kernel runs - the utterances this launch
// certainly has to process (its launch shape is chosen for them; any utterance may still be handed back by the guard).
int f2_launch_filterbank(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets,
                         const int64_t* h_offsets, const double* d_coefs, int B, int C, double* d_gfb,
                         const f2_handoff* handoff = nullptr, const int* d_uflag = nullptr, const int* h_flag0 = nullptr);
int f2_launch_envelope(f2_ctx* ctx, const double* d_gfb, const int64_t* d_offsets, const int64_t* h_offsets,
                       int B, int C, int lpf, double cutoff_hz, int precision, double* d_env,
                       const f2_handoff* handoff = nullptr, const int* d_uflag = nullptr, const int* h_flag0 = nullptr);
// Spectral filterbank + envelope (f2_spectral.hip): which utterances / coefficient tables it serves, and the launch for
// the utterances d_ulist[0..nutt) (all of length class log2h). Rows that fail its accuracy guard set d_uflag[b].
bool f2_spectral_supports_len(int64_t n, int min_pad);
bool f2_spectral_supports_coefs(const std::vector<double>& coefs, int C, std::vector<int>* Lgroup, int* min_pad);
int f2_launch_spectral(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const double* d_coefs,
                       int C, const int* d_ulist, int nutt, int64_t min_n /* shortest row of the group */, int log2h, int lpf,
                       double cutoff_hz, double* d_env, int* d_uflag);
// d_centers == NULL: window e is centred at first_center + e
int f2_launch_gather(f2_ctx* ctx, const double* d_env, int C, int64_t N, const int64_t* d_centers,
                     int64_t first_center, int64_t n_windows, int radius, int step, int normalize, float* d_out, int* d_flag);
// the same over a ragged batch in one launch: window e is centred at d_centers[e] (relative to its utterance) in utterance
// d_win_utt[e], whose (C, n_b) block starts at d_env + C * d_offsets[b]; windows must lie inside their utterance
int f2_launch_gather_ragged(f2_ctx* ctx, const double* d_env, int C, const int64_t* d_offsets, const int64_t* d_centers,
                            const int* d_win_utt, int64_t n_windows, int radius, int step, int normalize, float* d_out,
                            int* d_flag);
// a window list on the device, in ctx->work2: the centres and, with win_utt != NULL, the utterance of every window behind them
int f2_upload_windows(f2_ctx* ctx, const int64_t* centers, const int* win_utt, int64_t n_windows, const int64_t** d_centers,
                      const int** d_win_utt);
// Strided, normalised windows of a ragged batch (f2_eval_batch_strided): segment s is the windows first .. first + count - 1
// of utterance utt, window j centred at radius * step + j * hop of its utterance; the segments' windows are written to d_out
// one after the other. hop | step (and option "gather_blocked"): three launches for all segments, on the decimated envelope
// (f2_gather.hip); any other hop: f2_launch_gather_ragged at those centres. Uses ctx->work2 and ctx->gather_log; h_offsets host.
struct f2_win_seg {
    int utt;
    int64_t first, count;
};
int f2_launch_gather_strided(f2_ctx* ctx, const double* d_env, int C, const int64_t* d_offsets, const int64_t* h_offsets,
                             const f2_win_seg* segs, int nseg, int radius, int step, int hop, float* d_out, int* d_flag);
bool f2_gather_strided_blocked(const f2_ctx* ctx, int C, int step, int hop);    // the three-launch route serves this call
// ... and the columns of its scratch a segment of `count` windows takes (float64 values: C + 2 ceil(C / 16) per column)
int64_t f2_gather_strided_columns(int64_t count, int radius, int step, int hop);
// Which kernels a CNN launch takes - all false: the float32 kernels; split: the split-fp16 kernels (f2_cnn_split.h; needs a scale
// set); ws: its weight-stationary convolutions (f2_cnn_ws.hip); ws_dense: k_dense1_ws too. f2_cnn_capability: what the network can
// run (its shape and f2_cnn_create's self-check); f2_cnn_call_route: that, the context's options "cnn_f16x3" / "cnn_ws" /
// "cnn_ws_dense" and whether the call has a scale set. Every caller decides the route once per call (per chunk of a host-memory
// call, with the chunk's scale set) and hands it down; the launchers below test nothing else (f2_cnn.hip).
struct f2_cnn_route {
    bool split = false, ws = false, ws_dense = false;
};
f2_cnn_route f2_cnn_capability(const f2_cnn* cnn);
f2_cnn_route f2_cnn_call_route(const f2_ctx* ctx, const f2_cnn* cnn, bool have_scale_set);
// weight-stationary split-fp16 convolutions (f2_cnn_ws.hip): windows whose pooled conv2 output has four rows
bool f2_cnn_ws_supported(int rows, int channels);
bool f2_dense1_ws_takes(int K, int64_t n);   // k_dense1_ws serves n windows of K inputs (f2_launch_dense1_ws)
int f2_launch_dense1_ws(f2_ctx* ctx, const f2_cnn* cnn, const f2_scale_set* S, const float* a4, int64_t n, int K, float* a5);
int f2_launch_cnn_ws(f2_ctx* ctx, const f2_cnn* cnn, const f2_scale_set* S, const float* d_x, int64_t n, void* a2s, float* a4);
// runs the network on n windows (n <= chunk the workspace was sized for); d_ws: n * workspace floats. S: the scale set of the
// split path for inputs of this bound (f2_cnn_scale_set), NULL with a route that is not split
int f2_launch_cnn(f2_ctx* ctx, const f2_cnn* cnn, const f2_scale_set* S, f2_cnn_route route, const float* d_x, int64_t n, float* d_ws,
                  float* d_scores, uint8_t* d_labels);
// the two halves of f2_launch_cnn (f2_cnn.hip): convolutions per chunk of windows, dense layers over several chunks at once
int f2_launch_cnn_convs(f2_ctx* ctx, const f2_cnn* cnn, const f2_scale_set* S, f2_cnn_route route, const float* d_x, int64_t n,
                        float* d_ws, float* a4);
// (with_dense2 = false: dense1 alone, a5 filled and nothing else written - a training step masks a5 before its own dense2)
int f2_launch_cnn_dense(f2_ctx* ctx, const f2_cnn* cnn, const f2_scale_set* S, f2_cnn_route route, const float* a4, int64_t n, float* a5,
                        float* d_scores, uint8_t* d_labels, bool with_dense2 = true);
// what f2_launch_cnn_convs leaves a4 multiplied by on this route: dense1's input scale where the split conv4 kernels wrote it
// (windows with four pooled rows after conv2), 1 everywhere else
float f2_cnn_a4_scale(const f2_cnn* cnn, const f2_scale_set* S, f2_cnn_route route);
// d_dst[i] = d_src[i] * factor for count floats (f2_cnn_layers.hip)
int f2_launch_scale_copy(f2_ctx* ctx, const float* d_src, float* d_dst, int64_t count, float factor);
// k_cnn_input_range (f2_cnn_range.hip) over nwin windows of S floats at d_x: atomicMax of the bit pattern of max |x| over the finite
// values into d_words[0], of the complement of the quietest window's max |x| into d_words[2], and 1 into d_words[1] if a value is
// inf / NaN. The caller zeroes the three words first.
int f2_launch_cnn_input_range(f2_ctx* ctx, const float* d_x, int64_t nwin, int S, unsigned* d_words);
// f2_noise.hip, the kernels of f2_eval_noise_sweep. d_offsets: the B + 1 offsets of the clean batch; d_lin: K values
// 10^(snr_db / 10); d_sigma: (K + 1) * B, level-major, written by the first launch and read by the second, which writes the
// (K + 1) * total float64 samples of all levels (level K: the clean batch) to d_out.
int f2_launch_noise_sigma(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const double* d_lin, int B,
                          int K, double* d_sigma);
int f2_launch_noise_levels(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const double* d_sigma, int B,
                           int K, int64_t total, uint64_t seed, double* d_out);
// The kernels of f2_noise_pick: utterance b at level d_level[b] in [0, K] (K: clean), utterance first_utterance + b of its corpus.
// d_sigma (B) is written by the first launch and read by the second, which writes `total` float64 samples to d_out. d_sigma == NULL:
// every utterance is clean, d_lin and d_level are not read.
int f2_launch_noise_pick(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const double* d_lin,
                         const int32_t* d_level, int B, int K, int64_t total, uint32_t first_utterance, uint64_t seed, double* d_sigma,
                         double* d_out);
// ... and its first launch alone (k_noise_pick_sigma), for a stage whose second kernel is another (k_shaped_noise_pick)
int f2_launch_noise_pick_sigma(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const double* d_lin,
                               const int32_t* d_level, int B, int K, double* d_sigma);
// The noise stage of a window call or a render (f2_augment_args below). A coloured stage (fir != NULL, passed
// f2_check_noise_colours) filters the deviates of level l with the taps fir + fir_offsets[l] (host, K + 1 offsets) through
// k_shaped_noise_pick instead of k_noise_pick; sigma is k_noise_pick_sigma's in both. d_fir / d_fir_off: device copies that are up
// already (a render uploads them once for all its groups), or NULL.
struct f2_noise_pick_args {
    const double* snr_db;
    int K;
    const int32_t* level_of;
    uint32_t first_utterance;
    uint64_t seed;
    const double* fir = nullptr;
    const int64_t* fir_offsets = nullptr;
    const double* d_fir = nullptr;
    const int64_t* d_fir_off = nullptr;
    bool clean() const { return K == 0 || !level_of; }
    bool coloured() const { return fir && !clean(); }
};
int f2_check_noise_pick(f2_ctx* ctx, int B, const f2_noise_pick_args& N);
// The colours of a noise stage that passed f2_check_noise_pick, before anything is launched. Where every utterance is clean
// (N->clean(), or every level_of entry is K) no tap is read: fir and fir_offsets are cleared and never looked at. Otherwise a NULL
// fir is the white stage, or with need_fir (f2_shaped_noise_pick) F2_ERR_INVALID; a fir passes f2_check_fir_taps.
int f2_check_noise_colours(f2_ctx* ctx, int B, f2_noise_pick_args* N, bool need_fir);
// The coloured kernel of a stage (f2_noise_shaped.hip): f2_shaped_pick_meta names the tile list and, unless N.d_fir is given, the
// taps in the call's f2_meta_carve; the launch builds the list (option "noise_pick_sort": most taps first), uploads and runs
// k_shaped_noise_pick with the stage's d_level (B int32) and d_sigma (B, written by f2_launch_noise_pick_sigma on the stream).
struct f2_shaped_pick_arrays {
    int64_t *d_tiles = nullptr, *d_fir_off = nullptr;   // one entry per tile: utterance << 32 | tile; K + 1 tap offsets
    double* d_fir = nullptr;
};
void f2_shaped_pick_meta(f2_meta_carve* meta, int B, const int64_t* h_offsets, const f2_noise_pick_args& N, f2_shaped_pick_arrays* A);
int f2_launch_shaped_noise_pick(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const int64_t* h_offsets, int B,
                                const f2_noise_pick_args& N, const f2_shaped_pick_arrays& A, const int32_t* d_level,
                                const double* d_sigma, double* d_out);
// f2_masker.hip, the kernels of f2_masker_levels / f2_eval_masker_sweep / f2_masker_pick and of the masker stage of a window call or
// a render. A level l < K is the recording masker_of[l] at snr_db[l]; the recordings are host float64 samples, packed, with R + 1
// masker_offsets.
// f2_check_maskers: masker / masker_offsets / masker_of non-NULL and R >= 1 (F2_ERR_INVALID), R <= F2_MASKER_MAX_RECORDINGS and
// K <= F2_MASKER_MAX_LEVELS (F2_ERR_UNSUPPORTED), masker_offsets from 0 and non-decreasing, no empty recording (F2_ERR_INVALID), none
// above F2_MASKER_MAX_SAMPLES (F2_ERR_UNSUPPORTED), every sample finite and every masker_of entry in [0, R) (F2_ERR_INVALID), tested
// in that order; the messages name the recording or the level. f2_check_masker_levels: the white sweep's checks of K and snr_db
// before them. f2_upload_maskers: [masker_offsets | samples] into `area` (ctx->masker, or a buffer a trainer owns), enqueued.
// f2_masker_meta names the small device arrays of a launch in the call's f2_meta_carve (before its reserve()): [sigma | gain | start]
// as one run of 3 (K + 1) B values, level-major each, 10^(snr_db / 10) and masker_of. The launch uploads them and the recordings,
// runs f2_launch_noise_sigma and the two masker kernels, and writes (K + 1) * h_offsets[B] doubles, level-major, level K the clean
// samples.
#define F2_MASKER_MAX_RECORDINGS 64
#define F2_MASKER_MAX_LEVELS 64
#define F2_MASKER_MAX_SAMPLES (int64_t(1) << 26)
struct f2_masker_arrays {
    double *d_sigma = nullptr, *d_gain = nullptr, *d_lin = nullptr;
    int64_t *d_start = nullptr, *d_masker_of = nullptr;   // (masker_of: K int32 values in 8-byte slots)
};
int f2_check_maskers(f2_ctx* ctx, const double* masker, const int64_t* masker_offsets, int R, const int32_t* masker_of, int K);
int f2_check_masker_levels(f2_ctx* ctx, const double* snr_db, const double* masker, const int64_t* masker_offsets, int R,
                           const int32_t* masker_of, int K);
int f2_upload_maskers(f2_ctx* ctx, f2_scratch& area, const double* masker, const int64_t* masker_offsets, int R, const int64_t** d_moff,
                      const double** d_masker);
void f2_masker_meta(f2_meta_carve* meta, int B, int K, f2_masker_arrays* A);
int f2_launch_masker_levels(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const int64_t* h_offsets, int B,
                            const double* snr_db, const double* masker, const int64_t* masker_offsets, int R, const int32_t* masker_of,
                            int K, uint64_t seed, f2_masker_arrays& A, double* d_out);
// The masker stage of a window call or a render (f2_augment_args below) and the arguments of f2_masker_pick: utterance b at level
// level_of[b] in [0, K] (K: no masker), utterance first_utterance + b of its corpus. f2_check_masker_pick: f2_check_noise_pick's
// checks of K, snr_db, level_of and first_utterance; where every utterance is clean (silent(), or every level_of entry is K) nothing
// reads a recording and the stage becomes silent(); otherwise f2_check_maskers. d_masker / d_moff: device copies that are up already
// (a render uploads them once for all its groups), or NULL: the launch uploads them into ctx->masker. The launch runs
// k_noise_pick_sigma and the two pick kernels into d_out (total doubles); a silent stage converts alone.
struct f2_masker_pick_args {
    const double* snr_db = nullptr;
    const double* masker = nullptr;
    const int64_t* masker_offsets = nullptr;
    int R = 0;
    const int32_t* masker_of = nullptr;
    int K = 0;
    const int32_t* level_of = nullptr;
    uint32_t first_utterance = 0;
    uint64_t seed = 0;
    const double* d_masker = nullptr;
    const int64_t* d_moff = nullptr;
    bool silent() const { return K == 0 || !level_of; }
};
struct f2_masker_pick_arrays {
    double *d_sigma = nullptr, *d_gain = nullptr, *d_lin = nullptr;   // [sigma | gain | start] as one run of 3 B values
    int64_t *d_start = nullptr, *d_level = nullptr, *d_masker_of = nullptr;   // (level, masker_of: int32 values in 8-byte slots)
};
int f2_check_masker_pick(f2_ctx* ctx, int B, f2_masker_pick_args* M);
void f2_masker_pick_meta(f2_meta_carve* meta, int B, const f2_masker_pick_args& M, f2_masker_pick_arrays* A);
int f2_launch_masker_pick(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, int B, int64_t total,
                          const f2_masker_pick_args& M, f2_masker_pick_arrays& A, double* d_out);
// The argument checks of f2_input_batch, and behind them f2_check_noise_pick when the call has a noise stage (noise != NULL), all
// before anything is launched. `windows`: where the windows go (only tested for NULL). *n_windows == 0 on F2_OK: an empty call.
// win_utt: the utterance of every window.
int f2_check_input_batch(f2_ctx* ctx, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B, int C, int lpf,
                         double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers, int radius, int step,
                         const void* windows, int mem_space, const f2_noise_pick_args* noise, int64_t* n_windows,
                         std::vector<int>* win_utt);
// ... its checks of the window lists alone: offsets, center_offsets, and every window inside its utterance's envelope; data_given:
// the call's data pointers are all non-NULL (tested only where there are windows)
int f2_check_window_lists(f2_ctx* ctx, const int64_t* offsets, int B, const int64_t* center_offsets, const int64_t* centers, int radius,
                          int step, bool data_given, int64_t* n_windows, std::vector<int>* win_utt);
// d_stats ((K + 1) * B pairs, zeroed by the caller) += {windows labelled rising, windows labelled as the clean level labels them}
// per utterance of the (K + 1) * B batch whose window offsets are d_window_offsets; max_windows: the most any utterance has
int f2_launch_label_tally(f2_ctx* ctx, const uint8_t* d_labels, const int64_t* d_window_offsets, int B, int K, int64_t max_windows,
                          int64_t* d_stats);
// f2_lowpass.hip, the kernel of f2_lowpass_levels / f2_eval_cutoff_sweep. f2_check_cutoffs: K in 1 .. F2_LOWPASS_MAX_CUTOFFS (below:
// F2_ERR_INVALID, above: F2_ERR_UNSUPPORTED), cutoff_hz non-NULL, every value finite and in (0, 8000). f2_upload_lowpass_coefs: K x
// {b0, a1} of butter(1, cutoff / 8000) to d_coef (2 K doubles). The launch reads the (C, n_b) blocks of d_env (utterance b at
// C * d_offsets[b], total = offsets[B]) once and writes (K + 1) * C * total doubles, level-major, level K the copy.
#define F2_LOWPASS_MAX_CUTOFFS 64
int f2_check_cutoffs(f2_ctx* ctx, const double* cutoff_hz, int K);
int f2_upload_lowpass_coefs(f2_ctx* ctx, const double* cutoff_hz, int K, double* d_coef);
int f2_launch_lowpass_levels(f2_ctx* ctx, const double* d_env, const int64_t* d_offsets, int B, int C, int64_t total,
                             const double* d_coef, int K, double* d_levels);
// The cutoff stage of a window call or a render (f2_augment_args below) and the arguments of f2_lowpass_pick: utterance b at cutoff
// cutoff_of[b] in [0, K] (K: unfiltered). f2_check_lowpass_pick: K >= 0; unless the stage is unfiltered(), a non-NULL cutoff_hz,
// f2_check_cutoffs, every cutoff_of entry in [0, K] (F2_ERR_INVALID, the message names the utterance) and B * C rows that fit a grid
// (F2_ERR_UNSUPPORTED). d_coef: the K x {b0, a1} table on the device already (a render uploads it once for all its groups), or NULL:
// the launch uploads it into the array f2_lowpass_pick_meta named. The launch reads the (C, n_b) blocks of d_src and writes them to
// d_dst in the same layout; d_dst == d_src filters in place and touches nothing of an unfiltered utterance; an unfiltered() stage
// copies (nothing in place).
struct f2_lowpass_pick_args {
    const double* cutoff_hz = nullptr;
    int K = 0;
    const int32_t* cutoff_of = nullptr;
    const double* d_coef = nullptr;
    bool unfiltered() const { return K == 0 || !cutoff_of; }
};
struct f2_lowpass_pick_arrays {
    double* d_coef = nullptr;          // 2 K
    int64_t* d_cutoff_of = nullptr;    // B int32 values in 8-byte slots
};
int f2_check_lowpass_pick(f2_ctx* ctx, int B, int C, const f2_lowpass_pick_args& P);
void f2_lowpass_pick_meta(f2_meta_carve* meta, int B, const f2_lowpass_pick_args& P, f2_lowpass_pick_arrays* A);
int f2_launch_lowpass_pick(f2_ctx* ctx, const double* d_src, const int64_t* d_offsets, int B, int C, int64_t total,
                           const f2_lowpass_pick_args& P, const f2_lowpass_pick_arrays& A, double* d_dst);
// f2_reverb.hip, the kernel of f2_reverb_levels / f2_eval_reverb_sweep. A workgroup of k_reverb_levels makes F2_REVERB_BLOCK
// consecutive outputs of one utterance at one level and walks the taps in chunks of F2_REVERB_TAP_CHUNK (the input span of a chunk,
// F2_REVERB_BLOCK + F2_REVERB_TAP_CHUNK float64 samples, is what it stages in LDS).
// f2_check_rir: K in 1 .. F2_REVERB_MAX_LEVELS, rir / rir_offsets non-NULL, rir_offsets from 0 and non-decreasing, every response of
// 1 .. F2_REVERB_MAX_TAPS finite taps (F2_ERR_INVALID; too many levels or taps: F2_ERR_UNSUPPORTED). f2_reverb_meta names the
// device arrays of a launch in the call's f2_meta_carve (before its reserve()); the launch uploads them (tile sums, rir_offsets and
// taps, all from host memory), reads the B utterances of d_wave once per level and writes (K + 1) * h_offsets[B] doubles,
// level-major, level K the dry samples.
#define F2_REVERB_BLOCK 1024
#define F2_REVERB_TAP_CHUNK 1024
#define F2_REVERB_MAX_TAPS 32768
#define F2_REVERB_MAX_LEVELS 64
struct f2_reverb_arrays {
    int64_t *d_first = nullptr, *d_rir_off = nullptr;   // B + 1 running sums of the utterances' tiles; K + 1 tap offsets
    double* d_rir = nullptr;                            // rir_offsets[K] taps
};
int f2_check_rir(f2_ctx* ctx, const double* rir, const int64_t* rir_offsets, int K);
void f2_reverb_meta(f2_meta_carve* meta, int B, const int64_t* rir_offsets, int K, f2_reverb_arrays* A);
int f2_launch_reverb_levels(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const int64_t* h_offsets, int B,
                            const double* rir, const int64_t* rir_offsets, int K, const f2_reverb_arrays& A, double* d_out);
// The kernel of f2_reverb_pick: utterance b at room room_of[b] in [0, K] (K: dry), the output in the layout of the waves. The
// arguments of a stage (rir, rir_offsets, room_of: host) pass f2_check_reverb_pick before anything is launched: K >= 0; unless the
// stage is dry, a non-NULL rir, f2_check_rir, and every room_of entry in [0, K] (the message names the utterance).
// d_rir / d_rir_off: device copies of the taps and their offsets that are up already (a render uploads them once for all its
// groups), or NULL: the launch uploads them into the arrays f2_reverb_pick_meta named. The launch builds and uploads the tile list
// (option "reverb_pick_sort": most taps first), reads the B utterances once and writes h_offsets[B] doubles.
struct f2_reverb_pick_args {
    const double* rir;
    const int64_t* rir_offsets;
    int K;
    const int32_t* room_of;
    const double* d_rir;
    const int64_t* d_rir_off;
    bool dry() const { return K == 0 || !room_of; }
};
struct f2_reverb_pick_arrays {
    int64_t *d_tiles = nullptr, *d_rir_off = nullptr;   // one entry per tile: utterance << 32 | tile; K + 1 tap offsets
    int64_t* d_room = nullptr;                          // B int32 values in 8-byte slots
    double* d_rir = nullptr;
};
int f2_check_reverb_pick(f2_ctx* ctx, int B, const f2_reverb_pick_args& R);
void f2_reverb_pick_meta(f2_meta_carve* meta, int B, const int64_t* h_offsets, const f2_reverb_pick_args& R, f2_reverb_pick_arrays* A);
int f2_launch_reverb_pick(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const int64_t* h_offsets, int B,
                          const f2_reverb_pick_args& R, const f2_reverb_pick_arrays& A, double* d_out);
// f2_noise_shaped.hip, the kernel of f2_shaped_noise_levels / f2_eval_shaped_noise_sweep. A workgroup of k_shaped_noise_levels makes
// F2_SHAPED_BLOCK consecutive outputs of one utterance at one level; the deviates of its whole span, up to F2_SHAPED_BLOCK +
// F2_SHAPED_MAX_TAPS float64 values, are what it stages in LDS.
// f2_check_fir: the white sweep's checks of K and snr_db (K >= 1, snr_db non-NULL and finite: F2_ERR_INVALID), then fir / fir_offsets
// non-NULL (F2_ERR_INVALID), K <= F2_SHAPED_MAX_LEVELS (F2_ERR_UNSUPPORTED), fir_offsets from 0 and non-decreasing, every filter of
// 1 .. F2_SHAPED_MAX_TAPS finite taps (F2_ERR_INVALID; too many taps: F2_ERR_UNSUPPORTED); the messages name the level.
// f2_shaped_meta names the device arrays of a launch in the call's f2_meta_carve (before its reserve()); the launch uploads them
// (10^(snr_db / 10), tile sums, fir_offsets and taps, all from host memory), runs f2_launch_noise_sigma into d_sigma ((K + 1) * B,
// level-major), reads the B utterances of d_wave once per level and writes (K + 1) * h_offsets[B] doubles, level-major, level K the
// clean samples.
#define F2_SHAPED_BLOCK 1024
#define F2_SHAPED_MAX_TAPS 2048
#define F2_SHAPED_MAX_LEVELS 64
struct f2_shaped_arrays {
    double *d_sigma = nullptr, *d_lin = nullptr;        // (K + 1) * B sigmas; K values 10^(snr_db / 10)
    int64_t *d_first = nullptr, *d_fir_off = nullptr;   // B + 1 running sums of the utterances' tiles; K + 1 tap offsets
    double* d_fir = nullptr;                            // fir_offsets[K] taps
};
int f2_check_fir(f2_ctx* ctx, const double* snr_db, const double* fir, const int64_t* fir_offsets, int K);
// ... its checks of fir / fir_offsets alone, behind a caller's own checks of K and snr_db (`who` opens the NULL message)
int f2_check_fir_taps(f2_ctx* ctx, const double* fir, const int64_t* fir_offsets, int K, const char* who);
void f2_shaped_meta(f2_meta_carve* meta, int B, const int64_t* fir_offsets, int K, f2_shaped_arrays* A);
int f2_launch_shaped_noise_levels(f2_ctx* ctx, const void* d_wave, int wave_dtype, const int64_t* d_offsets, const int64_t* h_offsets,
                                  int B, const double* snr_db, const double* fir, const int64_t* fir_offsets, int K, uint64_t seed,
                                  const f2_shaped_arrays& A, double* d_out);
// f2_smear.hip, the kernel of f2_channel_mix_levels / f2_eval_smear_sweep. A workgroup of k_channel_mix_levels makes
// F2_SMEAR_TILE_CHANNELS output channels of F2_SMEAR_TILE_SAMPLES consecutive samples of one utterance at one level.
// f2_check_mix: K in 1 .. F2_SMEAR_MAX_LEVELS and mix non-NULL (F2_ERR_INVALID; too many levels, or C above
// F2_SMEAR_MAX_CHANNELS: F2_ERR_UNSUPPORTED), every weight finite (F2_ERR_INVALID, the message names level, row and column); in the
// same walk it finds every row's support, folds them into the span of each channel tile and builds the image the kernel reads
// (wT[l][c'][c] = mix[l][c][c'], rows padded with zeros to Cpad = nct * F2_SMEAR_TILE_CHANNELS). f2_smear_reserve sizes ctx->mix
// for a launch over B utterances (before the call's first launch); the launch uploads tile sums, spans and the image, reads the
// (C, n_b) blocks of d_env (utterance b at C * d_offsets[b]) and writes (K + 1) * C * h_offsets[B] doubles, level-major, level K
// the copy.
#define F2_SMEAR_TILE_SAMPLES 512
#define F2_SMEAR_TILE_CHANNELS 16
#define F2_SMEAR_MAX_CHANNELS 512
#define F2_SMEAR_MAX_LEVELS 64
struct f2_smear_plan {
    int K = 0, C = 0, Cpad = 0, nct = 0;      // nct: channel tiles
    std::vector<double> wT;                   // K * C * Cpad
    std::vector<int64_t> spans;               // K * nct: lo | hi << 32, the input channels lo .. hi - 1 a tile walks
};
int f2_check_mix(f2_ctx* ctx, const double* mix, int K, int C, f2_smear_plan* P);
int f2_smear_reserve(f2_ctx* ctx, const f2_smear_plan& P, int B);
int f2_launch_channel_mix_levels(f2_ctx* ctx, const double* d_env, const int64_t* d_offsets, const int64_t* h_offsets, int B,
                                 const f2_smear_plan& P, double* d_levels);
// f2_gather_mix.hip, the kernel of f2_gather_windows_mixed and the last stage of f2_input_batch_smeared / f2_trainer_render_smeared:
// the ragged gather of f2_launch_gather_ragged with the channels of every window mixed by the matrix of its utterance's level
// (mix_of[b] in [0, K], K: sharp) before the normaliser; bit for bit that gather on the level's block of f2_channel_mix_levels.
// The stage of a call (mix: K x C x C, mix_of: B, host) passes f2_check_mix_gather before anything is launched: K >= 0; unless the
// stage is sharp(), f2_check_mix (which builds `plan`), every mix_of entry in [0, K] (F2_ERR_INVALID, the message names the
// utterance) and a window whose two LDS arrays (f2_gather_mixed_lds bytes) fit a workgroup (F2_ERR_UNSUPPORTED). all_sharp: no
// utterance of the call is mixed - the call is the plain gather and takes f2_launch_gather_ragged.
// d_spans / d_wT: the device image of the plan, [spans | wT] in f2_mix_image_bytes bytes, which f2_upload_mix_image puts up - once
// per call into ctx->mix, or once per render into the trainer's buffer. d_mix_of: the B levels on the device (int32).
struct f2_mix_gather_args {
    const double* mix = nullptr;
    int K = 0;
    const int32_t* mix_of = nullptr;
    std::shared_ptr<f2_smear_plan> plan;   // (shared by the slices of a render)
    bool all_sharp = true;
    const int64_t* d_spans = nullptr;
    const double* d_wT = nullptr;
    bool sharp() const { return K == 0 || !mix_of; }
};
size_t f2_gather_mixed_lds(int radius, int C);
int f2_check_mix_gather(f2_ctx* ctx, int B, int C, int radius, f2_mix_gather_args* S);
size_t f2_mix_image_bytes(const f2_smear_plan& P);
int f2_upload_mix_image(f2_ctx* ctx, const f2_smear_plan& P, void* d_image, const int64_t** d_spans, const double** d_wT);
int f2_launch_gather_mixed(f2_ctx* ctx, const double* d_env, int C, const int64_t* d_offsets, const int64_t* d_centers, const int* d_win_utt,
                           int64_t n_windows, int radius, int step, int normalize, const f2_smear_plan& P, const int64_t* d_spans,
                           const double* d_wT, const int32_t* d_mix_of, float* d_out, int* d_flag);
// The augmentation stages of a window call (f2_input_batch_masked and the entries that telescope into it) or of a render
// (f2_trainer_render_masked likewise), in the order they run: rooms (f2_launch_reverb_pick into ctx->wet, skipped where dry()),
// maskers (f2_launch_masker_pick into ctx->masked, reading ctx->wet behind rooms; skipped where silent()), noise (k_noise_pick or
// k_shaped_noise_pick into ctx->levels, reading the last buffer written before it; converts alone where clean()), the
// envelopes, and smear (f2_launch_gather_mixed instead of f2_launch_gather_ragged unless sharp() or all_sharp; its image goes into
// ctx->mix unless smear.d_wT says it is up already). Cutoffs (f2_launch_lowpass_pick, in place on the envelopes, between them and the
// gather; skipped where unfiltered()) make the envelopes of the call unfiltered ones: lpf = 0, whatever X says - and a call with the
// stage and lpf = 1 does not pass check(). A further stage is a further record here: of() fills it from the C arguments
// (a render passes first_utterance 0), check() checks it, slice() advances it and f2_launch_noisy_windows runs it.
struct f2_augment_args {
    f2_reverb_pick_args rooms;
    f2_noise_pick_args noise;
    f2_mix_gather_args smear;
    f2_masker_pick_args maskers;   // (behind smear: the entries that have none leave it silent)
    f2_lowpass_pick_args cutoffs;  // (likewise: unfiltered)
    static f2_augment_args of(const double* rir, const int64_t* rir_offsets, int Kr, const int32_t* room_of, const double* snr_db,
                              const double* fir, const int64_t* fir_offsets, int K, const int32_t* level_of, uint32_t first_utterance,
                              uint64_t seed, const double* mix, int Km, const int32_t* mix_of) {
        f2_augment_args A = {{rir, rir_offsets, Kr, room_of, nullptr, nullptr}, {snr_db, K, level_of, first_utterance, seed, fir, fir_offsets}, {}};
        A.smear.mix = mix, A.smear.K = Km, A.smear.mix_of = mix_of;
        return A;
    }
    // ... and the masker stage of the entries that have one, drawn with the noise stage's seed and utterance numbers
    f2_augment_args& with_maskers(const double* snr_db, const double* masker, const int64_t* masker_offsets, int R, const int32_t* masker_of,
                                  int K, const int32_t* level_of) {
        maskers = {snr_db, masker, masker_offsets, R, masker_of, K, level_of, noise.first_utterance, noise.seed, nullptr, nullptr};
        return *this;
    }
    // ... and the cutoff stage of the entries that have one
    f2_augment_args& with_cutoffs(const double* cutoff_hz, int K, const int32_t* cutoff_of) {
        cutoffs.cutoff_hz = cutoff_hz, cutoffs.K = K, cutoffs.cutoff_of = cutoff_of;
        return *this;
    }
    // colours, rooms, mix, maskers, cutoffs, before anything is launched (builds smear.plan): the checks behind f2_check_noise_pick, which
    // every caller places itself - a window call runs it before its window lists. lpf: the call's own low-pass switch, which a cutoff
    // stage excludes
    int check(f2_ctx* ctx, int B, int C, int radius, int lpf) {
        F2_TRY(f2_check_noise_colours(ctx, B, &noise, false));
        F2_TRY(f2_check_reverb_pick(ctx, B, rooms));
        F2_TRY(f2_check_mix_gather(ctx, B, C, radius, &smear));
        F2_TRY(f2_check_masker_pick(ctx, B, &maskers));
        F2_TRY(f2_check_lowpass_pick(ctx, B, C, cutoffs));
        F2_CHECK(ctx, cutoffs.unfiltered() || !lpf, F2_ERR_INVALID,
                 "a cutoff stage (cutoff_of with K=%d cutoffs) and lpf = 1 exclude each other: the stage filters unfiltered envelopes",
                 cutoffs.K);
        return F2_OK;
    }
    // the stages of utterances b0 .. of the checked batch: their rows of the per-utterance tables, numbered on from b0 for the
    // generator; the taps, the plan and what is up on the device stay
    f2_augment_args slice(int b0) const {
        f2_augment_args G = *this;
        if (!rooms.dry()) G.rooms.room_of += b0;
        if (noise.level_of) G.noise.level_of += b0;
        if (!smear.sharp()) G.smear.mix_of += b0;
        if (!maskers.silent()) G.maskers.level_of += b0;
        if (!cutoffs.unfiltered()) G.cutoffs.cutoff_of += b0;
        G.noise.first_utterance += (uint32_t)b0, G.maskers.first_utterance += (uint32_t)b0;
        return G;
    }
};
// The windows of a call: centres and the utterance of every window (counted inside the batch), on the device already (on_device) or
// host arrays that go up behind the envelope launches, as in f2_input_batch
struct f2_window_list {
    const int64_t* centers;
    const int* win_utt;
    bool on_device;
    int64_t n_windows;
    int radius, step, normalize;
};
// f2_pipeline.hip, the driver f2_input_batch_smeared and f2_trainer_render_smeared share: the utterances of X (wave on the device,
// offsets from 0 on the host) through the stages of A (which passed f2_check_noise_pick and A.check) into ctx->levels, then
// f2_input_batch's envelopes and gather on that float64 buffer, the windows of W written to d_windows (device). Enqueues only; the
// gather ORs into word 0 of ctx->flags, which the caller clears before (f2_reset_flag) and reads after (f2_finish_positive: waits
// for the stream, F2_ERR_NONPOSITIVE for a window with a value <= 0 under normalisation).
int f2_launch_noisy_windows(f2_ctx* ctx, const f2_batch& X, const f2_window_list& W, const f2_augment_args& A, float* d_windows);
int f2_reset_flag(f2_ctx* ctx);
int f2_finish_positive(f2_ctx* ctx);
// f2_accuracy.hip, the kernel of f2_label_accuracy. d_counts (4 per utterance, zeroed by the caller)[4 u + 2 ref + pred] += rows
// of utterance u (rows d_window_offsets[u] .. [u + 1] of d_labels, row j at sample origin + j * hop) that the rule of the header
// counts against reference set u % R (d_ref_offsets: R + 1; timepoints strictly increasing inside a set, signs 0 / 1);
// max_rows: the most any utterance has
int f2_launch_label_accuracy(f2_ctx* ctx, const uint8_t* d_labels, const int64_t* d_window_offsets, int U, const int64_t* d_ref_offsets,
                             const int64_t* d_ref_timepoints, const uint8_t* d_ref_signs, int R, int64_t origin, int hop, int step,
                             int64_t max_rows, int64_t* d_counts);
// f2_segments.hip, the kernels of f2_decision_path / f2_decision_runs / f2_interval_tally / f2_eval_segments_batch. The plan of a
// call: set() takes the rows (host window_offsets, which must outlive the plan) and builds the tile table of F2_PATH_TILE rows;
// name_arrays() names the device arrays of the stages the call runs, name_bytes() whatever else the call keeps on the device (staged
// inputs, a host caller's outputs), reserve() places all of them in ctx->seg_ws, upload_tables() sends d_wo and d_first up.
struct f2_seg_plan {
    int U = 0;
    const int64_t* wo = nullptr;
    int64_t n_rows = 0, tiles = 0, max_rows = 0;
    std::vector<int64_t> first;   // U + 1 running sums of the utterances' tiles
    struct slot_at {
        void* slot;   // the T* to set
        size_t at;
    };
    std::vector<slot_at> slots;
    size_t bytes = 0;
    int64_t *d_wo = nullptr, *d_first = nullptr;
    int64_t *d_tprod = nullptr, *d_vin = nullptr, *d_value = nullptr;          // tile products (4 each), entering vectors (2 each), optima (U)
    uint8_t *d_tmap = nullptr, *d_xin = nullptr, *d_xlast = nullptr;           // tile maps, state of each tile's last row, of each utterance's
    int64_t *d_tcount = nullptr, *d_tqsum = nullptr, *d_ro = nullptr;          // tiles + 1 prefix sums of flags and of q, U + 1 run offsets
    int64_t *d_rstart = nullptr, *d_rsum = nullptr;                            // per run: first row in the batch, sum of q before it
    int64_t *d_ivo = nullptr, *d_ivb = nullptr;                                // R + 1 interval offsets, the bounds
    void set(const int64_t* window_offsets, int U);
    void name_arrays(bool want_path, bool want_runs, int64_t intervals, int R);
    void name_bytes(char** slot, size_t bytes);
    int reserve(f2_ctx* ctx);
    int upload_tables(f2_ctx* ctx) const;
};
// the argument errors of the three stages that do not depend on pointers: scale and penalty; the row count; the interval sets
// (*out_rows: the rows of the tally, (U / R) * iv_offsets[R])
int f2_check_decision_path(f2_ctx* ctx, double logit_scale, int64_t penalty);
int f2_check_segment_rows(f2_ctx* ctx, int64_t n_rows);
int f2_check_intervals(f2_ctx* ctx, int U, const int64_t* iv_offsets, const int64_t* iv_bounds, int R, int64_t origin, int hop,
                       int64_t max_rows, int64_t* out_rows);
// The launches, device pointers only, behind reserve() and upload_tables(). Path: d_q (n_rows) and S.d_value are written too.
// Runs: count fills S.d_ro; scatter writes at most most_runs rows of d_runs (the caller knows S.d_ro[U] <= most_runs). Tally: uploads
// the interval sets (host) and writes out_rows x 4.
int f2_launch_decision_path(f2_ctx* ctx, const f2_seg_plan& S, const float* d_scores, double logit_scale, int64_t penalty, uint8_t* d_path,
                            int32_t* d_q);
int f2_launch_runs_count(f2_ctx* ctx, const f2_seg_plan& S, const uint8_t* d_labels, const int32_t* d_q);
int f2_launch_runs_scatter(f2_ctx* ctx, const f2_seg_plan& S, const uint8_t* d_labels, const int32_t* d_q, int64_t most_runs, int64_t* d_runs);
int f2_launch_interval_tally(f2_ctx* ctx, const f2_seg_plan& S, const uint8_t* d_labels, const uint8_t* d_path, const int32_t* d_q,
                             const int64_t* iv_offsets, const int64_t* iv_bounds, int R, int64_t origin, int hop, int64_t out_rows,
                             int64_t* d_tally);
// f2_score.hip, the kernels of f2_cnn_score_windows. k_normalize_windows: n windows of `total` contiguous float32 values each,
// normalised with K3's arithmetic into d_out (may not alias d_in); a window with a value <= 0 or a NaN becomes zeros and ORs 1
// into *d_flag.
int f2_launch_normalize_windows(f2_ctx* ctx, const float* d_in, int64_t n, int total, float* d_out, int* d_flag);
// k_score_tally + k_score_loss_fold over m windows: d_counts (4 G, zeroed by the caller before the first launch of a call)
// [4 g + 2 sign + label] += windows, d_loss (G, likewise) [g] += the float64 loss terms in a fixed order; d_groups NULL: group 0.
// d_partial: room for f2_score_partial_doubles(m, G) values. A sign above 1 ORs 1, a group outside [0, G) ORs 2 into *d_flag.
int f2_launch_score_tally(f2_ctx* ctx, const float* d_scores, const uint8_t* d_labels, const uint8_t* d_signs, const int* d_groups,
                          int G, int64_t m, int64_t* d_counts, double* d_partial, double* d_loss, int* d_flag);
size_t f2_score_partial_doubles(int64_t max_windows, int G);
// f2_picture.hip, the kernels of f2_envelope_picture / f2_gammatonegram_batch. d_utt: 4 int64 per utterance {s_b, m_b, m_b / width,
// (m_b % width) << 8 | lg_b}, lg_b = f2_picture_lanes_log2(m_b, width) the log2 of the lanes per column; utterance b needs
// f2_picture_pool_blocks(C, width, lg_b) workgroups and every utterance gets blocks_per_utt, the largest of them. d_range: 2 words
// per utterance, preset to the bits of +inf and 0, left as the bits of the smallest and largest pixel > 0 (unchanged where there
// is none).
int f2_picture_lanes_log2(int64_t m, int width);
int64_t f2_picture_pool_blocks(int C, int width, int lg);
int f2_launch_picture_pool(f2_ctx* ctx, const double* d_env, const int64_t* d_offsets, const int64_t* d_utt, int B, int C, int width,
                           int pool, int64_t blocks_per_utt, double* d_pooled, uint64_t* d_range);
int f2_launch_picture_levels(f2_ctx* ctx, const double* d_pooled, const uint64_t* d_range, int B, int C, int width, uint8_t* d_levels);
// f2_track.hip, the kernel of f2_score_track / f2_eval_figure_batch. d_rec: 5 int64 per utterance {first row, rows, s_u, m_u, lg_u},
// lg_u = f2_track_lanes_log2(m_u, width, hop) the log2 of the lanes per column; utterance u needs f2_track_blocks(width, lg_u)
// workgroups and every utterance gets blocks_per_utt, the largest of them. d_track: (U, width, 5) float64.
int f2_track_lanes_log2(int64_t m, int width, int hop);
int64_t f2_track_blocks(int width, int lg);
int f2_launch_score_track(f2_ctx* ctx, const float* d_scores, const uint8_t* d_labels, const int64_t* d_rec, int U, int64_t origin,
                          int hop, int width, int64_t blocks_per_utt, double* d_track);
// f2_occlusion.hip, the kernels of f2_occlude_windows / f2_occlusion_map / f2_eval_occlusion_batch. d_x: n windows (R, C), d_out:
// (n, K + 1, R, C), neither needs more than element alignment; d_patches: K x {r0, r1, c0, c1}, inside the window (the caller checks).
// The map's d_rec, lanes and workgroups are those of f2_launch_score_track; d_scores (rows, K + 1, 2), d_labels (rows, K + 1),
// d_map (U, K, width, 4) float64.
int f2_launch_occlude_windows(f2_ctx* ctx, const float* d_x, int64_t n, int R, int C, const int32_t* d_patches, int K, float fill,
                              float* d_out);
int f2_launch_occlusion_map(f2_ctx* ctx, const float* d_scores, const uint8_t* d_labels, const int64_t* d_rec, int U, int K, int64_t origin,
                            int hop, int width, int64_t blocks_per_utt, double* d_map);
// f2_cnn_grad.hip, the kernels of f2_cnn_input_gradient / f2_saliency_map / f2_eval_saliency_batch. The gradient launch runs the
// recorded float32 forward and the backward-data chain over n windows at d_x in chunks of f2_cnn_grad_chunk windows through
// ctx->grad_ws (no other area of the context): d_grad (n, R, C) or NULL (the chain's own scratch), d_profile (n, C, 2) float64 or NULL,
// d_scores (n, 2) or NULL; with neither d_grad nor d_profile only the forward runs. Element alignment is enough for all four.
// The map's d_rec, lanes and workgroups are those of f2_launch_score_track; d_profile (rows, C, 2), d_map (U, C, width, 3) float64.
int64_t f2_cnn_grad_chunk(const f2_cnn* cnn);
// (f2_cnn_layers) the recorded forward's pooled conv4 output (m, flat) and dense1 output (m, 516) in ctx->grad_ws after a launch of
// m <= f2_cnn_grad_chunk windows, valid until the next gradient launch on the context
void f2_cnn_grad_recorded(const f2_ctx* ctx, const f2_cnn* cnn, int64_t m, const float** p2, const float** a5);
int f2_launch_cnn_input_gradient(f2_ctx* ctx, const f2_cnn* cnn, const float* d_x, int64_t n, float* d_grad, double* d_profile,
                                 float* d_scores);
int f2_launch_saliency_map(f2_ctx* ctx, const double* d_profile, const int64_t* d_rec, int U, int C, int64_t origin, int hop, int width,
                           int64_t blocks_per_utt, double* d_map);
// f2_resample.hip, the kernels of f2_resample_batch. F2_RESAMPLE_BLOCK outputs per workgroup, which stages at most
// F2_RESAMPLE_SPAN_MAX input frames (f2_resample_span: what (up, down, T) need, T = taps per phase).
// d_meta: 4 int64 per utterance {first input frame, frames, first output sample, output samples}, then B + 1 running sums of the
// workgroups ceil(output samples / F2_RESAMPLE_BLOCK) of the utterances. d_table: (up, T) float64, row p = the taps p + t * up
// in DESCENDING t (zero past the filter's end), so that a lane walks its row and its input frames upwards together.
#define F2_RESAMPLE_BLOCK 256
#define F2_RESAMPLE_SPAN_MAX 4096
int64_t f2_resample_span(int64_t up, int64_t down, int64_t T);
int f2_launch_resample(f2_ctx* ctx, const void* d_audio, int pcm_format, int channels, int channel, const int64_t* d_meta, int B,
                       int64_t total_blocks, int64_t up, int64_t down, int64_t half_len, int T, const double* d_table, double* d_out);
// up == down == 1: out[f] = frame f converted and mixed down, for the `frames` frames of the whole batch
int f2_launch_pcm_convert(f2_ctx* ctx, const void* d_audio, int pcm_format, int channels, int channel, int64_t frames, double* d_out);
size_t f2_cnn_flat_floats(const f2_cnn* cnn);    // floats per window of the conv4 output
size_t f2_cnn_dense_floats(const f2_cnn* cnn);   // ... plus dense1's output
