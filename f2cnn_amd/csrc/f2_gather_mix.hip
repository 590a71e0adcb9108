// A ragged window gather that mixes the channels of the window's own columns (include/f2cnn_hip.h: f2_gather_windows_mixed; the
// last stage of f2_input_batch_smeared / f2_trainer_render_smeared).
//   k_gather_windows_mixed  out[e][k][c] = normalise( sum_{c'} mix[l][c][c'] env_b[c'][centre_e + step (k - radius)] ), b the
//                           utterance of window e and l = mix_of[b] its level. One workgroup of 256 threads per window, as
//                           k_gather_windows<true> (f2_gather.hip). The window's R x C float64 values are read from the envelopes
//                           once into LDS (`raw`), the mixed window is formed into a second LDS array (`win`, the layout of the
//                           output) and from there on the kernel is k_gather_windows: gather_window_tail (f2_gather_tail.h) is the
//                           tail of both. Level K is sharp: the values go to `win` as they are, or without normalisation straight
//                           to the output - what k_gather_windows<true> does.
// Only the R columns a window touches are mixed: the sweep's kernel (k_channel_mix_levels, f2_smear.hip) mixes every sample of
// every envelope, 26 times the arithmetic of the windows of a training corpus, into a second envelope buffer.
//
// Arithmetic contract, f2_channel_mix_levels' word for word: one float64 accumulator per output starting from +0.0, c' ascending,
// acc = fma(w, x, acc), the sum of an output never split across lanes, no atomics, a closing acc + 0.0. A thread walks the span of
// its channel's tile of F2_SMEAR_TILE_CHANNELS rows - the union of their supports, which f2_check_mix found on the host - and that
// can be wider than the support of its own row; outside it the row's weights are zero, and fma(0, x, acc) leaves acc as it is for
// finite x up to the sign of a zero, which the closing addition settles (f2_smear.hip's header). The bits of a mixed value so
// depend on its envelope column and its matrix row alone, and a window is the plain gather of that level of the sweep.
//
// Layout. A thread owns one output channel c and the rows k = g, g + G, ... of it (G = 256 / C row groups when C < 256, else one
// group and channels c, c + 256, ...), KA accumulators at a time: a weight is loaded once for KA rows. Threads of neighbouring c
// read neighbouring doubles of the transposed image wT[l][c'][c] (f2_smear_plan::wT) and the same raw[k][c'] - one LDS address for
// the 16 lanes of a tile, a broadcast. Lanes of one 32-lane half that sit in different row groups read rows k, k + 1, ... at the
// same c'; with a row pitch of C doubles and C a multiple of 32 those would fall on one bank (ds_read_b64: bank = dword address
// mod 64), so the pitch of `raw` is C | 1: rows j apart then lie 2 j (C | 1) mod 64 != 0 banks apart for every j < 32. `win` is
// dense: it is written once per output and read along idx by the tail.
// gfx950, wave64; plain vector stores only, no inline assembly.
#include "f2_internal.h"
#include "f2_gather_tail.h"

namespace {

constexpr int GT = 256;
constexpr int KA_MAX = 6;   // rows a thread accumulates at a time: 11 rows in two groups (C = 128) are one walk

// The rows kb, kb + G, ... (KA of them, clamped to the window for the reads and not stored beyond it) of channel c: one walk of
// the span lo .. hi - 1. w: wT of the level at column c, rows Cpad apart.
template <int KA>
__device__ __forceinline__ void mix_rows(const double* raw, int Cp, const double* __restrict__ w, int Cpad, int lo, int hi, int kb, int G,
                                         int R, int C, int c, double* win, double& mn, double& mx) {
    const double* r[KA];
    double acc[KA];
#pragma unroll
    for (int m = 0; m < KA; ++m) {
        const int k = kb + m * G;
        r[m] = raw + (size_t)(k < R ? k : R - 1) * (size_t)Cp;
        acc[m] = 0.0;
    }
#pragma unroll 4
    for (int cp = lo; cp < hi; ++cp) {
        const double wv = w[(size_t)cp * (size_t)Cpad];
#pragma unroll
        for (int m = 0; m < KA; ++m) acc[m] = fma(wv, r[m][cp], acc[m]);
    }
#pragma unroll
    for (int m = 0; m < KA; ++m) {
        const int k = kb + m * G;
        if (k < R) {
            const double v = acc[m] + 0.0;
            win[k * C + c] = v;
            mn = fmin(mn, v);
            mx = fmax(mx, v);
        }
    }
}

// mix_of: the level of every utterance, in [0, K]. wT: per level C rows of Cpad doubles, wT[l][c'][c] = mix[l][c][c'], zero for
// c >= C; spans[l * nct + ct] = lo | hi << 32, the input channels lo .. hi - 1 the channels of tile ct walk (f2_check_mix).
// Dynamic LDS: win (R * C doubles) | raw (R * (C | 1) doubles).
__global__ __launch_bounds__(GT) void k_gather_windows_mixed(const double* __restrict__ env, int C, const int64_t* __restrict__ centers,
                                                             int radius, int step, int normalize, float* __restrict__ out,
                                                             int* __restrict__ flag, const int64_t* __restrict__ offsets,
                                                             const int* __restrict__ win_utt, const int32_t* __restrict__ mix_of, int K,
                                                             const double* __restrict__ wT, int Cpad, int nct,
                                                             const int64_t* __restrict__ spans) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* win = reinterpret_cast<double*>(smem_raw);
    __shared__ double red_min[GT / 64], red_max[GT / 64];

    const int tid = threadIdx.x;
    const int64_t e = blockIdx.x;
    const int R = 2 * radius + 1;
    const int total = R * C;
    const int b = win_utt[e];
    const int64_t o0 = offsets[b];
    const int64_t N = offsets[b + 1] - o0;
    env += (size_t)C * (size_t)o0;
    const int64_t centre = centers[e];
    const int l = mix_of[b];
    float* o = out + (size_t)e * (size_t)total;

    double mn = INFINITY, mx = -INFINITY;
    if (l == K) {   // sharp: k_gather_windows<true>
        if (!normalize) {
            for (int idx = tid; idx < total; idx += GT) {
                const int k = idx / C, c = idx - k * C;
                o[idx] = (float)env[(size_t)c * (size_t)N + (size_t)(centre + (int64_t)step * (k - radius))];
            }
            return;
        }
        for (int idx = tid; idx < total; idx += GT) {
            const int k = idx / C, c = idx - k * C;
            const double v = env[(size_t)c * (size_t)N + (size_t)(centre + (int64_t)step * (k - radius))];
            win[idx] = v;
            mn = fmin(mn, v);
            mx = fmax(mx, v);
        }
    } else {
        const int Cp = C | 1;
        double* raw = win + total;
        for (int idx = tid; idx < total; idx += GT) {
            const int k = idx / C, c = idx - k * C;
            raw[k * Cp + c] = env[(size_t)c * (size_t)N + (size_t)(centre + (int64_t)step * (k - radius))];
        }
        __syncthreads();
        const int G = C < GT ? GT / C : 1;     // row groups
        const int g = tid / C;                 // (0 for C >= GT)
        const int per = (R + G - 1) / G;       // rows of a thread at most: which walk serves them is the workgroup's choice
        const double* __restrict__ wl = wT + (size_t)l * (size_t)C * (size_t)Cpad;
        const int64_t* __restrict__ sl = spans + (size_t)l * (size_t)nct;
        if (g < G)                             // (the last GT % C threads have no channel)
            for (int c = tid - g * C; c < C; c += GT) {
                const int64_t span = sl[c / F2_SMEAR_TILE_CHANNELS];
                const int lo = (int)(span & 0xffffffff), hi = (int)(span >> 32);
                const double* __restrict__ w = wl + c;
                if (per == 1) mix_rows<1>(raw, Cp, w, Cpad, lo, hi, g, G, R, C, c, win, mn, mx);
                else if (per == 2) mix_rows<2>(raw, Cp, w, Cpad, lo, hi, g, G, R, C, c, win, mn, mx);
                else if (per <= 4) mix_rows<4>(raw, Cp, w, Cpad, lo, hi, g, G, R, C, c, win, mn, mx);
                else
                    for (int kb = g; kb < R; kb += G * KA_MAX) mix_rows<KA_MAX>(raw, Cp, w, Cpad, lo, hi, kb, G, R, C, c, win, mn, mx);
            }
    }
    gather_window_tail<GT>(win, total, mn, mx, normalize, o, flag, red_min, red_max);
}

}  // namespace

size_t f2_gather_mixed_lds(int radius, int C) {
    const size_t R = 2 * (size_t)radius + 1;
    return sizeof(double) * R * ((size_t)C + (size_t)(C | 1));
}

int f2_check_mix_gather(f2_ctx* ctx, int B, int C, int radius, f2_mix_gather_args* S) {
    F2_CHECK(ctx, S->K >= 0, F2_ERR_INVALID, "negative number of mixing matrices (K=%d)", S->K);
    S->all_sharp = true;
    if (S->sharp()) return F2_OK;
    S->plan = std::make_shared<f2_smear_plan>();
    F2_TRY(f2_check_mix(ctx, S->mix, S->K, C, S->plan.get()));
    for (int b = 0; b < B; ++b) {
        F2_CHECK(ctx, S->mix_of[b] >= 0 && S->mix_of[b] <= S->K, F2_ERR_INVALID, "utterance %d: mixing level %d is outside [0, %d]", b,
                 (int)S->mix_of[b], S->K);
        if (S->mix_of[b] != S->K) S->all_sharp = false;
    }
    F2_CHECK(ctx, f2_gather_mixed_lds(radius, C) <= 150 * 1024, F2_ERR_UNSUPPORTED,
             "window of %d x %d values and its mixed copy do not fit in LDS", 2 * radius + 1, C);
    return F2_OK;
}

size_t f2_mix_image_bytes(const f2_smear_plan& P) { return sizeof(int64_t) * P.spans.size() + sizeof(double) * P.wT.size(); }

int f2_upload_mix_image(f2_ctx* ctx, const f2_smear_plan& P, void* d_image, const int64_t** d_spans, const double** d_wT) {
    int64_t* s = (int64_t*)d_image;
    double* w = (double*)(s + P.spans.size());
    F2_TRY(f2_upload_async(ctx, s, P.spans.data(), sizeof(int64_t) * P.spans.size()));
    F2_TRY(f2_upload_async(ctx, w, P.wT.data(), sizeof(double) * P.wT.size()));
    *d_spans = s, *d_wT = w;
    return F2_OK;
}

int f2_launch_gather_mixed(f2_ctx* ctx, const double* d_env, int C, const int64_t* d_offsets, const int64_t* d_centers, const int* d_win_utt,
                           int64_t n_windows, int radius, int step, int normalize, const f2_smear_plan& P, const int64_t* d_spans,
                           const double* d_wT, const int32_t* d_mix_of, float* d_out, int* d_flag) {
    if (n_windows <= 0) return F2_OK;
    const size_t lds = f2_gather_mixed_lds(radius, C);
    F2_CHECK(ctx, lds <= 150 * 1024, F2_ERR_UNSUPPORTED, "window of %d x %d values and its mixed copy do not fit in LDS", 2 * radius + 1, C);
    F2_CHECK(ctx, n_windows < (int64_t(1) << 31), F2_ERR_UNSUPPORTED, "too many windows (%lld)", (long long)n_windows);
    if (lds > 64 * 1024)
        F2_HIP(ctx, hipFuncSetAttribute((const void*)k_gather_windows_mixed, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    F2_TRY(f2_prof_begin(ctx, F2_K_GATHER));
    hipLaunchKernelGGL(k_gather_windows_mixed, dim3((unsigned)n_windows), dim3(GT), lds, ctx->stream, d_env, C, d_centers, radius, step,
                       normalize, d_out, d_flag, d_offsets, d_win_utt, d_mix_of, P.K, d_wT, P.Cpad, P.nct, d_spans);
    F2_HIP(ctx, hipGetLastError());
    F2_TRY(f2_prof_end(ctx, F2_K_GATHER));
    return F2_OK;
}
