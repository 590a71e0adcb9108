// Kernels of f2_resample_batch (include/f2cnn_hip.h): interleaved PCM frames of a ragged batch to mono float64 samples in int16
// units at up / down times the rate.
//   k_resample     y[k] = sum_i x[i] taps[k down + half_len - i up], one lane per output sample, the input span of a workgroup
//                  converted and mixed down once, in LDS
//   k_pcm_convert  up == down == 1: the conversion and the mixdown alone
// gfx950, wave64. Everything that reaches memory is written by plain C++ stores.
#include "f2_internal.h"
#include "f2_tile_owner.h"

namespace {

constexpr int RT = F2_RESAMPLE_BLOCK;          // threads = outputs of a workgroup (4 waves)
constexpr int SPAN = F2_RESAMPLE_SPAN_MAX;     // input frames a workgroup can stage (32 KB of LDS)

// element type of a PCM format and its value in int16 units: every scaling is a power of two, every conversion exact
template <int FMT>
struct pcm;
template <>
struct pcm<F2_PCM_U8> {
    using type = uint8_t;
    static __device__ __forceinline__ double value(type v) { return (double)(((int)v - 128) * 256); }
};
template <>
struct pcm<F2_PCM_I16> {
    using type = int16_t;
    static __device__ __forceinline__ double value(type v) { return (double)v; }
};
template <>
struct pcm<F2_PCM_I32> {
    using type = int32_t;
    static __device__ __forceinline__ double value(type v) { return (double)v * (1.0 / 65536.0); }
};
template <>
struct pcm<F2_PCM_F32> {
    using type = float;
    static __device__ __forceinline__ double value(type v) { return (double)v * 32768.0; }
};
template <>
struct pcm<F2_PCM_F64> {
    using type = double;
    static __device__ __forceinline__ double value(type v) { return v * 32768.0; }
};

// Frame f of the interleaved audio as one float64: channel `channel`, or (((c0 + c1) + c2) + ...) / channels for channel < 0.
// Element loads only (1, 2, 4 or 8 bytes at their natural alignment): a row of frames starts wherever its offset puts it.
template <int FMT>
__device__ __forceinline__ double mono_frame(const typename pcm<FMT>::type* __restrict__ audio, int64_t f, int channels, int channel) {
    const typename pcm<FMT>::type* fr = audio + (size_t)f * (size_t)channels;
    if (channel >= 0) return pcm<FMT>::value(fr[channel]);
    double s = pcm<FMT>::value(fr[0]);
    for (int c = 1; c < channels; ++c) s += pcm<FMT>::value(fr[c]);
    return s / (double)channels;
}

// Workgroup blockIdx.x serves outputs k0 .. k0 + RT - 1 of the utterance that owns it (tile_owner over `first`: the running sums
// of the utterances' workgroups behind the 4 B records of `meta`).
// Output k reads x[i_hi - t] taps[p + t up], c = k down + half_len (64-bit), i_hi = c / up, p = c % up, t < T. The 64-bit division
// is made once per workgroup, for k0: c = c0 + j down for lane j, so i_hi = c0 / up + (c0 % up + j down) / up in 32 bits
// (up, down <= 2^22). The workgroup needs the frames i_lo = c0 / up - (T - 1) .. i_hi of its last lane: `span` <= SPAN of them
// (f2_resample_span, checked by the host), staged as float64, zero outside [0, n) - the zero padding of resample_poly.
// Lane j then adds xs[q + s] * row_p[s] for s = 0 .. T-1: ascending input index, the order of the header; row p of `table`
// holds the taps of phase p in descending t, zero past the filter's end.
template <int FMT>
__global__ __launch_bounds__(RT) void k_resample(const typename pcm<FMT>::type* __restrict__ audio, const int64_t* __restrict__ meta, int B,
                                                  int channels, int channel, unsigned up, unsigned down, int64_t half_len, int T,
                                                  const double* __restrict__ table, double* __restrict__ out) {
    __shared__ double xs[SPAN];
    const int tid = threadIdx.x;
    const int64_t* first = meta + 4 * (size_t)B;
    const int64_t blk = blockIdx.x;
    const int b = tile_owner(first, B, blk);
    const int64_t in0 = meta[4 * (size_t)b], n = meta[4 * (size_t)b + 1], out0 = meta[4 * (size_t)b + 2], n_out = meta[4 * (size_t)b + 3];
    const int64_t k0 = (blk - first[b]) * RT;
    const int nk = (int)min((int64_t)RT, n_out - k0);      // outputs of this workgroup, >= 1
    const int64_t c0 = k0 * (int64_t)down + half_len;
    const int64_t q0 = c0 / up;
    const unsigned r0 = (unsigned)(c0 % up);
    const int64_t i_lo = q0 - (T - 1);
    const int span = (int)((r0 + (unsigned)(nk - 1) * down) / up) + T;
    for (int j = tid; j < span; j += RT) {
        const int64_t i = i_lo + j;
        xs[j] = i >= 0 && i < n ? mono_frame<FMT>(audio, in0 + i, channels, channel) : 0.0;
    }
    __syncthreads();
    if (tid >= nk) return;
    const unsigned v = r0 + (unsigned)tid * down;
    const unsigned q = v / up, p = v % up;
    const double* __restrict__ row = table + (size_t)p * (size_t)T;
    const double* x = xs + q;
    double acc = 0.0;
#pragma unroll 4
    for (int s = 0; s < T; ++s) acc += x[s] * row[s];
    out[out0 + k0 + tid] = acc;
}

template <int FMT>
__global__ __launch_bounds__(RT) void k_pcm_convert(const typename pcm<FMT>::type* __restrict__ audio, int channels, int channel,
                                                     int64_t frames, double* __restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (f < frames) out[f] = mono_frame<FMT>(audio, f, channels, channel);
}

}  // namespace

int64_t f2_resample_span(int64_t up, int64_t down, int64_t T) { return (up - 1 + (F2_RESAMPLE_BLOCK - 1) * down) / up + T; }

#define F2_PCM_DISPATCH(fmt, CALL)                  \
    switch (fmt) {                                  \
        case F2_PCM_U8: CALL(F2_PCM_U8); break;     \
        case F2_PCM_I16: CALL(F2_PCM_I16); break;   \
        case F2_PCM_I32: CALL(F2_PCM_I32); break;   \
        case F2_PCM_F32: CALL(F2_PCM_F32); break;   \
        default: CALL(F2_PCM_F64); break;           \
    }

int f2_launch_resample(f2_ctx* ctx, const void* d_audio, int pcm_format, int channels, int channel, const int64_t* d_meta, int B,
                       int64_t total_blocks, int64_t up, int64_t down, int64_t half_len, int T, const double* d_table, double* d_out) {
    if (B <= 0 || total_blocks <= 0) return F2_OK;
    F2_TRY(f2_check_workgroups(ctx, total_blocks, "resampling", ""));
    const dim3 grid((unsigned)total_blocks);
#define F2_RS_CALL(F)                                                                                                              \
    k_resample<F><<<grid, dim3(RT), 0, ctx->stream>>>((const pcm<F>::type*)d_audio, d_meta, B, channels, channel, (unsigned)up, \
                                                       (unsigned)down, half_len, T, d_table, d_out)
    F2_PCM_DISPATCH(pcm_format, F2_RS_CALL)
#undef F2_RS_CALL
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

int f2_launch_pcm_convert(f2_ctx* ctx, const void* d_audio, int pcm_format, int channels, int channel, int64_t frames, double* d_out) {
    if (frames <= 0) return F2_OK;
    const int64_t blocks = (frames + RT - 1) / RT;
    F2_CHECK(ctx, blocks < (int64_t(1) << 31), F2_ERR_UNSUPPORTED, "%lld frames need too many workgroups", (long long)frames);
    const dim3 grid((unsigned)blocks);
#define F2_CV_CALL(F) \
    k_pcm_convert<F><<<grid, dim3(RT), 0, ctx->stream>>>((const pcm<F>::type*)d_audio, channels, channel, frames, d_out)
    F2_PCM_DISPATCH(pcm_format, F2_CV_CALL)
#undef F2_CV_CALL
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}
