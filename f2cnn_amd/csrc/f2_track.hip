// Kernel of f2_score_track / f2_eval_figure_batch (include/f2cnn_hip.h): the decisions of a strided evaluation reduced to the time
// columns of a picture.
//   k_score_track  track[u][x] = {rows, rising rows, mean, minimum, maximum of scores[j][1]} over the rows j of utterance u whose
//                  sample origin + j * hop lies in column x of the span - the columns of k_picture_pool (f2_picture.hip)
// gfx950, wave64. Everything that reaches memory is written by plain C++ stores.
#include "f2_internal.h"

namespace {

constexpr int TT = 256;          // threads of a workgroup (4 waves)
constexpr int AHEAD = 4;         // rows a lane loads before it adds them (long columns)

// One wave per run of 64 / G consecutive columns of one utterance, G = 2^lg lanes per column, G the smallest power of two that
// holds the most rows any column of the utterance can own (64 beyond: the lanes then stride through the column's rows, however
// many there are). Lane l works for column l / G of the run with row phase l % G, so the lanes of a wave read consecutive rows.
//   rows     j_hi - j_lo, the rows with lo_x <= origin + j hop < hi_x: j_lo = ceil((lo_x - origin) / hop), j_hi likewise from
//            hi_x, both kept inside [0, n_u]
//   mean     every lane adds (double)scores[j][1] of its own rows in index order, then a butterfly over the G lanes (lane ^ G/2,
//            ..., lane ^ 1) whose two operands are the same pair in both partners: the order is fixed by (n_u, span, origin, hop, W)
//            alone - no atomics, the same bits on every call. A NaN score makes the sum NaN.
//   rising   counted in float64 (integers below 2^53 add exactly in any order)
//   min/max  fminf / fmaxf drop NaNs, so a lane that meets one remembers it and the three values become NaN
// Workgroup blockIdx.x serves utterance blockIdx.x / bpu (bpu: the most workgroups any utterance of the call needs; the spare waves
// of the others leave at once): rec[5u .. 5u + 4] = {first row, n_u, s_u, m_u, lg_u}. m_u == 0: no column owns a row.
__global__ __launch_bounds__(TT) void k_score_track(const float* __restrict__ scores, const uint8_t* __restrict__ labels,
                                                     const int64_t* __restrict__ rec, int64_t origin, int64_t hop, int W, unsigned bpu,
                                                     double* __restrict__ track) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned u = blockIdx.x / bpu, local = blockIdx.x % bpu;
    const int64_t first = rec[5 * (size_t)u], n = rec[5 * (size_t)u + 1], s = rec[5 * (size_t)u + 2], m = rec[5 * (size_t)u + 3];
    const int lg = (int)rec[5 * (size_t)u + 4];
    const int G = 1 << lg, per = 64 >> lg;              // lanes per column, columns per run
    const int run = (int)(local * (TT / 64) + wv);
    if ((int64_t)run * per >= W) return;                // (the whole wave)
    const int sub = lane & (G - 1), x = run * per + (lane >> lg);
    const bool has = x < W;

    int64_t j_lo = 0, j_hi = 0;
    if (has && m > 0) {
        // floor(x m / W) = x q + floor(x r / W) with m = q W + r: x, r < 2^16 + 1, the products stay far inside 64 bits
        const int64_t q = m / W, r = m % W;
        const int64_t lo = s + (int64_t)x * q + (int64_t)x * r / W;
        int64_t hi = s + (int64_t)(x + 1) * q + (int64_t)(x + 1) * r / W;
        if (hi == lo) hi = lo + 1;
        j_lo = lo <= origin ? 0 : min(n, (lo - origin - 1) / hop + 1);        // (ceil of a positive value, without a sum that
        j_hi = hi <= origin ? 0 : min(n, (hi - origin - 1) / hop + 1);        //  could leave int64)
    }

    const float* p = scores + 2 * (size_t)first + 1;
    const uint8_t* lab = labels + (size_t)first;
    double sum = 0.0, rising = 0.0;
    float vmin = INFINITY, vmax = -INFINITY;
    int nan = 0;
    int64_t j = j_lo + sub;
    for (; j + (int64_t)(AHEAD - 1) * G < j_hi; j += (int64_t)AHEAD * G) {     // AHEAD independent loads, added in index order
        float v[AHEAD];
        uint8_t l[AHEAD];
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) {
            v[k] = p[2 * (size_t)(j + (int64_t)k * G)];
            l[k] = lab[(size_t)(j + (int64_t)k * G)];
        }
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) {
            sum += (double)v[k];
            rising += l[k] != 0 ? 1.0 : 0.0;
            nan |= v[k] != v[k];
            vmin = fminf(vmin, v[k]);
            vmax = fmaxf(vmax, v[k]);
        }
    }
    for (; j < j_hi; j += G) {
        const float v = p[2 * (size_t)j];
        sum += (double)v;
        rising += lab[(size_t)j] != 0 ? 1.0 : 0.0;
        nan |= v != v;
        vmin = fminf(vmin, v);
        vmax = fmaxf(vmax, v);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        if (d >= G) continue;      // (uniform: G belongs to the utterance)
        sum += __shfl_xor(sum, d);
        rising += __shfl_xor(rising, d);
        nan |= __shfl_xor(nan, d);
        vmin = fminf(vmin, __shfl_xor(vmin, d));
        vmax = fmaxf(vmax, __shfl_xor(vmax, d));
    }
    if (has && sub == 0) {
        const int64_t rows = j_hi - j_lo;
        double* t = track + ((size_t)u * (size_t)W + (size_t)x) * 5;
        const double none = (double)NAN;
        t[0] = (double)rows;
        t[1] = rising;
        t[2] = rows > 0 ? sum / (double)rows : none;
        t[3] = rows > 0 && !nan ? (double)vmin : none;
        t[4] = rows > 0 && !nan ? (double)vmax : none;
    }
}

}  // namespace

int f2_track_lanes_log2(int64_t m, int width, int hop) {
    const int64_t bin = m > width ? (m + width - 1) / width : 1;   // the longest column in samples ...
    const int64_t longest = (bin + hop - 1) / hop;                 // ... owns at most this many rows
    int lg = 0;
    while (lg < 6 && (int64_t(1) << lg) < longest) ++lg;
    return lg;
}

int64_t f2_track_blocks(int width, int lg) {
    const int per = 64 >> lg;
    const int64_t runs = (width + per - 1) / per;
    return (runs + TT / 64 - 1) / (TT / 64);
}

int f2_launch_score_track(f2_ctx* ctx, const float* d_scores, const uint8_t* d_labels, const int64_t* d_rec, int U, int64_t origin,
                          int hop, int width, int64_t blocks_per_utt, double* d_track) {
    if (U <= 0 || blocks_per_utt <= 0) return F2_OK;
    F2_CHECK(ctx, blocks_per_utt * U < (int64_t(1) << 31), F2_ERR_UNSUPPORTED, "track of %d x %d columns needs too many workgroups", U, width);
    k_score_track<<<dim3((unsigned)(blocks_per_utt * U)), dim3(TT), 0, ctx->stream>>>(d_scores, d_labels, d_rec, origin, (int64_t)hop, width,
                                                                                     (unsigned)blocks_per_utt, d_track);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}
