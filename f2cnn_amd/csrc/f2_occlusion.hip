// Kernels of f2_occlude_windows / f2_occlusion_map / f2_eval_occlusion_batch (include/f2cnn_hip.h): the occlusion map of a strided
// evaluation - which channel bands of its input the network's decisions rest on.
//   k_occlude_windows  n windows (R, C) -> n * L windows, window-major (n, L, R, C): level 0 the window, level k + 1 the window with
//                      patch k = [r0, r1) x [c0, c1) replaced by `fill`
//   k_occlusion_map    map[u][k][x] = {rows, flipped rows, mean d, mean |d|} of d_j = scores[j][k + 1][1] - scores[j][0][1] over the
//                      rows j of utterance u that column x owns - the columns and the lane scheme of k_score_track (f2_track.hip)
// gfx950, wave64. Everything that reaches memory is written by plain C++ stores.
#include "f2_internal.h"

namespace {

constexpr int TO = 256;          // threads of a k_occlude_windows workgroup
constexpr int LEVEL_GROUP = 32;  // levels one workgroup writes from the words it holds in registers (at most)
constexpr int TT = 256;          // threads of a k_occlusion_map workgroup (4 waves): f2_track_blocks counts with this size
constexpr int AHEAD = 4;         // rows a lane loads before it adds them (long columns)

// The windows move as bit patterns (a NaN payload in x or in `fill` survives): one 32-bit word per element, four where the pointers
// and C allow 16-byte accesses (C % 4 == 0: the four elements share a row, every window starts on a 16-byte boundary).
template <int VEC>
struct occ_word;
template <>
struct occ_word<1> {
    using type = uint32_t;
    static __device__ __forceinline__ type blank(type v, bool row, int c, int c0, int c1, uint32_t fill) {
        return row && c >= c0 && c < c1 ? fill : v;
    }
};
template <>
struct occ_word<4> {
    using type = uint4;
    static __device__ __forceinline__ type blank(type v, bool row, int c, int c0, int c1, uint32_t fill) {
        v.x = row && c >= c0 && c < c1 ? fill : v.x;
        v.y = row && c + 1 >= c0 && c + 1 < c1 ? fill : v.y;
        v.z = row && c + 2 >= c0 && c + 2 < c1 ? fill : v.z;
        v.w = row && c + 3 >= c0 && c + 3 < c1 ? fill : v.w;
        return v;
    }
};

// The n * SV words (SV = R C / VEC per window) of x are dealt to the workgroups in runs of TO, window boundaries ignored: every lane
// loads one word, finds its window, row and column, and stores it to the levels [l0, l1) of blockIdx.y, blanked where the level's
// patch covers it. The source is read from HBM by the first level group that comes to it and from L2 by the others (L <= LEVEL_GROUP:
// there is one group, every level is served from the register). The patch of a level is the same for the whole workgroup: the
// table is read through the scalar cache.
template <int VEC>
__global__ __launch_bounds__(TO) void k_occlude_windows(const uint32_t* __restrict__ x, int64_t n, int C, int SV,
                                                         const int32_t* __restrict__ patches, int L, int lper, uint32_t fill,
                                                         uint32_t* __restrict__ out) {
    using W = typename occ_word<VEC>::type;
    const W* src = reinterpret_cast<const W*>(x);
    W* dst = reinterpret_cast<W*>(out);
    const int64_t total = n * (int64_t)SV;
    const int l0 = (int)blockIdx.y * lper, l1 = min(L, l0 + lper);
    for (int64_t e0 = (int64_t)blockIdx.x * TO; e0 < total; e0 += (int64_t)gridDim.x * TO) {
        if (e0 + (int64_t)threadIdx.x >= total) continue;
        const int64_t w0 = e0 / SV;                                    // (uniform)
        const unsigned t = (unsigned)(e0 - w0 * SV) + threadIdx.x;     // < SV + TO
        const int64_t w = w0 + t / (unsigned)SV;
        const unsigned i = t % (unsigned)SV;
        const W v = src[e0 + (int64_t)threadIdx.x];
        const unsigned el = i * VEC;                                   // < R C
        const int r = (int)(el / (unsigned)C), c = (int)(el % (unsigned)C);
        W* o = dst + ((size_t)w * (size_t)L + (size_t)l0) * (size_t)SV + i;
        for (int l = l0; l < l1; ++l, o += SV) {
            W y = v;
            if (l > 0) {
                const int32_t* p = patches + 4 * (size_t)(l - 1);
                const int r0 = p[0], r1 = p[1], c0 = p[2], c1 = p[3];
                y = occ_word<VEC>::blank(v, r >= r0 && r < r1, c, c0, c1, fill);
            }
            *o = y;
        }
    }
}

// One wave per run of 64 / G consecutive columns of one utterance and one patch (blockIdx.y), G = 2^lg lanes per column: the column
// ownership rule, the records rec[5u .. 5u + 4] = {first row, n_u, s_u, m_u, lg_u} and the workgroup numbering are k_score_track's
// (f2_track.hip), so that f2_track_lanes_log2 / f2_track_blocks size this launch too.
//   rows     j_hi - j_lo, the rows with lo_x <= origin + j hop < hi_x
//   mean d   every lane adds d_j = (double)scores[j][k + 1][1] - (double)scores[j][0][1] of its own rows in index order, then a
//            butterfly over the G lanes (lane ^ G/2, ..., lane ^ 1) whose two operands are the same pair in both partners: the order
//            is fixed by (n_u, span, origin, hop, W) alone - no atomics, the same bits on every call. |d_j| likewise. A NaN score
//            makes both sums NaN.
//   flips    counted in float64 (integers below 2^53 add exactly in any order)
// Row j of the utterance is row first + j of the (rows, L, 2) scores and the (rows, L) labels.
__global__ __launch_bounds__(TT) void k_occlusion_map(const float* __restrict__ scores, const uint8_t* __restrict__ labels,
                                                       const int64_t* __restrict__ rec, int64_t origin, int64_t hop, int W, unsigned bpu,
                                                       int L, double* __restrict__ map) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned u = blockIdx.x / bpu, local = blockIdx.x % bpu;
    const unsigned k = blockIdx.y, K = gridDim.y;
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

    const size_t pitch = 2 * (size_t)L, lev = 2 * ((size_t)k + 1);
    const float* p = scores + pitch * (size_t)first + 1;
    const uint8_t* lab = labels + (size_t)L * (size_t)first;
    double sum = 0.0, sum_abs = 0.0, flips = 0.0;
    int64_t j = j_lo + sub;
    for (; j + (int64_t)(AHEAD - 1) * G < j_hi; j += (int64_t)AHEAD * G) {     // AHEAD independent loads, added in index order
        float a[AHEAD], b[AHEAD];
        uint8_t la[AHEAD], lb[AHEAD];
#pragma unroll
        for (int q = 0; q < AHEAD; ++q) {
            const size_t row = (size_t)(j + (int64_t)q * G);
            a[q] = p[pitch * row];
            b[q] = p[pitch * row + lev];
            la[q] = lab[(size_t)L * row];
            lb[q] = lab[(size_t)L * row + k + 1];
        }
#pragma unroll
        for (int q = 0; q < AHEAD; ++q) {
            const double d = (double)b[q] - (double)a[q];
            sum += d;
            sum_abs += fabs(d);
            flips += (lb[q] != 0) != (la[q] != 0) ? 1.0 : 0.0;
        }
    }
    for (; j < j_hi; j += G) {
        const double d = (double)p[pitch * (size_t)j + lev] - (double)p[pitch * (size_t)j];
        sum += d;
        sum_abs += fabs(d);
        flips += (lab[(size_t)L * (size_t)j + k + 1] != 0) != (lab[(size_t)L * (size_t)j] != 0) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        if (d >= G) continue;      // (uniform: G belongs to the utterance)
        sum += __shfl_xor(sum, d);
        sum_abs += __shfl_xor(sum_abs, d);
        flips += __shfl_xor(flips, d);
    }
    if (has && sub == 0) {
        const int64_t rows = j_hi - j_lo;
        double* t = map + (((size_t)u * K + k) * (size_t)W + (size_t)x) * 4;
        const double none = (double)NAN;
        t[0] = (double)rows;
        t[1] = flips;
        t[2] = rows > 0 ? sum / (double)rows : none;
        t[3] = rows > 0 ? sum_abs / (double)rows : none;
    }
}

}  // namespace

int f2_launch_occlude_windows(f2_ctx* ctx, const float* d_x, int64_t n, int R, int C, const int32_t* d_patches, int K, float fill,
                              float* d_out) {
    if (n <= 0 || R <= 0 || C <= 0) return F2_OK;
    const int L = K + 1;
    const bool vec = (((uintptr_t)d_x | (uintptr_t)d_out) & 15) == 0 && C % 4 == 0;
    const int SV = R * C / (vec ? 4 : 1);
    const int groups = (L + LEVEL_GROUP - 1) / LEVEL_GROUP, lper = (L + groups - 1) / groups;
    const int64_t want = (n * (int64_t)SV + TO - 1) / TO;
    const int64_t cap = (int64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 64;
    const dim3 grid((unsigned)(want < cap ? want : cap), (unsigned)groups);
    uint32_t fill_bits;
    memcpy(&fill_bits, &fill, sizeof(fill_bits));
    if (vec)
        k_occlude_windows<4><<<grid, dim3(TO), 0, ctx->stream>>>((const uint32_t*)d_x, n, C, SV, d_patches, L, lper, fill_bits, (uint32_t*)d_out);
    else
        k_occlude_windows<1><<<grid, dim3(TO), 0, ctx->stream>>>((const uint32_t*)d_x, n, C, SV, d_patches, L, lper, fill_bits, (uint32_t*)d_out);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

int f2_launch_occlusion_map(f2_ctx* ctx, const float* d_scores, const uint8_t* d_labels, const int64_t* d_rec, int U, int K, int64_t origin,
                            int hop, int width, int64_t blocks_per_utt, double* d_map) {
    if (U <= 0 || K <= 0 || blocks_per_utt <= 0) return F2_OK;
    F2_CHECK(ctx, blocks_per_utt * U < (int64_t(1) << 31), F2_ERR_UNSUPPORTED, "map of %d x %d columns needs too many workgroups", U, width);
    k_occlusion_map<<<dim3((unsigned)(blocks_per_utt * U), (unsigned)K), dim3(TT), 0, ctx->stream>>>(
        d_scores, d_labels, d_rec, origin, (int64_t)hop, width, (unsigned)blocks_per_utt, K + 1, d_map);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}
