// The direct-form FIR tile walk of k_reverb_levels / k_reverb_pick (f2_reverb.hip) and k_shaped_noise_levels (f2_noise_shaped.hip):
// a workgroup of FT_NT lanes makes FT_BLOCK consecutive outputs, lane L the FT_R outputs from 4 L on, from a span of float64 values
// the kernel has staged in LDS. What is staged - samples with zeros outside the utterance, or Philox deviates - and whether the taps
// come in chunks is the kernel's business; the image of the span and the walk over it are here, once.
// Arithmetic contract of include/f2cnn_hip.h: one float64 accumulator per output, taps in ascending t, acc = fma(h[t], x, acc).
#pragma once

constexpr int FT_NT = 256;                  // threads of a workgroup
constexpr int FT_R = 4;                     // consecutive outputs of a lane
constexpr int FT_BLOCK = FT_NT * FT_R;      // outputs of a workgroup
static_assert(FT_R == 4, "ft_at and the unrolled window below are written for four outputs per lane");

// LDS image of a span: value j at plane j % FT_R, place j / FT_R, the planes PLANE doubles apart (the kernel's: the places of its
// longest span and one more). The odd pitch keeps the compiler from pairing the four reads of a step into ds_read2st64_b64, which
// the LDS serves at a quarter of the rate of single ds_read_b64.
// Value j of the span. Lane L reads j = const - 4 L at every tap: with the values of equal j % 4 side by side the lanes of a wave
// read consecutive doubles (conflict-free ds_read_b64) although each owns four consecutive outputs.
template <int PLANE>
__device__ __forceinline__ int ft_at(int j) {
    return (j & (FT_R - 1)) * PLANE + (j >> 2);
}

// The walk of taps h[0 .. ns) over the staged span xs for the lane whose first output sits at xs[base + o] (base a multiple of
// FT_R, o = FT_R * lane): a_c = fma(h[s], xs[base + o + c - s], a_c) for s ascending, c < 4. The lane slides a register window of
// its four outputs over the span - one 8-byte LDS read and four FMAs per tap, the tap itself a wave-uniform load from global
// memory. No tap at or beyond ns is read; base + o - (ns rounded up to FT_R) >= 0 is the caller's to see to.
template <int PLANE>
__device__ __forceinline__ void ft_walk(const double* __restrict__ xs, int base, int o, const double* __restrict__ h, int ns, double& a0,
                                        double& a1, double& a2, double& a3) {
    // window at tap s: w_c = xs[base + o + c - s]
    double w0 = xs[ft_at<PLANE>(base + o)], w1 = xs[ft_at<PLANE>(base + o + 1)], w2 = xs[ft_at<PLANE>(base + o + 2)],
           w3 = xs[ft_at<PLANE>(base + o + 3)];
    // value base + o - s - 1 enters at the bottom after tap s: plane (3 - s) & 3, place (base + o) / 4 - 1 - s / 4
    // Four taps from tap s (a multiple of four) with the four values that enter at place q
    auto step4 = [&](int s, int q) {
        const double h0 = h[s], h1 = h[s + 1], h2 = h[s + 2], h3 = h[s + 3];
        const double n3 = xs[q + 3 * PLANE], n2 = xs[q + 2 * PLANE], n1 = xs[q + PLANE], n0 = xs[q];
        a0 = fma(h0, w0, a0), a1 = fma(h0, w1, a1), a2 = fma(h0, w2, a2), a3 = fma(h0, w3, a3);
        a0 = fma(h1, n3, a0), a1 = fma(h1, w0, a1), a2 = fma(h1, w1, a2), a3 = fma(h1, w2, a3);
        a0 = fma(h2, n2, a0), a1 = fma(h2, n3, a1), a2 = fma(h2, w0, a2), a3 = fma(h2, w1, a3);
        a0 = fma(h3, n1, a0), a1 = fma(h3, n2, a1), a2 = fma(h3, n3, a2), a3 = fma(h3, w0, a3);
        w3 = n3, w2 = n2, w1 = n1, w0 = n0;
    };
    // Two steps per turn, so that the window comes back to its registers without moves. The second step's place goes through an
    // address register of its own that the compiler cannot relate to the first (the empty asm): it would pair reads 8 bytes apart
    // into ds_read2_b64, a quarter of the rate again.
    int qa = (base + o) / FT_R - 1, qb = qa - 1;
    asm volatile("" : "+v"(qb));
    int s = 0;
    for (; s + 2 * FT_R <= ns; s += 2 * FT_R, qa -= 2, qb -= 2) {
        step4(s, qa);
        step4(s + FT_R, qb);
    }
    if (s + FT_R <= ns) {
        step4(s, qa);
        s += FT_R;
    }
    for (; s < ns; ++s) {                                    // the last taps of a table that is no multiple of four
        const double hs = h[s];
        a0 = fma(hs, w0, a0), a1 = fma(hs, w1, a1), a2 = fma(hs, w2, a2), a3 = fma(hs, w3, a3);
        w3 = w2, w2 = w1, w1 = w0, w0 = xs[ft_at<PLANE>(base + o - s - 1)];
    }
}

// The level that adds nothing: outputs o .. o + 3 below nk of the tile at k0 are the samples themselves (y: at the tile's first output)
template <typename T>
__device__ __forceinline__ void ft_copy(const T* __restrict__ x, int64_t k0, double* __restrict__ y, int o, int nk) {
#pragma unroll
    for (int c = 0; c < FT_R; ++c)
        if (o + c < nk) y[o + c] = (double)x[k0 + o + c];
}

// ... and the lane's four sums, those below nk
__device__ __forceinline__ void ft_store(double* __restrict__ y, int o, int nk, double a0, double a1, double a2, double a3) {
    if (o < nk) y[o] = a0;
    if (o + 1 < nk) y[o + 1] = a1;
    if (o + 2 < nk) y[o + 2] = a2;
    if (o + 3 < nk) y[o + 3] = a3;
}
