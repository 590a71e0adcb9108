// K2 -- Hilbert-magnitude envelope + optional first-order Butterworth low-pass
// (reference: scripts/processing/EnvelopeExtraction.py:20-67 paddedHilbert / lowPassFilter /
// ExtractEnvelopeFromMatrix).
//
// One workgroup (256, 512 or 1024 threads: 16 points per thread for the benchmark sizes) owns one (utterance,
// channel) row of n samples, zero-padded to M = 2^ceil(log2 n) exactly as the reference does, and keeps the whole
// transform on chip:
//
//   1. the real row is read as H = M/2 complex points  z[m] = x[2m] + i x[2m+1]  (16-byte loads of float64 rows, or
//      8-byte loads of the filterbank kernel's float32 hand-off) straight into the registers of the first FFT pass;
//      float transforms keep their x values in registers for step 5
//   2. Z = FFT_H(z): Stockham passes with a symmetric radix plan (first radix = last radix; 16-8-4-16 for H = 8192,
//      f2_fft_lds.h); data moves registers -> LDS -> registers -> ..., every pass holds its inputs in registers across
//      the barrier so the transform is in place. Twiddles of passes >= 1 are copied to LDS once per workgroup; a
//      radix-16 first pass derives its 15 per-butterfly twiddles from two loaded ones
//   3. the Hilbert transform h = H[x] is real, so its packed spectrum follows from Z by one pass over the
//      pairs (k, H-k):  W[k] = i sin(t_k) Z[k] + cos(t_k) conj(Z[H-k]),  t_k = 2 pi k / M,  W[0] = 0
//      (derivation in DESIGN.md); scipy.signal.hilbert's analytic signal is x + i h
//   4. w = IFFT_H(W), run as conj(FFT(conj W)) (only squares of w are used); because first and last radix
//      are equal, the last pass leaves in each thread exactly the points it loaded in step 1:
//      h[2m] = Re w[m], h[2m+1] = Im w[m]
//   5. env[n] = sqrt(x[n]^2 + h[n]^2) from registers; without low-pass it is stored at once (16-byte stores). With
//      low-pass, y[n] = b0 (env[n] + env[n-1]) - a1 y[n-1] runs time-parallel in the register layout the FFT left
//      (lowpass_pairs_store, f2_envelope_core.h: pair -> DPP wave scan -> wave totals -> block chain) and the
//      outputs leave as 16-byte stores; rows whose first pass does not give every thread whole butterflies (small H)
//      go through LDS instead: contiguous chunk per thread, zero-state run, multiplicative scan of the chunk ends,
//      second run, with the envelope TRANSPOSED in LDS (sample t*L+j at j*(NT+1)+t) so sweeps and copy-out are
//      conflict free.
//
// Two real FFTs of length M cost two complex FFTs of length M/2 on 8-byte (f32) points: 64 KiB (+pad) of
// LDS for the 1 s / 16 kHz row of the benchmark, two workgroups per CU.
// Bound: HBM, 12-16 bytes per sample-channel (4 or 8 read + 8 written). Rows that do not fit in LDS: f2_envelope_split.hip
// (four-step transform), f2_envelope_large.hip (global-memory passes).
//
// This header is the one text of that row. Included inside the anonymous namespace of a translation unit, after
// f2_fft_lds.h, it gives
//   - f2_envelope.hip: the kernel k_envelope<F, LOG2H, P13>, one workgroup per row, u and c from blockIdx.x
//     (P13: passes of the H = 8192 plan, f2_fft_lds.h; the launcher instantiates <F, 13, 3> beside the defaults);
//   - f2_envelope_flagged.hip, which defines F2_ENVELOPE_ROW_IS_FUNCTION first: the device function
//     envelope_row<F, LOG2H, P13>(P, tw, u, c) and the kernel k_envelope_flagged that walks the channels of a flagged
//     utterance with it.
// The switch changes the signature and where u and c come from, nothing else. The body is not a device function that both
// kernels call: the row kernels sit at their register limit and the allocator's result depends on the function's exit
// structure (figures in DESIGN.md, K2 section).
#pragma once

template <typename F, int LOG2H, int P13 = 4>
#ifdef F2_ENVELOPE_ROW_IS_FUNCTION
__device__ __forceinline__ void envelope_row(const EnvParams& P, const cpx<F>* __restrict__ tw, const int u, const int c) {
#else
__global__ __launch_bounds__((threads_for<F, LOG2H>()), (min_waves_for<F, LOG2H>())) void k_envelope(EnvParams P, const cpx<F>* __restrict__ tw) {
#endif
    constexpr int NT = threads_for<F, LOG2H>();
    constexpr int H = 1 << LOG2H;
    constexpr int M = 2 * H;
    constexpr int CS = cpad_size(H);
    constexpr int L = M >= NT ? M / NT : 1;   // samples per thread in the low-pass (contiguous chunk)
    constexpr int TP = NT + 1;                // row pitch of the transposed envelope image
    constexpr int RS = L * TP;
    constexpr int LDS_BYTES = (CS * 2 > RS ? CS * 2 : RS) * (int)sizeof(F);
    // register shape of the first/last pass
    constexpr int R0 = 1 << plan_bits(LOG2H, 0, P13);
    constexpr int NB0 = H / R0;
    constexpr int ITER0 = (NB0 + NT - 1) / NT;
    constexpr int PT = plan_points_per_thread(LOG2H, NT, P13);   // complex points per thread (all passes)
    constexpr bool KEEP_X = sizeof(F) == 4 && 2 * ITER0 * R0 <= 64;   // x stays in registers for step 5
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];
    __shared__ double wave_tot[NT / 64];
    __shared__ F qpow[L];   // (-a1)^(j+1), j < L
    constexpr int TWL = plan_tw_lds_count(LOG2H, P13);
    __shared__ __attribute__((aligned(16))) cpx<F> twl[TWL > 0 ? TWL : 1];   // twiddles of passes >= 1
    cpx<F>* lds = reinterpret_cast<cpx<F>*>(smem);
    F* rl = reinterpret_cast<F*>(smem);
    const cpx<F>* __restrict__ V = tw + plan_tw_total(LOG2H, P13);   // exp(-2 pi i k / M), k <= H/2

    const int tid = threadIdx.x;
#ifndef F2_ENVELOPE_ROW_IS_FUNCTION
    const int u = blockIdx.x / P.C;
    const int c = blockIdx.x - u * P.C;
#endif
    const int b = P.ulist ? P.ulist[u] : u;
    if (P.uflag && !P.uflag[b]) return;   // (whole workgroup) this utterance was served by the spectral kernel
    const int64_t off = P.offsets[b];
    const int n = (int)(P.offsets[b + 1] - off);
    const size_t row = (size_t)P.C * (size_t)off + (size_t)c * (size_t)n;
    const double* __restrict__ x = P.gfb + row;
    double* __restrict__ y = P.env + row;

    F2_STAMP_ARRAY(st, 10);   // (-DF2_STAMPS: phase boundaries, tools/k2_stamps.py)
    F2_STAMP(st, 0);
    // (visible to every wave after the first pass's barrier; pass 0 never reads it)
    for (int i = tid; i < TWL; i += NT) twl[i] = tw[plan_tw_offset(LOG2H, 1, P13) + i];
    // 1. load: point (i, j) of this thread is m = tid + i*NT + j*NB0
    constexpr bool FULL0 = NB0 % NT == 0;
    cpx<F> v[PT];
    [[maybe_unused]] F xr[KEEP_X ? ITER0 * R0 : 1], xi[KEEP_X ? ITER0 * R0 : 1];
    // branch-free inside each variant (clamped address + select) so that all loads are in flight together
    auto load_row = [&](auto* __restrict__ xs, auto odd) {
#pragma unroll
        for (int i = 0; i < ITER0; ++i) {
            const int bf = tid + i * NT;
            if (FULL0 || bf < NB0) {
#pragma unroll
                for (int j = 0; j < R0; ++j) {
                    F a, bb;
                    row_pair<decltype(odd)::value>(xs, n, 2 * (bf + j * NB0), a, bb);
                    v[i * R0 + j] = {a, bb};
                    if constexpr (KEEP_X) {
                        xr[i * R0 + j] = a;
                        xi[i * R0 + j] = bb;
                    }
                }
            }
        }
    };
    if (n < 2) {
        // a one-sample row: M = 1, no pair to load
        const F a = (KEEP_X && P.f32_in) ? (F) reinterpret_cast<const float*>(x)[0] : (F)x[0];
#pragma unroll
        for (int q = 0; q < ITER0 * R0; ++q) {
            v[q] = {F(0), F(0)};
            if constexpr (KEEP_X) xr[q] = xi[q] = F(0);
        }
        if (tid == 0) {
            v[0] = {a, F(0)};
            if constexpr (KEEP_X) xr[0] = a;
        }
    } else if (KEEP_X && P.f32_in) {
        // float32 hand-off from the filterbank kernel: the row's samples sit at the start of its float64 slot
        const float* __restrict__ xf = reinterpret_cast<const float*>(x);
        if ((n & 1) == 0) load_row(xf, std::false_type{});
        else load_row(xf, std::true_type{});
    } else {
        if ((n & 1) == 0) load_row(x, std::false_type{});
        else load_row(x, std::true_type{});
    }
    F2_STAMP(st, 1);
    // 2. forward transform (first pass straight from the registers)
    constexpr bool T0R = derive_tw0<F, LOG2H>();
    fft_all<F, LOG2H, false, PT, NT, T0R, 0, P13>(lds, tw, twl, tid, v);
    F2_STAMP(st, 2);
    // 3. packed spectrum of the Hilbert transform, conjugated and scaled by 1/H for step 4:
    //    W[k] = i sin(t_k) Z[k] + cos(t_k) conj(Z[H-k]), W[0] = 0. Either folded into the first pass of
    //    step 4 (fuse_hilbert) or one sweep over the pairs (k, H-k) here, all loads issued up front.
    if constexpr (LOG2H >= 1 && !fuse_hilbert<F, LOG2H>()) {
        constexpr int NPAIR = H / 2 - 1;                       // pairs (k, H-k), 1 <= k < H/2
        constexpr int ITERP = (NPAIR + NT - 1) / NT;
        const F sc = F(1.0 / H);
        if constexpr (NPAIR > 0) {
            cpx<F> zk[ITERP], zh[ITERP], vk[ITERP];
#pragma unroll
            for (int i = 0; i < ITERP; ++i) {
                const int k = min(1 + tid + i * NT, H / 2 - 1);
                zk[i] = lds[cpad(k)];
                zh[i] = lds[cpad(H - k)];
                vk[i] = V[k];                                   // (cos t, -sin t)
            }
#pragma unroll
            for (int i = 0; i < ITERP; ++i) {
                const int k = 1 + tid + i * NT;
                const F cs = vk[i].re * sc, sn = -vk[i].im * sc;
                // W[k] = i sn Z[k] + cs conj(Z[H-k]);  W[H-k] = i sn Z[H-k] - cs conj(Z[k]); stored conjugated
                if (k < H / 2) {
                    lds[cpad(k)] = {-sn * zk[i].im + cs * zh[i].re, -(sn * zk[i].re - cs * zh[i].im)};
                    lds[cpad(H - k)] = {-sn * zh[i].im - cs * zk[i].re, -(sn * zh[i].re + cs * zk[i].im)};
                }
            }
        }
        if (tid == 0) {
            const cpx<F> zq = lds[cpad(H / 2)];                 // t = pi/2: W = i Z -> conj(W) = (-zim, -zre)
            lds[cpad(H / 2)] = {-zq.im * sc, -zq.re * sc};
            lds[cpad(0)] = {F(0), F(0)};
        }
        __syncthreads();
    }
    F2_STAMP(st, 3);
    // 4. inverse transform (forward transform of the conjugate); outputs stay in v
    fft_all<F, LOG2H, true, PT, NT, T0R, 0, P13>(lds, tw, twl, tid, v);
    if constexpr (LOG2H == 0) v[0] = {F(0), F(0)};   // H = 1: W[0] = 0, the envelope is |x|

    F2_STAMP(st, 4);
    // 5. magnitude (in F: the FFT already limits the accuracy to F). The last pass left point j of
    //    butterfly i in v[i*R0 + brev(j)]; the envelope pair replaces it there.
#pragma unroll
    for (int i = 0; i < ITER0; ++i) {
        const int bf = tid + i * NT;
        if (FULL0 || bf < NB0) {
#pragma unroll
            for (int j = 0; j < R0; ++j) {
                const int i0 = 2 * (bf + j * NB0);
                F a, bb;
                if constexpr (KEEP_X) {
                    a = xr[i * R0 + j];
                    bb = xi[i * R0 + j];
                } else {
                    a = i0 < n ? (F)x[i0] : F(0);
                    bb = i0 + 1 < n ? (F)x[i0 + 1] : F(0);
                }
                const cpx<F> w = v[i * R0 + brev<R0>(j)];
                v[i * R0 + brev<R0>(j)] = {fsqrt(a * a + w.re * w.re), fsqrt(bb * bb + w.im * w.im)};
            }
        }
    }
    if (!P.lpf) {
#pragma unroll
        for (int i = 0; i < ITER0; ++i) {
            const int bf = tid + i * NT;
            if (FULL0 || bf < NB0) {
#pragma unroll
                for (int j = 0; j < R0; ++j) {
                    const cpx<F> e = v[i * R0 + brev<R0>(j)];
                    // (the points of a butterfly index j are NB0 apart: block j of 2 NB0 samples; inside the row - a wave-uniform
                    // test - it stores without a test per lane)
                    if (FULL0 && 2 * NB0 * (j + 1) <= n) store_pair(y + 2 * (bf + j * NB0), (double)e.re, (double)e.im);
                    else store_row_pair(y, n, 2 * (bf + j * NB0), (double)e.re, (double)e.im);
                }
            }
        }
        return;
    }
    F2_STAMP(st, 5);
    if constexpr (FULL0) {
        // block jj = i + ITER0*j of this thread's envelope pairs sits in v[i*R0 + brev(j)]
        constexpr int NBLK = ITER0 * R0;
        static_assert(lowpass_lds_bytes<F, NT, NBLK>() <= (size_t)LDS_BYTES, "LDS too small");
        F er[NBLK], ei[NBLK];
#pragma unroll
        for (int i = 0; i < ITER0; ++i)
#pragma unroll
            for (int j = 0; j < R0; ++j) {
                er[i + ITER0 * j] = v[i * R0 + brev<R0>(j)].re;
                ei[i + ITER0 * j] = v[i * R0 + brev<R0>(j)].im;
            }
        lowpass_pairs_store<F, NT, NBLK>(er, ei, P.a1, P.b0, smem, y, n, tid);
        F2_STAMP(st, 6);
#ifdef F2_STAMPS
        st[7] = st[8] = st[9] = st[6];
#endif
        F2_STAMP_STORE(st, 10, P.stamps);
        return;
    }
    // With the low-pass the envelope goes to LDS, TRANSPOSED: thread t will own the contiguous samples
    // [t*L, (t+1)*L), so sample t*L + j is kept at j*TP + t. (The last FFT pass ended with a barrier after
    // its LDS reads, so the array is free.)
    auto tpos = [](int i) { return (i % L) * TP + i / L; };
#pragma unroll
    for (int i = 0; i < ITER0; ++i) {
        const int bf = tid + i * NT;
        if (FULL0 || bf < NB0) {
#pragma unroll
            for (int j = 0; j < R0; ++j) {
                const int i0 = 2 * (bf + j * NB0);
                rl[tpos(i0)] = v[i * R0 + brev<R0>(j)].re;
                rl[tpos(i0 + 1)] = v[i * R0 + brev<R0>(j)].im;
            }
        }
    }
    __syncthreads();

    F2_STAMP(st, 6);
    // low-pass: chunked recurrence + multiplicative scan over the chunks. Each thread runs its chunk once
    // from zero state (float64 accumulator, float32 input term) keeping the zero-state responses; the true
    // output is that plus carry * (-a1)^(j+1), one float FMA per sample with the powers from an LDS table.
    const int n0 = tid * L;
    const double na1 = -P.a1;
    const F b0f = (F)P.b0;
    const F eprev = (n0 > 0 && n0 <= n) ? rl[tpos(n0 - 1)] : F(0);
    if (tid < L) {
        double pw = na1;
        for (int j = 0; j < tid; ++j) pw *= na1;
        qpow[tid] = (F)pw;   // (-a1)^(tid+1)
    }
    // The chunk is cut into NS sub-chunks whose recurrences run interleaved (independent float64 chains:
    // the FMA latency is ~25 cycles, a single 32-sample chain would cost more than the arithmetic).
    constexpr int NS = L >= 64 ? 8 : L >= 16 ? 4 : 1;   // sub-chunks of at most 16 samples
    constexpr int LS = L / NS;
    F yzs[L];                 // zero-state response of every sub-chunk
    double zend[NS];
    {
        // inside a sub-chunk (<= 16 samples) the recurrence runs in F: the rounding of so few steps stays at a few
        // ulp of the (positive) partial sums; everything that crosses sub-chunks, chunks and waves is float64
        F ep[NS], z[NS];
        const F na1f = (F)na1;
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            z[q] = F(0);
            ep[q] = q == 0 ? eprev : rl[(q * LS - 1) * TP + tid];
        }
#pragma unroll
        for (int j = 0; j < LS; ++j) {
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const F e = rl[(q * LS + j) * TP + tid];   // samples past n hold |0| = 0
                z[q] = na1f * z[q] + b0f * (e + ep[q]);
                yzs[q * LS + j] = z[q];
                ep[q] = e;
            }
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) zend[q] = (double)z[q];
    }
    // gs = (-a1)^LS, g = (-a1)^L
    double gs = na1;
#pragma unroll
    for (int s2 = 1; s2 < LS; s2 <<= 1) gs *= gs;
    double g = gs;
#pragma unroll
    for (int s2 = 1; s2 < NS; s2 <<= 1) g *= g;
    // chunk-level zero-state value at the end of every sub-chunk
    double ysub[NS];
    ysub[0] = zend[0];
#pragma unroll
    for (int q = 1; q < NS; ++q) ysub[q] = fma(gs, ysub[q - 1], zend[q]);
    const double yz = ysub[NS - 1];
    // inclusive scan inside the wave: v_t = sum_{j<=t} g^(t-j) yz_j
    const int lane = tid & 63, wv = tid >> 6;
    double sc = yz, gd = g;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double up = shfl_up_f64(sc, d);
        if (lane >= d) sc = fma(gd, up, sc);
        gd *= gd;
    }
    // gd == g^64 now
    F2_STAMP(st, 7);
    if (lane == 63) wave_tot[wv] = sc;
    // g^(lane+1) (data independent; placed before the barrier to overlap with the other waves' scans)
    double gl = 1.0, gp = g;
    for (int bits = lane + 1; bits; bits >>= 1) {
        if (bits & 1) gl *= gp;
        gp *= gp;
    }
    __syncthreads();
    double carry = 0.0;  // true y at the end of the previous wave's last chunk
    for (int w2 = 0; w2 < wv; ++w2) carry = fma(gd, carry, wave_tot[w2]);
    const double incl = fma(gl, carry, sc);                 // true y at the end of this chunk
    double yprev = shfl_up_f64(incl, 1);                    // ... of the previous chunk
    if (lane == 0) yprev = carry;
    {
        // value entering sub-chunk q: chunk-level zero-state part + (-a1)^(q*LS) * yprev
        double gq = 1.0;
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const F cq = (F)(q == 0 ? yprev : fma(gq, yprev, ysub[q - 1]));
#pragma unroll
            for (int j = 0; j < LS; ++j) rl[(q * LS + j) * TP + tid] = cq * qpow[j] + yzs[q * LS + j];
            gq *= gs;
        }
    }
    __syncthreads();
    F2_STAMP(st, 8);
#pragma unroll 4
    for (int i = 2 * tid; i < n; i += 2 * NT) store_row_pair(y, n, i, (double)rl[tpos(i)], (double)rl[tpos(min(i + 1, n - 1))]);
    F2_STAMP(st, 9);
    F2_STAMP_STORE(st, 10, P.stamps);
}

#ifdef F2_ENVELOPE_ROW_IS_FUNCTION
// The rows of a length class for launches that exist to serve utterances the spectral kernel's accuracy guard sends back
// (normally none): one workgroup per (utterance, slice of C / ENV_SLICES channels) that leaves at once when its utterance
// is not flagged and otherwise walks its channels. 1 / 16 of k_envelope's workgroups to dispatch when there is nothing to
// do (5 us instead of 75 us per 1000 x 128 rows), and a flagged utterance still spreads over ENV_SLICES workgroups.
constexpr int ENV_SLICES = 8;
template <typename F, int LOG2H>
__global__ __launch_bounds__((threads_for<F, LOG2H>()), (min_waves_for<F, LOG2H>())) void k_envelope_flagged(EnvParams P, const cpx<F>* __restrict__ tw) {
    const int u = blockIdx.x / ENV_SLICES, sl = blockIdx.x - u * ENV_SLICES;
    const int b = P.ulist ? P.ulist[u] : u;
    if (!P.uflag[b]) return;
    const int per = (P.C + ENV_SLICES - 1) / ENV_SLICES;
    for (int c = sl * per; c < min(P.C, (sl + 1) * per); ++c) {
        envelope_row<F, LOG2H>(P, tw, u, c);
        __syncthreads();   // the next row reuses the LDS arrays
    }
}
#endif  // F2_ENVELOPE_ROW_IS_FUNCTION
