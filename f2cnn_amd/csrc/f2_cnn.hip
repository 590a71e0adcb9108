// K4 -- forward pass of the F2CNN network (reference: architecture scripts/CNN/Training.py:93-114,
// predict + label rule scripts/CNN/Evaluating.py:85-87).
//
//   x (n, R, C, 1) -> Conv 3x3 same, 32 + ReLU -> Conv 3x3 valid, 32 + ReLU -> MaxPool 2x2
//                  -> Conv 3x3 same, 64 + ReLU -> Conv 3x3 valid, 64 + ReLU -> MaxPool 2x2
//                  -> Flatten (H,W,C order) -> Dense 516 + ReLU -> Dense 2 -> softmax
//
// Accumulation is float32 throughout (what Keras/TensorFlow computes). conv2..conv4 and dense1 (98 % of the 21.0 M MAC
// per window) run as implicit GEMMs on the matrix cores: the f32-input ones (v_mfma_f32_32x32x2_f32: bit-for-bit an fmaf
// chain, so results are deterministic) or, for conv2..conv4 and dense1 by default (option cnn_f16x3), the fp16 ones with both
// operands split in two fp16 pieces - three MFMAs per product, scores at the float32 rounding level of the former
// (f2_cnn_split.h; k_conv12_h16x3, k_conv34_h16x3 below). In the float32 kernels the weights are used in
// their Keras layouts: a (3,3,Cin,Cout) HWIO kernel flattened is exactly the K x N operand
// (k = (dy*3+dx)*Cin + ci). Activations are NHWC in HBM between layers, processed in chunks of windows.
//
// Implicit-GEMM tile of the float32 kernels: one task = 2 output rows x 32 output columns of one window, its 4 x 34 x Cin
// input patch in LDS; f2_cnn_f32_tile.h describes it and holds its pieces - the 9-tap loop, the patch staging, the pool
// exchange, the row GEMM - and the per-layer kernel k_conv3x3_f32 that conv3 / conv4 of windows without four pooled rows
// run on (ReLU, bias and the 2x2 max-pool applied from the accumulators). The reference's window shape runs two fused
// kernels instead: k_conv12_mfma (conv1 computed inside conv2's staging, two waves per task) and k_conv34_mfma (conv3's
// output stays in LDS).
#include <algorithm>
#include <cmath>

#include "f2_cnn_f32_tile.h"

namespace {

// ---- conv1 ('same', Cin = 1) + conv2 ('valid') + 2x2 max-pool in one kernel ----
// One task = 2 conv2 output rows x 32 columns of one window (one pooled row x 16). conv1 has no tensor of its own: the
// task's 4 x 34 x 32 conv2 input patch is *computed* - conv1 + ReLU from a 6 x 36 region of the raw window (VALU, 36 FMAs
// per pixel and channel quad) - instead of being read back, which removed a 180 KB/window activation round trip.
// Two waves share a task and its patch: each stages half of it and then runs the matrix-core loop for ONE of the two
// output rows (144 MFMAs), so a CU holds 16 waves for the same LDS as 8 whole-task waves and one wave's staging hides
// behind another's MFMAs; the rows meet through LDS for the pool.
__global__ __launch_bounds__(512) void k_conv12_mfma(const float* __restrict__ x, const float* __restrict__ w1,
                                                     const float* __restrict__ b1, const float* __restrict__ w2,
                                                     const float* __restrict__ b2, float* __restrict__ out, int Hin,
                                                     int Win, int64_t nwin) {
    constexpr int PS = C1 + 4, PATCH = 4 * PW * PS, XW = PW + 2, HALF = C1 / 2;
    extern __shared__ __attribute__((aligned(16))) float lds_all[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pair = wave >> 1, r = wave & 1;                  // r: which of the task's two output rows this wave computes
    float* patch = lds_all + pair * PATCH;
    float* xin = lds_all + 4 * PATCH + pair * (6 * XW);

    const int Ho = Hin - 2, Wo = Win - 2, Wout = Wo / 2;
    const int row_pairs = Ho / 2, xtiles = ((Wo / 2) * 2 + 31) / 32;
    const int64_t tasks = nwin * row_pairs * xtiles;
    int64_t task = (int64_t)blockIdx.x * 4 + pair;
    const bool live = task < tasks;
    if (!live) task = tasks - 1;
    const int xt = (int)(task % xtiles);
    const int64_t t2 = task / xtiles;
    const int rp = (int)(t2 % row_pairs);
    const int64_t win = t2 / row_pairs;
    const int y0 = 2 * rp, x0 = 32 * xt;

    // raw input region rows y0-1..y0+4, cols x0-1..x0+34 (zero outside the window: conv1's 'same' padding)
    const float* img = x + win * (int64_t)Hin * Win;
    const int l2 = lane + 64 * r;                              // 0..127 inside the pair
    for (int e = l2; e < 6 * XW; e += 128) {
        const int r6 = e / XW, p6 = e - r6 * XW;
        const int yi = y0 - 1 + r6, xi = x0 - 1 + p6;
        xin[e] = (yi >= 0 && yi < Hin && xi >= 0 && xi < Win) ? img[(int64_t)yi * Win + xi] : 0.f;
    }
    // conv1 weights of this lane's channel quad
    const int c4 = l2 & 7, pg = l2 >> 3;                       // 8 channel quads x 16 pixel groups
    float wr[9][4], br[4];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int q = 0; q < 4; ++q) wr[tap][q] = w1[tap * C1 + c4 * 4 + q];
#pragma unroll
    for (int q = 0; q < 4; ++q) br[q] = b1[c4 * 4 + q];
    __syncthreads();
#pragma unroll 1
    for (int e = pg; e < 4 * PW; e += 16) {
        const int pr = e / PW, pc = e - pr * PW;
        float xv[9];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) xv[dy * 3 + dx] = xin[(pr + dy) * XW + pc + dx];
        float o4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float acc = 0.f;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) acc = fmaf(xv[tap], wr[tap][q], acc);   // same order as the oracle's conv1
            o4[q] = fmaxf(acc + br[q], 0.f);
        }
        *reinterpret_cast<float4*>(patch + e * PS + c4 * 4) = make_float4(o4[0], o4[1], o4[2], o4[3]);
    }
    __syncthreads();

    // conv2 row y0 + r: lane = (pixel i, half h)
    const int i = lane & 31, h = lane >> 5;
    f32x16 acc[1][1];
    conv_taps<C1, C2, PS, 1, 1>(patch + (r * PW + i) * PS + h * HALF, reinterpret_cast<const float4*>(w2) + (int64_t)h * (HALF / 4) * C2 + i, acc);
    // 2x2 pool: row 1 hands its pair maxima to row 0 through the (now idle) patch
    float m[8];
    __syncthreads();
    pool_exchange(acc[0][0], patch, r == 1, lane, m);
    if (r == 0 && live) {
        const float bv = b2[i];
        float* o = out + win * (int64_t)row_pairs * Wout * C2;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int px = (x0 + acc_row(2 * k, h)) >> 1;
            if (px < Wout) o[((int64_t)rp * Wout + px) * C2 + i] = fmaxf(m[k] + bv, 0.f);
        }
    }
}

// ---- conv3 ('same') + conv4 ('valid') + 2x2 max-pool in one kernel, for networks whose pooled conv2 output has four
// rows (the 11 x C windows of the reference): conv3's output never leaves the CU. One 4-wave workgroup = one window x
// one tile of 30 conv4 output columns (15 pooled). Phase 1: wave w computes conv3 row w, 32 columns x 64 channels
// (two N tiles) from a 6 x 34 x 32 patch of the pooled conv2 tensor, writes bias + ReLU into a 4 x 34 x 64 LDS patch.
// Phase 2: wave w computes conv4 row w & 1, N tile w >> 1 from that patch; the rows meet through LDS for the pool.
__global__ __launch_bounds__(256) void k_conv34_mfma(const float* __restrict__ in, const float* __restrict__ w3,
                                                     const float* __restrict__ b3, const float* __restrict__ w4,
                                                     const float* __restrict__ b4, float* __restrict__ out, int Win,
                                                     int xtiles, int64_t nwin) {
    constexpr int PSA = C2 + 4, PSB = C3 + 4;                 // pixel pitches of the two patches (floats)
    constexpr int NA = 6 * PW * PSA, NB = 4 * PW * PSB;
    extern __shared__ __attribute__((aligned(16))) float lds_all[];
    float* pA = lds_all;                                      // [6][34][36]: pooled conv2 rows -1..4, cols c0-1..c0+32
    float* pB = lds_all + NA;                                 // [4][34][68]: conv3 rows 0..3, cols c0..c0+33 (32, 33 = 0)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int64_t win = blockIdx.x / xtiles;
    const int xt = (int)(blockIdx.x - win * xtiles);
    const int c0 = T34 * xt;
    const int Wo4 = Win - 2, Wp = Wo4 / 2;                   // conv4 output / pooled width
    if (win >= nwin) return;

    stage_patch<6, C2>(pA, in + win * (int64_t)4 * Win * C2, nullptr, 4, Win, -1, c0 - 1, tid, 256);
    for (int e = tid; e < 4 * 2 * PSB; e += 256) {            // the two columns conv4's discarded outputs touch
        const int r = e / (2 * PSB), rem = e - r * (2 * PSB);
        pB[(r * PW + 32) * PSB + rem] = 0.f;
    }
    __syncthreads();

    // ---- phase 1: conv3, row = wave ----
    {
        f32x16 acc[1][2];
        conv_taps<C2, C3, PSA, 1, 2>(pA + (wave * PW + i) * PSA + h * (C2 / 2), reinterpret_cast<const float4*>(w3) + (int64_t)h * (C2 / 8) * C3 + i, acc);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int co = nt * 32 + i;
            const float bv = b3[co];
#pragma unroll
            for (int q = 0; q < 16; ++q) pB[(wave * PW + acc_row(q, h)) * PSB + co] = fmaxf(acc[0][nt][q] + bv, 0.f);
        }
    }
    __syncthreads();

    // ---- phase 2: conv4, row = wave & 1, N tile = wave >> 1 ----
    const int r4 = wave & 1, nt4 = wave >> 1;
    f32x16 acc4[1][1];
    conv_taps<C3, C4, PSB, 1, 1>(pB + (r4 * PW + i) * PSB + h * (C3 / 2), reinterpret_cast<const float4*>(w4) + (int64_t)h * (C3 / 8) * C4 + nt4 * 32 + i,
                                 acc4);
    // 2x2 pool: row 1 hands its pair maxima to row 0 through LDS (pA is free)
    float m[8];
    pool_exchange(acc4[0][0], pA + nt4 * (8 * 64), r4 == 1, lane, m);
    if (r4 == 0) {
        const int co = nt4 * 32 + i;
        const float bv = b4[co];
        float* o = out + win * (int64_t)Wp * C4;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int xl = acc_row(2 * k, h);                    // even conv4 column inside the tile
            const int pxp = (c0 + xl) >> 1;
            if (xl < T34 && pxp < Wp) o[(int64_t)pxp * C4 + co] = fmaxf(m[k] + bv, 0.f);
        }
    }
}

// ---- the same kernel on the fp16 matrix cores, operands split in two fp16 pieces (option "cnn_f16x3"; f2_cnn_split.h) ----
// Three MFMAs per product with float32 accumulation, 5.3 x the f32 matrix rate. (Rounds 3-4 used bf16 pieces: 2^-16 per product,
// scores within 7e-7 and two referee ties among the 113 920 cfg4 labels; fp16 pieces with per-layer power-of-two scales carry
// 2^-22: float32 rounding level, every label identical.)
// Layouts: lane (i, h) of an MFMA supplies K = 8 h .. 8 h + 7 of row / column i, so 16 input channels are one MFMA step and a
// lane's operand is ONE 16-byte read of a pixel's channels: patches are [pixel][channel] fp16 (pitch + 16 bytes: conflict-
// free ds_read_b128), one for the first pieces and one for the second; weights arrive pre-split (and scaled) from the host as
// w[piece][tap][kb][h][cout][8]. Activations are split where they are written into LDS (staging, conv3's epilogue); between the
// kernels they travel as float32 in the NEXT layer's scaled units.
constexpr int PA16 = C2 * 2 + 16;   // bytes per pixel of the conv3 input patches
constexpr int PB16 = C3 * 2 + 16;   // ... of the conv4 input patches

__global__ __launch_bounds__(256) void k_conv34_h16x3(const float* __restrict__ in, const h16x8* __restrict__ w3s,
                                                       const float* __restrict__ b3, const h16x8* __restrict__ w4s,
                                                       const float* __restrict__ b4, float* __restrict__ out, int Win,
                                                       int xtiles, int64_t nwin, f2_split_scales S) {
    // (in: pooled conv2 outputs x sa_3; b3 = conv3's biases x sa_4, b4 = conv4's x sa_dense1; out x sa_dense1)
    constexpr int NA = 6 * PW * PA16, NB = 4 * PW * PB16;     // bytes per piece
    extern __shared__ __attribute__((aligned(16))) unsigned char lds16[];
    // The second piece of the conv4 input lives where the conv3 input was (a barrier between conv3's matrix loop and its
    // epilogue): 52 KB per workgroup instead of 72, three workgroups per CU instead of two.
    static_assert(NB + 4096 <= 2 * NA, "conv4 input piece + pool exchange inside the conv3 input patches");
    unsigned char* pAh = lds16;                               // [6][34] pixels x 32 channels: pooled conv2 rows -1..4
    unsigned char* pAl = pAh + NA;
    unsigned char* pBh = pAl + NA;                            // [4][34] pixels x 64 channels: conv3 rows 0..3
    unsigned char* pBl = lds16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int64_t win = blockIdx.x / xtiles;
    const int xt = (int)(blockIdx.x - win * xtiles);
    const int c0 = T34 * xt;
    const int Wo4 = Win - 2, Wp = Wo4 / 2;
    if (win >= nwin) return;

    const float* img = in + win * (int64_t)4 * Win * C2;
    for (int e = tid; e < 6 * PW * (C2 / 4); e += 256) {
        const int r = e / (PW * (C2 / 4));
        const int rem = e - r * (PW * (C2 / 4));
        const int p = rem / (C2 / 4), c4 = rem - p * (C2 / 4);
        const int yi = r - 1, xi = c0 - 1 + p;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (yi >= 0 && yi < 4 && xi >= 0 && xi < Win)
            v = *reinterpret_cast<const float4*>(img + ((int64_t)yi * Win + xi) * C2 + c4 * 4);
        _Float16 h4[4], l4[4];
        split_h16(v.x, h4[0], l4[0]);
        split_h16(v.y, h4[1], l4[1]);
        split_h16(v.z, h4[2], l4[2]);
        split_h16(v.w, h4[3], l4[3]);
        const h16x4 vh = {h4[0], h4[1], h4[2], h4[3]}, vl = {l4[0], l4[1], l4[2], l4[3]};
        *reinterpret_cast<h16x4*>(pAh + (r * PW + p) * PA16 + c4 * 8) = vh;
        *reinterpret_cast<h16x4*>(pAl + (r * PW + p) * PA16 + c4 * 8) = vl;
    }
    __syncthreads();

    // ---- phase 1: conv3, row = wave, both N tiles ----
    {
        constexpr int KB = C2 / 16, NIT = 9 * KB;
        f32x16 acc[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[nt][q] = 0.f;
        const int pa0 = (wave * PW + i) * PA16 + h * 16;
        const h16x8* wh = w3s + h * C3 + i;                  // [tap][kb][h][cout]
        const h16x8* wl = wh + 9 * KB * 2 * C3;
        // A (LDS) one step ahead; B (weights, L2: a step is only 192 matrix-core cycles) WD steps ahead
        constexpr int WD = 4;
        h16x8 ah[2], al[2], bh[WD][2], bl[WD][2];
        auto fetch_a = [&](int it, int buf) {
            const int tap = it / KB, kb = it - tap * KB;
            const int dy = tap / 3, dx = tap - dy * 3;
            const int off = pa0 + (dy * PW + dx) * PA16 + kb * 32;
            ah[buf] = *reinterpret_cast<const h16x8*>(pAh + off);
            al[buf] = *reinterpret_cast<const h16x8*>(pAl + off);
        };
        auto fetch_b = [&](int it, int slot) {
            const int wo = it * 2 * C3;                       // (tap * KB + kb) = it
            bh[slot][0] = wh[wo];
            bh[slot][1] = wh[wo + 32];
            bl[slot][0] = wl[wo];
            bl[slot][1] = wl[wo + 32];
        };
#pragma unroll
        for (int k = 0; k < WD - 1; ++k) fetch_b(k, k);
        fetch_a(0, 0);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int cur = it & 1, ws = it % WD;
            if (it + WD - 1 < NIT) fetch_b(it + WD - 1, (it + WD - 1) % WD);
            if (it + 1 < NIT) fetch_a(it + 1, cur ^ 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                acc[nt] = MFMA16(al[cur], bh[ws][nt], acc[nt]);
                acc[nt] = MFMA16(ah[cur], bl[ws][nt], acc[nt]);
                acc[nt] = MFMA16(ah[cur], bh[ws][nt], acc[nt]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();                                      // every wave is done reading the conv3 input
        for (int e = tid; e < 4 * 2 * (PB16 / 4); e += 256) { // the two columns conv4's discarded outputs touch
            const int r = e / (2 * (PB16 / 4)), rem = e - r * (2 * (PB16 / 4));
            reinterpret_cast<unsigned*>(pBh + (r * PW + 32) * PB16)[rem] = 0u;
            reinterpret_cast<unsigned*>(pBl + (r * PW + 32) * PB16)[rem] = 0u;
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int co = nt * 32 + i;
            const float bv = b3[co];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int px = acc_row(q, h);
                _Float16 vh, vl;
                split_h16(fmaxf(fmaf(acc[nt][q], S.c3, bv), 0.f), vh, vl);
                *reinterpret_cast<_Float16*>(pBh + (wave * PW + px) * PB16 + co * 2) = vh;
                *reinterpret_cast<_Float16*>(pBl + (wave * PW + px) * PB16 + co * 2) = vl;
            }
        }
    }
    __syncthreads();

    // ---- phase 2: conv4, row = wave & 1, N tile = wave >> 1 ----
    const int r4 = wave & 1, nt4 = wave >> 1;
    f32x16 acc4;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc4[q] = 0.f;
    {
        constexpr int KB = C3 / 16, NIT = 9 * KB;
        const int pa0 = (r4 * PW + i) * PB16 + h * 16;
        const h16x8* wh = w4s + h * C4 + nt4 * 32 + i;
        const h16x8* wl = wh + 9 * KB * 2 * C4;
        constexpr int WD = 6;
        h16x8 ah[2], al[2], bh[WD], bl[WD];
        auto fetch_a = [&](int it, int buf) {
            const int tap = it / KB, kb = it - tap * KB;
            const int dy = tap / 3, dx = tap - dy * 3;
            const int off = pa0 + (dy * PW + dx) * PB16 + kb * 32;
            ah[buf] = *reinterpret_cast<const h16x8*>(pBh + off);
            al[buf] = *reinterpret_cast<const h16x8*>(pBl + off);
        };
        auto fetch_b = [&](int it, int slot) {
            bh[slot] = wh[it * 2 * C4];
            bl[slot] = wl[it * 2 * C4];
        };
#pragma unroll
        for (int k = 0; k < WD - 1; ++k) fetch_b(k, k);
        fetch_a(0, 0);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int cur = it & 1, ws = it % WD;
            if (it + WD - 1 < NIT) fetch_b(it + WD - 1, (it + WD - 1) % WD);
            if (it + 1 < NIT) fetch_a(it + 1, cur ^ 1);
            __builtin_amdgcn_sched_barrier(0);
            acc4 = MFMA16(al[cur], bh[ws], acc4);
            acc4 = MFMA16(ah[cur], bl[ws], acc4);
            acc4 = MFMA16(ah[cur], bh[ws], acc4);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // 2x2 pool as in k_conv34_mfma (the conv3 input patches are free)
    float hm[8];
#pragma unroll
    for (int q = 0; q < 16; q += 2) hm[q / 2] = fmaxf(acc4[q], acc4[q + 1]);
    float* xch = reinterpret_cast<float*>(lds16 + ((NB + 1023) & ~1023)) + nt4 * (8 * 64);   // behind the conv4 input piece
    if (r4 == 1) {
#pragma unroll
        for (int k = 0; k < 8; ++k) xch[k * 64 + lane] = hm[k];
    }
    __syncthreads();
    if (r4 == 0) {
        const int co = nt4 * 32 + i;
        const float bv = b4[co];
        float* o = out + win * (int64_t)Wp * C4;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int q = 2 * k;
            const int xl = acc_row(q, h);
            const int pxp = (c0 + xl) >> 1;
            const float m = fmaxf(hm[k], xch[k * 64 + lane]);
            if (xl < T34 && pxp < Wp) o[(int64_t)pxp * C4 + co] = fmaxf(fmaf(m, S.c4, bv), 0.f);
        }
    }
}

// ---- conv1 + conv2 + pool with conv2 on the fp16 matrix cores (as k_conv34_h16x3; structure of k_conv12_mfma) ----
// The conv2 input patch (computed by conv1, float32 VALU as before, then scaled by sa_2) is written as two fp16 pieces at 64 bytes per pixel:
// no room for a padded pitch (four tasks per workgroup, two workgroups per CU), so the 16-byte chunk c of pixel p sits at
// chunk c ^ ((p >> 2) & 3) - sixteen consecutive pixels then cover all sixteen bank quads for any chunk a wave reads.
__device__ __forceinline__ int patch16_offset(int pixel, int chunk) { return pixel * 64 + ((chunk ^ ((pixel >> 2) & 3)) << 4); }

// RP = pooled rows (conv2 row pairs) per task, TPW = tasks per workgroup; a task is 2 RP waves, one per conv2 output row,
// sharing a (2 RP + 2)-row patch: with RP = 2 conv1 computes six patch rows for four output rows instead of eight (its
// float32 VALU work is what bounds the kernel: 968 VALU instructions per wave against 54 MFMAs at RP = 1), and the raw-input
// loads, the conv1 weight loads and the barriers are shared by twice the output (1.14 -> 0.98 ms per 14 240 windows; RP = 4,
// ten patch rows for eight output rows in an 8-wave workgroup, measured the same as RP = 2).
template <int RP, int TPW>
__global__ __launch_bounds__(128 * RP * TPW) void k_conv12_h16x3(const float* __restrict__ x, const float* __restrict__ w1,
                                                                   const float* __restrict__ b1, const h16x8* __restrict__ w2s,
                                                                   const float* __restrict__ b2, float* __restrict__ out, int Hin,
                                                                   int Win, int64_t nwin, f2_split_scales S) {
    // (b2 = conv2's biases x sa_3; out x sa_3)
    constexpr int PR = 2 * RP + 2, PIECE = PR * PW * 64, XW = PW + 2, XR = PR + 2, KB = C1 / 16, NIT = 9 * KB;
    constexpr int TW = 2 * RP;                                 // waves per task
    extern __shared__ __attribute__((aligned(16))) unsigned char lds16[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tk = wave / TW, r = wave % TW;                   // r: the conv2 output row of the task this wave computes
    unsigned char* ph = lds16 + tk * (2 * PIECE);
    unsigned char* pl = ph + PIECE;
    float* xin = reinterpret_cast<float*>(lds16 + TPW * (2 * PIECE)) + tk * (XR * XW);

    const int Ho = Hin - 2, Wo = Win - 2, Wout = Wo / 2;
    const int row_pairs = Ho / 2, row_groups = row_pairs / RP, xtiles = ((Wo / 2) * 2 + 31) / 32;   // (host: RP divides row_pairs)
    const int64_t tasks = nwin * row_groups * xtiles;
    int64_t task = (int64_t)blockIdx.x * TPW + tk;
    const bool live = task < tasks;
    if (!live) task = tasks - 1;
    const int xt = (int)(task % xtiles);
    const int64_t t2 = task / xtiles;
    const int rg = (int)(t2 % row_groups);
    const int64_t win = t2 / row_groups;
    const int y0 = 2 * RP * rg, x0 = 32 * xt;

    // raw input region rows y0-1..y0+PR, cols x0-1..x0+34 (zero outside the window: conv1's 'same' padding)
    const float* img = x + win * (int64_t)Hin * Win;
    const int l2 = lane + 64 * r;                              // 0 .. 64 TW - 1 inside the task
    for (int e = l2; e < XR * XW; e += 64 * TW) {
        const int r6 = e / XW, p6 = e - r6 * XW;
        const int yi = y0 - 1 + r6, xi = x0 - 1 + p6;
        xin[e] = (yi >= 0 && yi < Hin && xi >= 0 && xi < Win) ? img[(int64_t)yi * Win + xi] : 0.f;
    }
    const int c4 = l2 & 7, pg = l2 >> 3;                       // 8 channel quads x 8 TW pixel groups
    float wr[9][4], br[4];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int q = 0; q < 4; ++q) wr[tap][q] = w1[tap * C1 + c4 * 4 + q];
#pragma unroll
    for (int q = 0; q < 4; ++q) br[q] = b1[c4 * 4 + q];
    __syncthreads();
#pragma unroll 1
    for (int e = pg; e < PR * PW; e += 8 * TW) {
        const int pr = e / PW, pc = e - pr * PW;
        float xv[9];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) xv[dy * 3 + dx] = xin[(pr + dy) * XW + pc + dx];
        _Float16 h4[4], l4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float acc = 0.f;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) acc = fmaf(xv[tap], wr[tap][q], acc);   // same order as the oracle's conv1
            split_h16(fmaxf(acc + br[q], 0.f) * S.sa2, h4[q], l4[q]);
        }
        const int off = patch16_offset(e, c4 >> 1) + (c4 & 1) * 8;
        *reinterpret_cast<h16x4*>(ph + off) = h16x4{h4[0], h4[1], h4[2], h4[3]};
        *reinterpret_cast<h16x4*>(pl + off) = h16x4{l4[0], l4[1], l4[2], l4[3]};
    }
    __syncthreads();

    const int i = lane & 31, h = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    const int p0 = r * PW + i;
    const h16x8* wh = w2s + h * C2 + i;                      // [tap][kb][h][cout]
    const h16x8* wl = wh + 9 * KB * 2 * C2;
    // A (LDS) one step ahead; B (weights, L2) WD steps ahead: a step is only 96 matrix-core cycles
    constexpr int WD = 5;
    h16x8 ah[2], al[2], bh[WD], bl[WD];
    auto fetch_a = [&](int it, int buf) {
        const int tap = it / KB, kb = it - tap * KB;
        const int dy = tap / 3, dx = tap - dy * 3;
        const int off = patch16_offset(p0 + dy * PW + dx, 2 * kb + h);
        ah[buf] = *reinterpret_cast<const h16x8*>(ph + off);
        al[buf] = *reinterpret_cast<const h16x8*>(pl + off);
    };
    auto fetch_b = [&](int it, int slot) {
        bh[slot] = wh[it * 2 * C2];
        bl[slot] = wl[it * 2 * C2];
    };
#pragma unroll
    for (int k = 0; k < WD - 1; ++k) fetch_b(k, k);
    fetch_a(0, 0);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int cur = it & 1, ws = it % WD;
        if (it + WD - 1 < NIT) fetch_b(it + WD - 1, (it + WD - 1) % WD);
        if (it + 1 < NIT) fetch_a(it + 1, cur ^ 1);
        __builtin_amdgcn_sched_barrier(0);
        acc = MFMA16(al[cur], bh[ws], acc);
        acc = MFMA16(ah[cur], bl[ws], acc);
        acc = MFMA16(ah[cur], bh[ws], acc);
        __builtin_amdgcn_sched_barrier(0);
    }
    // 2x2 pool: horizontal pairs sit in one lane; the odd row of a pair hands its eight pair maxima to the even one through
    // the (now idle) patch
    float hm[8];
#pragma unroll
    for (int q = 0; q < 16; q += 2) hm[q / 2] = fmaxf(acc[q], acc[q + 1]);
    float* xch = reinterpret_cast<float*>(ph) + (r >> 1) * (8 * 64);
    __syncthreads();
    if (r & 1) {
#pragma unroll
        for (int k = 0; k < 8; ++k) xch[k * 64 + lane] = hm[k];
    }
    __syncthreads();
    if (!(r & 1) && live) {
        const float bv = b2[i];
        const int rp = RP * rg + (r >> 1);
        float* o = out + win * (int64_t)row_pairs * Wout * C2;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int q = 2 * k;
            const int px = (x0 + acc_row(q, h)) >> 1;
            const float m = fmaxf(hm[k], xch[k * 64 + lane]);
            if (px < Wout) o[((int64_t)rp * Wout + px) * C2 + i] = fmaxf(fmaf(m, S.c2, bv), 0.f);
        }
    }
}

// `fused`: the outputs feed k_conv34_h16x3 (scaled by sa_3); otherwise the float32 conv3 (true units)
template <int RP, int TPW>
int launch_conv12_h16(f2_ctx* ctx, const f2_cnn* cnn, const f2_scale_set* S, const float* d_x, float* a2, int H1, int W1, int64_t n,
                      bool fused) {
    const int Ho = H1 - 2, Wo = W1 - 2;
    const int64_t tasks = n * (Ho / 2 / RP) * (((Wo / 2) * 2 + 31) / 32);
    if (tasks <= 0) return F2_OK;
    constexpr size_t lds = TPW * (2 * (size_t)((2 * RP + 2) * PW * 64) + sizeof(float) * (2 * RP + 4) * (PW + 2));
    static_assert(lds <= 80 * 1024, "at least two workgroups per CU");
    auto kern = k_conv12_h16x3<RP, TPW>;
    F2_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    unsigned blocks;
    F2_TRY(cnn_grid(ctx, (tasks + TPW - 1) / TPW, &blocks));
    f2_split_scales sc = S->sc;
    if (!fused) sc.c2 = S->c2_true;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(128 * RP * TPW), lds, ctx->stream, d_x, cnn->t(0), cnn->t(1),
                       (const h16x8*)(cnn->blob16 + cnn->off16[0]), fused ? S->sbias + F2_SB_B2 : cnn->t(3), a2, H1, W1, n, sc);
    return F2_OK;
}

// ---- dense1: (n, K) x (K, 516) on the same MFMA: gemm_rows_tile with N = the padded 544, then bias + ReLU ----
// One 6-wave workgroup = 64 windows (two M tiles) x 6 of the 17 output tiles (blockIdx.y picks the group, one output
// tile per wave); weights wt[chunk][h][q][n (padded to 544)][4].
constexpr int D1_MT = 2;                   // M tiles (32 windows each) per workgroup: every weight load feeds 2 MFMA tiles
static_assert(32 * D1_MT == GEMM_ROWS, "k_dense1_mfma and k_dense1_h16x3 share a grid");
__global__ __launch_bounds__(D1_WAVES * 64) void k_dense1_mfma(const float* __restrict__ a, const float* __restrict__ wt,
                                                               const float* __restrict__ bias, float* __restrict__ out,
                                                               int K, int64_t n) {
    __shared__ __attribute__((aligned(16))) float As[2][GEMM_ROWS * GEMM_PS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w0 = (int64_t)blockIdx.x * GEMM_ROWS;
    const int nt = blockIdx.y * D1_WAVES + wave;       // this wave's output tile
    const bool live = nt < D1_TILES;
    f32x16 acc[2];
    gemm_rows_tile<D1_WAVES>(a, wt, K, D1_NPAD, n, w0, nt, live, As, acc);
    const int col = nt * 32 + (lane & 31);
    if (live && col < D1) {
        const float b = bias[col];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int64_t wr = w0 + t * 32 + acc_row(q, lane >> 5);
                if (wr < n) out[wr * D1 + col] = fmaxf(acc[t][q] + b, 0.f);
            }
    }
}

// ---- dense1 on the fp16 matrix cores, operands split in two pieces (as the convolutions above; a = conv4 outputs x sa_dense1) ----
// Same tiling as k_dense1_mfma (64 windows x 6 output tiles per 6-wave workgroup, K in chunks of 64). A chunk is only 24
// MFMAs per wave now, so the next chunk's activations (global -> registers) and weights (8 x 16 bytes per lane) are
// requested before the current chunk's MFMAs and land while they run; the activations are split when they are written to
// LDS ([row][64] fp16 per piece, pitch + 16 bytes). Weights: w[piece][chunk][ks][h][n (544)][8], k = 64 chunk + 16 ks + 8 h + e.
constexpr int D1_PITCH16 = D1_KC * 2 + 16;
// MT = M tiles (32 windows each) per workgroup. With 64 windows (MT = 2) a 14 240-window chunk is 223 x 3 = 669 workgroups for
// the 512 that are resident at two per CU: a second round one third full. 96 windows (MT = 3): 149 x 3 = 447 workgroups, one
// round, and every weight fragment feeds nine MFMAs instead of six.
template <int MT>
__global__ __launch_bounds__(D1_WAVES * 64) void k_dense1_h16x3(const float* __restrict__ a, const h16x8* __restrict__ ws,
                                                                 const float* __restrict__ bias, float* __restrict__ out,
                                                                 int K, int64_t n, f2_split_scales S) {
    constexpr int D1_MT = MT;
    constexpr int ROWS = 32 * D1_MT, NTHR = D1_WAVES * 64;
    constexpr int PER = (ROWS * (D1_KC / 4) + NTHR - 1) / NTHR;      // float4 of a chunk per thread (3, the last partly)
    __shared__ __attribute__((aligned(16))) unsigned char Ah[2][ROWS * D1_PITCH16];
    __shared__ __attribute__((aligned(16))) unsigned char Al[2][ROWS * D1_PITCH16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t w0 = (int64_t)blockIdx.x * ROWS;
    const int i = lane & 31, h = lane >> 5;
    const int nchunks = K / D1_KC;
    const int nt = blockIdx.y * D1_WAVES + wave;
    const bool live = nt < D1_TILES;
    const int ntc = live ? nt : D1_TILES - 1;                        // (idle waves load a valid tile and discard it)
    const h16x8* wh = ws + (int64_t)h * D1_NPAD + ntc * 32 + i;
    const h16x8* wl = wh + (int64_t)nchunks * 4 * 2 * D1_NPAD;

    float4 ar[PER];
    auto load_a = [&](int kc) {
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int e = tid + p * NTHR;
            const int row = e / (D1_KC / 4), c4 = e - row * (D1_KC / 4);
            const int64_t wr = w0 + row < n ? w0 + row : n - 1;
            if (e < ROWS * (D1_KC / 4)) ar[p] = *reinterpret_cast<const float4*>(a + wr * K + (int64_t)kc * D1_KC + c4 * 4);
        }
    };
    auto store_a = [&](int buf) {
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int e = tid + p * NTHR;
            const int row = e / (D1_KC / 4), c4 = e - row * (D1_KC / 4);
            if (e < ROWS * (D1_KC / 4)) {
                _Float16 h4[4], l4[4];
                split_h16(ar[p].x * S.sin_d, h4[0], l4[0]);
                split_h16(ar[p].y * S.sin_d, h4[1], l4[1]);
                split_h16(ar[p].z * S.sin_d, h4[2], l4[2]);
                split_h16(ar[p].w * S.sin_d, h4[3], l4[3]);
                *reinterpret_cast<h16x4*>(&Ah[buf][row * D1_PITCH16 + c4 * 8]) = h16x4{h4[0], h4[1], h4[2], h4[3]};
                *reinterpret_cast<h16x4*>(&Al[buf][row * D1_PITCH16 + c4 * 8]) = h16x4{l4[0], l4[1], l4[2], l4[3]};
            }
        }
    };
    h16x8 bh[2][4], bl[2][4];
    auto load_b = [&](int kc, int slot) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            bh[slot][ks] = wh[(int64_t)(kc * 4 + ks) * 2 * D1_NPAD];
            bl[slot][ks] = wl[(int64_t)(kc * 4 + ks) * 2 * D1_NPAD];
        }
    };

    f32x16 acc[D1_MT];
#pragma unroll
    for (int t = 0; t < D1_MT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;

    load_a(0);
    load_b(0, 0);
    store_a(0);
    __syncthreads();
    auto chunk = [&](int kc, int cur) {                              // cur = kc & 1, compile-time in the unrolled pair below
        if (kc + 1 < nchunks) {
            load_a(kc + 1);
            load_b(kc + 1, cur ^ 1);
        }
        __builtin_amdgcn_sched_barrier(0);
        const unsigned char* pah = &Ah[cur][i * D1_PITCH16 + h * 16];
        const unsigned char* pal = &Al[cur][i * D1_PITCH16 + h * 16];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
            for (int t = 0; t < D1_MT; ++t) {
                const h16x8 ah = *reinterpret_cast<const h16x8*>(pah + t * 32 * D1_PITCH16 + ks * 32);
                const h16x8 al = *reinterpret_cast<const h16x8*>(pal + t * 32 * D1_PITCH16 + ks * 32);
                acc[t] = MFMA16(al, bh[cur][ks], acc[t]);
                acc[t] = MFMA16(ah, bl[cur][ks], acc[t]);
                acc[t] = MFMA16(ah, bh[cur][ks], acc[t]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (kc + 1 < nchunks) store_a(cur ^ 1);
        __syncthreads();
    };
    for (int kc = 0; kc < nchunks; kc += 2) {
        chunk(kc, 0);
        if (kc + 1 < nchunks) chunk(kc + 1, 1);
    }
    const int col = nt * 32 + i;
    if (live && col < D1) {
        const float b = bias[col];
#pragma unroll
        for (int t = 0; t < D1_MT; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int64_t wr = w0 + t * 32 + acc_row(q, h);
                if (wr < n) out[wr * D1 + col] = fmaxf(fmaf(acc[t][q], S.cd, b), 0.f);
            }
    }
}

// ---- dense2 + softmax + label: eight threads per window ----
// (one thread per window read its 516-float row with a 2 KB stride between lanes; eight neighbouring lanes now walk a row in
// 16-byte pieces - 128 contiguous bytes per load instruction and window - and meet through three DPP-free shuffles. The sum is
// formed in a different order than the oracle's k = 0 .. 515 chain: float32 rounding level, far inside the 2e-5 score tolerance.)
__global__ __launch_bounds__(256) void k_dense2_softmax(const float* __restrict__ a, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ scores,
                                                        uint8_t* __restrict__ labels, int64_t n) {
    static_assert(D1 % 4 == 0, "rows walked in float4 pieces");
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
    const int part = threadIdx.x & 7;
    const int64_t row = i < n ? i : n - 1;
    const float4* r = reinterpret_cast<const float4*>(a + row * D1);
    const float4* w4 = reinterpret_cast<const float4*>(w);          // (k, class) pairs: two k per float4
    float z0 = 0.f, z1 = 0.f;
    for (int q = part; q < D1 / 4; q += 8) {
        const float4 v = r[q];
        const float4 wa = w4[2 * q], wb = w4[2 * q + 1];
        z0 = fmaf(v.x, wa.x, z0);
        z1 = fmaf(v.x, wa.y, z1);
        z0 = fmaf(v.y, wa.z, z0);
        z1 = fmaf(v.y, wa.w, z1);
        z0 = fmaf(v.z, wb.x, z0);
        z1 = fmaf(v.z, wb.y, z1);
        z0 = fmaf(v.w, wb.z, z0);
        z1 = fmaf(v.w, wb.w, z1);
    }
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) {
        z0 += __shfl_xor(z0, d);
        z1 += __shfl_xor(z1, d);
    }
    if (part != 0 || i >= n) return;
    z0 += bias[0];
    z1 += bias[1];
    const float m = fmaxf(z0, z1);
    const float e0 = expf(z0 - m), e1 = expf(z1 - m);
    const float s = e0 + e1;
    const float s0 = e0 / s, s1 = e1 / s;
    if (scores) {
        scores[2 * i] = s0;
        scores[2 * i + 1] = s1;
    }
    if (labels) labels[i] = s1 > s0 ? 1 : 0;   // ties -> 0 ("falling"), Evaluating.py:87
}

// conv1 + conv2 + pool of the per-tile kernels (conv1 is evaluated inside conv2's patch staging)
int launch_conv12(f2_ctx* ctx, const f2_cnn* cnn, const f2_scale_set* S, bool split, const Dims& d, const float* d_x, int64_t n,
                  float* a2) {
    if (split) {
        // four output rows per task where the pooled height allows (the reference's 11-row windows: 4 pooled rows)
        F2_TRY(d.Hp1 % 2 == 0 ? (launch_conv12_h16<2, 1>(ctx, cnn, S, d_x, a2, d.H1, d.W1, n, d.Hp1 == 4))
                              : (launch_conv12_h16<1, 2>(ctx, cnn, S, d_x, a2, d.H1, d.W1, n, d.Hp1 == 4)));
    } else {
        constexpr size_t lds12 = sizeof(float) * 4 * (4 * PW * (C1 + 4) + 6 * (PW + 2));
        F2_HIP(ctx, hipFuncSetAttribute((const void*)k_conv12_mfma, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds12));
        unsigned blocks;
        F2_TRY(cnn_grid(ctx, (n * d.Hp1 * d.xtiles12() + 3) / 4, &blocks));
        hipLaunchKernelGGL(k_conv12_mfma, dim3(blocks), dim3(512), lds12, ctx->stream, d_x, cnn->t(0), cnn->t(1), cnn->t(2), cnn->t(3),
                           a2, d.H1, d.W1, n);
    }
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

// conv3 + conv4 + pool of the per-tile kernels. Four pooled rows (the reference's 11-row windows): one kernel, conv3's output
// stays in LDS; any other height: the float32 kernels layer by layer, through a3
int launch_conv34(f2_ctx* ctx, const f2_cnn* cnn, const f2_scale_set* S, bool split, const Dims& d, const float* a2, int64_t n,
                  float* a3, float* a4) {
    if (d.Hp1 != 4) {
        F2_TRY((launch_conv3x3<C2, C3, 1, ST_PLAIN, EP_RELU, 8, 2>(ctx, a2, nullptr, cnn->t(4), cnn->t(5), a3, d.Hp1, d.Wp1, n)));
        return launch_conv3x3<C3, C4, 0, ST_PLAIN, EP_POOL, 4, 2>(ctx, a3, nullptr, cnn->t(6), cnn->t(7), a4, d.Hp1, d.Wp1, n);
    }
    const int xtiles = d.xtiles34();
    unsigned blocks;
    F2_TRY(cnn_grid(ctx, n * xtiles, &blocks));
    if (split) {
        constexpr size_t lds16 = 2 * (size_t)(6 * PW * PA16) + (size_t)(4 * PW * PB16);
        static_assert(3 * lds16 <= 160 * 1024, "three workgroups per CU");
        F2_HIP(ctx, hipFuncSetAttribute((const void*)k_conv34_h16x3, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds16));
        hipLaunchKernelGGL(k_conv34_h16x3, dim3(blocks), dim3(256), lds16, ctx->stream, a2, (const h16x8*)(cnn->blob16 + cnn->off16[1]),
                           S->sbias + F2_SB_B3F, (const h16x8*)(cnn->blob16 + cnn->off16[2]), S->sbias + F2_SB_B4, a4, d.Wp1, xtiles, n,
                           S->sc);
    } else {
        constexpr size_t lds34 = sizeof(float) * (6 * PW * (C2 + 4) + 4 * PW * (C3 + 4));
        static_assert(lds34 <= 80 * 1024, "two workgroups per CU");
        F2_HIP(ctx, hipFuncSetAttribute((const void*)k_conv34_mfma, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds34));
        hipLaunchKernelGGL(k_conv34_mfma, dim3(blocks), dim3(256), lds34, ctx->stream, a2, cnn->t(4), cnn->t(5), cnn->t(6), cnn->t(7), a4,
                           d.Wp1, xtiles, n);
    }
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

}  // namespace

size_t f2_cnn_workspace_floats(const f2_cnn* cnn) {
    const Dims d = make_dims(cnn->rows, cnn->channels);
    return (size_t)d.Hp1 * d.Wp1 * C2 + (size_t)d.Hp1 * d.Wp1 * C3 + (size_t)d.flat + D1;   // conv1's output never exists
}
size_t f2_cnn_flat_floats(const f2_cnn* cnn) { return (size_t)make_dims(cnn->rows, cnn->channels).flat; }
size_t f2_cnn_dense_floats(const f2_cnn* cnn) { return (size_t)make_dims(cnn->rows, cnn->channels).flat + D1; }

// ---- the route: which kernels run (f2_internal.h: f2_cnn_route). These two functions are the only readers of the self-check's
// verdicts and of the context's three CNN options ----
f2_cnn_route f2_cnn_capability(const f2_cnn* cnn) {
    f2_cnn_route r;
    r.split = cnn->blob16 && cnn->f16x3_ok;
    r.ws = cnn->blob16 && cnn->ws_ok && f2_cnn_ws_supported(cnn->rows, cnn->channels);
    r.ws_dense = r.ws && cnn->ws_dense_ok && f2_dense1_ws_takes(cnn->flat, 1);
    return r;
}

f2_cnn_route f2_cnn_call_route(const f2_ctx* ctx, const f2_cnn* cnn, bool have_scale_set) {
    const f2_cnn_route can = f2_cnn_capability(cnn);
    f2_cnn_route r;
    r.split = have_scale_set && ctx->opt_cnn_f16x3 && can.split;
    r.ws = r.split && ctx->opt_cnn_ws && can.ws;
    r.ws_dense = r.ws && ctx->opt_cnn_ws_dense && can.ws_dense;
    return r;
}

int f2_launch_cnn(f2_ctx* ctx, const f2_cnn* cnn, const f2_scale_set* S, f2_cnn_route route, const float* d_x, int64_t n, float* d_ws,
                  float* d_scores, uint8_t* d_labels) {
    if (n <= 0) return F2_OK;
    const Dims d = make_dims(cnn->rows, cnn->channels);
    float* a4 = d_ws + (size_t)n * d.Hp1 * d.Wp1 * (C2 + C3);
    F2_TRY(f2_launch_cnn_convs(ctx, cnn, S, route, d_x, n, d_ws, a4));
    return f2_launch_cnn_dense(ctx, cnn, S, route, a4, n, a4 + (size_t)n * d.flat, d_scores, d_labels);
}

// conv1 .. conv4 + pools of n windows: d_ws = workspace of (Hp1 Wp1 (C2 + C3)) floats per window, a4 = [n][flat] out
int f2_launch_cnn_convs(f2_ctx* ctx, const f2_cnn* cnn, const f2_scale_set* S, f2_cnn_route route, const float* d_x, int64_t n,
                        float* d_ws, float* a4) {
    if (n <= 0) return F2_OK;
    const Dims d = make_dims(cnn->rows, cnn->channels);
    float* a2 = d_ws;
    float* a3 = a2 + (size_t)n * d.Hp1 * d.Wp1 * C2;
    F2_TRY(f2_prof_begin(ctx, F2_K_CNN));
    if (route.ws) {
        // weight-stationary persistent kernels (f2_cnn_ws.hip): conv1 on the matrix cores, one barrier per tile
        F2_TRY(f2_launch_cnn_ws(ctx, cnn, S, d_x, n, a2, a4));
    } else {
        F2_TRY(launch_conv12(ctx, cnn, S, route.split, d, d_x, n, a2));
        F2_TRY(launch_conv34(ctx, cnn, S, route.split, d, a2, n, a3, a4));
    }
    return f2_prof_end(ctx, F2_K_CNN);
}

// dense1 + dense2 + softmax + labels of n windows from a4 = [n][flat]; a5 = workspace of D1 floats per window. Its workgroups
// are (64 windows x 6 of the 17 output tiles): launched per 14 240-window utterance that is 669 workgroups for 512 resident
// ones - a second round one third full - so f2_eval_batch hands it the windows of several utterances at once.
int f2_launch_cnn_dense(f2_ctx* ctx, const f2_cnn* cnn, const f2_scale_set* S, f2_cnn_route route, const float* a4, int64_t n, float* a5,
                        float* d_scores, uint8_t* d_labels, bool with_dense2) {
    if (n <= 0) return F2_OK;
    const Dims d = make_dims(cnn->rows, cnn->channels);
    F2_TRY(f2_prof_begin(ctx, F2_K_CNN));
    constexpr int MT16 = D1_MT;   // (3 - 96 windows, one round of workgroups per 14 240-window chunk - measured slower: 0.165 against 0.157 ms)
    const dim3 grid((unsigned)((n + 32 * D1_MT - 1) / (32 * D1_MT)), (D1_TILES + D1_WAVES - 1) / D1_WAVES);
    if (route.ws_dense && f2_dense1_ws_takes(d.flat, n)) {   // (a launch beyond its 4 GB of activations: the per-tile kernel)
        F2_TRY(f2_launch_dense1_ws(ctx, cnn, S, a4, n, d.flat, a5));
    } else if (route.split) {
        f2_split_scales sc = S->sc;
        if (d.Hp1 != 4) sc.sin_d = S->sa_d1;     // (conv3 / conv4 of such windows ran on the float32 kernels: true units)
        hipLaunchKernelGGL(k_dense1_h16x3<MT16>, grid, dim3(D1_WAVES * 64), 0, ctx->stream, a4, (const h16x8*)(cnn->blob16 + cnn->off16[3]),
                           cnn->t(9), a5, d.flat, n, sc);
    } else {
        hipLaunchKernelGGL(k_dense1_mfma, grid, dim3(D1_WAVES * 64), 0, ctx->stream, a4, cnn->t(8), cnn->t(9), a5, d.flat, n);
    }
    F2_HIP(ctx, hipGetLastError());
    if (with_dense2) {
        hipLaunchKernelGGL(k_dense2_softmax, dim3((unsigned)((n * 8 + 255) / 256)), dim3(256), 0, ctx->stream, a5, cnn->t(10),
                           cnn->t(11), d_scores, d_labels, n);
        F2_HIP(ctx, hipGetLastError());
    }
    return f2_prof_end(ctx, F2_K_CNN);
}

// (the counterpart of sin_d above: the routes whose conv4 output is not in true units)
float f2_cnn_a4_scale(const f2_cnn* cnn, const f2_scale_set* S, f2_cnn_route route) {
    return route.split && S && make_dims(cnn->rows, cnn->channels).Hp1 == 4 ? S->sa_d1 : 1.f;
}

// the split path's scales are powers of two inside [2^-20, 2^20]
static double pow2_floor(double v) { return v > 0 && std::isfinite(v) ? std::exp2(std::floor(std::log2(v))) : 1.0; }
constexpr double SCALE_LO = 0x1p-20, SCALE_HI = 0x1p20;
static double clamp_scale(double v) { return std::min(std::max(v, SCALE_LO), SCALE_HI); }

// Scales of the split path for network inputs bounded by |x| <= B = 2^e (f2_cnn_split.h): the L1 cascade from conv1's outputs for
// inputs up to B (upper bounds of every layer's input from the L1 norms of the weights before it) to the largest power of two that
// keeps each layer's scaled input at or below 2^14. e = 0 gives the scales f2_cnn_create has always used, and they are used
// whatever they are; for e > 0 S.ok is false when a scale would have to leave the clamp (the inputs are too large for fp16
// pieces: f2_cnn_forward takes the float32 kernels).
static void derive_scale_set(const f2_cnn_cascade& K, int e, f2_scale_set& S, std::vector<float>& sbias) {
    // upper bound of layer l's outputs for inputs bounded by `inb`
    auto l1_bound = [&](int l, double inb) {
        double worst = 0.0;
        for (size_t co = 0; co < K.l1[l].size(); ++co) worst = std::max(worst, K.l1[l][co] * inb + K.absb[l][co]);
        return worst;
    };
    const double B = std::exp2((double)e);
    double sa[5];                 // sa[l]: input scale of conv2, conv3, conv4, dense1; sa[4] = 1 (dense2 runs in float32)
    bool ok = true;
    double bound = l1_bound(0, B);       // conv1 outputs for inputs bounded by B
    for (int l = 0; l < 4; ++l) {
        const double q = 16384.0 / std::max(bound, 1e-30);
        ok = ok && q >= SCALE_LO;          // (false for an infinite or NaN bound too)
        sa[l] = clamp_scale(pow2_floor(q));
        bound = l1_bound(l + 1, bound);
    }
    sa[4] = 1.0;
    const double* sb = K.sb;
    S.sc.sa2 = (float)sa[0];
    S.sc.c2 = (float)(sa[1] / (sa[0] * sb[0]));
    S.sc.c3 = (float)(sa[2] / (sa[1] * sb[1]));
    S.sc.c4 = (float)(sa[3] / (sa[2] * sb[2]));
    S.sc.cd = (float)(1.0 / (sa[3] * sb[3]));
    S.sc.sin_d = 1.f;
    const double sin = e == 0 ? 1.0 : 16384.0 / B;   // k_conv12_ws's input scale (f2_cnn_split.h)
    S.sc.sin = (float)sin;
    S.sc.sw1 = (float)(sa[0] / sin);
    S.c2_true = (float)(1.0 / (sa[0] * sb[0]));
    S.sa_d1 = (float)sa[3];
    S.ok = e == 0 || (ok && e <= 126 && std::isfinite(S.sc.sw1));   // (sin stays a normal float32)
    sbias.assign(F2_SB_FLOATS, 0.f);
    for (size_t co = 0; co < K.b2.size(); ++co) sbias[F2_SB_B2 + co] = (float)(K.b2[co] * sa[1]);
    for (size_t co = 0; co < K.b3.size(); ++co) {
        sbias[F2_SB_B3I + co] = (float)(K.b3[co] * (sa[1] * sb[1]));   // accumulator-initial form (f2_cnn_ws.hip)
        sbias[F2_SB_B3F + co] = (float)(K.b3[co] * sa[2]);             // epilogue form
    }
    for (size_t co = 0; co < K.b4.size(); ++co) sbias[F2_SB_B4 + co] = (float)(K.b4[co] * sa[3]);
}

int f2_cnn_scale_set(f2_ctx* ctx, const f2_cnn* cnn, int e, const f2_scale_set** out) {
    *out = nullptr;
    if (!f2_cnn_capability(cnn).split || e < 0 || e > F2_BOUND_EXP_MAX) return F2_OK;
    std::lock_guard<std::mutex> lock(cnn->sets_mu);
    f2_scale_set* S = cnn->sets[e];
    if (!S) {
        S = new f2_scale_set();
        std::vector<float> sbias;
        derive_scale_set(cnn->cascade, e, *S, sbias);
        if (S->ok) {
            // a buffer of its own, filled in stream order (kernels in flight keep theirs); complete before any context can see it
            hipError_t err = hipMalloc((void**)&S->sbias, sbias.size() * sizeof(float));
            int rc = err == hipSuccess ? f2_upload_async(ctx, S->sbias, sbias.data(), sbias.size() * sizeof(float)) : F2_OK;
            if (err == hipSuccess && rc == F2_OK) err = hipStreamSynchronize(ctx->stream);
            if (err != hipSuccess || rc != F2_OK) {
                if (S->sbias) (void)hipFree(S->sbias);
                delete S;
                return rc != F2_OK ? rc : f2_fail(ctx, F2_ERR_HIP, "scale set 2^%d of the CNN -> %s", e, hipGetErrorString(err));
            }
        }
        cnn->sets[e] = S;
    }
    if (S->ok) *out = S;
    return F2_OK;
}

// The weight-stationary kernels (f2_cnn_ws.hip) issue their global loads through inline asm and wait for them with hand-
// counted s_waitcnt; the compiler believes a loaded register valid at once, so a copy or spill it placed between load and
// wait would read stale data without any diagnostic - their correctness depends on the register allocation of the hipcc
// that built this library (round-4 advisor finding). So every network is run once, on a fixed batch, through those kernels
// and through the per-tile split-fp16 kernels (compiler-scheduled waits); a kernel that disagrees beyond the rounding level
// of the two summation orders is switched off for this network, loudly. The split path as a whole is then held against the
// float32 kernels, on that batch (B = 1) and on the batch times 2^10 with the scales of B = 2^10 (the sets f2_cnn_forward takes
// for inputs beyond [-1, 1]); if it disagrees, this network runs on the float32 kernels. Every run names its route: the
// context's options play no part.
static int cnn_selfcheck(f2_ctx* ctx, f2_cnn* cnn) {
    if (!cnn->blob16) return F2_OK;
    const bool ws_shape = f2_cnn_ws_supported(cnn->rows, cnn->channels);
    constexpr int NCHK = 200;     // two 96-window dense tiles + a partial one
    constexpr float TOL = 5e-6f;  // softmax scores; the two paths agree to ~1e-6 (tests/test_gpu_windows_cnn.py)
    constexpr int EBIG = 10;
    const size_t per = (size_t)cnn->rows * cnn->channels;
    std::vector<float> x(2 * per * NCHK);   // [the batch in [0, 1) | the batch x 2^EBIG]
    uint32_t lcg = 12345u;
    for (size_t k = 0; k < per * NCHK; ++k) {
        lcg = lcg * 1664525u + 1013904223u;
        x[k] = (float)(lcg >> 8) * (1.0f / 16777216.0f);
        x[per * NCHK + k] = x[k] * (float)(1 << EBIG);
    }
    const f2_scale_set* S1 = nullptr;
    const f2_scale_set* Sbig = nullptr;
    F2_TRY(f2_cnn_scale_set(ctx, cnn, 0, &S1));
    F2_TRY(f2_cnn_scale_set(ctx, cnn, EBIG, &Sbig));
    // runs: 0 per-tile split, 1 ws convolutions, 2 ws convolutions + ws dense1, 3 float32 kernels (B = 1 batch);
    //       4 per-tile split, 5 the weight-stationary kernels as decided from runs 0-2, 6 float32 kernels (2^10 batch)
    constexpr int NRUN = 7;
    const f2_cnn_route F32 = {false, false, false}, TILE = {true, false, false}, WS = {true, true, false}, WS_DENSE = {true, true, true};
    float *d_x = nullptr, *d_ws = nullptr, *d_sc = nullptr;
    const size_t wsf = f2_cnn_workspace_floats(cnn) * NCHK;
    auto cleanup = [&]() {
        if (d_x) (void)hipFree(d_x);
        if (d_ws) (void)hipFree(d_ws);
        if (d_sc) (void)hipFree(d_sc);
    };
    if (hipMalloc((void**)&d_x, x.size() * 4) != hipSuccess || hipMalloc((void**)&d_ws, wsf * 4) != hipSuccess ||
        hipMalloc((void**)&d_sc, NRUN * 2 * NCHK * 4) != hipSuccess) {
        cleanup();
        return f2_fail(ctx, F2_ERR_NOMEM, "self-check buffers of the CNN kernels");
    }
    const bool prof = ctx->prof_on;
    ctx->prof_on = false;
    std::vector<float> sc(NRUN * 2 * NCHK, 0.f);
    std::vector<bool> ran(NRUN, false);
    int rc = F2_OK;
    hipError_t e = hipMemcpyAsync(d_x, x.data(), x.size() * 4, hipMemcpyHostToDevice, ctx->stream);
    auto run = [&](int k, int big, const f2_scale_set* S, f2_cnn_route route) {
        if (e != hipSuccess || rc != F2_OK) return;
        rc = f2_launch_cnn(ctx, cnn, S, route, d_x + (size_t)big * per * NCHK, NCHK, d_ws, d_sc + (size_t)k * 2 * NCHK, nullptr);
        ran[k] = true;
    };
    auto fetch = [&]() {
        if (e == hipSuccess && rc == F2_OK) e = hipMemcpyAsync(sc.data(), d_sc, sc.size() * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && rc == F2_OK) e = hipStreamSynchronize(ctx->stream);
    };
    auto maxdiff = [&](int a, int b) {
        float m = 0.f;
        for (int i = 0; i < 2 * NCHK; ++i) {
            const float dv = fabsf(sc[(size_t)a * 2 * NCHK + i] - sc[(size_t)b * 2 * NCHK + i]);
            m = dv == dv ? fmaxf(m, dv) : INFINITY;   // NaN counts as a mismatch
        }
        return m;
    };
    run(0, 0, S1, TILE);
    if (ws_shape) {
        run(1, 0, S1, WS);
        run(2, 0, S1, WS_DENSE);
    }
    run(3, 0, nullptr, F32);
    fetch();
    if (ws_shape && e == hipSuccess && rc == F2_OK) {
        cnn->ws_check_diff = maxdiff(1, 0);
        cnn->ws_dense_check_diff = maxdiff(2, 1);
        if (!(cnn->ws_check_diff <= TOL)) {
            cnn->ws_ok = cnn->ws_dense_ok = false;
            fprintf(stderr, "[libf2cnn_hip] weight-stationary CNN kernels disagree with the per-tile kernels by %.3g on the "
                            "self-check batch (built by another hipcc than they were validated with?): not used for this network\n",
                    (double)cnn->ws_check_diff);
        } else if (!(cnn->ws_dense_check_diff <= TOL)) {
            cnn->ws_dense_ok = false;
            fprintf(stderr, "[libf2cnn_hip] weight-stationary dense1 kernel disagrees with the per-tile kernel by %.3g on the "
                            "self-check batch: not used for this network\n", (double)cnn->ws_dense_check_diff);
        }
    }
    const f2_cnn_route can = f2_cnn_capability(cnn);   // the kernels this network will use, as decided from runs 0-2
    const int def1 = !can.ws ? 0 : can.ws_dense ? 2 : 1;   // ... and their B = 1 run
    if (Sbig) {
        run(4, 1, Sbig, TILE);
        if (can.ws) run(5, 1, Sbig, can.ws_dense ? WS_DENSE : WS);
        run(6, 1, nullptr, F32);
        fetch();
    }
    ctx->prof_on = prof;
    cleanup();
    if (rc != F2_OK) return rc;
    if (e != hipSuccess) return f2_fail(ctx, F2_ERR_HIP, "self-check of the CNN kernels -> %s", hipGetErrorString(e));
    // (at 2^10 the logits are ~2^10 x larger, and so is the score difference the same relative rounding in them makes near the
    // decision boundary - between the float32 kernels and the float64 referee as much as here: it is taken per unit of input bound)
    float d16 = fmaxf(maxdiff(0, 3), maxdiff(def1, 3));
    if (ran[4]) d16 = fmaxf(d16, maxdiff(4, 6) / (float)(1 << EBIG));
    if (ran[5]) d16 = fmaxf(d16, maxdiff(5, 6) / (float)(1 << EBIG));
    cnn->f16x3_check_diff = d16;
    if (!(d16 <= TOL)) {
        cnn->f16x3_ok = false;
        fprintf(stderr, "[libf2cnn_hip] split-fp16 CNN kernels disagree with the float32 kernels by %.3g on the self-check "
                        "batch: this network runs on the float32 kernels\n", (double)d16);
    }
    return F2_OK;
}

static void free_cnn(f2_cnn* cnn) {
    if (cnn->blob) (void)hipFree(cnn->blob);
    if (cnn->blob16) (void)hipFree(cnn->blob16);
    if (cnn->grad_blob) (void)hipFree(cnn->grad_blob);
    for (f2_scale_set* S : cnn->sets) {
        if (!S) continue;
        if (S->sbias) (void)hipFree(S->sbias);
        delete S;
    }
    delete cnn;
}

// ---- f2_cnn_create's packing of the weights. A layer's kernel in its Keras layout is the K x N operand w[k][n] of its GEMM
// (convolutions: k = (dy*3+dx)*Cin + ci) ----

// The float32 kernels' MFMA B operand (cnn_b_operand_index, zero beyond N): conv2 .. conv4 with blk = Cin (a block per tap), dense1
// with blk = D1_KC
static std::vector<float> relayout_f32(const float* w, size_t K, int N, int blk, int npad) {
    std::vector<float> dst(K * npad, 0.f);
    for (size_t k = 0; k < K; ++k)
        for (int n = 0; n < N; ++n) dst[cnn_b_operand_index(k, n, blk, npad)] = w[k * N + n];
    return dst;
}

// What the scales' L1 cascade needs (derive_scale_set): per layer and output column the L1 norm of the weights and |bias|, the
// weight scales sb = the power of two that puts max |w| into [2^10, 2^11), and the biases of conv2 .. conv4
static void capture_cascade(f2_cnn_cascade& K, const float* const* tensors, int flat) {
    auto keep_l1 = [&](int l, const float* w, const float* b, size_t kin, size_t cout) {
        K.l1[l].resize(cout);
        K.absb[l].resize(cout);
        for (size_t co = 0; co < cout; ++co) {
            double acc = 0.0;
            for (size_t k = 0; k < kin; ++k) acc += std::fabs((double)w[k * cout + co]);
            K.l1[l][co] = acc;
            K.absb[l][co] = std::fabs((double)b[co]);
        }
    };
    const size_t kin[4] = {9 * (size_t)C1, 9 * (size_t)C2, 9 * (size_t)C3, (size_t)flat};
    const size_t cout[4] = {C2, C3, C4, D1};
    keep_l1(0, tensors[0], tensors[1], 9, C1);
    for (int l = 0; l < 4; ++l) {
        const float* w = tensors[2 + 2 * l];
        double m = 0.0;
        for (size_t k = 0; k < kin[l] * cout[l]; ++k) m = std::max(m, std::fabs((double)w[k]));
        K.sb[l] = clamp_scale(pow2_floor(2048.0 / std::max(m, 1e-30)));
        keep_l1(l + 1, w, tensors[3 + 2 * l], kin[l], cout[l]);
    }
    K.b2.assign(tensors[3], tensors[3] + C2);
    K.b3.assign(tensors[5], tensors[5] + C3);
    K.b4.assign(tensors[7], tensors[7] + C4);
}

// A layer for the split-fp16 kernels (f2_cnn_split.h), appended to w16: w[piece][k / 16][h][n (npad, zero beyond N)][8] with
// k = 16 (k / 16) + 8 h + e (convolutions: [tap][kb]; dense1: [chunk][ks]), piece 0 = fp16(w scale), piece 1 = fp16(w scale - piece 0).
// Returns the layer's element offset in w16.
static size_t pack_f16_pieces(std::vector<uint16_t>& w16, const float* w, size_t K, int N, int npad, float scale) {
    const size_t pos = w16.size(), per_piece = K * npad;
    w16.resize(pos + 2 * per_piece, 0);
    for (size_t k = 0; k < K; ++k)
        for (int n = 0; n < N; ++n) {
            const float wv = w[k * N + n] * scale;
            const _Float16 p0 = (_Float16)wv, p1 = (_Float16)(wv - (float)p0);   // round to nearest even, subnormals kept (as v_cvt_f16_f32)
            const size_t idx = ((k / 8) * npad + n) * 8 + k % 8;
            memcpy(&w16[pos + idx], &p0, 2);
            memcpy(&w16[pos + per_piece + idx], &p1, 2);
        }
    return pos;
}

extern "C" {

int f2_cnn_create(f2_ctx* ctx, const float* const* tensors, int rows, int channels, f2_cnn** out) {
    F2_CHECK(nullptr, ctx, F2_ERR_INVALID, "ctx is NULL");
    F2_CHECK(ctx, tensors && out, F2_ERR_INVALID, "null argument");
    *out = nullptr;
    const Dims d = make_dims(rows, channels);
    F2_CHECK(ctx, rows >= 3 && channels >= 3 && d.flat > 0, F2_ERR_INVALID,
             "input of %d x %d is too small for the network (needs a non-empty flatten)", rows, channels);
    // (every shape f2_cnn_ws_supported accepts has Hp2 = 1 and Wp2 >= 3: flat = 64 Wp2 >= 192 meets k_dense1_ws's conditions on K,
    // so whether it takes a launch depends on the window count alone - f2_launch_cnn_dense)
    const size_t sizes[12] = {9 * C1, C1, 9 * (size_t)C1 * C2, C2, 9 * (size_t)C2 * C3, C3, 9 * (size_t)C3 * C4, C4,
                              (size_t)d.flat * D1, D1, (size_t)D1 * D2, D2};
    for (int i = 0; i < 12; ++i) F2_CHECK(ctx, tensors[i], F2_ERR_INVALID, "weight tensor %d is NULL", i);
    size_t dev_sizes[12];   // (dense1 kernel: output dimension padded to whole MFMA tiles)
    for (int i = 0; i < 12; ++i) dev_sizes[i] = i == 8 ? (size_t)d.flat * D1_NPAD : sizes[i];
    F2_HIP(ctx, hipSetDevice(ctx->device));
    f2_cnn* cnn = new f2_cnn();
    cnn->rows = rows;
    cnn->channels = channels;
    cnn->flat = d.flat;
    cnn->dev = ctx->device;
    size_t total = 0;
    for (int i = 0; i < 12; ++i) {
        cnn->off[i] = total;
        total += (dev_sizes[i] + 63) & ~size_t(63);   // keep every tensor 256-byte aligned
    }
    hipError_t e = hipMalloc((void**)&cnn->blob, total * sizeof(float));
    if (e != hipSuccess) {
        delete cnn;
        return f2_fail(ctx, F2_ERR_NOMEM, "hipMalloc(%zu) -> %s", total * sizeof(float), hipGetErrorString(e));
    }
    // conv2 .. conv4 and dense1 kernels are stored as the MFMA B operand; everything else stays in its Keras layout
    const int conv_cin[3] = {C1, C2, C3}, conv_cout[3] = {C2, C3, C4};
    std::vector<std::vector<float>> relaid(12);
    for (int l = 0; l < 3; ++l) relaid[2 + 2 * l] = relayout_f32(tensors[2 + 2 * l], 9 * (size_t)conv_cin[l], conv_cout[l], conv_cin[l], conv_cout[l]);
    relaid[8] = relayout_f32(tensors[8], (size_t)d.flat, D1, D1_KC, D1_NPAD);
    // ... and once more, scaled and in two fp16 pieces, for the split-fp16 kernels
    capture_cascade(cnn->cascade, tensors, d.flat);
    const double* sb = cnn->cascade.sb;
    std::vector<uint16_t> w16;
    for (int l = 0; l < 3; ++l)
        cnn->off16[l] = pack_f16_pieces(w16, tensors[2 + 2 * l], 9 * (size_t)conv_cin[l], conv_cout[l], conv_cout[l], (float)sb[l]);
    cnn->off16[3] = pack_f16_pieces(w16, tensors[8], (size_t)d.flat, D1, D1_NPAD, (float)sb[3]);
    const size_t zeros_at = (w16.size() + 127) & ~size_t(127);
    w16.resize(zeros_at + 128, 0);   // 256 zero bytes, 256-byte aligned
    e = hipMalloc((void**)&cnn->blob16, w16.size() * sizeof(uint16_t));
    if (e == hipSuccess) cnn->zeros = cnn->blob16 + zeros_at;
    if (e == hipSuccess)
        e = hipMemcpyAsync(cnn->blob16, w16.data(), w16.size() * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream);
    for (int i = 0; e == hipSuccess && i < 12; ++i) {
        const float* src = relaid[i].empty() ? tensors[i] : relaid[i].data();
        e = hipMemcpyAsync(cnn->blob + cnn->off[i], src, dev_sizes[i] * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        free_cnn(cnn);
        return f2_fail(ctx, F2_ERR_HIP, "uploading CNN weights -> %s", hipGetErrorString(e));
    }
    const int rc = cnn_selfcheck(ctx, cnn);   // (builds the scale set of B = 1 first)
    if (rc != F2_OK) {
        free_cnn(cnn);
        return rc;
    }
    *out = cnn;
    return F2_OK;
}

int f2_cnn_get_info(f2_ctx* ctx, const f2_cnn* cnn, const char* key, double* value) {
    F2_CHECK(nullptr, ctx, F2_ERR_INVALID, "ctx is NULL");
    F2_CHECK(ctx, cnn && key && value, F2_ERR_INVALID, "null argument");
    const f2_cnn_route can = f2_cnn_capability(cnn);
    if (strcmp(key, "ws_ok") == 0) *value = can.ws ? 1.0 : 0.0;
    else if (strcmp(key, "ws_dense_ok") == 0) *value = can.ws_dense ? 1.0 : 0.0;
    else if (strcmp(key, "ws_check_diff") == 0) *value = (double)cnn->ws_check_diff;
    else if (strcmp(key, "ws_dense_check_diff") == 0) *value = (double)cnn->ws_dense_check_diff;
    else if (strcmp(key, "flat") == 0) *value = (double)cnn->flat;
    else if (strcmp(key, "f16x3_ok") == 0) *value = can.split ? 1.0 : 0.0;
    else if (strcmp(key, "f16x3_check_diff") == 0) *value = (double)cnn->f16x3_check_diff;
    else if (strcmp(key, "last_input_bound") == 0) *value = cnn->last_input_bound;
    else return f2_fail(ctx, F2_ERR_INVALID, "unknown key '%s'", key);
    return F2_OK;
}

int f2_cnn_destroy(f2_ctx* ctx, f2_cnn* cnn) {
    if (!cnn) return F2_OK;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    free_cnn(cnn);
    return F2_OK;
}

}  // extern "C"
