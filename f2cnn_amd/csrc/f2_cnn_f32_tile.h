// Device pieces of K4's float32 matrix-core kernels (v_mfma_f32_32x32x2_f32: bit for bit an fmaf chain), shared by f2_cnn.hip,
// f2_cnn_grad.hip and f2_cnn_train.hip; f2_cnn_dims.h has the shape arithmetic, f2_cnn_unpool.h the un-pool rule.
//
// The tile. One task = 2 output rows x 32 output columns of one window. Its 4 x 34 x CIN input patch sits in LDS at a
// (CIN + 4)-float pitch per pixel (16-byte aligned, conflict-free for ds_read_b128). Lane = (pixel i, half h): MFMA step s of a
// tap multiplies channel s (h = 0) and channel CIN / 2 + s (h = 1), so four steps are one 16-byte LDS read of the patch (A operand,
// lane = pixel) and one 16-byte load of the re-laid-out weights wt[tap][h][s/4][cout][s%4] (B operand, lane = Cout;
// cnn_b_operand_index). The 32 x 32 accumulator keeps output pixels acc_row(q, h) of channel i in register q: pixel pairs
// (2t, 2t + 1) share a lane, so a 2 x 2 max-pool needs no cross-lane traffic inside a row.
#ifndef F2_CNN_F32_TILE_H
#define F2_CNN_F32_TILE_H

#include "f2_cnn_dims.h"
#include "f2_cnn_unpool.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the row of a 32 x 32 MFMA accumulator that register q of the lanes of half h holds
__device__ __forceinline__ int acc_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

// ---- the 9-tap loop: acc[r][t] = sum over taps and channels of patch row r (shifted by the tap) x weight tile t ----
// pa0: this lane's pixel of the first output row in the patch (pitch PS floats, + h CIN / 2); row r is PW pixels further.
// wq: this lane's float4 of the first tile (+ h CIN / 8 weight rows of WS float4); tile t is 32 float4 further.
// The (tap, q) steps are software pipelined: the A (LDS) and B (weights) operands of step it + 1 are requested before the
// 4 ROWS NT MFMAs of step it are issued, so their latency hides behind matrix-core time instead of stalling the wave after them.
template <int CIN, int WS, int PS, int ROWS, int NT>
__device__ __forceinline__ void conv_taps(const float* pa0, const float4* wq, f32x16 (&acc)[ROWS][NT]) {
    constexpr int QN = CIN / 8, NIT = 9 * QN;
#pragma unroll
    for (int rr = 0; rr < ROWS; ++rr)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[rr][nt][q] = 0.f;
    float4 av[2][ROWS], bq[2][NT];
    auto fetch = [&](int it, int buf) {
        const int tap = it / QN, q = it - tap * QN;
        const int dy = tap / 3, dx = tap - dy * 3;
        const float* pa = pa0 + (dy * PW + dx) * PS;
        const float4* pb = wq + (int64_t)tap * 2 * QN * WS;
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) av[buf][rr] = *reinterpret_cast<const float4*>(pa + rr * PW * PS + 4 * q);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bq[buf][nt] = pb[(int64_t)q * WS + nt * 32];
    };
    fetch(0, 0);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int cur = it & 1;
        if (it + 1 < NIT) fetch(it + 1, cur ^ 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float4 bb = bq[cur][nt];
                const float bv = r == 0 ? bb.x : r == 1 ? bb.y : r == 2 ? bb.z : bb.w;
#pragma unroll
                for (int rr = 0; rr < ROWS; ++rr) {
                    const float4 aa = av[cur][rr];
                    const float a = r == 0 ? aa.x : r == 1 ? aa.y : r == 2 ? aa.z : aa.w;
                    acc[rr][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[rr][nt], 0, 0, 0);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- patch[r][p][c] (ROWS x 34 pixels at pitch CIN + 4) = the input at row y0 + r, column x0 + p, zero outside the image ('same'
// and 'full' padding, tile overhang); 16-byte pieces first, first + stride, .. are the caller's ----
//   ST_PLAIN   img (Hin, Win, CIN) is the input
//   ST_UNPOOL  the input is the un-pooled gradient of a 2 x 2 max-pool over (Hin, Win): img the pooled tensor's gradient, act the
//              pool's post-ReLU input
// UNROLL: the per-layer kernel's figures are recorded with two pieces in flight; the kernels that hold accumulators or a second
// tile across the staging keep the rolled loop, which costs them fewer registers.
template <int ROWS, int CIN, int STAGE = ST_PLAIN, int UNROLL = 1>
__device__ __forceinline__ void stage_patch(float* patch, const float* img, const float* act, int Hin, int Win, int y0, int x0, int first,
                                            int stride) {
    constexpr int PS = CIN + 4, Q4 = CIN / 4;
#pragma unroll UNROLL
    for (int e = first; e < ROWS * PW * Q4; e += stride) {
        const int r = e / (PW * Q4);
        const int rem = e - r * (PW * Q4);
        const int p = rem / Q4, c4 = rem - p * Q4;
        const int yi = y0 + r, xi = x0 + p;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (STAGE == ST_PLAIN) {
            if (yi >= 0 && yi < Hin && xi >= 0 && xi < Win) v = *reinterpret_cast<const float4*>(img + ((int64_t)yi * Win + xi) * CIN + c4 * 4);
        } else {
            v = unpool4<CIN>(img, act, Hin, Win, yi, xi, c4);
        }
        *reinterpret_cast<float4*>(patch + (r * PW + p) * PS + c4 * 4) = v;
    }
}

// ---- 2 x 2 max-pool of two waves' accumulators, the two conv rows of one pooled row: horizontal pairs sit in one lane; the wave
// of the odd row hands its eight pair maxima to the other through xch (512 floats nobody else uses), where m[k] becomes the
// maximum of columns acc_row(2 k, h), + 1 of both rows. One barrier inside. ----
__device__ __forceinline__ void pool_exchange(const f32x16& acc, float* xch, bool odd, int lane, float (&m)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) m[k] = fmaxf(acc[2 * k], acc[2 * k + 1]);
    if (odd) {
#pragma unroll
        for (int k = 0; k < 8; ++k) xch[k * 64 + lane] = m[k];
    }
    __syncthreads();
    if (!odd) {
#pragma unroll
        for (int k = 0; k < 8; ++k) m[k] = fmaxf(m[k], xch[k * 64 + lane]);
    }
}

// ---- the row GEMM: acc[t] = rows w0 + 32 t .. of a (n, K) . output tile nt of w (K, N), K a multiple of 64 and N of 32 ----
// One workgroup of WAVES waves = GEMM_ROWS rows (two M tiles) x WAVES output tiles, every weight load feeds both M tiles. K is walked
// in chunks of 64: the 64 x 64 chunk of a is staged in LDS (As, double buffered, 16-byte loads, pitch 68) and read back as the A
// operand with ds_read_b128; the B operand comes from wt[chunk][h][q][n][4], k = 64 chunk + 32 h + 4 q + e, one 16-byte load per
// four MFMA steps. Waves that are not `live` (no tile) only stage.
constexpr int GEMM_ROWS = 64;
constexpr int GEMM_PS = D1_KC + 4;
template <int WAVES>
__device__ __forceinline__ void gemm_rows_tile(const float* __restrict__ a, const float* __restrict__ wt, int K, int N, int64_t n, int64_t w0,
                                               int nt, bool live, float (&As)[2][GEMM_ROWS * GEMM_PS], f32x16 (&acc)[2]) {
    constexpr int KC = D1_KC, PS = GEMM_PS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const int nchunks = K / KC;

    auto stage = [&](int kc, int buf) {
        for (int e = tid; e < GEMM_ROWS * (KC / 4); e += WAVES * 64) {
            const int row = e / (KC / 4), c4 = e - row * (KC / 4);
            const int64_t wr = w0 + row < n ? w0 + row : n - 1;
            *reinterpret_cast<float4*>(&As[buf][row * PS + c4 * 4]) = *reinterpret_cast<const float4*>(a + wr * K + (int64_t)kc * KC + c4 * 4);
        }
    };
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;

    stage(0, 0);
    __syncthreads();
    for (int kc = 0; kc < nchunks; ++kc) {
        const int buf = kc & 1;
        if (kc + 1 < nchunks) stage(kc + 1, buf ^ 1);
        if (live) {
            const float* pa = &As[buf][i * PS + h * (KC / 2)];
            const float4* pb = reinterpret_cast<const float4*>(wt) + ((int64_t)(kc * 2 + h) * (KC / 8)) * N + nt * 32 + i;
#pragma unroll
            for (int q = 0; q < KC / 8; ++q) {
                const float4 bv = pb[(int64_t)q * N];
                float4 av[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) av[t] = *reinterpret_cast<const float4*>(pa + t * 32 * PS + 4 * q);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float b = r == 0 ? bv.x : r == 1 ? bv.y : r == 2 ? bv.z : bv.w;
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const float av_r = r == 0 ? av[t].x : r == 1 ? av[t].y : r == 2 ? av[t].z : av[t].w;
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av_r, b, acc[t], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ---- a 3 x 3 convolution layer with padding PAD (0 'valid', 1 'same', 2 'full') as an implicit GEMM: the forward layers and, with
// the kernel rotated by 180 degrees and Cin and Cout swapped, their backward-data passes ----
// Output (Ho, Wo) = (Hin, Win) + 2 PAD - 2, COUT channels. NSPLIT waves share one task (one patch): each stages its share of it and
// takes COUT / 32 / NSPLIT of the output tiles, so a 64-channel layer keeps twice the waves per CU for the same LDS.
// Staging: stage_patch's ST_PLAIN (`in` (n, Hin, Win, CIN)) or ST_UNPOOL (`in` (n, Hin / 2, Win / 2, CIN), `act` (n, Hin, Win, CIN)).
//   EP_RELU    out (n, Ho, Wo, COUT) = max(acc + aux[cout], 0)          (aux: the layer's biases)
//   EP_MASK    out = aux[same index as out] > 0 ? acc : 0               (aux: the post-ReLU activations of the layer the gradient enters)
//   EP_NONE    out = acc
//   EP_POOL    out (n, Ho / 2, Wo / 2, COUT) = the 2 x 2 max-pool of EP_RELU's, from the accumulators: the second row of a pooled
//              cell is the wave's second M tile. Its tasks are the Ho / 2 row pairs and (Wo / 2) * 2 columns the pool keeps.
__host__ __device__ __forceinline__ void conv3x3_tasks(int Ho, int Wo, bool pool, int* row_pairs, int* xtiles) {
    *row_pairs = pool ? Ho / 2 : (Ho + 1) / 2;
    *xtiles = ((pool ? (Wo / 2) * 2 : Wo) + 31) / 32;
}

template <int CIN, int COUT, int PAD, int STAGE, int EPI, int WAVES, int NSPLIT>
__global__ __launch_bounds__(WAVES * 64) void k_conv3x3_f32(const float* __restrict__ in, const float* __restrict__ act,
                                                            const float* __restrict__ w, const float* __restrict__ aux, float* __restrict__ out,
                                                            int Hin, int Win, int64_t nwin) {
    constexpr int PS = CIN + 4;
    constexpr int PATCH = 4 * PW * PS;
    constexpr int NT = COUT / 32 / NSPLIT;
    constexpr int TPB = WAVES / NSPLIT;
    constexpr int HALF = CIN / 2;
    static_assert(NT >= 1 && TPB >= 1 && CIN % 8 == 0, "tile shape");
    extern __shared__ __attribute__((aligned(16))) float lds_all[];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ns = wave % NSPLIT;
    float* patch = lds_all + (wave / NSPLIT) * PATCH;

    const int Ho = Hin + 2 * PAD - 2, Wo = Win + 2 * PAD - 2;
    int row_pairs, xtiles;
    conv3x3_tasks(Ho, Wo, EPI == EP_POOL, &row_pairs, &xtiles);
    const int64_t tasks = nwin * row_pairs * xtiles;
    int64_t task = (int64_t)blockIdx.x * TPB + wave / NSPLIT;
    const bool live = task < tasks;
    if (!live) task = tasks - 1;
    const int xt = (int)(task % xtiles);
    const int64_t t2 = task / xtiles;
    const int rp = (int)(t2 % row_pairs);
    const int64_t win = t2 / row_pairs;
    const int y0 = 2 * rp, x0 = 32 * xt;

    const float* img = in + win * (STAGE == ST_UNPOOL ? (int64_t)(Hin / 2) * (Win / 2) : (int64_t)Hin * Win) * CIN;
    const float* aimg = STAGE == ST_UNPOOL ? act + win * (int64_t)Hin * Win * CIN : nullptr;
    stage_patch<4, CIN, STAGE, 2>(patch, img, aimg, Hin, Win, y0 - PAD, x0 - PAD, lane + 64 * ns, 64 * NSPLIT);
    __syncthreads();

    const int i = lane & 31, h = lane >> 5;
    f32x16 acc[2][NT];
    conv_taps<CIN, COUT, PS, 2, NT>(patch + i * PS + h * HALF, reinterpret_cast<const float4*>(w) + (int64_t)h * (HALF / 4) * COUT + ns * NT * 32 + i,
                                    acc);

    if (!live) return;
    if constexpr (EPI == EP_POOL) {
        const int Wout = Wo / 2;
        float* o = out + win * (int64_t)row_pairs * Wout * COUT;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int co = (ns * NT + nt) * 32 + i;
            const float bv = aux[co];
#pragma unroll
            for (int q = 0; q < 16; q += 2) {
                const int px = (x0 + acc_row(q, h)) >> 1;
                const float m = fmaxf(fmaxf(acc[0][nt][q], acc[0][nt][q + 1]), fmaxf(acc[1][nt][q], acc[1][nt][q + 1]));
                if (px < Wout) o[((int64_t)rp * Wout + px) * COUT + co] = fmaxf(m + bv, 0.f);
            }
        }
    } else {
        const int64_t obase = win * (int64_t)Ho * Wo * COUT;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int co = (ns * NT + nt) * 32 + i;
            const float bv = EPI == EP_RELU ? aux[co] : 0.f;
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int y = y0 + rr;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int xo = x0 + acc_row(q, h);
                    if (y < Ho && xo < Wo) {
                        const int64_t idx = obase + ((int64_t)y * Wo + xo) * COUT + co;
                        float v = acc[rr][nt][q];
                        if constexpr (EPI == EP_RELU) v = fmaxf(v + bv, 0.f);
                        if constexpr (EPI == EP_MASK) v = aux[idx] > 0.f ? v : 0.f;
                        out[idx] = v;
                    }
                }
            }
        }
    }
}

template <int CIN, int COUT, int PAD, int STAGE, int EPI, int WAVES, int NSPLIT>
int launch_conv3x3(f2_ctx* ctx, const float* in, const float* act, const float* w, const float* aux, float* out, int Hin, int Win, int64_t n) {
    int row_pairs, xtiles;
    conv3x3_tasks(Hin + 2 * PAD - 2, Win + 2 * PAD - 2, EPI == EP_POOL, &row_pairs, &xtiles);
    const int64_t tasks = n * row_pairs * xtiles;
    if (tasks <= 0) return F2_OK;
    constexpr int TPB = WAVES / NSPLIT;
    constexpr size_t lds = sizeof(float) * TPB * 4 * PW * (CIN + 4);
    static_assert(lds <= 160 * 1024, "a workgroup's patches fit the CU's LDS");
    auto kern = k_conv3x3_f32<CIN, COUT, PAD, STAGE, EPI, WAVES, NSPLIT>;
    if (lds > 64 * 1024) F2_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    unsigned blocks;
    F2_TRY(cnn_grid(ctx, (tasks + TPB - 1) / TPB, &blocks));
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(WAVES * 64), lds, ctx->stream, in, act, w, aux, out, Hin, Win, n);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

#endif
