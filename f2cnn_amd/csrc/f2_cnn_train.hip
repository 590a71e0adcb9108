// A training step of K4 on the device: f2_cnn_loss_gradient and the f2_trainer_* entry points (include/f2cnn_hip.h).
//
// The recorded forward and the backward-data chain are f2_cnn_grad.hip's, as the steps of an f2_grad_chain (f2_cnn_train.h);
// launch_loss_gradient here strings a step together from them and from what training adds, the kernels of this file:
//   k_dropout          inverted dropout in place on p1, p2 and a5, masks from Philox4x32-10 (the formula is in the header)
//   k_dense2_train     dense2 + softmax on the dropped a5, dz = softmax - onehot, the float64 loss term and the hit of every window
//   k_loss_seed        g5 = [a5 > 0] / keep (dz0 W2[k][0] + dz1 W2[k][1]), padded like k_grad_dense2's
//   k_mask_scale       the backward factor of a dropout layer: g = p > 0 ? g / keep : 0
//   k_wgrad_conv       conv2 .. conv4: dW[tap][ci][co] = sum over windows and pixels of in[pixel + tap][ci] g[pixel][co] on
//                      v_mfma_f32_32x32x2_f32 with the pixel as the MFMA's k; the task and the patch of f2_cnn_f32_tile.h
//                      (stage_patch) and beside the patch the task's 64 x COUT gradient tile, un-pooled while it is staged
//                      for conv2 / conv4 (unpool4). Wave w of a workgroup takes the kernel row w % 3 and
//                      the w / 3-th share of the output channels. The layer's bias gradient is the column sum of the same tile.
//   k_wgrad_conv1      conv1 (Cin = 1) and its bias on the VALU, float64
//   k_wgrad_dense1     p2^T g5 on the float64 matrix cores (exact products, float64 sums), the window as the MFMA's k
//   k_wgrad_head       dense2's kernel and bias and dense1's bias, float64 throughout
//   k_reduce_partials  the float64 sum of the partial sums, added to the float64 gradient
//   k_round_f32, k_rmsprop, k_relayout
// Summation rule. No float32 chain is longer than 1024 terms: a k_wgrad_conv workgroup takes at most WGRAD_MAX_PER = 16 tasks
// (64 pixels each) of ONE window - the window's tasks in equal shares, a function of the window shape alone - and writes its
// accumulators out as one partial sum, so a window's partial sums have the same bits wherever it stands and whatever else is in
// the batch. conv1, dense1, dense2 and the dense biases are float64 sums of exact products of float32 values. Partial sums are added in float64, in an order fixed by the shapes and the window count alone (eight
// interleaved runs over the partial index, then those eight in order), onto a float64 gradient that also carries the sum over
// the chain's chunks of <= 1024 windows and is rounded to float32 once (k_round_f32). No floating-point atomics, no atomics at all.
// gfx950, wave64. Everything that reaches memory is written by plain C++ stores.
#include <algorithm>
#include <cmath>

#include "f2_cnn_f32_tile.h"
#include "f2_cnn_train.h"
#include "f2_philox.h"

namespace {

constexpr int WGRAD_MAX_PER = 16;       // tasks of 64 pixels per partial sum, at most: 1024 terms
constexpr int C1_PIX = 256;             // pixels of a k_wgrad_conv1 workgroup: 8 runs of 32
constexpr int D1_SEG = 64;              // windows of a k_wgrad_dense1 partial sum (16 dependent steps of loads per wave)
constexpr int HEAD_COLS = D1 * D2 + D2 + D1;   // dense2 kernel, dense2 bias, dense1 bias

// ---- dropout: a thread per four elements (one Philox call), element e of window b uses word e & 3 of
// Philox(counter = (e >> 2, b, layer, step & 0xffffffff), key = (seed & 0xffffffff, seed >> 32)); kept iff word >= rate 2^32 ----
__global__ __launch_bounds__(256) void k_dropout(float* __restrict__ a, int64_t m, int per4, uint32_t layer, int64_t b0, double thresh,
                                                 float scale, uint32_t k0, uint32_t k1, uint32_t step) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= m * per4) return;
    const uint32_t q = (uint32_t)(t % per4);
    const int64_t wv = t / per4;
    const philox_words w = philox4x32_10(q, (uint32_t)(b0 + wv), layer, step, k0, k1);
    float4* p = reinterpret_cast<float4*>(a) + t;
    float4 v = *p;
    v.x = (double)w.w0 >= thresh ? v.x * scale : 0.f;
    v.y = (double)w.w1 >= thresh ? v.y * scale : 0.f;
    v.z = (double)w.w2 >= thresh ? v.z * scale : 0.f;
    v.w = (double)w.w3 >= thresh ? v.w * scale : 0.f;
    *p = v;
}

// ---- dense2 + softmax in training mode: k_dense2_softmax's eight threads per window and summation order ----
__global__ __launch_bounds__(256) void k_dense2_train(const float* __restrict__ a, const float* __restrict__ w, const float* __restrict__ bias,
                                                      const uint8_t* __restrict__ y, float* __restrict__ scores, float* __restrict__ dz,
                                                      double* __restrict__ lossw, uint8_t* __restrict__ hit, int64_t n) {
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
    const float mx = fmaxf(z0, z1);
    const float e0 = expf(z0 - mx), e1 = expf(z1 - mx);
    const float s = e0 + e1;
    const float s0 = e0 / s, s1 = e1 / s;
    scores[2 * i] = s0;
    scores[2 * i + 1] = s1;
    const bool rising = y[i] != 0;
    // softmax - onehot: the true class's entry is minus the other score (s - 1 would lose it where s is close to 1)
    const float d1 = rising ? -s0 : s1;
    dz[2 * i] = -d1;
    dz[2 * i + 1] = d1;
    // -ln softmax(z)[y] = ln(exp(z0 - mx) + exp(z1 - mx)) - (z_y - mx), in float64 from the float32 logits, no clipping
    const double t0 = (double)z0 - (double)mx, t1 = (double)z1 - (double)mx;
    lossw[i] = log(exp(t0) + exp(t1)) - (rising ? t1 : t0);
    hit[i] = (s1 > s0) == rising ? 1 : 0;
}

// ---- tally[0] += sum of lossw (float64: 256 interleaved runs, then those in thread order), tally[1] (int64) += hits ----
__global__ __launch_bounds__(256) void k_train_tally(const double* __restrict__ lossw, const uint8_t* __restrict__ hit, int64_t m,
                                                     double* __restrict__ tally) {
    __shared__ double sl[256];
    __shared__ int sh[256];
    double s = 0.0;
    int h = 0;
    for (int64_t i = threadIdx.x; i < m; i += 256) {
        s += lossw[i];
        h += hit[i];
    }
    sl[threadIdx.x] = s;
    sh[threadIdx.x] = h;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double total = 0.0;
    int64_t hits = 0;
    for (int t = 0; t < 256; ++t) {
        total += sl[t];
        hits += sh[t];
    }
    tally[0] += total;
    reinterpret_cast<int64_t*>(tally)[1] += hits;
}

__global__ __launch_bounds__(256) void k_loss_seed(const float* __restrict__ a5, const float* __restrict__ dz, const float* __restrict__ w2,
                                                   float scale, float* __restrict__ g5, int gk, int64_t n) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * gk) return;
    const int k = (int)(t % gk);
    const int64_t wv = t / gk;
    float g = 0.f;
    if (k < D1 && a5[wv * D1 + k] > 0.f) g = scale * fmaf(dz[2 * wv + 1], w2[2 * k + 1], dz[2 * wv] * w2[2 * k]);
    g5[t] = g;
}

__global__ __launch_bounds__(256) void k_mask_scale(float* __restrict__ g, const float* __restrict__ p, float scale, int64_t count) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    g[t] = p[t] > 0.f ? g[t] * scale : 0.f;
}

__global__ __launch_bounds__(256) void k_gather_indexed(const float* __restrict__ x, const uint8_t* __restrict__ y,
                                                        const int64_t* __restrict__ index, int64_t m, int64_t xs, float* __restrict__ xg,
                                                        uint8_t* __restrict__ yg) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= m * xs) return;
    const int64_t j = t / xs, e = t - j * xs;
    const int64_t src = index[j];
    xg[t] = x[src * xs + e];
    if (e == 0) yg[j] = y[src];
}

// ---- conv2 .. conv4 weight and bias gradients ----
// in (n, Hin, Win, CIN) the layer's input, padding PAD; the gradient at its pre-activations over (Ho, Wo) = (Hin, Win) + 2 PAD - 2:
//   ST_PLAIN   g (n, Ho, Wo, COUT)
//   ST_UNPOOL  g (n, Ho / 2, Wo / 2, COUT) the gradient of the pooled tensor, act (n, Ho, Wo, COUT) the pool's post-ReLU input
// Cells of a task outside the output - the second x-tile's unused columns, the missing row of an odd row pair, rows and columns the
// pool dropped - are zeros in the gradient tile, so their products are exact zeros.
// Workgroup b takes the tasks (b % gpw) per .. + per - 1 of window b / gpw and writes partial[b] = {dW (9, CIN, COUT) | db (COUT)}.
// MFMA operands: A[ci][k] = patch value of pixel 2 s + k shifted by the tap (lane = ci, conflict-free: a row of 32 floats), B[k][co] =
// the gradient tile's pixel 2 s + k (lane = co, likewise).
template <int CIN, int COUT, int PAD, int STAGE, int COSPLIT>
__global__ __launch_bounds__(3 * COSPLIT * 64) void k_wgrad_conv(const float* __restrict__ in, const float* __restrict__ g,
                                                                 const float* __restrict__ act, float* __restrict__ partial, int Hin, int Win,
                                                                 int64_t nwin, int per, int gpw) {
    constexpr int NTHR = 3 * COSPLIT * 64;
    constexpr int PS = CIN + 4, GS = COUT + 4;
    constexpr int CIT = CIN / 32, COT = COUT / 32 / COSPLIT;
    constexpr int QG = COUT / 4;
    constexpr int BPARTS = NTHR / COUT;   // the bias sum: thread (bpart, bco) adds every BPARTS-th pixel of column bco
    static_assert(COT >= 1 && CIN % 32 == 0 && COUT % 32 == 0 && NTHR % COUT == 0 && BPARTS * COUT <= 64 * GS, "tile shape");
    __shared__ __attribute__((aligned(16))) float patch[4 * PW * PS];
    __shared__ __attribute__((aligned(16))) float gt[64 * GS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int dy = wave % 3, cs = wave / 3;
    const int bco = tid % COUT, bpart = tid / COUT;
    const int Ho = Hin + 2 * PAD - 2, Wo = Win + 2 * PAD - 2;
    const int row_pairs = (Ho + 1) / 2, xtiles = (Wo + 31) / 32;
    const int tpw = row_pairs * xtiles;   // tasks per window
    const int64_t win = blockIdx.x / gpw;
    const int first = (int)(blockIdx.x % gpw) * per;
    const int last = first + per < tpw ? first + per : tpw;
    const float* img = in + win * (int64_t)Hin * Win * CIN;
    const float* gimg = g + win * (STAGE == ST_UNPOOL ? (int64_t)(Ho / 2) * (Wo / 2) : (int64_t)Ho * Wo) * COUT;
    const float* aimg = STAGE == ST_UNPOOL ? act + win * (int64_t)Ho * Wo * COUT : nullptr;

    f32x16 acc[3][CIT][COT];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx)
#pragma unroll
        for (int a = 0; a < CIT; ++a)
#pragma unroll
            for (int b = 0; b < COT; ++b)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[dx][a][b][q] = 0.f;
    float bsum = 0.f;

    for (int task = first; task < last; ++task) {
        const int xt = task % xtiles, rp = task / xtiles;
        const int y0 = 2 * rp, x0 = 32 * xt;
        stage_patch<4, CIN>(patch, img, nullptr, Hin, Win, y0 - PAD, x0 - PAD, tid, NTHR);
        for (int e = tid; e < 64 * QG; e += NTHR) {
            const int pix = e / QG, c4 = e - pix * QG;
            const int yo = y0 + (pix >> 5), xo = x0 + (pix & 31);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (STAGE == ST_PLAIN) {
                if (yo < Ho && xo < Wo) v = *reinterpret_cast<const float4*>(gimg + ((int64_t)yo * Wo + xo) * COUT + c4 * 4);
            } else {
                v = unpool4<COUT>(gimg, aimg, Ho, Wo, yo, xo, c4);
            }
            *reinterpret_cast<float4*>(gt + pix * GS + c4 * 4) = v;
        }
        __syncthreads();

#pragma unroll 2
        for (int s = 0; s < 32; ++s) {
            const int pix = 2 * s + h;
            const int rr = pix >> 5, col = pix & 31;
            float bv[COT];
#pragma unroll
            for (int b = 0; b < COT; ++b) bv[b] = gt[pix * GS + (cs * COT + b) * 32 + i];
            const float* pa = patch + ((rr + dy) * PW + col) * PS + i;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                for (int a = 0; a < CIT; ++a) {
                    const float av = pa[dx * PS + a * 32];
#pragma unroll
                    for (int b = 0; b < COT; ++b) acc[dx][a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[b], acc[dx][a][b], 0, 0, 0);
                }
        }
#pragma unroll 4
        for (int pix = bpart; pix < 64; pix += BPARTS) bsum += gt[pix * GS + bco];
        __syncthreads();
    }
    gt[bpart * COUT + bco] = bsum;   // (behind the loop's last barrier: nobody reads the tile any more)
    __syncthreads();

    float* P = partial + (int64_t)blockIdx.x * (9 * CIN * COUT + COUT);
#pragma unroll
    for (int dx = 0; dx < 3; ++dx)
#pragma unroll
        for (int a = 0; a < CIT; ++a)
#pragma unroll
            for (int b = 0; b < COT; ++b)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int ci = a * 32 + acc_row(q, h);
                    const int co = (cs * COT + b) * 32 + i;
                    P[((dy * 3 + dx) * CIN + ci) * COUT + co] = acc[dx][a][b][q];
                }
    if (tid < COUT) {
        float t = gt[tid];
        for (int part = 1; part < BPARTS; ++part) t += gt[part * COUT + tid];
        P[9 * CIN * COUT + tid] = t;
    }
}

// ---- conv1 ('same', Cin = 1): dW[tap][co] = sum x[y + dy - 1][x + dx - 1] g1[y][x][co], db[co] = sum g1 ----
// Workgroup b takes the pixels C1_PIX b .. of the chunk (all windows end to end): thread (run, co) adds every eighth of them in
// float64 (the products of two float32 values are exact there), the eight runs are added in run order
// -> partial[b] = {dW (9, 32) | db (32)} float64
__global__ __launch_bounds__(256) void k_wgrad_conv1(const float* __restrict__ x, const float* __restrict__ g1, double* __restrict__ partial, int H,
                                                     int W, int64_t nwin) {
    __shared__ double sm[8][10][C1];
    const int co = threadIdx.x & 31, run = threadIdx.x >> 5;
    const int64_t npix = nwin * H * W;
    const int64_t base = (int64_t)blockIdx.x * C1_PIX;
    double acc[10];
#pragma unroll
    for (int t = 0; t < 10; ++t) acc[t] = 0.0;
    const int HW = H * W;
    int64_t win = (base + run) / HW;
    int rem = (int)(base + run - win * HW);   // the pixel's place in its window; eight further on every turn
    for (int j = 0; j < C1_PIX / 8; ++j, rem += 8) {
        const int64_t pix = base + run + 8 * j;
        if (pix >= npix) break;
        while (rem >= HW) rem -= HW, ++win;
        const int y = rem / W, xo = rem - y * W;
        const float* img = x + win * (int64_t)HW;
        const double gv = (double)g1[pix * C1 + co];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int yi = y - 1 + tap / 3, xi = xo - 1 + tap % 3;
            const float v = (yi >= 0 && yi < H && xi >= 0 && xi < W) ? img[(int64_t)yi * W + xi] : 0.f;
            acc[tap] = fma((double)v, gv, acc[tap]);
        }
        acc[9] += gv;
    }
#pragma unroll
    for (int t = 0; t < 10; ++t) sm[run][t][co] = acc[t];
    __syncthreads();
    for (int e = threadIdx.x; e < 10 * C1; e += 256) {
        double s = 0.0;
        for (int r = 0; r < 8; ++r) s += sm[r][e / C1][e % C1];
        partial[(int64_t)blockIdx.x * (10 * C1) + e] = s;
    }
}

// ---- dense1: dW[j][k] = sum over windows of p2[w][j] g5[w][k] ----
// On v_mfma_f64_16x16x4_f64 with the window as the MFMA's k: the product of two float32 values is exact in float64 and the sums
// are float64, so the gradient of a batch is the float64 sum of its windows' products, rounded once (a float32 chain over the
// windows of a batch is not: its roundings are as large as those of the terms themselves). A wave owns 64 rows j x 32 columns k of
// segment blockIdx.y (D1_SEG windows): 4 x 2 tiles of 16 x 16, operands straight from memory (lane & 15 = j resp. k, lane >> 4 =
// the window of the step's four). partial[seg] = dW (flat, 516) of that segment's windows, float64.
// C/D of this instruction: column = lane & 15, row = (lane >> 4) + 4 v for register v.
typedef double f64x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_wgrad_dense1(const float* __restrict__ p2, const float* __restrict__ g5, double* __restrict__ partial, int flat,
                                                      int gk, int64_t m) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int tile = blockIdx.x * 4 + wave;
    const int jt = tile / D1_TILES, kt = tile - jt * D1_TILES;
    if (jt >= flat / 64) return;   // (the whole wave; no barrier in this kernel)
    const int64_t w0 = (int64_t)blockIdx.y * D1_SEG;
    const int64_t w1 = w0 + D1_SEG < m ? w0 + D1_SEG : m;
    f64x4 acc[4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[a][b][v] = 0.0;
    const float* pa = p2 + jt * 64 + r;
    const float* pb = g5 + kt * 32 + r;
    const int steps = (int)((w1 - w0 + 3) / 4);
    for (int s = 0; s < steps; ++s) {
        const int64_t w = w0 + 4 * s + kq;
        const bool has = w < w1;
        double av[4], bv[2];
#pragma unroll
        for (int a = 0; a < 4; ++a) av[a] = has ? (double)pa[w * flat + a * 16] : 0.0;
#pragma unroll
        for (int b = 0; b < 2; ++b) bv[b] = has ? (double)pb[w * gk + b * 16] : 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
    double* P = partial + (int64_t)blockIdx.y * flat * D1;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int k = kt * 32 + b * 16 + r;
            if (k >= D1) continue;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int j = jt * 64 + a * 16 + kq + 4 * v;
                P[(int64_t)j * D1 + k] = acc[a][b][v];
            }
        }
}

// ---- dense2's kernel a5^T dz (516, 2), its bias sum dz (2) and dense1's bias sum g5 (516): float64 products and sums ----
// thread (run, column): every eighth window in ascending order, the eight runs added in run order
__global__ __launch_bounds__(256) void k_wgrad_head(const float* __restrict__ a5, const float* __restrict__ dz, const float* __restrict__ g5, int gk,
                                                    int64_t m, double* __restrict__ d2w, double* __restrict__ d2b, double* __restrict__ d1b) {
    __shared__ double sm[8][32];
    const int cx = threadIdx.x & 31, run = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cx;
    double s = 0.0;
    if (c < HEAD_COLS) {
        for (int64_t w = run; w < m; w += 8) {
            double v;
            if (c < D1 * D2) v = (double)a5[w * D1 + c / D2] * (double)dz[w * D2 + c % D2];
            else if (c < D1 * D2 + D2) v = (double)dz[w * D2 + (c - D1 * D2)];
            else v = (double)g5[w * gk + (c - D1 * D2 - D2)];
            s += v;
        }
    }
    sm[run][cx] = s;
    __syncthreads();
    if (run != 0 || c >= HEAD_COLS) return;
    double t = sm[0][cx];
    for (int r = 1; r < 8; ++r) t += sm[r][cx];
    if (c < D1 * D2) d2w[c] += t;
    else if (c < D1 * D2 + D2) d2b[c - D1 * D2] += t;
    else d1b[c - D1 * D2 - D2] += t;
}

// ---- acc[e] += sum over the np partial sums of partial[p][e], in float64: thread (run, e) adds every eighth partial in ascending
// order, the eight runs are added in run order ----
template <class T>
__global__ __launch_bounds__(256) void k_reduce_partials(const T* __restrict__ partial, int64_t np, int64_t stride, int64_t count,
                                                         double* __restrict__ acc) {
    __shared__ double sm[8][32];
    const int ex = threadIdx.x & 31, run = threadIdx.x >> 5;
    const int64_t e = (int64_t)blockIdx.x * 32 + ex;
    double s = 0.0;
    if (e < count) {
#pragma unroll 4
        for (int64_t p = run; p < np; p += 8) s += (double)partial[p * stride + e];
    }
    sm[run][ex] = s;
    __syncthreads();
    if (run != 0 || e >= count) return;
    double t = sm[0][ex];
    for (int r = 1; r < 8; ++r) t += sm[r][ex];
    acc[e] += t;
}

__global__ __launch_bounds__(256) void k_round_f32(const double* __restrict__ acc, float* __restrict__ out, int64_t count) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < count) out[t] = (float)acc[t];
}

__global__ __launch_bounds__(256) void k_rmsprop(float* __restrict__ p, float* __restrict__ a, const float* __restrict__ g, int64_t count, float m,
                                                 float lr_t, float rho, float one_minus_rho, float eps) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    const float gm = g[t] / m;
    const float an = fmaf(rho, a[t], one_minus_rho * (gm * gm));
    a[t] = an;
    p[t] = p[t] - lr_t * gm / (sqrtf(an) + eps);
}

struct relayout_args {
    size_t src[13];    // f2_train_tensor_layout
    size_t dst[12];    // cnn->off
    size_t gdst[4];    // conv2T, conv3T, conv4T, dense1T in grad_blob
    int flat;
};
// a thread per master weight: its place in cnn->blob (conv2 .. conv4 and dense1 as the MFMA B operand, the rest as they are) and,
// for those four, in grad_blob (the kernel turned by 180 degrees with Cin and Cout swapped; dense1 transposed)
__global__ __launch_bounds__(256) void k_relayout(const float* __restrict__ w, float* __restrict__ blob, float* __restrict__ gblob, relayout_args A) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= A.src[12]) return;
    int l = 0;
    size_t first = 0, dst = A.dst[0];
#pragma unroll
    for (int k = 1; k < 12; ++k)
        if (t >= A.src[k]) l = k, first = A.src[k], dst = A.dst[k];
    const size_t e = t - first;
    const float v = w[t];
    if (l == 2 || l == 4 || l == 6) {
        const int cin = l == 6 ? C3 : l == 4 ? C2 : C1, cout = l == 2 ? C2 : l == 4 ? C3 : C4;
        const int co = (int)(e % cout);
        const size_t k = e / cout;             // tap cin + ci
        const int ci = (int)(k % cin), tap = (int)(k / cin);
        blob[dst + cnn_b_operand_index(k, co, cin, cout)] = v;
        gblob[(l == 2 ? A.gdst[0] : l == 4 ? A.gdst[1] : A.gdst[2]) + cnn_b_operand_index((size_t)(8 - tap) * cout + co, ci, cout, cin)] = v;
    } else if (l == 8) {
        const int k = (int)(e % D1);
        const size_t j = e / D1;
        blob[dst + cnn_b_operand_index(j, k, D1_KC, D1_NPAD)] = v;
        gblob[A.gdst[3] + cnn_b_operand_index((size_t)k, (int)j, 64, A.flat)] = v;
    } else {
        blob[dst + e] = v;
    }
}

// a window's tasks of 64 pixels in gpw equal shares of per <= WGRAD_MAX_PER: a function of the window shape alone
struct wgrad_share {
    int per, gpw;
};
wgrad_share wgrad_shares(int Ho, int Wo) {
    const int tpw = ((Ho + 1) / 2) * ((Wo + 31) / 32);
    wgrad_share s;
    s.gpw = std::max(1, (tpw + WGRAD_MAX_PER - 1) / WGRAD_MAX_PER);
    s.per = (tpw + s.gpw - 1) / s.gpw;
    return s;
}

template <class T>
int reduce_partials(f2_ctx* ctx, const T* partial, int64_t np, int64_t stride, int64_t count, double* acc) {
    unsigned g;
    F2_TRY(cnn_grid(ctx, (count + 31) / 32, &g));
    hipLaunchKernelGGL(k_reduce_partials<T>, dim3(g), dim3(256), 0, ctx->stream, partial, np, stride, count, acc);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

template <int CIN, int COUT, int PAD, int STAGE, int COSPLIT>
int launch_wgrad_conv(f2_ctx* ctx, const float* in, const float* g, const float* act, float* partial, int Hin, int Win, int64_t m, double* acc) {
    const wgrad_share sh = wgrad_shares(Hin + 2 * PAD - 2, Win + 2 * PAD - 2);
    const int64_t groups = m * sh.gpw;
    if (groups <= 0) return F2_OK;
    unsigned grid;
    F2_TRY(cnn_grid(ctx, groups, &grid));
    hipLaunchKernelGGL((k_wgrad_conv<CIN, COUT, PAD, STAGE, COSPLIT>), dim3(grid), dim3(3 * COSPLIT * 64), 0, ctx->stream, in, g, act, partial,
                       Hin, Win, m, sh.per, sh.gpw);
    F2_HIP(ctx, hipGetLastError());
    constexpr int64_t count = 9 * CIN * COUT + COUT;   // (kernel and bias stand one after the other in the gradient too)
    return reduce_partials(ctx, partial, groups, count, count, acc);
}

float keep_scale(double rate) { return (float)(1.0 / (1.0 - rate)); }   // the float32 nearest 1 / (1 - rate)

// Dropout of a training step: rates, mask seed and step
struct train_masks {
    const double* drop;
    uint64_t seed, step;
};
// a (m, per) *= the inverted-dropout mask of layer `layer` for the windows b0 .. b0 + m - 1 of the call's batch (rate 0: nothing)
int launch_dropout(f2_ctx* ctx, float* a, int64_t m, int per, int layer, int64_t b0, const train_masks& K) {
    const double rate = K.drop[layer];
    if (rate <= 0.0 || m <= 0) return F2_OK;
    F2_CHECK(ctx, per % 4 == 0, F2_ERR_UNSUPPORTED, "dropout over %d values per window", per);
    return launch256(ctx, k_dropout, m * (per / 4), a, m, per / 4, (uint32_t)layer, b0, rate * 4294967296.0, keep_scale(rate), (uint32_t)K.seed,
                     (uint32_t)(K.seed >> 32), (uint32_t)K.step);
}

// bytes of partial sums the weight gradients of a chunk of m windows need
size_t wgrad_partial_bytes(const Dims& d, int64_t m) {
    auto conv = [&](int Ho, int Wo, int cin, int cout) {
        return sizeof(float) * (size_t)(m * wgrad_shares(Ho, Wo).gpw) * (9 * (size_t)cin * cout + cout);
    };
    size_t need = conv(d.H2, d.W2, C1, C2);
    need = std::max(need, conv(d.Hp1, d.Wp1, C2, C3));
    need = std::max(need, conv(d.H4, d.W4, C3, C4));
    need = std::max(need, sizeof(double) * (size_t)((m * d.H1 * d.W1 + C1_PIX - 1) / C1_PIX) * 10 * C1);
    need = std::max(need, sizeof(double) * (size_t)((m + D1_SEG - 1) / D1_SEG) * d.flat * D1);
    return need;
}

// The weight gradients of one chunk of m windows, added in float64 to acc (f2_train_tensor_layout L), from the chain's arrays as they
// stand when the call is reached; `partial`: wgrad_partial_bytes(d, m) bytes of scratch
struct wgrad_target {
    f2_train_layout L;
    void* partial;
    double* acc;
};
// dense2's kernel and bias, dense1's bias and kernel: once G5 stands
int wgrad_head(const f2_grad_chain& c, const float* dz, int64_t m, const wgrad_target& T) {
    f2_ctx* ctx = c.ctx;
    const float *a5 = c.arr[f2_grad_chain::A5], *g5 = c.arr[f2_grad_chain::G5];
    hipLaunchKernelGGL(k_wgrad_head, dim3((HEAD_COLS + 31) / 32), dim3(256), 0, ctx->stream, a5, dz, g5, GK, m, T.acc + T.L.off[10],
                       T.acc + T.L.off[11], T.acc + T.L.off[9]);
    F2_HIP(ctx, hipGetLastError());
    const int tiles = (c.d.flat / 64) * D1_TILES;
    const int64_t segs = (m + D1_SEG - 1) / D1_SEG;
    hipLaunchKernelGGL(k_wgrad_dense1, dim3((unsigned)((tiles + 3) / 4), (unsigned)segs), dim3(256), 0, ctx->stream, c.arr[f2_grad_chain::P2], g5,
                       (double*)T.partial, c.d.flat, GK, m);
    F2_HIP(ctx, hipGetLastError());
    const int64_t count = (int64_t)c.d.flat * D1;
    return reduce_partials(ctx, (const double*)T.partial, segs, count, count, T.acc + T.L.off[8]);
}

// conv4 (once GP2 stands), conv3 (G3), conv2 (GP1), conv1 (G1; x: the chunk's windows)
int wgrad_conv(const f2_grad_chain& c, int layer, const float* x, int64_t m, const wgrad_target& T) {
    typedef f2_grad_chain A;
    f2_ctx* ctx = c.ctx;
    const Dims& d = c.d;
    float* const* arr = c.arr;
    float* part = (float*)T.partial;
    switch (layer) {
    case 4: return launch_wgrad_conv<C3, C4, 0, ST_UNPOOL, 2>(ctx, arr[A::A3], arr[A::GP2], arr[A::A4], part, d.Hp1, d.Wp1, m, T.acc + T.L.off[6]);
    case 3: return launch_wgrad_conv<C2, C3, 1, ST_PLAIN, 1>(ctx, arr[A::P1], arr[A::G3], nullptr, part, d.Hp1, d.Wp1, m, T.acc + T.L.off[4]);
    case 2: return launch_wgrad_conv<C1, C2, 0, ST_UNPOOL, 1>(ctx, arr[A::A1], arr[A::GP1], arr[A::A2], part, d.H1, d.W1, m, T.acc + T.L.off[2]);
    default: break;
    }
    const int64_t groups = (m * d.H1 * d.W1 + C1_PIX - 1) / C1_PIX;
    unsigned g;
    F2_TRY(cnn_grid(ctx, groups, &g));
    hipLaunchKernelGGL(k_wgrad_conv1, dim3(g), dim3(256), 0, ctx->stream, x, arr[A::G1], (double*)T.partial, d.H1, d.W1, m);
    F2_HIP(ctx, hipGetLastError());
    return reduce_partials(ctx, (const double*)T.partial, groups, (int64_t)10 * C1, (int64_t)10 * C1, T.acc + T.L.off[0]);
}

// the master weights w (f2_train_tensor_layout) into cnn->blob's layouts and into the rotated / transposed grad_blob
int launch_relayout(f2_ctx* ctx, const float* w, const f2_cnn* cnn, float* grad_blob, const size_t grad_off[4]) {
    relayout_args A;
    const f2_train_layout L = f2_train_tensor_layout(cnn->flat);
    for (int i = 0; i < 13; ++i) A.src[i] = L.off[i];
    for (int i = 0; i < 12; ++i) A.dst[i] = cnn->off[i];
    for (int i = 0; i < 4; ++i) A.gdst[i] = grad_off[i];
    A.flat = cnn->flat;
    return launch256(ctx, k_relayout, (int64_t)L.total(), w, cnn->blob, grad_blob, A);
}

// the launch's scratch besides ctx->grad_ws, for chunks of `chunk` windows (byte offsets, each on a 256-byte boundary)
struct loss_ws {
    enum { XG, DZ, LOSSW, YG, HIT, PARTIAL, COUNT };
    size_t off[COUNT], total;
};
loss_ws loss_ws_layout(const Dims& d, int64_t chunk) {
    const size_t bytes[loss_ws::COUNT] = {sizeof(float) * (size_t)d.H1 * d.W1 * (size_t)chunk, sizeof(float) * 2 * (size_t)chunk,
                                          sizeof(double) * (size_t)chunk, (size_t)chunk, (size_t)chunk, wgrad_partial_bytes(d, chunk)};
    loss_ws w;
    w.total = f2_carve(bytes, loss_ws::COUNT, 256, w.off);
    return w;
}
// bytes of scratch a loss-gradient launch over at most `m` windows per call needs besides ctx->grad_ws
size_t loss_gradient_ws_bytes(const f2_cnn* cnn, int64_t m) {
    return loss_ws_layout(make_dims(cnn->rows, cnn->channels), std::min(std::max<int64_t>(m, 1), f2_cnn_grad_chunk(cnn))).total;
}
// windows a host call stages at a time: whole chunks of the chain
int64_t loss_gradient_host_chunk(const f2_cnn* cnn) {
    const int64_t chunk = f2_cnn_grad_chunk(cnn);
    return std::max<int64_t>(1, GRAD_HOST_CHUNK / chunk) * chunk;
}

// Recorded forward in training mode, loss seed, backward-data chain and weight gradients of the n windows x[index[j]] (index NULL:
// the first n), window j being window b0 + j of the call's batch for the dropout masks. acc (f2_train_tensor_layout doubles) is
// zeroed first if zero_acc, then += the gradient of the summed loss; tally += {loss sum, hits}. ws: loss_gradient_ws_bytes.
// Every line of the loop is a step of the chain (f2_cnn_grad.hip) or a kernel of this file.
int launch_loss_gradient(f2_ctx* ctx, const f2_cnn* cnn, const float* d_x, const uint8_t* d_y, const int64_t* d_index, int64_t n, int64_t b0,
                         const train_masks& K, void* ws, double* d_acc, bool zero_acc, double* d_tally) {
    typedef f2_grad_chain A;
    wgrad_target T;
    T.L = f2_train_tensor_layout(cnn->flat), T.acc = d_acc;
    if (zero_acc) F2_HIP(ctx, hipMemsetAsync(d_acc, 0, sizeof(double) * T.L.total(), ctx->stream));
    if (n <= 0) return F2_OK;
    f2_grad_chain c;
    F2_TRY(f2_grad_chain_open(ctx, cnn, n, true, &c));
    const Dims& d = c.d;
    float* const* arr = c.arr;
    const loss_ws W = loss_ws_layout(d, c.chunk);
    char* wb = (char*)ws;
    float* xg = (float*)(wb + W.off[loss_ws::XG]);
    float* dz = (float*)(wb + W.off[loss_ws::DZ]);
    double* lossw = (double*)(wb + W.off[loss_ws::LOSSW]);
    uint8_t* yg = (uint8_t*)(wb + W.off[loss_ws::YG]);
    uint8_t* hit = (uint8_t*)(wb + W.off[loss_ws::HIT]);
    T.partial = wb + W.off[loss_ws::PARTIAL];
    const float keep[3] = {keep_scale(K.drop[0]), keep_scale(K.drop[1]), keep_scale(K.drop[2])};
    for (int64_t s = 0; s < n; s += c.chunk) {
        const int64_t m = std::min(c.chunk, n - s);
        const float* x = d_x + (size_t)s * c.xs;
        const uint8_t* y = d_y + s;
        if (d_index) {
            F2_TRY(launch256(ctx, k_gather_indexed, m * (int64_t)c.xs, d_x, d_y, d_index + s, m, (int64_t)c.xs, xg, yg));
            x = xg, y = yg;
        }
        // recorded forward, training mode: the masks go onto p1, p2 and a5 in place
        F2_TRY(f2_prof_begin(ctx, F2_K_CNN));
        F2_TRY(c.conv12(x, m));
        F2_TRY(launch_dropout(ctx, arr[A::P1], m, d.Hp1 * d.Wp1 * C2, 0, b0 + s, K));
        F2_TRY(c.conv34(m));
        F2_TRY(launch_dropout(ctx, arr[A::P2], m, d.flat, 1, b0 + s, K));
        F2_TRY(f2_prof_end(ctx, F2_K_CNN));
        F2_TRY(c.dense(m, false));
        F2_TRY(f2_prof_begin(ctx, F2_K_CNN));
        F2_TRY(launch_dropout(ctx, arr[A::A5], m, D1, 2, b0 + s, K));
        F2_TRY(launch256(ctx, k_dense2_train, m * 8, arr[A::A5], cnn->t(10), cnn->t(11), y, arr[A::SC], dz, lossw, hit, m));
        hipLaunchKernelGGL(k_train_tally, dim3(1), dim3(256), 0, ctx->stream, lossw, hit, m, d_tally);
        F2_HIP(ctx, hipGetLastError());
        // backward-data chain from the loss seed, each layer's weight gradient as soon as its two operands stand
        F2_TRY(launch256(ctx, k_loss_seed, m * GK, arr[A::A5], dz, cnn->t(10), keep[2], arr[A::G5], GK, m));
        F2_TRY(wgrad_head(c, dz, m, T));
        F2_TRY(c.dense1T(m));
        F2_TRY(launch256(ctx, k_mask_scale, m * d.flat, arr[A::GP2], arr[A::P2], keep[1], m * d.flat));
        F2_TRY(wgrad_conv(c, 4, x, m, T));
        F2_TRY(c.conv4T(m));
        F2_TRY(wgrad_conv(c, 3, x, m, T));
        F2_TRY(c.conv3T(m));
        F2_TRY(launch256(ctx, k_mask_scale, m * d.Hp1 * d.Wp1 * C2, arr[A::GP1], arr[A::P1], keep[0], m * d.Hp1 * d.Wp1 * C2));
        F2_TRY(wgrad_conv(c, 2, x, m, T));
        F2_TRY(c.conv2T(m));
        F2_TRY(wgrad_conv(c, 1, x, m, T));
        F2_TRY(f2_prof_end(ctx, F2_K_CNN));
    }
    return F2_OK;
}

// the 12 tensors between 12 arrays (`tensors`) and one array in layout L (`flat`), on the stream: into `flat` or out of it
hipError_t copy_tensors(f2_ctx* ctx, const f2_train_layout& L, float* flat, float* const* tensors, bool into_flat, hipMemcpyKind kind) {
    hipError_t e = hipSuccess;
    for (int i = 0; e == hipSuccess && i < 12; ++i)
        e = hipMemcpyAsync(into_flat ? flat + L.off[i] : tensors[i], into_flat ? tensors[i] : flat + L.off[i], sizeof(float) * L.count(i), kind,
                           ctx->stream);
    return e;
}

// {loss sum, hits} of a tally on the device, as host values: waits for the stream
int read_tally(f2_ctx* ctx, const double* d_tally, double* loss_sum_or_null, int64_t* correct_or_null) {
    double t[2];
    F2_HIP(ctx, hipMemcpyAsync(t, d_tally, sizeof(t), hipMemcpyDeviceToHost, ctx->stream));
    F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (loss_sum_or_null) *loss_sum_or_null = t[0];
    if (correct_or_null) memcpy(correct_or_null, &t[1], sizeof(int64_t));
    return F2_OK;
}

int check_drop(f2_ctx* ctx, const double* drop) {
    F2_CHECK(ctx, drop, F2_ERR_INVALID, "drop is NULL");
    for (int l = 0; l < 3; ++l) F2_CHECK(ctx, drop[l] >= 0.0 && drop[l] < 1.0, F2_ERR_INVALID, "dropout rate %d is %g, not in [0, 1)", l, drop[l]);
    return F2_OK;
}

size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

}  // namespace

// ---- entry points ----
struct f2_trainer {
    f2_cnn* cnn = nullptr;   // private: the float32 recorded route reads its blob and grad_blob, nothing reads its split-fp16 tables
    int rows = 0, channels = 0, dev = 0;
    f2_train_layout L;
    f2_scratch w, a, g, acc;   // master weights, RMSprop accumulators, the last step's gradient (float32); float64 gradient + tally
    f2_scratch x, y, order;    // the training windows, their labels, the order of the steps call in flight
    int64_t n = 0;
    float* grad_blob = nullptr;
    size_t grad_off[4] = {0, 0, 0, 0};
    double lr = 0, rho = 0, eps = 0, decay = 0, drop[3] = {0, 0, 0};
    uint64_t seed = 0;
    int64_t iterations = 0;
    // f2_trainer_set_waves: the corpus x is rendered from (f2_trainer_render), instead of windows handed in by set_data
    bool have_waves = false;
    f2_scratch wave, centers;   // the waves; [the centres | the utterance of every window, counted inside its group]
    f2_scratch rir;             // f2_trainer_render_wet: [rir_offsets | taps] of the render in flight, uploaded once for all groups
    f2_scratch fir;             // f2_trainer_render_coloured: [fir_offsets | taps] of the render in flight, likewise
    f2_scratch mix;             // f2_trainer_render_smeared: [tile spans | transposed mixing matrices] of the render in flight, likewise
    f2_scratch masker;          // f2_trainer_render_masked: [masker_offsets | samples] of the recordings of the render in flight, likewise
    f2_scratch lp_coef;         // f2_trainer_render_filtered: the {b0, a1} pairs of the cutoffs of the render in flight, likewise
    std::vector<int64_t> offsets, center_offsets;
    std::vector<double> coefs;
    int wave_dtype = 0, B = 0, lpf = 0, fft_precision = 0, radius = 0, step = 0, group = 1;
    double cutoff_hz = 0;
};

extern "C" {

int f2_cnn_loss_gradient(f2_ctx* ctx, const f2_cnn* cnn, const float* x, const uint8_t* y, const int64_t* index_or_null, int64_t m,
                         const double* drop, uint64_t seed, uint64_t step, float* const* grads_or_null, double* loss_sum_or_null,
                         int64_t* correct_or_null, int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_cnn(ctx, cnn, 0, 0));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_CHECK(ctx, m >= 0, F2_ERR_INVALID, "negative window count");
    F2_TRY(check_drop(ctx, drop));
    F2_CHECK(ctx, m == 0 || (x && y), F2_ERR_INVALID, "x or y is NULL");
    const bool host = mem_space != F2_MEM_DEVICE;
    if (host && index_or_null)
        for (int64_t j = 0; j < m; ++j) F2_CHECK(ctx, index_or_null[j] >= 0, F2_ERR_INVALID, "index[%lld] is negative", (long long)j);
    if (grads_or_null)
        for (int i = 0; i < 12; ++i) F2_CHECK(ctx, grads_or_null[i], F2_ERR_INVALID, "gradient tensor %d is NULL", i);
    const f2_train_layout L = f2_train_tensor_layout(cnn->flat);
    const size_t T = L.total(), xs = (size_t)cnn->rows * cnn->channels;
    const int64_t piece = host ? loss_gradient_host_chunk(cnn) : std::max<int64_t>(m, 1);
    // scratch of the call: [the launch's | float64 gradient | {loss sum, hits} | float32 gradient]
    const size_t ws_bytes = align256(loss_gradient_ws_bytes(cnn, std::min<int64_t>(std::max<int64_t>(m, 1), piece)));
    const size_t at_tally = ws_bytes + align256(sizeof(double) * T), at_g32 = at_tally + 256;
    F2_TRY(f2_reserve(ctx, ctx->train_ws, at_g32 + sizeof(float) * T));
    char* base = (char*)ctx->train_ws.ptr;
    double* d_acc = (double*)(base + ws_bytes);
    double* d_tally = (double*)(base + at_tally);
    float* d_g32 = (float*)(base + at_g32);
    F2_HIP(ctx, hipMemsetAsync(d_acc, 0, at_g32 - ws_bytes, ctx->stream));   // (m == 0: zero gradients, loss 0, 0 hits)
    std::vector<float> hx;
    std::vector<uint8_t> hy;
    for (int64_t s = 0; s < m; s += piece) {
        const int64_t mm = std::min(piece, m - s);
        const float* d_x = x;
        const uint8_t* d_y = y;
        const int64_t* d_index = index_or_null ? index_or_null + s : nullptr;
        if (host) {   // only the windows of the call go up: gathered here, staged, and waited for before the next piece reuses the buffers
            const void *px, *py;
            if (index_or_null) {
                hx.resize((size_t)mm * xs);
                hy.resize((size_t)mm);
                for (int64_t j = 0; j < mm; ++j) {
                    memcpy(hx.data() + (size_t)j * xs, x + (size_t)index_or_null[s + j] * xs, sizeof(float) * xs);
                    hy[(size_t)j] = y[index_or_null[s + j]];
                }
                F2_TRY(f2_stage_input(ctx, hx.data(), sizeof(float) * xs * (size_t)mm, mem_space, &px));
                F2_TRY(f2_stage_into(ctx, ctx->stage_aux, hy.data(), (size_t)mm, mem_space, &py));
            } else {
                F2_TRY(f2_stage_input(ctx, x + (size_t)s * xs, sizeof(float) * xs * (size_t)mm, mem_space, &px));
                F2_TRY(f2_stage_into(ctx, ctx->stage_aux, y + s, (size_t)mm, mem_space, &py));
            }
            d_x = (const float*)px, d_y = (const uint8_t*)py, d_index = nullptr;
        } else if (!index_or_null) {
            d_x = x + (size_t)s * xs, d_y = y + s;
        }
        F2_TRY(launch_loss_gradient(ctx, cnn, d_x, d_y, d_index, mm, s, {drop, seed, step}, base, d_acc, false, d_tally));
        if (host) F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (grads_or_null) {
        F2_TRY(launch256(ctx, k_round_f32, (int64_t)T, d_acc, d_g32, (int64_t)T));
        F2_HIP(ctx, copy_tensors(ctx, L, d_g32, grads_or_null, false, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    }
    // the two tallies are host values in both memory spaces: the call waits for them
    if (loss_sum_or_null || correct_or_null) F2_TRY(read_tally(ctx, d_tally, loss_sum_or_null, correct_or_null));
    return f2_host_wait(ctx, mem_space);
}

int f2_trainer_create(f2_ctx* ctx, const float* const* tensors, int rows, int channels, double lr, double rho, double eps, double decay,
                      const double* drop, uint64_t seed, f2_trainer** out) {
    F2_TRY(f2_check_ctx(ctx));
    F2_CHECK(ctx, tensors && out, F2_ERR_INVALID, "null argument");
    *out = nullptr;
    F2_TRY(check_drop(ctx, drop));
    F2_CHECK(ctx, std::isfinite(lr) && lr >= 0.0 && rho >= 0.0 && rho <= 1.0 && eps >= 0.0 && std::isfinite(eps) && decay >= 0.0 &&
                      std::isfinite(decay),
             F2_ERR_INVALID, "bad optimiser constants (lr %g, rho %g, eps %g, decay %g)", lr, rho, eps, decay);
    f2_cnn* cnn = nullptr;
    F2_TRY(f2_cnn_create(ctx, tensors, rows, channels, &cnn));
    f2_trainer* t = new f2_trainer();
    t->cnn = cnn, t->rows = rows, t->channels = channels, t->dev = ctx->device;
    t->L = f2_train_tensor_layout(cnn->flat);
    t->lr = lr, t->rho = rho, t->eps = eps, t->decay = decay, t->seed = seed;
    for (int l = 0; l < 3; ++l) t->drop[l] = drop[l];
    const size_t T = t->L.total();
    int rc = f2_reserve(ctx, t->w, sizeof(float) * T);
    if (rc == F2_OK) rc = f2_reserve(ctx, t->a, sizeof(float) * T);
    if (rc == F2_OK) rc = f2_reserve(ctx, t->g, sizeof(float) * T);
    if (rc == F2_OK) rc = f2_reserve(ctx, t->acc, align256(sizeof(double) * T) + 256);
    f2_grad_chain c;   // (of no windows: the rotated / transposed weights alone)
    if (rc == F2_OK) rc = f2_grad_chain_open(ctx, cnn, 0, true, &c);
    hipError_t e = hipSuccess;
    if (rc == F2_OK) {
        t->grad_blob = c.gw;
        for (int i = 0; i < 4; ++i) t->grad_off[i] = c.goff[i];
        e = copy_tensors(ctx, t->L, (float*)t->w.ptr, const_cast<float* const*>(tensors), true, hipMemcpyHostToDevice);
    }
    if (rc == F2_OK && e == hipSuccess) e = hipMemsetAsync(t->a.ptr, 0, sizeof(float) * T, ctx->stream);
    if (rc == F2_OK && e == hipSuccess) e = hipMemsetAsync(t->g.ptr, 0, sizeof(float) * T, ctx->stream);
    if (rc == F2_OK && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (rc == F2_OK && e != hipSuccess) rc = f2_fail(ctx, F2_ERR_HIP, "uploading the master weights -> %s", hipGetErrorString(e));
    if (rc != F2_OK) {
        (void)f2_cnn_destroy(ctx, cnn);
        delete t;
        return rc;
    }
    *out = t;
    return F2_OK;
}

int f2_trainer_destroy(f2_ctx* ctx, f2_trainer* t) {
    if (!t) return F2_OK;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    (void)f2_cnn_destroy(ctx, t->cnn);
    delete t;
    return F2_OK;
}

static int check_trainer(f2_ctx* ctx, const f2_trainer* t) {
    F2_CHECK(ctx, t, F2_ERR_INVALID, "trainer is NULL");
    F2_CHECK(ctx, t->dev == ctx->device, F2_ERR_INVALID, "trainer lives on device %d, context on %d", t->dev, ctx->device);
    return F2_OK;
}

int f2_trainer_set_data(f2_ctx* ctx, f2_trainer* t, const float* x, const uint8_t* y, int64_t n) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(check_trainer(ctx, t));
    F2_CHECK(ctx, n >= 0 && (n == 0 || (x && y)), F2_ERR_INVALID, "bad training set (n %lld)", (long long)n);
    const size_t xs = (size_t)t->rows * t->channels;
    t->n = 0, t->have_waves = false, t->B = 0;
    if (n == 0) return F2_OK;
    F2_TRY(f2_reserve(ctx, t->x, sizeof(float) * xs * (size_t)n));
    F2_TRY(f2_reserve(ctx, t->y, (size_t)n));
    F2_HIP(ctx, hipMemcpyAsync(t->x.ptr, x, sizeof(float) * xs * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    F2_HIP(ctx, hipMemcpyAsync(t->y.ptr, y, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    t->n = n;
    return F2_OK;
}

int f2_trainer_set_waves(f2_ctx* ctx, f2_trainer* t, const void* wave, int wave_dtype, const int64_t* offsets, const double* coefs, int B,
                         int C, int lpf, double cutoff_hz, int fft_precision, const int64_t* center_offsets, const int64_t* centers,
                         const uint8_t* signs, int radius, int step, int group) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(check_trainer(ctx, t));
    F2_CHECK(ctx, C == t->channels && 2 * (int64_t)radius + 1 == t->rows, F2_ERR_INVALID,
             "the trainer was built for %d x %d windows, asked for %lld x %d", t->rows, t->channels, 2 * (long long)radius + 1, C);
    F2_CHECK(ctx, group >= 1, F2_ERR_INVALID, "group must be at least 1 utterance (got %d)", group);
    int64_t n = 0;
    std::vector<int> win_utt;
    F2_TRY(f2_check_input_batch(ctx, wave, wave_dtype, offsets, coefs, B, C, lpf, cutoff_hz, fft_precision, center_offsets, centers, radius, step,
                                t, F2_MEM_HOST, nullptr, &n, &win_utt));
    F2_CHECK(ctx, n == 0 || signs, F2_ERR_INVALID, "signs is NULL");
    for (int64_t e = 0; e < n; ++e) F2_CHECK(ctx, signs[e] <= 1, F2_ERR_INVALID, "signs[%lld] = %d is neither 0 nor 1", (long long)e, (int)signs[e]);
    F2_CHECK(ctx, B == 0 || coefs, F2_ERR_INVALID, "coefs is NULL");

    t->n = 0, t->have_waves = false, t->B = 0;
    t->wave_dtype = wave_dtype, t->lpf = lpf, t->cutoff_hz = cutoff_hz, t->fft_precision = fft_precision, t->radius = radius, t->step = step;
    t->group = group;
    if (B > 0) {
        t->offsets.assign(offsets, offsets + B + 1);
        t->center_offsets.assign(center_offsets, center_offsets + B + 1);
        t->coefs.assign(coefs, coefs + 10 * (size_t)C);
    }
    if (n > 0) {
        for (int64_t e = 0; e < n; ++e) win_utt[(size_t)e] %= group;
        const size_t wbytes = (wave_dtype == F2_WAVE_I16 ? 2 : 8) * (size_t)offsets[B], cbytes = sizeof(int64_t) * (size_t)n;
        F2_TRY(f2_reserve(ctx, t->wave, wbytes));
        F2_TRY(f2_reserve(ctx, t->centers, cbytes + sizeof(int) * (size_t)n));
        F2_TRY(f2_reserve(ctx, t->x, sizeof(float) * (size_t)t->rows * t->channels * (size_t)n));
        F2_TRY(f2_reserve(ctx, t->y, (size_t)n));
        F2_HIP(ctx, hipMemcpyAsync(t->wave.ptr, wave, wbytes, hipMemcpyHostToDevice, ctx->stream));
        F2_HIP(ctx, hipMemcpyAsync(t->centers.ptr, centers, cbytes, hipMemcpyHostToDevice, ctx->stream));
        F2_HIP(ctx, hipMemcpyAsync((char*)t->centers.ptr + cbytes, win_utt.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        F2_HIP(ctx, hipMemcpyAsync(t->y.ptr, signs, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    t->n = n, t->B = B, t->have_waves = true;
    return F2_OK;
}

// [offsets | taps] of the K filters of a stage into `area`, enqueued once for every group of the render in flight
static int upload_taps(f2_ctx* ctx, f2_scratch& area, const int64_t* offsets, const double* taps, int K, const int64_t** d_offsets,
                       const double** d_taps) {
    const size_t obytes = sizeof(int64_t) * ((size_t)K + 1), tbytes = sizeof(double) * (size_t)offsets[K];
    F2_TRY(f2_reserve(ctx, area, obytes + tbytes));
    F2_TRY(f2_upload_async(ctx, area.ptr, offsets, obytes));
    F2_TRY(f2_upload_async(ctx, (char*)area.ptr + obytes, taps, tbytes));
    *d_offsets = (const int64_t*)area.ptr, *d_taps = (const double*)((const char*)area.ptr + obytes);
    return F2_OK;
}

int f2_trainer_render_filtered(f2_ctx* ctx, f2_trainer* t, const double* rir, const int64_t* rir_offsets, int Kr, const int32_t* room_of,
                               const double* snr_db, const double* fir, const int64_t* fir_offsets, int K, const int32_t* level_of,
                               uint64_t seed, const double* mix, int Km, const int32_t* mix_of, const double* masker_snr_db,
                               const double* masker, const int64_t* masker_offsets, int R, const int32_t* masker_of, int Kk,
                               const int32_t* masker_level_of, const double* cutoff_levels_hz, int Kc, const int32_t* cutoff_of) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(check_trainer(ctx, t));
    F2_CHECK(ctx, t->have_waves, F2_ERR_INVALID, "the trainer has no waves to render from (f2_trainer_set_waves)");
    f2_augment_args A = f2_augment_args::of(rir, rir_offsets, Kr, room_of, snr_db, fir, fir_offsets, K, level_of, 0, seed, mix, Km, mix_of)
                            .with_maskers(masker_snr_db, masker, masker_offsets, R, masker_of, Kk, masker_level_of)
                            .with_cutoffs(cutoff_levels_hz, Kc, cutoff_of);
    F2_TRY(f2_check_noise_pick(ctx, t->B, A.noise));
    F2_TRY(A.check(ctx, t->B, t->channels, t->radius, t->lpf));   // (a trainer set with lpf = 1 refuses a cutoff stage)
    if (t->n == 0) return F2_OK;
    const size_t xs = (size_t)t->rows * t->channels, ws = t->wave_dtype == F2_WAVE_I16 ? 2 : 8;
    const int64_t* d_centers = (const int64_t*)t->centers.ptr;
    const int* d_win_utt = (const int*)((const char*)t->centers.ptr + sizeof(int64_t) * (size_t)t->n);
    // what every group reads goes up once: the rooms' taps, the filters of the noise (a group whose utterances are all clean keeps
    // the colours: its tiles copy), the mixing matrices as the image the gather reads (a group whose utterances are all sharp
    // takes the mixing gather's sharp path), the recordings of the maskers, and the filter coefficients of the cutoffs
    if (!A.rooms.dry()) F2_TRY(upload_taps(ctx, t->rir, rir_offsets, rir, Kr, &A.rooms.d_rir_off, &A.rooms.d_rir));
    if (A.noise.coloured()) F2_TRY(upload_taps(ctx, t->fir, fir_offsets, fir, K, &A.noise.d_fir_off, &A.noise.d_fir));
    if (!A.smear.sharp() && !A.smear.all_sharp) {
        F2_TRY(f2_reserve(ctx, t->mix, f2_mix_image_bytes(*A.smear.plan)));
        F2_TRY(f2_upload_mix_image(ctx, *A.smear.plan, t->mix.ptr, &A.smear.d_spans, &A.smear.d_wT));
    }
    if (!A.maskers.silent()) F2_TRY(f2_upload_maskers(ctx, t->masker, masker, masker_offsets, R, &A.maskers.d_moff, &A.maskers.d_masker));
    if (!A.cutoffs.unfiltered()) {
        F2_TRY(f2_reserve(ctx, t->lp_coef, sizeof(double) * 2 * (size_t)Kc));
        F2_TRY(f2_upload_lowpass_coefs(ctx, cutoff_levels_hz, Kc, (double*)t->lp_coef.ptr));
        A.cutoffs.d_coef = (const double*)t->lp_coef.ptr;
    }
    F2_TRY(f2_reset_flag(ctx));
    std::vector<int64_t> off;
    // group after group onto the stream, each into its rows of x; one wait at the end
    for (int b0 = 0; b0 < t->B; b0 += std::min(t->group, t->B - b0)) {
        const int nb = std::min(t->group, t->B - b0);
        const int64_t w0 = t->center_offsets[(size_t)b0], nw = t->center_offsets[(size_t)b0 + nb] - w0;
        if (nw == 0) continue;
        off.resize((size_t)nb + 1);
        for (int b = 0; b <= nb; ++b) off[(size_t)b] = t->offsets[(size_t)b0 + b] - t->offsets[(size_t)b0];
        const f2_batch X = {(const char*)t->wave.ptr + ws * (size_t)t->offsets[(size_t)b0], t->wave_dtype, off.data(), t->coefs.data(), nb,
                            t->channels, t->lpf, t->cutoff_hz, t->fft_precision, F2_MEM_DEVICE};
        const f2_window_list W = {d_centers + w0, d_win_utt + w0, true, nw, t->radius, t->step, 1};
        F2_TRY(f2_launch_noisy_windows(ctx, X, W, A.slice(b0), (float*)t->x.ptr + xs * (size_t)w0));
    }
    return f2_finish_positive(ctx);
}

// the render without cutoffs: the same code, whose envelopes are then the trainer's own (lpf as it was set) and go to the gather as they are
int f2_trainer_render_masked(f2_ctx* ctx, f2_trainer* t, const double* rir, const int64_t* rir_offsets, int Kr, const int32_t* room_of,
                             const double* snr_db, const double* fir, const int64_t* fir_offsets, int K, const int32_t* level_of,
                             uint64_t seed, const double* mix, int Km, const int32_t* mix_of, const double* masker_snr_db,
                             const double* masker, const int64_t* masker_offsets, int R, const int32_t* masker_of, int Kk,
                             const int32_t* masker_level_of) {
    return f2_trainer_render_filtered(ctx, t, rir, rir_offsets, Kr, room_of, snr_db, fir, fir_offsets, K, level_of, seed, mix, Km, mix_of,
                                      masker_snr_db, masker, masker_offsets, R, masker_of, Kk, masker_level_of, nullptr, 0, nullptr);
}

// the render without maskers: the same code, whose masker stage is then skipped altogether
int f2_trainer_render_smeared(f2_ctx* ctx, f2_trainer* t, const double* rir, const int64_t* rir_offsets, int Kr, const int32_t* room_of,
                              const double* snr_db, const double* fir, const int64_t* fir_offsets, int K, const int32_t* level_of,
                              uint64_t seed, const double* mix, int Km, const int32_t* mix_of) {
    return f2_trainer_render_masked(ctx, t, rir, rir_offsets, Kr, room_of, snr_db, fir, fir_offsets, K, level_of, seed, mix, Km, mix_of, nullptr,
                                    nullptr, nullptr, 0, nullptr, 0, nullptr);
}

// the render at full resolution: the same code, whose last call is then the plain gather
int f2_trainer_render_coloured(f2_ctx* ctx, f2_trainer* t, const double* rir, const int64_t* rir_offsets, int Kr, const int32_t* room_of,
                               const double* snr_db, const double* fir, const int64_t* fir_offsets, int K, const int32_t* level_of,
                               uint64_t seed) {
    return f2_trainer_render_smeared(ctx, t, rir, rir_offsets, Kr, room_of, snr_db, fir, fir_offsets, K, level_of, seed, nullptr, 0, nullptr);
}

// the render under white noise: the same code, whose noise stage is then k_noise_pick
int f2_trainer_render_wet(f2_ctx* ctx, f2_trainer* t, const double* rir, const int64_t* rir_offsets, int Kr, const int32_t* room_of,
                          const double* snr_db, int K, const int32_t* level_of, uint64_t seed) {
    return f2_trainer_render_coloured(ctx, t, rir, rir_offsets, Kr, room_of, snr_db, nullptr, nullptr, K, level_of, seed);
}

// the render without rooms: the same code, whose reverberant stage is then skipped altogether
int f2_trainer_render(f2_ctx* ctx, f2_trainer* t, const double* snr_db, int K, const int32_t* level_of, uint64_t seed) {
    return f2_trainer_render_wet(ctx, t, nullptr, nullptr, 0, nullptr, snr_db, K, level_of, seed);
}

int f2_trainer_get_windows(f2_ctx* ctx, const f2_trainer* t, int64_t first, int64_t count, float* x, uint8_t* y) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(check_trainer(ctx, t));
    F2_CHECK(ctx, first >= 0 && count >= 0 && first <= t->n && count <= t->n - first, F2_ERR_INVALID,
             "windows %lld .. + %lld are outside the %lld of the training set", (long long)first, (long long)count, (long long)t->n);
    if (count == 0) return F2_OK;
    const size_t xs = (size_t)t->rows * t->channels;
    if (x) F2_HIP(ctx, hipMemcpyAsync(x, (const float*)t->x.ptr + xs * (size_t)first, sizeof(float) * xs * (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
    if (y) F2_HIP(ctx, hipMemcpyAsync(y, (const uint8_t*)t->y.ptr + first, (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
    F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return F2_OK;
}

int f2_trainer_steps(f2_ctx* ctx, f2_trainer* t, const int64_t* order, int64_t count, int batch, double* loss_sum_or_null,
                     int64_t* correct_or_null) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(check_trainer(ctx, t));
    F2_CHECK(ctx, count >= 0 && batch >= 1, F2_ERR_INVALID, "bad step shape (count %lld, batch %d)", (long long)count, batch);
    F2_CHECK(ctx, count == 0 || order, F2_ERR_INVALID, "order is NULL");
    for (int64_t j = 0; j < count; ++j)
        F2_CHECK(ctx, order[j] >= 0 && order[j] < t->n, F2_ERR_INVALID, "order[%lld] = %lld is outside the %lld windows of the training set",
                 (long long)j, (long long)order[j], (long long)t->n);
    const size_t T = t->L.total();
    double* d_acc = (double*)t->acc.ptr;
    double* d_tally = (double*)((char*)t->acc.ptr + align256(sizeof(double) * T));
    if (count > 0) {
        F2_TRY(f2_reserve(ctx, t->order, sizeof(int64_t) * (size_t)count));
        F2_TRY(f2_upload_async(ctx, t->order.ptr, order, sizeof(int64_t) * (size_t)count));
        F2_TRY(f2_reserve(ctx, ctx->train_ws, loss_gradient_ws_bytes(t->cnn, std::min<int64_t>(count, batch))));
        F2_HIP(ctx, hipMemsetAsync(d_tally, 0, 16, ctx->stream));
    }
    // the steps go onto the stream back to back; one wait at the end
    for (int64_t s = 0; s < count; s += batch) {
        const int64_t mb = std::min<int64_t>(batch, count - s);
        F2_TRY(launch_loss_gradient(ctx, t->cnn, (const float*)t->x.ptr, (const uint8_t*)t->y.ptr, (const int64_t*)t->order.ptr + s, mb, 0,
                                    {t->drop, t->seed, (uint64_t)t->iterations}, ctx->train_ws.ptr, d_acc, true, d_tally));
        F2_TRY(launch256(ctx, k_round_f32, (int64_t)T, d_acc, (float*)t->g.ptr, (int64_t)T));
        // RMSprop as Keras 2.2 runs it, g / mb the gradient of the mean loss: a = rho a + (1 - rho) (g / mb)^2, p -= lr_t (g / mb) / (sqrt(a) + eps)
        const double lr_t = t->lr / (1.0 + t->decay * (double)t->iterations);
        F2_TRY(launch256(ctx, k_rmsprop, (int64_t)T, (float*)t->w.ptr, (float*)t->a.ptr, (const float*)t->g.ptr, (int64_t)T, (float)mb, (float)lr_t,
                         (float)t->rho, (float)(1.0 - t->rho), (float)t->eps));
        F2_TRY(launch_relayout(ctx, (const float*)t->w.ptr, t->cnn, t->grad_blob, t->grad_off));
        ++t->iterations;
    }
    if (loss_sum_or_null) *loss_sum_or_null = 0.0;
    if (correct_or_null) *correct_or_null = 0;
    return count > 0 ? read_tally(ctx, d_tally, loss_sum_or_null, correct_or_null) : F2_OK;
}

int f2_trainer_get(f2_ctx* ctx, const f2_trainer* t, int what, float* const* tensors) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(check_trainer(ctx, t));
    F2_CHECK(ctx, what == F2_TRAINER_WEIGHTS || what == F2_TRAINER_ACCUMULATORS || what == F2_TRAINER_GRADIENT, F2_ERR_INVALID,
             "what = %d is not one of F2_TRAINER_*", what);
    F2_CHECK(ctx, tensors, F2_ERR_INVALID, "tensors is NULL");
    for (int i = 0; i < 12; ++i) F2_CHECK(ctx, tensors[i], F2_ERR_INVALID, "tensor %d is NULL", i);
    float* src = (float*)(what == F2_TRAINER_WEIGHTS ? t->w.ptr : what == F2_TRAINER_ACCUMULATORS ? t->a.ptr : t->g.ptr);
    F2_HIP(ctx, copy_tensors(ctx, t->L, src, tensors, false, hipMemcpyDeviceToHost));
    F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return F2_OK;
}

int f2_trainer_get_info(f2_ctx* ctx, const f2_trainer* t, const char* key, double* value) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(check_trainer(ctx, t));
    F2_CHECK(ctx, key && value, F2_ERR_INVALID, "null argument");
    if (strcmp(key, "iterations") == 0) *value = (double)t->iterations;
    else if (strcmp(key, "windows") == 0) *value = (double)t->n;
    else if (strcmp(key, "utterances") == 0) *value = (double)t->B;
    else return f2_fail(ctx, F2_ERR_INVALID, "unknown key '%s'", key);
    return F2_OK;
}

}  // extern "C"
