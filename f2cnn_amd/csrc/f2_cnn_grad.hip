// Backward-data pass of K4 (f2_cnn.hip's head comment has the network): G = dP(rising)/dx for every cell of every window, the
// kernels of f2_cnn_input_gradient / f2_saliency_map / f2_eval_saliency_batch (include/f2cnn_hip.h).
//
// Recorded forward: conv1 .. dense2 in float32 (fmaf chains: k_conv1_fwd on the VALU, the other layers on v_mfma_f32_32x32x2_f32),
// every layer's post-ReLU output kept in HBM, the two pools as kernels of their own. A post-ReLU value is > 0 exactly where the
// pre-activation is, so the activations are the ReLU masks; and where a 2 x 2 block's maximum is > 0 the first maximal post-ReLU
// element is the first maximal pre-activation, so they are the pool positions too.
//
// Backward chain (all float32, fixed summation order, no atomics):
//   k_grad_dense2     g5 = P (1 - P) (W2[:,1] - W2[:,0]) where a5 > 0, rows padded with zeros to GK = 576
//   k_gemm_rows       dense1 transposed: (n x 576) . W1T (576 x flat)
//   k_conv3x3_f32 UNPOOL/MASK   conv4 transposed: the un-pool of the flat gradient through a4 happens while the patch is staged,
//                               the conv3 mask (a3 > 0) in the epilogue
//   k_conv3x3_f32 PLAIN/NONE    conv3 transposed
//   k_conv3x3_f32 UNPOOL/MASK   conv2 transposed: un-pool through a2 in the staging, conv1 mask (a1 > 0) in the epilogue
//   k_conv1_bwd       conv1 transposed (32 -> 1), VALU
//   k_grad_profile    profile[w][c] = {sum_r G x, sum_r |G|} in float64
// Backward-data of a 3 x 3 convolution with padding p is a 3 x 3 convolution with padding 2 - p whose kernel is the forward one
// rotated by 180 degrees with Cin and Cout swapped: k_conv3x3_f32 (f2_cnn_f32_tile.h, which describes the tile) is one implicit-GEMM
// template for the forward layers, here and in f2_cnn.hip's layer-by-layer route, and for the transposed ones. k_gemm_rows is the
// row GEMM of that header. The transposed weights are built from cnn->blob on an f2_cnn's first gradient call.
// Host side: every launch of the forward and of the chain is a step of f2_grad_chain (f2_cnn_train.h), defined once below;
// f2_launch_cnn_input_gradient here and the training step of f2_cnn_train.hip are two drivers over those steps.
// gfx950, wave64. Everything that reaches memory is written by plain C++ stores.
#include <algorithm>
#include <cmath>

#include "f2_cnn_f32_tile.h"
#include "f2_cnn_train.h"

namespace {

constexpr int GEMM_WAVES = 4;    // waves (output tiles) of a k_gemm_rows workgroup
constexpr int64_t GRAD_WS_BYTES = int64_t(1) << 30;   // everything the chain holds between kernels
constexpr int64_t GRAD_WS_CHUNK = 1024;               // windows of a chunk, at most

// ---- conv1 ('same', Cin = 1) + ReLU, recorded: eight threads per pixel, a channel quad each; the oracle's tap order ----
__global__ __launch_bounds__(256) void k_conv1_fwd(const float* __restrict__ x, const float* __restrict__ w1, const float* __restrict__ b1,
                                                   float* __restrict__ a1, int H, int W, int64_t nwin) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = nwin * H * W * (C1 / 4);
    if (t >= total) return;
    const int c4 = (int)(t % (C1 / 4));
    const int64_t pix = t / (C1 / 4);
    const int xo = (int)(pix % W);
    const int64_t t2 = pix / W;
    const int y = (int)(t2 % H);
    const int64_t win = t2 / H;
    const float* img = x + win * (int64_t)H * W;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int yi = y - 1 + tap / 3, xi = xo - 1 + tap % 3;
        const float v = (yi >= 0 && yi < H && xi >= 0 && xi < W) ? img[(int64_t)yi * W + xi] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = fmaf(v, w1[tap * C1 + c4 * 4 + q], acc[q]);
    }
    float4 o;
    o.x = fmaxf(acc[0] + b1[c4 * 4 + 0], 0.f);
    o.y = fmaxf(acc[1] + b1[c4 * 4 + 1], 0.f);
    o.z = fmaxf(acc[2] + b1[c4 * 4 + 2], 0.f);
    o.w = fmaxf(acc[3] + b1[c4 * 4 + 3], 0.f);
    *reinterpret_cast<float4*>(a1 + pix * C1 + c4 * 4) = o;
}

// ---- 2 x 2 max-pool of an (n, H, W, CH) tensor -> (n, H / 2, W / 2, CH): a thread per channel quad of a pooled pixel ----
__global__ __launch_bounds__(256) void k_pool2x2(const float* __restrict__ a, float* __restrict__ p, int H, int W, int CH, int64_t nwin) {
    const int Hp = H / 2, Wp = W / 2, Q = CH / 4;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nwin * Hp * Wp * Q) return;
    const int c4 = (int)(t % Q);
    const int64_t pix = t / Q;
    const int px = (int)(pix % Wp);
    const int64_t t2 = pix / Wp;
    const int py = (int)(t2 % Hp);
    const int64_t win = t2 / Hp;
    const float* s = a + ((win * H + 2 * py) * (int64_t)W + 2 * px) * CH + c4 * 4;
    const float4 v00 = *reinterpret_cast<const float4*>(s), v01 = *reinterpret_cast<const float4*>(s + CH);
    const float4 v10 = *reinterpret_cast<const float4*>(s + (int64_t)W * CH), v11 = *reinterpret_cast<const float4*>(s + (int64_t)W * CH + CH);
    float4 o;
    o.x = fmaxf(fmaxf(v00.x, v01.x), fmaxf(v10.x, v11.x));
    o.y = fmaxf(fmaxf(v00.y, v01.y), fmaxf(v10.y, v11.y));
    o.z = fmaxf(fmaxf(v00.z, v01.z), fmaxf(v10.z, v11.z));
    o.w = fmaxf(fmaxf(v00.w, v01.w), fmaxf(v10.w, v11.w));
    *reinterpret_cast<float4*>(p + pix * CH + c4 * 4) = o;
}

// ---- g5 (n, GK): the gradient of P = softmax(z)[1] at dense1's pre-activations ----
// dP/dz1 = -dP/dz0 = P (1 - P) = s0 s1 with the recorded scores (the product keeps its precision where P is close to 1)
__global__ __launch_bounds__(256) void k_grad_dense2(const float* __restrict__ a5, const float* __restrict__ scores, const float* __restrict__ w2,
                                                     float* __restrict__ g5, int64_t n) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * GK) return;
    const int k = (int)(t % GK);
    const int64_t wv = t / GK;
    float g = 0.f;
    if (k < D1 && a5[wv * D1 + k] > 0.f) g = scores[2 * wv] * scores[2 * wv + 1] * (w2[2 * k + 1] - w2[2 * k]);
    g5[t] = g;
}

// ---- out (n, N) = a (n, K) . w (K, N), K a multiple of 64 and N of 32: gemm_rows_tile (k_dense1_mfma's body), stored plain ----
__global__ __launch_bounds__(GEMM_WAVES * 64) void k_gemm_rows(const float* __restrict__ a, const float* __restrict__ wt, float* __restrict__ out,
                                                               int K, int N, int64_t n) {
    __shared__ __attribute__((aligned(16))) float As[2][GEMM_ROWS * GEMM_PS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w0 = (int64_t)blockIdx.x * GEMM_ROWS;
    const int nt = blockIdx.y * GEMM_WAVES + wave;
    const bool live = nt < N / 32;
    f32x16 acc[2];
    gemm_rows_tile<GEMM_WAVES>(a, wt, K, N, n, w0, nt, live, As, acc);
    if (!live) return;
    const int col = nt * 32 + (lane & 31);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int64_t wr = w0 + t * 32 + acc_row(q, lane >> 5);
            if (wr < n) out[wr * N + col] = acc[t][q];
        }
}

// ---- conv1 transposed ('same', 32 -> 1): a thread per cell of G, taps then channels in ascending order ----
// G[y][x] = sum over (dy, dx, c) of g1[y + 1 - dy][x + 1 - dx][c] w1[dy][dx][c], g1 already masked by a1 > 0
__global__ __launch_bounds__(256) void k_conv1_bwd(const float* __restrict__ g1, const float* __restrict__ w1, float* __restrict__ G, int H, int W,
                                                   int64_t nwin) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nwin * H * W) return;
    const int xo = (int)(t % W);
    const int64_t t2 = t / W;
    const int y = (int)(t2 % H);
    const int64_t win = t2 / H;
    const float* img = g1 + win * (int64_t)H * W * C1;
    float acc = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int yi = y + 1 - tap / 3, xi = xo + 1 - tap % 3;
        if (yi < 0 || yi >= H || xi < 0 || xi >= W) continue;
        const float4* gp = reinterpret_cast<const float4*>(img + ((int64_t)yi * W + xi) * C1);
        const float4* wp = reinterpret_cast<const float4*>(w1 + tap * C1);
#pragma unroll
        for (int q = 0; q < C1 / 4; ++q) {
            const float4 g = gp[q], wv = wp[q];
            acc = fmaf(g.x, wv.x, acc);
            acc = fmaf(g.y, wv.y, acc);
            acc = fmaf(g.z, wv.z, acc);
            acc = fmaf(g.w, wv.w, acc);
        }
    }
    G[t] = acc;
}

// ---- profile[w][c] = {sum_r (double)G (double)x, sum_r |(double)G|}, r ascending: a thread per (window, channel) ----
__global__ __launch_bounds__(256) void k_grad_profile(const float* __restrict__ G, const float* __restrict__ x, double* __restrict__ profile, int R,
                                                      int C, int64_t nwin) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nwin * C) return;
    const int c = (int)(t % C);
    const int64_t win = t / C;
    const float* g = G + win * (int64_t)R * C + c;
    const float* xv = x + win * (int64_t)R * C + c;
    double s = 0.0, sa = 0.0;
    for (int r = 0; r < R; ++r) {
        const double gv = (double)g[(int64_t)r * C];
        s += gv * (double)xv[(int64_t)r * C];   // (the product of two float32 values is exact in float64)
        sa += fabs(gv);
    }
    profile[2 * t] = s;
    profile[2 * t + 1] = sa;
}

// ---- f2_saliency_map: k_occlusion_map's columns, lanes and fixed order (f2_occlusion.hip) over a (rows, C, 2) float64 profile ----
// blockIdx.y = channel c. map[u][c][x] = {rows, mean of profile[..][c][0], mean of profile[..][c][1]} over the rows column x owns.
constexpr int TT = 256;
constexpr int AHEAD = 4;
__global__ __launch_bounds__(TT) void k_saliency_map(const double* __restrict__ profile, const int64_t* __restrict__ rec, int64_t origin, int64_t hop,
                                                      int W, unsigned bpu, double* __restrict__ map) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned u = blockIdx.x / bpu, local = blockIdx.x % bpu;
    const unsigned c = blockIdx.y, C = gridDim.y;
    const int64_t first = rec[5 * (size_t)u], n = rec[5 * (size_t)u + 1], s = rec[5 * (size_t)u + 2], m = rec[5 * (size_t)u + 3];
    const int lg = (int)rec[5 * (size_t)u + 4];
    const int G = 1 << lg, per = 64 >> lg;
    const int run = (int)(local * (TT / 64) + wv);
    if ((int64_t)run * per >= W) return;                // (the whole wave)
    const int sub = lane & (G - 1), x = run * per + (lane >> lg);
    const bool has = x < W;

    int64_t j_lo = 0, j_hi = 0;
    if (has && m > 0) {
        const int64_t q = m / W, r = m % W;
        const int64_t lo = s + (int64_t)x * q + (int64_t)x * r / W;
        int64_t hi = s + (int64_t)(x + 1) * q + (int64_t)(x + 1) * r / W;
        if (hi == lo) hi = lo + 1;
        j_lo = lo <= origin ? 0 : min(n, (lo - origin - 1) / hop + 1);
        j_hi = hi <= origin ? 0 : min(n, (hi - origin - 1) / hop + 1);
    }
    const size_t pitch = 2 * (size_t)C;
    const double* p = profile + pitch * (size_t)first + 2 * (size_t)c;
    double sum = 0.0, sum_abs = 0.0;
    int64_t j = j_lo + sub;
    for (; j + (int64_t)(AHEAD - 1) * G < j_hi; j += (int64_t)AHEAD * G) {     // AHEAD independent loads, added in index order
        double a[AHEAD], b[AHEAD];
#pragma unroll
        for (int q = 0; q < AHEAD; ++q) {
            const size_t row = (size_t)(j + (int64_t)q * G);
            a[q] = p[pitch * row];
            b[q] = p[pitch * row + 1];
        }
#pragma unroll
        for (int q = 0; q < AHEAD; ++q) {
            sum += a[q];
            sum_abs += b[q];
        }
    }
    for (; j < j_hi; j += G) {
        sum += p[pitch * (size_t)j];
        sum_abs += p[pitch * (size_t)j + 1];
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        if (d >= G) continue;      // (uniform: G belongs to the utterance)
        sum += __shfl_xor(sum, d);
        sum_abs += __shfl_xor(sum_abs, d);
    }
    if (has && sub == 0) {
        const int64_t rows = j_hi - j_lo;
        double* t = map + (((size_t)u * C + c) * (size_t)W + (size_t)x) * 3;
        const double none = (double)NAN;
        t[0] = (double)rows;
        t[1] = rows > 0 ? sum / (double)rows : none;
        t[2] = rows > 0 ? sum_abs / (double)rows : none;
    }
}

// ---- the weights of the transposed layers, from cnn->blob (both in cnn_b_operand_index's layout) ----
// where conv2T, conv3T, conv4T and dense1T start in grad_blob (floats); returns the floats of all four
size_t grad_weight_layout(int flat, size_t off[4]) {
    const size_t sizes[4] = {9 * (size_t)C2 * C1, 9 * (size_t)C3 * C2, 9 * (size_t)C4 * C3, (size_t)GK * flat};
    return f2_carve(sizes, 4, 64, off);
}

// Rotated, transposed convolution kernels and W1T of `cnn`, built on its first gradient call and kept until f2_cnn_destroy
int grad_weights(f2_ctx* ctx, const f2_cnn* cnn, float** out) {
    std::lock_guard<std::mutex> lock(cnn->sets_mu);
    if (cnn->grad_blob) {
        *out = cnn->grad_blob;
        return F2_OK;
    }
    size_t off[4];
    const size_t total = grad_weight_layout(cnn->flat, off);
    std::vector<float> dst(total, 0.f);
    const int cin[3] = {C1, C2, C3}, cout[3] = {C2, C3, C4};
    std::vector<float> src;
    for (int l = 0; l < 3; ++l) {
        // forward k = tap cin + ci, n = co  ->  transposed k' = tap' cout + co, n' = ci, tap' = 8 - tap (the 180 degree turn)
        const size_t count = 9 * (size_t)cin[l] * cout[l];
        src.resize(count);
        F2_HIP(ctx, hipMemcpyAsync(src.data(), cnn->t(2 + 2 * l), sizeof(float) * count, hipMemcpyDeviceToHost, ctx->stream));
        F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
        float* d = dst.data() + off[l];
        for (int tap = 0; tap < 9; ++tap)
            for (int ci = 0; ci < cin[l]; ++ci)
                for (int co = 0; co < cout[l]; ++co)
                    d[cnn_b_operand_index((size_t)(8 - tap) * cout[l] + co, ci, cout[l], cin[l])] =
                        src[cnn_b_operand_index((size_t)tap * cin[l] + ci, co, cin[l], cout[l])];
    }
    {
        const size_t count = (size_t)cnn->flat * D1_NPAD;
        src.resize(count);
        F2_HIP(ctx, hipMemcpyAsync(src.data(), cnn->t(8), sizeof(float) * count, hipMemcpyDeviceToHost, ctx->stream));
        F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
        float* d = dst.data() + off[3];
        for (int j = 0; j < cnn->flat; ++j)
            for (int k = 0; k < D1; ++k) d[cnn_b_operand_index((size_t)k, j, 64, cnn->flat)] = src[cnn_b_operand_index((size_t)j, k, D1_KC, D1_NPAD)];
    }
    float* blob = nullptr;
    hipError_t e = hipMalloc((void**)&blob, sizeof(float) * total);
    if (e != hipSuccess) return f2_fail(ctx, F2_ERR_NOMEM, "hipMalloc(%zu) -> %s", sizeof(float) * total, hipGetErrorString(e));
    e = hipMemcpyAsync(blob, dst.data(), sizeof(float) * total, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(blob);
        return f2_fail(ctx, F2_ERR_HIP, "uploading the transposed CNN weights -> %s", hipGetErrorString(e));
    }
    cnn->grad_blob = blob;
    *out = blob;
    return F2_OK;
}

// floats per window of the chain's arrays
void grad_ws_per(const Dims& d, size_t per[f2_grad_chain::COUNT]) {
    per[f2_grad_chain::A1] = (size_t)d.H1 * d.W1 * C1;
    per[f2_grad_chain::A2] = (size_t)d.H2 * d.W2 * C2;
    per[f2_grad_chain::P1] = (size_t)d.Hp1 * d.Wp1 * C2;
    per[f2_grad_chain::A3] = (size_t)d.Hp1 * d.Wp1 * C3;
    per[f2_grad_chain::A4] = (size_t)d.H4 * d.W4 * C4;
    per[f2_grad_chain::P2] = (size_t)d.flat;
    per[f2_grad_chain::A5] = D1;
    per[f2_grad_chain::G5] = GK;
    per[f2_grad_chain::GP2] = (size_t)d.flat;
    per[f2_grad_chain::G3] = (size_t)d.Hp1 * d.Wp1 * C3;
    per[f2_grad_chain::GP1] = (size_t)d.Hp1 * d.Wp1 * C2;
    per[f2_grad_chain::G1] = (size_t)d.H1 * d.W1 * C1;
    per[f2_grad_chain::GX] = (size_t)d.H1 * d.W1;
    per[f2_grad_chain::SC] = 2;
}
// where the arrays of a chunk of `chunk` windows stand in ctx->grad_ws (float offsets, each on a 256-byte boundary); returns the
// floats all of them take
size_t grad_ws_offsets(const Dims& d, int64_t chunk, size_t off[f2_grad_chain::COUNT]) {
    size_t sizes[f2_grad_chain::COUNT];
    grad_ws_per(d, sizes);
    for (size_t& s : sizes) s *= (size_t)chunk;
    return f2_carve(sizes, f2_grad_chain::COUNT, 64, off);
}

}  // namespace

// conv4's pooled output (m, flat) and dense1's output (m, 516) of the recorded forward, as the last f2_launch_cnn_input_gradient
// on this context left them for a call of m <= f2_cnn_grad_chunk windows (valid until the next gradient launch reuses the area)
void f2_cnn_grad_recorded(const f2_ctx* ctx, const f2_cnn* cnn, int64_t m, const float** p2, const float** a5) {
    size_t off[f2_grad_chain::COUNT];
    grad_ws_offsets(make_dims(cnn->rows, cnn->channels), m, off);
    *p2 = (const float*)ctx->grad_ws.ptr + off[f2_grad_chain::P2];
    *a5 = (const float*)ctx->grad_ws.ptr + off[f2_grad_chain::A5];
}

int64_t f2_cnn_grad_chunk(const f2_cnn* cnn) {
    size_t per[f2_grad_chain::COUNT], floats = 0;
    grad_ws_per(make_dims(cnn->rows, cnn->channels), per);
    for (size_t p : per) floats += p;
    const int64_t fit = (GRAD_WS_BYTES - 64 * f2_grad_chain::COUNT * (int64_t)sizeof(float)) / (int64_t)(sizeof(float) * floats);
    return std::max<int64_t>(1, std::min<int64_t>(fit, GRAD_WS_CHUNK));
}

int f2_grad_chain_open(f2_ctx* ctx, const f2_cnn* cnn, int64_t n, bool need_backward, f2_grad_chain* c) {
    c->ctx = ctx, c->cnn = cnn;
    c->d = make_dims(cnn->rows, cnn->channels);
    c->xs = (size_t)c->d.H1 * c->d.W1;
    c->gw = nullptr;
    if (need_backward) F2_TRY(grad_weights(ctx, cnn, &c->gw));
    grad_weight_layout(cnn->flat, c->goff);
    c->chunk = std::min(n, f2_cnn_grad_chunk(cnn));
    size_t off[f2_grad_chain::COUNT];
    F2_TRY(f2_reserve(ctx, ctx->grad_ws, sizeof(float) * grad_ws_offsets(c->d, c->chunk, off)));
    for (int k = 0; k < f2_grad_chain::COUNT; ++k) c->arr[k] = (float*)ctx->grad_ws.ptr + off[k];
    return F2_OK;
}

// ---- the steps of the chain: every launch of the recorded forward and of the backward-data pass stands here, once ----
int f2_grad_chain::conv12(const float* x, int64_t m) const {
    F2_TRY(launch256(ctx, k_conv1_fwd, m * d.H1 * d.W1 * (C1 / 4), x, cnn->t(0), cnn->t(1), arr[A1], d.H1, d.W1, m));
    F2_TRY((launch_conv3x3<C1, C2, 0, ST_PLAIN, EP_RELU, 4, 1>(ctx, arr[A1], nullptr, cnn->t(2), cnn->t(3), arr[A2], d.H1, d.W1, m)));
    return launch256(ctx, k_pool2x2, m * d.Hp1 * d.Wp1 * (C2 / 4), arr[A2], arr[P1], d.H2, d.W2, C2, m);
}

int f2_grad_chain::conv34(int64_t m) const {
    F2_TRY((launch_conv3x3<C2, C3, 1, ST_PLAIN, EP_RELU, 4, 2>(ctx, arr[P1], nullptr, cnn->t(4), cnn->t(5), arr[A3], d.Hp1, d.Wp1, m)));
    F2_TRY((launch_conv3x3<C3, C4, 0, ST_PLAIN, EP_RELU, 4, 2>(ctx, arr[A3], nullptr, cnn->t(6), cnn->t(7), arr[A4], d.Hp1, d.Wp1, m)));
    return launch256(ctx, k_pool2x2, m * d.Hp2 * d.Wp2 * (C4 / 4), arr[A4], arr[P2], d.H4, d.W4, C4, m);
}

int f2_grad_chain::dense(int64_t m, bool with_dense2) const {
    return f2_launch_cnn_dense(ctx, cnn, nullptr, f2_cnn_route(), arr[P2], m, arr[A5], with_dense2 ? arr[SC] : nullptr, nullptr, with_dense2);
}

int f2_grad_chain::dense1T(int64_t m) const {
    const int ntiles = d.flat / 32;
    hipLaunchKernelGGL(k_gemm_rows, dim3((unsigned)((m + GEMM_ROWS - 1) / GEMM_ROWS), (unsigned)((ntiles + GEMM_WAVES - 1) / GEMM_WAVES)),
                       dim3(GEMM_WAVES * 64), 0, ctx->stream, arr[G5], gw + goff[3], arr[GP2], GK, d.flat, m);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

int f2_grad_chain::conv4T(int64_t m) const {
    return launch_conv3x3<C4, C3, 2, ST_UNPOOL, EP_MASK, 4, 2>(ctx, arr[GP2], arr[A4], gw + goff[2], arr[A3], arr[G3], d.H4, d.W4, m);
}

int f2_grad_chain::conv3T(int64_t m) const {
    return launch_conv3x3<C3, C2, 1, ST_PLAIN, EP_NONE, 2, 1>(ctx, arr[G3], nullptr, gw + goff[1], nullptr, arr[GP1], d.Hp1, d.Wp1, m);
}

int f2_grad_chain::conv2T(int64_t m) const {
    return launch_conv3x3<C2, C1, 2, ST_UNPOOL, EP_MASK, 4, 1>(ctx, arr[GP1], arr[A2], gw + goff[0], arr[A1], arr[G1], d.H2, d.W2, m);
}

int f2_grad_chain::conv1T(float* G, int64_t m) const {
    return launch256(ctx, k_conv1_bwd, m * d.H1 * d.W1, arr[G1], cnn->t(0), G, d.H1, d.W1, m);
}

int f2_launch_cnn_input_gradient(f2_ctx* ctx, const f2_cnn* cnn, const float* d_x, int64_t n, float* d_grad, double* d_profile,
                                 float* d_scores) {
    if (n <= 0) return F2_OK;
    const bool backward = d_grad || d_profile;
    f2_grad_chain c;
    F2_TRY(f2_grad_chain_open(ctx, cnn, n, backward, &c));
    for (int64_t s = 0; s < n; s += c.chunk) {
        const int64_t m = std::min(c.chunk, n - s);
        const float* x = d_x + (size_t)s * c.xs;
        // recorded forward
        F2_TRY(f2_prof_begin(ctx, F2_K_CNN));
        F2_TRY(c.conv12(x, m));
        F2_TRY(c.conv34(m));
        F2_TRY(f2_prof_end(ctx, F2_K_CNN));
        F2_TRY(c.dense(m, true));
        float* sc = c.arr[f2_grad_chain::SC];
        if (d_scores) F2_HIP(ctx, hipMemcpyAsync(d_scores + 2 * (size_t)s, sc, sizeof(float) * 2 * (size_t)m, hipMemcpyDeviceToDevice, ctx->stream));
        if (!backward) continue;
        // backward-data chain
        float* G = d_grad ? d_grad + (size_t)s * c.xs : c.arr[f2_grad_chain::GX];
        F2_TRY(f2_prof_begin(ctx, F2_K_CNN));
        F2_TRY(launch256(ctx, k_grad_dense2, m * GK, c.arr[f2_grad_chain::A5], sc, cnn->t(10), c.arr[f2_grad_chain::G5], m));
        F2_TRY(c.dense1T(m));
        F2_TRY(c.conv4T(m));
        F2_TRY(c.conv3T(m));
        F2_TRY(c.conv2T(m));
        F2_TRY(c.conv1T(G, m));
        if (d_profile) F2_TRY(launch256(ctx, k_grad_profile, m * c.d.W1, G, x, d_profile + 2 * (size_t)s * c.d.W1, c.d.H1, c.d.W1, m));
        F2_TRY(f2_prof_end(ctx, F2_K_CNN));
    }
    return F2_OK;
}

int f2_launch_saliency_map(f2_ctx* ctx, const double* d_profile, const int64_t* d_rec, int U, int C, int64_t origin, int hop, int width,
                           int64_t blocks_per_utt, double* d_map) {
    if (U <= 0 || C <= 0 || blocks_per_utt <= 0) return F2_OK;
    F2_CHECK(ctx, blocks_per_utt * U < (int64_t(1) << 31), F2_ERR_UNSUPPORTED, "map of %d x %d columns needs too many workgroups", U, width);
    k_saliency_map<<<dim3((unsigned)(blocks_per_utt * U), (unsigned)C), dim3(TT), 0, ctx->stream>>>(d_profile, d_rec, origin, (int64_t)hop, width,
                                                                                                  (unsigned)blocks_per_utt, d_map);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

extern "C" {

int f2_cnn_input_gradient(f2_ctx* ctx, const f2_cnn* cnn, const float* x, int64_t n, float* grad_or_null, double* profile_or_null,
                          float* scores_or_null, int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_cnn(ctx, cnn, 0, 0));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_CHECK(ctx, n >= 0, F2_ERR_INVALID, "negative window count");
    if (n == 0) return F2_OK;
    F2_CHECK(ctx, x, F2_ERR_INVALID, "x is NULL");
    const size_t xs = (size_t)cnn->rows * cnn->channels, C = (size_t)cnn->channels;
    // Device memory: the whole call at once (the chain works through its scratch in chunks of its own). Host memory: GRAD_HOST_CHUNK
    // windows at a time through stage_in / stage_out / stage_aux, each chunk's outputs back before the next one goes up.
    const bool host = mem_space != F2_MEM_DEVICE;
    const int64_t chunk = !host || n < GRAD_HOST_CHUNK ? n : GRAD_HOST_CHUNK;
    f2_output grad;
    F2_TRY(f2_place(ctx, ctx->stage_out, grad_or_null, sizeof(float) * xs * (size_t)chunk, mem_space, false, &grad));
    grad.bytes = sizeof(float) * xs * (size_t)n;
    const size_t tail_bytes = host && profile_or_null ? sizeof(double) * 2 * C * (size_t)chunk : 0;
    f2_score_outputs out;
    F2_TRY(f2_place_scores(ctx, scores_or_null, nullptr, chunk, mem_space, false, false, tail_bytes, &out));
    for (int64_t s = 0; s < n; s += chunk) {
        const int64_t m = n - s < chunk ? n - s : chunk;
        const void* d_x;
        F2_TRY(f2_stage_input(ctx, x + (size_t)s * xs, sizeof(float) * xs * (size_t)m, mem_space, &d_x));
        const f2_output go = grad.chunk(sizeof(float) * xs * (size_t)s, sizeof(float) * xs * (size_t)m);
        const f2_output sc = out.scores.chunk(sizeof(float) * 2 * (size_t)s, sizeof(float) * 2 * (size_t)m);
        f2_output po;
        if (profile_or_null) {
            const size_t first = sizeof(double) * 2 * C * (size_t)s;
            po.bytes = sizeof(double) * 2 * C * (size_t)m;
            po.dev = host ? out.tail : (char*)profile_or_null + first, po.host = host ? (char*)profile_or_null + first : nullptr;
            po.callers = !host;
        }
        F2_TRY(f2_launch_cnn_input_gradient(ctx, cnn, (const float*)d_x, m, go.as<float>(), po.as<double>(), sc.as<float>()));
        F2_TRY(f2_copy_back(ctx, go));
        F2_TRY(f2_copy_back(ctx, po));
        F2_TRY(f2_copy_back(ctx, sc));
        F2_TRY(f2_host_wait(ctx, mem_space));
    }
    return F2_OK;
}

}  // extern "C"
