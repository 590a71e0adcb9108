// Shape arithmetic of K4 that f2_cnn.hip and f2_cnn_ws.hip have to agree on (f2_cnn_f32_tile.h beside it: the device pieces of
// the float32 matrix-core kernels): layer widths, tile constants of the fused convolution
// kernels and of dense1's weight layouts, the sizes of every layer's output for a rows x channels window, the index rule of the
// MFMA B operand and the launcher of the thread-per-element kernels.
#ifndef F2_CNN_DIMS_H
#define F2_CNN_DIMS_H

#include "f2_internal.h"

constexpr int C1 = 32, C2 = 32, C3 = 64, C4 = 64, D1 = 516, D2 = 2;
constexpr int PW = 34;    // patch width: 32 output columns + 2
constexpr int T34 = 30;   // conv4 output columns per tile (32 conv3 columns)
// dense1: K walked in chunks of D1_KC, one 32-column output tile per wave, the output dimension padded to whole tiles
constexpr int D1_TILES = (D1 + 31) / 32;   // 17
constexpr int D1_NPAD = D1_TILES * 32;     // 544
constexpr int D1_KC = 64;
constexpr int D1_WAVES = 6;

struct Dims {
    int H1, W1;        // input / conv1 output
    int H2, W2;        // conv2 output (valid)
    int Hp1, Wp1;      // after pool 1 (= conv3 output, same)
    int H4, W4;        // conv4 output (valid)
    int Hp2, Wp2;      // after pool 2
    int flat;
    int xtiles12() const { return (Wp1 * 2 + 31) / 32; }      // 32-column tiles of a conv2 row the pool keeps
    int xtiles34() const { return (2 * Wp2 + T34 - 1) / T34; }  // T34-column tiles of a conv4 row the pool keeps
};

inline Dims make_dims(int rows, int channels) {
    Dims d;
    d.H1 = rows;
    d.W1 = channels;
    d.H2 = rows - 2;
    d.W2 = channels - 2;
    d.Hp1 = d.H2 / 2;
    d.Wp1 = d.W2 / 2;
    d.H4 = d.Hp1 - 2;
    d.W4 = d.Wp1 - 2;
    d.Hp2 = d.H4 / 2;
    d.Wp2 = d.W4 / 2;
    d.flat = d.Hp2 > 0 && d.Wp2 > 0 ? d.Hp2 * d.Wp2 * C4 : 0;
    return d;
}

// the grid of a per-tile launch: `blocks` as an unsigned, after the check that it is one
inline int cnn_grid(f2_ctx* ctx, int64_t blocks, unsigned* grid) {
    F2_CHECK(ctx, blocks < (int64_t(1) << 31), F2_ERR_UNSUPPORTED, "CNN chunk too large");
    *grid = (unsigned)blocks;
    return F2_OK;
}

// a kernel of one thread per element, 256 to a workgroup, on ctx->stream: the grid check, the launch and its error
template <class... P, class... A>
int launch256(f2_ctx* ctx, void (*kernel)(P...), int64_t threads, A... args) {
    unsigned grid;
    F2_TRY(cnn_grid(ctx, (threads + 255) / 256, &grid));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, ctx->stream, args...);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

// Where w[k][n] of a K x N matrix stands in the float32 kernels' MFMA B operand wt[block][h][s/4][n (npad)][s%4],
// k = block blk + h blk/2 + s: conv2 .. conv4 with blk = Cin (a block per tap), dense1 with blk = D1_KC, the transposed layers of
// the backward chain likewise. f2_cnn_create, the chain's transposed weights and the trainer's k_relayout all place by it.
__host__ __device__ __forceinline__ size_t cnn_b_operand_index(size_t k, int n, int blk, int npad) {
    const int half = blk / 2;
    const size_t b = k / blk, hh = k % blk / half, s = k % half;
    return (((b * 2 + hh) * (half / 4) + s / 4) * npad + n) * 4 + s % 4;
}

#endif
