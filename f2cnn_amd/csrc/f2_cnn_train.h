// What f2_cnn_grad.hip (the recorded forward and the backward-data chain, step by step) and f2_cnn_train.hip (the training step
// that interleaves its own kernels with those steps) share.
#ifndef F2_CNN_TRAIN_H
#define F2_CNN_TRAIN_H

#include "f2_cnn_dims.h"

constexpr int GK = 576;                    // dense1's 516 outputs padded to whole 64-value chunks: the K of the transposed dense1
constexpr int64_t GRAD_HOST_CHUNK = 4096;  // windows a host call of the gradient entry points stages at a time

// The 12 tensors of the network in their Keras layouts, one after the other without gaps (f2_cnn_create's order): element offsets,
// off[12] = the count of all of them. Gradients, master weights and RMSprop accumulators all use it.
struct f2_train_layout {
    size_t off[13];
    size_t total() const { return off[12]; }
    size_t count(int i) const { return off[i + 1] - off[i]; }
};
inline f2_train_layout f2_train_tensor_layout(int flat) {
    const size_t sizes[12] = {9 * C1, C1, 9 * (size_t)C1 * C2, C2, 9 * (size_t)C2 * C3, C3, 9 * (size_t)C3 * C4, C4,
                              (size_t)flat * D1, D1, (size_t)D1 * D2, D2};
    f2_train_layout L;
    L.off[0] = 0;
    for (int i = 0; i < 12; ++i) L.off[i + 1] = L.off[i] + sizes[i];
    return L;
}

// `count` pieces of sizes[k] units carved out of one block, each on a boundary of `align` units (a power of two): off[k], returns
// what all of them take
inline size_t f2_carve(const size_t* sizes, int count, size_t align, size_t* off) {
    size_t total = 0;
    for (int k = 0; k < count; ++k) off[k] = total, total += (sizes[k] + align - 1) & ~(align - 1);
    return total;
}

// The chain over one chunk of windows: every array the recorded forward and the backward-data pass leave in ctx->grad_ws, and the
// rotated / transposed weights of the backward layers. Its steps enqueue on ctx->stream; the caller holds the f2_prof brackets.
struct f2_grad_chain {
    enum { A1, A2, P1, A3, A4, P2, A5, G5, GP2, G3, GP1, G1, GX, SC, COUNT };
    f2_ctx* ctx;
    const f2_cnn* cnn;
    Dims d;
    int64_t chunk;       // windows a step takes at most
    size_t xs;           // floats of a window
    float* arr[COUNT];   // (chunk, per-window shape) each, on 256-byte boundaries
    float* gw;           // cnn->grad_blob, built on the network's first backward chain (NULL without need_backward)
    size_t goff[4];      // conv2T, conv3T, conv4T, dense1T in it (floats)

    // the steps (f2_cnn_grad.hip), each over the first m <= chunk windows of the arrays.
    // Recorded forward of the m windows at x: conv1, conv2, pool1 -> A1, A2, P1; conv3, conv4, pool2 -> A3, A4, P2; dense1 -> A5,
    // with_dense2 also dense2 + softmax -> SC (f2_launch_cnn_dense, which brackets itself)
    int conv12(const float* x, int64_t m) const;
    int conv34(int64_t m) const;
    int dense(int64_t m, bool with_dense2) const;
    // backward-data: G5 -> GP2 (dense1 transposed), -> G3 (un-pool through A4, conv4 transposed, conv3's mask), -> GP1 (conv3
    // transposed), -> G1 (un-pool through A2, conv2 transposed, conv1's mask), -> G (m, rows, channels) (conv1 transposed)
    int dense1T(int64_t m) const;
    int conv4T(int64_t m) const;
    int conv3T(int64_t m) const;
    int conv2T(int64_t m) const;
    int conv1T(float* G, int64_t m) const;
};
// the chain for calls of n windows in chunks of min(n, f2_cnn_grad_chunk); n == 0 reserves nothing and only builds the weights
int f2_grad_chain_open(f2_ctx* ctx, const f2_cnn* cnn, int64_t n, bool need_backward, f2_grad_chain* c);

#endif
