// What f2_cnn_grad.hip (the chain of a training step), f2_cnn_train.hip (its new kernels) and the entry points share.
#ifndef F2_CNN_TRAIN_H
#define F2_CNN_TRAIN_H

#include "f2_cnn_dims.h"

// The 12 tensors of the network in their Keras layouts, one after the other without gaps (f2_cnn_create's order): element offsets,
// off[12] = the count of all of them. Gradients, master weights and RMSprop accumulators all use it.
struct f2_train_layout {
    size_t off[13];
    size_t total() const { return off[12]; }
};
f2_train_layout f2_train_tensor_layout(int flat);

// ---- kernels of f2_cnn_train.hip (device pointers, enqueued on ctx->stream) ----
// a (m, per) *= the inverted-dropout mask of layer `layer` for the windows b0 .. b0 + m - 1 of the call's batch (rate 0: nothing)
int f2_train_dropout(f2_ctx* ctx, float* a, int64_t m, int per, int layer, int64_t b0, double rate, uint64_t seed, uint64_t step);
float f2_train_keep_scale(double rate);   // the float32 nearest 1 / (1 - rate)
// dense2 + softmax on a5 (m, 516) with the labels y: scores (m, 2), dz = softmax - onehot (m, 2), the float64 loss terms and
// whether the decision (scores[1] > scores[0]) equals the label
int f2_train_dense2(f2_ctx* ctx, const float* a5, const float* w2, const float* b2, const uint8_t* y, int64_t m, float* scores, float* dz,
                    double* lossw, uint8_t* hit);
// tally[0] += the loss terms (float64, fixed order), ((int64_t*)tally)[1] += the hits
int f2_train_tally(f2_ctx* ctx, const double* lossw, const uint8_t* hit, int64_t m, double* tally);
// g5 (m, gk) = [a5 > 0] scale (dz0 W2[k][0] + dz1 W2[k][1]), zeros from column 516 on
int f2_train_seed(f2_ctx* ctx, const float* a5, const float* dz, const float* w2, float scale, float* g5, int gk, int64_t m);
// g[i] = p[i] > 0 ? g[i] * scale : 0 (the backward factor of a dropout layer, and of the ReLU in front of it)
int f2_train_mask_scale(f2_ctx* ctx, float* g, const float* p, float scale, int64_t count);
// xg[j] = x[index[j]], yg[j] = y[index[j]] for j < m, windows of xs floats
int f2_train_gather(f2_ctx* ctx, const float* x, const uint8_t* y, const int64_t* index, int64_t m, size_t xs, float* xg, uint8_t* yg);

// The weight gradients of one chunk of m windows, added in float64 to acc (f2_train_tensor_layout): every array as the chain left
// it in ctx->grad_ws. `partial`: f2_train_partial_bytes(d, m) bytes of scratch.
struct f2_train_chunk {
    Dims d;
    int64_t m;
    int gk;
    const float *x, *a1, *a2, *p1, *a3, *a4, *p2, *a5, *g5, *gp2, *g3, *gp1, *g1, *dz;
    void* partial;
    double* acc;
};
size_t f2_train_partial_bytes(const Dims& d, int64_t m);
int f2_train_wgrad_head(f2_ctx* ctx, const f2_train_chunk& T);    // dense2, dense1 (before the chain overwrites nothing: any time)
int f2_train_wgrad_conv(f2_ctx* ctx, const f2_train_chunk& T, int layer /* 4, 3, 2, 1 */);
// out[i] = (float)acc[i]
int f2_train_round(f2_ctx* ctx, const double* acc, float* out, size_t count);
// RMSprop as Keras 2.2 runs it, g / m the gradient of the mean loss: a = rho a + (1 - rho) (g / m)^2, p -= lr_t (g / m) / (sqrt(a) + eps)
int f2_train_rmsprop(f2_ctx* ctx, float* p, float* a, const float* g, size_t count, int64_t m, float lr_t, float rho, float one_minus_rho,
                     float eps);
// the master weights w (f2_train_tensor_layout) into cnn->blob's layouts and into the rotated / transposed grad_blob
int f2_train_relayout(f2_ctx* ctx, const float* w, const f2_cnn* cnn, float* grad_blob, const size_t grad_off[4]);

// ---- f2_cnn_grad.hip ----
// the rotated / transposed weights of `cnn` (built on first use) and where conv2T, conv3T, conv4T and dense1T start in them
int f2_cnn_grad_blob(f2_ctx* ctx, const f2_cnn* cnn, float** blob, size_t off[4]);
// bytes of scratch a loss-gradient launch over at most `m` windows per call needs besides ctx->grad_ws
size_t f2_cnn_loss_gradient_ws_bytes(const f2_cnn* cnn, int64_t m);
// Recorded forward in training mode, loss seed, backward-data chain and weight gradients of the m windows x[index[j]] (index NULL:
// the first m), window j being window b0 + j of the call's batch for the dropout masks. acc (f2_train_tensor_layout doubles) is
// zeroed first if zero_acc, then += the gradient of the summed loss; tally += {loss sum, hits}. ws: f2_cnn_loss_gradient_ws_bytes.
int f2_launch_cnn_loss_gradient(f2_ctx* ctx, const f2_cnn* cnn, const float* d_x, const uint8_t* d_y, const int64_t* d_index, int64_t m,
                                int64_t b0, const double drop[3], uint64_t seed, uint64_t step, void* ws, double* d_acc, bool zero_acc,
                                double* d_tally);
int64_t f2_cnn_loss_gradient_host_chunk(const f2_cnn* cnn);   // windows a host call stages at a time: whole chunks of the chain

#endif
