// The one kernel of the inspection entry f2_cnn_layers (f2_pipeline.hip): conv4's pooled output out of the activation workspace into
// the caller's array, in true units. The split routes leave it multiplied by dense1's input scale, a power of two (f2_cnn_split.h),
// so the multiplication by its reciprocal is exact; the other routes pass 1.
#include "f2_internal.h"

namespace {

__global__ __launch_bounds__(256) void k_scale_copy(const float* __restrict__ src, float* __restrict__ dst, int64_t count, float factor) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) dst[i] = src[i] * factor;
}

}  // namespace

int f2_launch_scale_copy(f2_ctx* ctx, const float* d_src, float* d_dst, int64_t count, float factor) {
    if (count <= 0) return F2_OK;
    const int64_t blocks = (count + 255) / 256;
    hipLaunchKernelGGL(k_scale_copy, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, ctx->stream, d_src, d_dst, count, factor);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}
