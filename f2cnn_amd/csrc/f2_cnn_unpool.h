// What the kernels of the backward-data chain (f2_cnn_grad.hip) and of the weight gradients (f2_cnn_train.hip) share on the
// device: the accumulator type, the staging and epilogue switches of their templates, and the un-pool rule.
#ifndef F2_CNN_UNPOOL_H
#define F2_CNN_UNPOOL_H

#include <hip/hip_runtime.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum { ST_PLAIN = 0, ST_UNPOOL = 1 };               // how a kernel stages its gradient: as it stands / un-pooled on the way
enum { EP_RELU = 0, EP_MASK = 1, EP_NONE = 2 };     // k_gconv's epilogue

// the gradient a pooled cell hands to element `me` (0 .. 3 in (row, column) order) of its block: all of it to the first maximal
// element where that maximum is > 0 (the ReLU in front of the pool passes it), nothing otherwise
__device__ __forceinline__ float unpool_pick(float g, float v0, float v1, float v2, float v3, int me) {
    const float m = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
    const int first = v0 == m ? 0 : v1 == m ? 1 : v2 == m ? 2 : v3 == m ? 3 : 4;
    return m > 0.f && first == me ? g : 0.f;
}

#endif
