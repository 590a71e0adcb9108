// What the kernels of the backward-data chain (f2_cnn_grad.hip) and of the weight gradients (f2_cnn_train.hip) share with the
// convolution kernel of f2_cnn_f32_tile.h: the staging and epilogue switches of their templates, and the un-pool rule.
#ifndef F2_CNN_UNPOOL_H
#define F2_CNN_UNPOOL_H

#include <hip/hip_runtime.h>

enum { ST_PLAIN = 0, ST_UNPOOL = 1 };                        // how a kernel stages its input: as it stands / un-pooled on the way
enum { EP_RELU = 0, EP_MASK = 1, EP_NONE = 2, EP_POOL = 3 }; // k_conv3x3_f32's epilogue

// the gradient a pooled cell hands to element `me` (0 .. 3 in (row, column) order) of its block: all of it to the first maximal
// element where that maximum is > 0 (the ReLU in front of the pool passes it), nothing otherwise
__device__ __forceinline__ float unpool_pick(float g, float v0, float v1, float v2, float v3, int me) {
    const float m = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
    const int first = v0 == m ? 0 : v1 == m ? 1 : v2 == m ? 2 : v3 == m ? 3 : 4;
    return m > 0.f && first == me ? g : 0.f;
}

// channels 4 c4 .. 4 c4 + 3 of cell (y, x) of the un-pooled gradient of a 2 x 2 max-pool over (H, W): g (H / 2, W / 2, CH) the
// gradient of the pooled tensor, act (H, W, CH) the pool's post-ReLU input. Zero outside, and in rows / columns the pool dropped.
template <int CH>
__device__ __forceinline__ float4 unpool4(const float* g, const float* act, int H, int W, int y, int x, int c4) {
    const int Hp = H / 2, Wp = W / 2;
    const int py = y >> 1, px = x >> 1;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (y >= 0 && x >= 0 && py < Hp && px < Wp) {
        const float4 gv = *reinterpret_cast<const float4*>(g + ((int64_t)py * Wp + px) * CH + c4 * 4);
        const float* s = act + ((int64_t)(2 * py) * W + 2 * px) * CH + c4 * 4;
        const float4 v00 = *reinterpret_cast<const float4*>(s), v01 = *reinterpret_cast<const float4*>(s + CH);
        const float4 v10 = *reinterpret_cast<const float4*>(s + (int64_t)W * CH);
        const float4 v11 = *reinterpret_cast<const float4*>(s + (int64_t)W * CH + CH);
        const int me = (y & 1) * 2 + (x & 1);
        v.x = unpool_pick(gv.x, v00.x, v01.x, v10.x, v11.x, me);
        v.y = unpool_pick(gv.y, v00.y, v01.y, v10.y, v11.y, me);
        v.z = unpool_pick(gv.z, v00.z, v01.z, v10.z, v11.z, me);
        v.w = unpool_pick(gv.w, v00.w, v01.w, v10.w, v11.w, me);
    }
    return v;
}

#endif
