// Philox4x32-10, shared by the noise generator (f2_noise.hip) and the dropout masks (f2_cnn_train.hip).
#ifndef F2_PHILOX_H
#define F2_PHILOX_H

#include <cstdint>

struct philox_words {
    uint32_t w0, w1, w2, w3;
};

// Philox4x32-10 (Salmon et al., SC'11), the standard constants
__device__ inline philox_words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return {c0, c1, c2, c3};
}

// the standard normal deviate of (seed, level, utterance, sample): the cosine branch of Box-Muller on two 53-bit uniforms. One
// function for the white noise kernels (f2_noise.hip) and the coloured one (f2_noise_shaped.hip): the same bits in both.
__device__ inline double noise_deviate(uint64_t seed, uint32_t level, uint32_t utt, uint64_t i) {
    const philox_words w = philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), level, utt, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double u1 = ((double)(w.w0 >> 5) * 67108864.0 + (double)(w.w1 >> 6) + 1.0) * 0x1p-53;   // (0, 1]
    const double u2 = ((double)(w.w2 >> 5) * 67108864.0 + (double)(w.w3 >> 6)) * 0x1p-53;         // [0, 1)
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

#endif
