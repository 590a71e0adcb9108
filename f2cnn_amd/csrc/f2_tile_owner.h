// Which utterance a tile of a ragged batch belongs to (k_reverb_levels, k_shaped_noise_levels, k_channel_mix_levels, k_resample).
// first: the B + 1 running sums of the utterances' tiles the host builds (f2_tile_table; an utterance without output has no tile).
#pragma once
#include <cstdint>

// the b with first[b] <= t < first[b + 1], for a tile 0 <= t < first[B]
__device__ __forceinline__ int tile_owner(const int64_t* __restrict__ first, int B, int64_t t) {
    int hi = B, b = 0;      // first[b] <= t < first[hi]
    while (hi - b > 1) {
        const int mid = (b + hi) >> 1;
        const bool below = first[mid] <= t;
        hi = below ? hi : mid;
        b = below ? mid : b;
    }
    return b;
}
