// ss_feature_algebra.hpp -- the feature algebra of get_subgraph_features (reference hashing.py:276-320): the h(h+2) features of
// a pair from its intersections I[k1][k2] and the two cardinality rows, in the reference's own fp32 operation order.  Shared by the
// sketch query (ss_pairs.hip: I = J * U, cards from HLL++) and the exact query (ss_exact.hip: I and the ball sizes counted exactly).
#pragma once
#include "ss_common.hpp"

namespace ss {

// feature algebra of get_subgraph_features (hashing.py:276-320); I is indexed [k1-1][k2-1].
template <int H>
__device__ __forceinline__ void assemble_features(const float (&I)[H][H], const float (&c1)[H], const float (&c2)[H],
                                                  uint32_t flags, float (&f)[H * (H + 2)])
{
    f[0] = I[0][0];
    if constexpr (H == 1) {
        f[1] = c2[0] - f[0];
        f[2] = c1[0] - f[0];
    } else if constexpr (H == 2) {
        f[1] = I[1][0] - f[0];
        f[2] = I[0][1] - f[0];
        f[3] = I[1][1] - f[0] - f[1] - f[2];
        f[4] = c2[0] - (f[0] + f[1]);
        f[5] = c1[0] - f[0] - f[2];
        f[6] = c2[1] - ((((f[0] + f[4]) + f[1]) + f[2]) + f[3]);  /* torch.sum order over 5 strided floats, see note */
        f[7] = c1[1] - f[0] - (((f[0] + f[1]) + f[2]) + f[3]) - f[5];  // f0 twice, as the reference (:287)
    } else {
        f[1] = I[1][0] - f[0];
        f[2] = I[0][1] - f[0];
        f[3] = I[1][1] - f[0] - f[1] - f[2];
        f[4] = I[2][0] - f[0] - f[1];
        f[5] = I[0][2] - f[0] - f[2];
        const float s04 = ((f[0] + f[1]) + f[2]) + f[3];
        f[6] = I[2][1] - s04 - f[4];
        f[7] = I[1][2] - s04 - f[5];
        f[8] = I[2][2] - (((((((f[0] + f[1]) + f[2]) + f[3]) + f[4]) + f[5]) + f[6]) + f[7]);
        f[9] = c2[0] - f[0] - f[1] - f[4];
        f[10] = c1[0] - f[0] - f[2] - f[5];
        const float s05 = (((f[0] + f[4]) + f[1]) + f[2]) + f[3];
        f[11] = c2[1] - s05 - f[6] - f[9];
        f[12] = c1[1] - s05 - f[7] - f[10];
        const float s09 = (((((((f[8] + f[0]) + f[1]) + f[2]) + f[3]) + f[4]) + f[5]) + f[6]) + f[7];
        f[13] = c2[2] - s09 - f[9] - f[11];
        f[14] = c1[2] - s09 - f[10] - f[12];
    }
    if (!(flags & SS_FLAG_USE_ZERO_ONE)) {
        if constexpr (H == 2) { f[4] = 0.0f; f[5] = 0.0f; }
        if constexpr (H == 3) { f[4] = 0.0f; f[5] = 0.0f; f[11] = 0.0f; f[12] = 0.0f; }
    }
    if (flags & SS_FLAG_FLOOR_SF) {
#pragma unroll
        for (int k = 0; k < H * (H + 2); ++k) f[k] = f[k] < 0.0f ? 0.0f : f[k];
    }
}

}  // namespace ss
