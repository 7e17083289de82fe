// ss_negatives.hpp -- the random draws of ss_sample_negatives (ss_negatives.hip): a pure function of (seed, slot,
// attempt, which of the attempt's two draws), built on hash_u64.  tests/negatives_restatement.py restates it in Python ints.
#pragma once
#include "ss_common.hpp"

namespace ss {

constexpr uint64_t kNegGolden = 0x9E3779B97F4A7C15ULL;

// what the draws of one slot share: slot q of a call with this seed
__device__ __forceinline__ uint64_t neg_slot_key(uint64_t seed, uint64_t q) { return hash_u64(seed ^ hash_u64(q + 1)); }

// draw c (0 or 1) of attempt a: draw(seed, q, a, c) = hash_u64(neg_slot_key(seed, q) + golden * (2 a + c + 1)), wrapping
__device__ __forceinline__ uint64_t neg_draw(uint64_t slot_key, int a, int c) { return hash_u64(slot_key + kNegGolden * (uint64_t)(2 * a + c + 1)); }

// a draw mapped to [0, n): the high 64 bits of r * n
__device__ __forceinline__ int64_t neg_pick(uint64_t r, int64_t n) { return (int64_t)__umul64hi(r, (uint64_t)n); }

}  // namespace ss
