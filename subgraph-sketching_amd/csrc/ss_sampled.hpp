// ss_sampled.hpp -- the sampling rule of the sampled enclosing subgraphs (ss_sampled_nodes.hip): the key that orders a
// hop's fringe, how many of the fringe are kept, and the selection of the kept ones -- a radix select over keys that are RECOMPUTED from
// the node id on every pass (no key array: a fringe can be 1000 times what is kept).  tests/sampled_subgraph_restatement.py restates
// the rule in Python sets and numpy uint64.
#pragma once
#include "ss_negatives.hpp"

namespace ss {

constexpr int kSelThreads = 256;  // the select is written for workgroups of this size (one histogram bin per thread)

// what every key of link (u, v) shares: K = hash_u64(seed ^ hash_u64(((u << 32) | v) + 1)), u and v after the negative-id wrap
__device__ __forceinline__ uint64_t sampled_link_key(uint64_t seed, int64_t u, int64_t v)
{
    return hash_u64(seed ^ hash_u64((((uint64_t)u << 32) | (uint64_t)v) + 1));
}
// what the keys of one hop share
__device__ __forceinline__ uint64_t sampled_hop_key(uint64_t link_key, int hop) { return hash_u64(link_key + kNegGolden * (uint64_t)hop); }
// key(x): hash_u64 is a bijection of 64-bit words, so the keys of distinct nodes of one fringe are distinct
__device__ __forceinline__ uint64_t sampled_key(uint64_t hop_key, int64_t x) { return hash_u64(hop_key ^ (uint64_t)(x + 1)); }

// how many of a fringe of F nodes are kept: Python's int(ratio * F) in IEEE double (all of them for ratio == 1.0), then the cap
__device__ __forceinline__ int sampled_take(int F, double ratio, int cap)
{
    int m = ratio < 1.0 ? (int)(ratio * (double)F) : F;
    return m < cap ? m : cap;
}

struct SampledSelect {
    int hist[256];
    int wave_sum[kSelThreads / kWave];
    unsigned long long prefix;
    int remaining, ties;
};

// the threshold of the m smallest (key, id) of the fringe id_at(0 .. F), 0 < m < F (whole workgroup of kSelThreads threads; the caller
// has passed a barrier since the fringe was written).  Eight passes over 8-bit digits from the top: a 256-bin LDS histogram of the
// digit among the nodes whose key agrees with the prefix found so far, a workgroup prefix sum over the bins, and the bin in which
// the m-th smallest lies extends the prefix.  Afterwards keep(x) decides a node; every thread has passed a barrier after the last
// write when this returns.
struct SampledThreshold {
    uint64_t key;  // the m-th smallest key
    int take;      // how many of the nodes with exactly that key are kept (the lowest ids)
    int ties;      // how many nodes have exactly that key (1: hash_u64 is a bijection; kept general)
};

template <class IdAt>
__device__ __forceinline__ SampledThreshold sampled_select(SampledSelect &sel, IdAt id_at, int F, int m, uint64_t hop_key)
{
    const int t = threadIdx.x;
    const int wave = t / kWave, wl = t & (kWave - 1);
    uint64_t prefix = 0;
    int remaining = m, ties = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        sel.hist[t] = 0;
        __syncthreads();
        for (int i = t; i < F; i += kSelThreads) {
            const uint64_t k = sampled_key(hop_key, id_at(i));
            if (shift == 56 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&sel.hist[(int)(k >> shift) & 0xFF], 1);
        }
        __syncthreads();
        const int mine = sel.hist[t];
        int inc = mine;  // inclusive prefix sum over the bins: within the wave, then across the waves
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int y = __shfl_up(inc, d);
            if (wl >= d) inc += y;
        }
        if (wl == kWave - 1) sel.wave_sum[wave] = inc;
        __syncthreads();
        for (int k = 0; k < wave; ++k) inc += sel.wave_sum[k];
        if (inc - mine < remaining && remaining <= inc) {  // exactly one bin: the counts sum to at least `remaining`
            sel.prefix = prefix | ((unsigned long long)t << shift);
            sel.remaining = remaining - (inc - mine);
            sel.ties = mine;
        }
        __syncthreads();
        prefix = sel.prefix;
        remaining = sel.remaining;
        ties = sel.ties;
    }
    __syncthreads();  // (every thread has read sel before a later select writes it)
    return {prefix, remaining, ties};
}

// is x among the kept?  Below the threshold key: yes.  At it: the `take` lowest ids of the nodes that share it -- all of them when
// take == ties (always, keys being distinct); otherwise by counting the lower ids with the same key in the fringe
template <class IdAt>
__device__ __forceinline__ bool sampled_keep(const SampledThreshold &th, IdAt id_at, int F, uint64_t hop_key, int64_t x)
{
    const uint64_t k = sampled_key(hop_key, x);
    if (k != th.key) return k < th.key;
    if (th.take == th.ties) return true;
    int lower = 0;
    for (int i = 0; i < F; ++i) {
        const int64_t y = id_at(i);
        lower += y < x && sampled_key(hop_key, y) == th.key;
    }
    return lower < th.take;
}

}  // namespace ss
