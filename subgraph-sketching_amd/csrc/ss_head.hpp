// ss_head.hpp -- the structure-feature head behind a pair's feature row (ss_pair_scores).
//
// Replaces, for inference, what both reference models do with a feature row the moment they receive it (models/elph.py:73-86
// LinkPredictor.forward, :324-352 BUDDY.forward):  x = relu(bn_labels(label_lin_layer(sf)));  lin(cat([x, ...]))  -- the label
// branch's share of the logit.  BatchNorm (eval mode) is folded into the linear layer on the host (head.py), so the device sees
//     score = bias + sum_j w2[j] * max(0, shift[j] + sum_i W[j][i] * x[i]),      dim = h(h+2) or 2h(h+2) <= 30.
//
// Mapping: the 16-lane row that has just assembled a pair's features (every lane holds all of f[]) owns the pair's head too: lane l
// computes hidden units l and l + 16.  The parameters live in LDS, W transposed to [i][j] so that the 16 lanes of a row read 16
// consecutive words per step (the four rows of a wavefront read the same words: one broadcast).  Every sum has ONE order -- i
// ascending through fmaf, then row16_sum_f's butterfly -- so a pair's score does not depend on the grid, the batch, the walk order
// or the register budget of the kernel around it.
#pragma once
#include "ss_common.hpp"

namespace ss {

constexpr int kHeadMaxDim = 2 * SS_MAX_HOPS * (SS_MAX_HOPS + 2);  // 30: h = 3 with the degree-normalised copy

// the kernel's view of ss_structure_head (device pointers; dim validated by the host: NF or 2 NF of the kernel's hop count)
struct HeadArgs {
    const float *w1;     // [dim][dim] row-major: W[j][i], hidden unit j, input i
    const float *shift;  // [dim]
    const float *w2;     // [dim]
    float bias;
    int dim;
};

// ss_structure_head (host struct, device pointers) -> the kernel's view.  false: no head, not a head of hop count h, or its width and
// `degrees` disagree (the head's width decides whether the normalised copy exists, not the pointer)
inline bool make_head_args(const ss_structure_head *head, int h, const float *degrees, HeadArgs &out)
{
    const int nf = h * (h + 2);
    if (!head || head->dim != (head->normalised ? 2 * nf : nf) || !head->w1 || !head->shift || !head->w2) return false;
    if ((head->normalised != 0) != (degrees != nullptr)) return false;
    out = {head->w1, head->shift, head->w2, head->bias, head->dim};
    return true;
}

// (the pair kernel carries its head as a parameter pack that is empty for the feature query: this names the one element)
__device__ __forceinline__ const HeadArgs &the_head(const HeadArgs &h) { return h; }

struct HeadLds {
    float w[kHeadMaxDim * kHeadMaxDim];  // [i][j], row stride = dim
    float shift[kHeadMaxDim];
    float w2[kHeadMaxDim];
};

// every thread of the workgroup; NO barrier of its own: the caller runs it right before stage_tables(), whose barrier covers both
__device__ __forceinline__ void stage_head(HeadLds &s, const HeadArgs &h)
{
    const int dim = h.dim;
    for (int e = threadIdx.x; e < dim * dim; e += blockDim.x) {  // coalesced read of W[j][i], transposed on the way in
        const int j = e / dim, i = e - j * dim;
        s.w[i * dim + j] = h.w1[e];
    }
    for (int j = threadIdx.x; j < dim; j += blockDim.x) {
        s.shift[j] = h.shift[j];
        s.w2[j] = h.w2[j];
    }
}

// hidden unit j of a pair before the ReLU: shift[j] + sum_i W[j][i] x[i], i ascending; x = f[0 .. NF) followed, when `normalised`
// (kernel-uniform), by the degree-normalised copies fn[0 .. NF)
template <int NF>
__device__ __forceinline__ float head_unit(const HeadLds &s, int dim, int j, const float (&f)[NF], const float (&fn)[NF], bool normalised)
{
    float acc = s.shift[j];
#pragma unroll
    for (int i = 0; i < NF; ++i) acc = fmaf(s.w[i * dim + j], f[i], acc);
    if (normalised) {
#pragma unroll
        for (int i = 0; i < NF; ++i) acc = fmaf(s.w[(NF + i) * dim + j], fn[i], acc);
    }
    return acc;
}

// The score of the row's pair, in every lane of the row.  f: the pair's features (every lane); normed: lane i < NF of the row holds
// the degree-normalised copy of feature i, computed as the feature epilogue computes it, and hands it to the other lanes here.
// Every lane of the row must be active.
template <int NF>
__device__ __forceinline__ float head_score(const HeadLds &s, int dim, float bias, const float (&f)[NF], float normed,
                                            bool normalised, int l, int row_base)
{
    float fn[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) fn[i] = normalised ? __shfl(normed, row_base + i) : 0.0f;
    const bool has0 = l < dim;
    float partial = s.w2[has0 ? l : 0] * fmaxf(head_unit<NF>(s, dim, has0 ? l : 0, f, fn, normalised), 0.0f);
    partial = has0 ? partial : 0.0f;
    if (dim > kRow) {  // kernel-uniform: a second unit per lane only where there are more than 16
        const bool has1 = l + kRow < dim;
        const int j1 = has1 ? l + kRow : 0;
        const float second = s.w2[j1] * fmaxf(head_unit<NF>(s, dim, j1, f, fn, normalised), 0.0f);
        partial = has1 ? partial + second : partial;
    }
    return row16_sum_f(partial) + bias;
}

}  // namespace ss
