"""The structure-feature head restated in float64 numpy, and the error bound score_links is held to: shared by
test_score_host.py and test_score_gpu.py.  Nothing here touches the engine."""
import numpy as np
import torch

U = 2.0 ** -24  # float32 unit roundoff


def raw_head(dim, seed, out_bias=True):
    """seeded tensors of one structure branch, float32 as a trained model holds them (keyword arguments of StructureHead)"""
    rng = np.random.RandomState(seed)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    return dict(weight=f32(rng.randn(dim, dim) / np.sqrt(dim)), bias=f32(rng.randn(dim) * 0.3), bn_weight=f32(rng.uniform(0.5, 1.5, dim)),
                bn_bias=f32(rng.randn(dim) * 0.2), bn_mean=f32(rng.randn(dim)), bn_var=f32(rng.uniform(0.2, 3.0, dim)), bn_eps=1e-5,
                out_weight=f32(rng.randn(dim)), out_bias=f32(rng.randn(1)) if out_bias else None)


def unfolded64(raw, x):
    """Linear -> BatchNorm1d(eval) -> ReLU -> Linear in float64 on rows x [L, dim], nothing folded"""
    d = {k: (v.double().numpy() if isinstance(v, torch.Tensor) else v) for k, v in raw.items()}
    y = np.asarray(x, dtype=np.float64) @ d['weight'].T + d['bias']
    y = (y - d['bn_mean']) / np.sqrt(d['bn_var'] + d['bn_eps']) * d['bn_weight'] + d['bn_bias']
    return np.maximum(y, 0.0) @ d['out_weight'] + (float(d['out_bias'][0]) if d['out_bias'] is not None else 0.0)


def magnitude(head, x):
    """A(q) = |b2| + sum_j |w2_j| (|t'_j| + sum_i |W'_ji| |x_qi|), float64 from the folded float32 parameters"""
    w1, t, w2 = (np.abs(a.astype(np.float64)) for a in (head.w1, head.shift, head.w2))
    return abs(head.b2) + (np.abs(np.asarray(x, dtype=np.float64)) @ w1.T + t) @ w2


def e_fp(head, x):
    """|score - ref64| <= (2 dim + 6) u A(q): folding rounds W' and t' once (u), each of the two layers is a dot product of at most
    dim + 1 terms ((dim + 2) u per layer), ReLU is 1-Lipschitz"""
    return (2 * head.dim + 6) * U * magnitude(head, x)


def feature_slack(head, x, rtol, atol):
    """what a tolerance of rtol |x_i| + atol on every feature can move the score by: sum_j |w2_j| sum_i |W'_ji| (rtol |x_i| + atol)"""
    w1, w2 = np.abs(head.w1.astype(np.float64)), np.abs(head.w2.astype(np.float64))
    return ((rtol * np.abs(np.asarray(x, dtype=np.float64)) + atol) @ w1.T) @ w2
