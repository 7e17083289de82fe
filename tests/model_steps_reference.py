"""ELPH- and SEAL-shaped training steps, restated once and run in three forms (tests/test_model_steps_host.py, test_model_steps_gpu.py).

Every model below is ONE torch.nn.Module class that takes an `ops` namespace -- the layer classes `gcn`, `sage`, `gin` and the functions
`gather`, `hadamard`, `sort_pool`, `mean_pool`, `center_pool` -- so the same module code, and therefore the same autograd graph
topology, runs
  * with the package's ops (the GPU test builds that namespace: this file imports nothing from the package),
  * with `twin_ops()`: every op a torch.autograd.Function that moves its input to the host and calls the existing numpy restatement
    for the forward and for the backward (gcn_restatement.propagate, aggr_restatement.aggregate / aggregate_grad, link_decoder_restatement
    .gather / hadamard / grad, pooling_restatement.*); Linear, BatchNorm1d, Conv1d, relu, BCE and cat stay the device's own torch ops,
  * with `plain_ops()`: index_add_ with gcn_norm from its definition, x[links], and the torch_* pooling forms, in any dtype.
The models are restated shapes (reference models/elph.py:48-86, 131-160, 180-218 with runners/train.py:198-204; models/seal.py:116-173,
177-256, 259-328), not copies; dropout is 0 everywhere.

Layout: the package's products pad a width that is no multiple of 4 and return the [n, F + pad] buffer sliced to F.  The twins
return the same layout (`_padded`), so that the GEMMs around them are handed identical bits at identical strides.

Centre pooling in the plain form is written here, from subgraphs.roots: pooling_restatement.torch_center_pool assumes the roots at
local indices 0 and 1, which the engine's batches do not promise.  The plain sort pool takes its order as an argument (the package
run's perm: a float64 sort may break near-ties differently; that the order is a valid one is pinned in tests/test_pooling_gpu.py).

The float64 comparison (`error_table`): for a tensor with s = max|R64|, e_hip = max|got - R64| / s must not exceed 4 * e_32 + 2^-23,
e_32 = max|R32 - R64| / s the plain form's own float32 error.  One mend: the bias of a Linear that feeds a training-mode BatchNorm1d
has a gradient that is identically 0 in exact arithmetic (the batch mean is subtracted), so max|R64| of it is float64 rounding noise
(about 1e-17) and says nothing about scale.  For those biases (`Model.annihilated`) s is max|R64| of the same Linear's weight gradient,
and the table checks that the float64 gradient is indeed below 1e-9 of it.  Every other tensor is measured exactly as stated.
R32 runs on ONE CPU thread (`float64_runs`).  torch's threaded CPU reductions cut a sum into per-thread pieces whose number and order
are not fixed, so e_32 changed from run to run and from host to host -- for a one-element tensor that is a cancelling sum, by enough
to change the verdict.  On one thread R32 is one well-defined evaluation: long sums in one running order, as the kernels' pinned
order sums a row, which is the pair the bound's premise speaks of (two float32 evaluations that differ only in summation order).
"""
import copy
import functools
import types
from collections import OrderedDict

import numpy as np
import torch
from torch.autograd.function import once_differentiable
from torch.nn import functional as F
from torch.utils.checkpoint import checkpoint as _checkpoint

import aggr_restatement as ar
import gcn_restatement as gr
import link_decoder_restatement as lr
import pooling_restatement as pr

F_IN, HIDDEN, SEAL_HIDDEN = 20, 30, 32  # HIDDEN is deliberately no multiple of 4: the padded products, the decoder's scalar path
MAX_Z = 1000  # the reference's max_z: the rows of SEAL's label embedding; larger labels (unreachable nodes) are clamped to the last one
MARGIN, FLOOR = 4.0, 2.0 ** -23
LABEL_SEEDS = (101, 102, 103)  # the three SGD steps
STEP_SEED = 100                # the labels of the single step


# ---- what the twins and the plain forms are given in place of the package's plans ---------------------------------------------------
class HostGraph(object):
    """an edge list on the host: n, ei int64 [2, E], w float32 [E] or None (unit weights)"""

    def __init__(self, n, edge_index, weight=None):
        self.n = int(n)
        self.ei = np.ascontiguousarray(edge_index, dtype=np.int64).reshape(2, -1)
        self.w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float32)

    def weights(self):
        return np.ones(self.ei.shape[1], dtype=np.float32) if self.w is None else self.w

    def torch(self, dtype):
        return torch.from_numpy(self.ei[0]), torch.from_numpy(self.ei[1]), torch.from_numpy(self.weights()).to(dtype)


class HostLinks(object):
    def __init__(self, n, links):
        self.n, self.links = int(n), np.ascontiguousarray(links, dtype=np.int64).reshape(-1, 2)


class HostPools(object):
    """the graphs of a readout: rowptr int64 [L + 1], roots int32 [L, 2] (centre pooling), k (sort pooling), and for the plain sort
    pool the order to use, perm int32 [L, k] (-1: no node)"""

    def __init__(self, rowptr, roots=None, k=None, perm=None):
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        self.roots = None if roots is None else np.ascontiguousarray(roots, dtype=np.int32)
        self.k, self.perm = k, perm

    @property
    def num_graphs(self):
        return len(self.rowptr) - 1

    def batch(self):
        return torch.from_numpy(np.repeat(np.arange(self.num_graphs, dtype=np.int64), np.diff(self.rowptr)))


def _host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)


def _device(a, like):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(like.device)


def _padded(a, like):
    """float32 [n, F] on like's device in the layout of the package's products: a [n, F + pad] buffer, pad = -F % 4, sliced to F"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    pad = (-t.size(1)) % 4
    if not pad:
        return t.to(like.device)
    return F.pad(t, (0, pad)).to(like.device)[:, :t.size(1)]


# ---- the twins: the restatements behind autograd ------------------------------------------------------------------------------------
class _TwinPropagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g):
        ctx.g = g
        return _padded(gr.propagate(g.ei, g.weights(), g.n, _host(x), 'target'), x)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        g = ctx.g
        return _padded(gr.propagate(g.ei, g.weights(), g.n, _host(grad), 'source'), grad), None  # (the other flow is the backward)


class _TwinAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, root, g, mean):
        ctx.g, ctx.aggr, ctx.has_root = g, 'mean' if mean else 'sum', root is not None
        ctx.save_for_backward(*((x.contiguous(), root) if ctx.has_root else ()))
        r = _host(root)[0] if ctx.has_root else None
        return _padded(ar.aggregate(g.ei, g.w, g.n, _host(x), 'target', ctx.aggr, r), x)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        g, grad, saved = ctx.g, grad.contiguous(), ctx.saved_tensors  # (read once: torch.utils.checkpoint unpacks a tensor once)
        r = _host(saved[1])[0] if ctx.has_root else None
        grad_x = _padded(ar.aggregate_grad(g.ei, g.w, g.n, _host(grad), 'target', ctx.aggr, r), grad)
        grad_root = (grad * saved[0]).sum().reshape(1) if ctx.has_root else None
        return grad_x, grad_root, None, None


class _TwinGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, links):
        ctx.links = links
        return _device(lr.gather(_host(x), links.links), x)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return _device(lr.grad(ctx.links.links, ctx.links.n, _host(grad)), grad), None


class _TwinHadamard(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, links):
        ctx.links = links
        ctx.save_for_backward(x)
        return _device(lr.hadamard(_host(x), links.links), x)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        (x,) = ctx.saved_tensors
        return _device(lr.grad(ctx.links.links, ctx.links.n, _host(grad), _host(x)), grad), None


class _TwinSortPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pools):
        out, perm = pr.sort_pool(_host(x), pools.rowptr, pools.k)
        ctx.pools, ctx.perm, ctx.T = pools, perm, x.size(0)
        return _device(out, x)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return _device(pr.sort_pool_backward(_host(grad), ctx.pools.rowptr, ctx.perm, ctx.T), grad), None


class _TwinMeanPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pools):
        ctx.pools, ctx.T = pools, x.size(0)
        return _device(pr.segment_pool(_host(x), pools.rowptr, mean=True), x)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return _device(pr.segment_pool_backward(_host(grad), ctx.pools.rowptr, ctx.T, mean=True), grad), None


class _TwinCenterPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pools):
        ctx.pools = pools
        ctx.save_for_backward(x)
        return _device(pr.center_pool(_host(x), pools.rowptr, pools.roots), x)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        (x,) = ctx.saved_tensors
        return _device(pr.center_pool_backward(_host(x), _host(grad), ctx.pools.rowptr, ctx.pools.roots), grad), None


def twin_aggregate(x, g, mean, root):
    return _TwinAggregate.apply(x, root, g, mean)


# ---- the plain forms: torch ops from the definitions, any dtype ---------------------------------------------------------------------
def plain_norm(g, dtype):
    """gcn_norm from its definition -> (row, col, norm): existing self loops are removed, every node gets one loop -- of weight 1, or
    of the weight of its last explicit loop --, deg is the weighted in-degree over edge_index[1], norm = deg^-1/2[row] w deg^-1/2[col]
    with 1 / sqrt(0) taken as 0"""
    row, col, w = g.torch(dtype)
    keep = row != col
    loop_w = torch.ones(g.n, dtype=dtype)
    for e in torch.nonzero(~keep).view(-1).tolist():  # ascending: the last explicit loop wins
        loop_w[int(row[e])] = w[e]
    ids = torch.arange(g.n)
    row, col, w = torch.cat([row[keep], ids]), torch.cat([col[keep], ids]), torch.cat([w[keep], loop_w])
    deg = torch.zeros(g.n, dtype=dtype).index_add_(0, col, w)
    dinv = deg.pow(-0.5)
    dinv = torch.where(torch.isinf(dinv), torch.zeros_like(dinv), dinv)
    return row, col, dinv[row] * w * dinv[col]


def plain_propagate(x, g):
    row, col, norm = plain_norm(g, x.dtype)
    return x.new_zeros((g.n, x.size(1))).index_add_(0, col, norm[:, None] * x[row])


def plain_aggregate(x, g, mean, root):
    row, col, w = g.torch(x.dtype)
    out = x.new_zeros((g.n, x.size(1))).index_add_(0, col, w[:, None] * x[row])
    if mean:
        den = torch.zeros(g.n, dtype=x.dtype).index_add_(0, col, w)
        den = torch.where(torch.bincount(col, minlength=g.n) == 0, torch.ones_like(den), den)
        out = out / den[:, None]
    return out if root is None else out + root * x


def plain_gather(x, links):
    return x[torch.from_numpy(links.links)]


def plain_hadamard(x, links):
    at = torch.from_numpy(links.links)
    return x[at[:, 0]] * x[at[:, 1]]


def plain_mean_pool(x, pools):
    return pr.torch_segment_pool(x, pools.batch(), pools.num_graphs, mean=True)


def plain_center_pool(x, pools):
    roots, start = torch.from_numpy(pools.roots).to(torch.int64), torch.from_numpy(pools.rowptr[:-1])
    live = roots[:, 0] >= 0  # (a row emptied by max_nodes has roots (-1, -1) and gives zeros)
    last = max(x.size(0) - 1, 0)
    a, b = (start + roots[:, 0].clamp(min=0)).clamp(max=last), (start + roots[:, 1].clamp(min=0)).clamp(max=last)
    return x[a] * x[b] * live[:, None].to(x.dtype)


def plain_sort_pool(x, pools):
    if pools.perm is None:
        raise ValueError('the plain sort pool is given its order (HostPools.perm)')
    perm = torch.from_numpy(np.asarray(pools.perm)).to(torch.int64)
    at = (torch.from_numpy(pools.rowptr[:-1])[:, None] + perm.clamp(min=0)).clamp(max=max(x.size(0) - 1, 0))
    out = x[at] * (perm >= 0)[:, :, None].to(x.dtype)
    return out.reshape(perm.size(0), perm.size(1) * x.size(1))


# ---- the layers, restated with the package's (PyG's) parameter names -----------------------------------------------------------------
class GCNConv(torch.nn.Module):
    """out = propagate(x W^T) + bias; parameters `lin.weight`, `bias`"""

    def __init__(self, propagate, in_channels, out_channels):
        super().__init__()
        self._propagate = propagate
        self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.bias = torch.nn.Parameter(torch.zeros(out_channels))

    def forward(self, x, graph):
        return self._propagate(F.linear(x, self.lin.weight), graph) + self.bias


class SAGEConv(torch.nn.Module):
    """out = lin_l(mean aggregate(x)) + lin_r(x); parameters `lin_l.weight`, `lin_l.bias`, `lin_r.weight`"""

    def __init__(self, aggregate, in_channels, out_channels):
        super().__init__()
        self._aggregate = aggregate
        self.lin_l = torch.nn.Linear(in_channels, out_channels, bias=True)
        self.lin_r = torch.nn.Linear(in_channels, out_channels, bias=False)

    def forward(self, x, graph):
        out = self.lin_l(self._aggregate(x, graph, True, None))
        return out + self.lin_r(x)


class GINConv(torch.nn.Module):
    """out = nn(sum aggregate(x) + (1 + eps) x); state `nn.*`, `eps`"""

    def __init__(self, aggregate, nn, train_eps=False):
        super().__init__()
        self._aggregate = aggregate
        self.nn = nn
        if train_eps:
            self.eps = torch.nn.Parameter(torch.zeros(1))
        else:
            self.register_buffer('eps', torch.zeros(1))

    def forward(self, x, graph):
        return self.nn(self._aggregate(x, graph, False, 1.0 + self.eps))


def _ops(propagate, aggregate, gather, hadamard, sort_pool, mean_pool, center_pool):
    return types.SimpleNamespace(gcn=functools.partial(GCNConv, propagate), sage=functools.partial(SAGEConv, aggregate),
                                 gin=functools.partial(GINConv, aggregate), gather=gather, hadamard=hadamard, sort_pool=sort_pool,
                                 mean_pool=mean_pool, center_pool=center_pool)


def twin_ops():
    return _ops(_TwinPropagate.apply, twin_aggregate, _TwinGather.apply, _TwinHadamard.apply, _TwinSortPool.apply, _TwinMeanPool.apply,
                _TwinCenterPool.apply)


def plain_ops():
    return _ops(plain_propagate, plain_aggregate, plain_gather, plain_hadamard, plain_sort_pool, plain_mean_pool, plain_center_pool)


# ---- the models -------------------------------------------------------------------------------------------------------------------
def _args(graph):
    """what a conv is called with behind x: a plan (or a HostGraph), or a tuple (edge_index, edge_weight) of plain tensors"""
    return graph if isinstance(graph, tuple) else (graph,)


class _Model(torch.nn.Module):
    """forward(b, taps) -> logits [L].  b: a namespace of the inputs; taps (a dict) receives the conv stack's output ('stack') and the
    decoded / pooled tensor ('readout').  checkpoint: None, or use_reentrant for torch.utils.checkpoint around the conv stack."""
    annihilated = {}  # bias -> the weight of the same Linear, for every Linear that feeds a training-mode BatchNorm1d
    checkpoint = None

    def _stack(self, h, graph):
        if self.checkpoint is None:
            return self.stack(h, graph)
        return _checkpoint(self.stack, h, graph, use_reentrant=self.checkpoint)


class Elph(_Model):
    """Linear encoder, two residual GCNConv, the link predictor on (a) link_gather and the product of its halves or (b) link_hadamard,
    concatenated with the structure-feature branch.  b: x [N, F_IN], graph, links, sf [L, sf_dim]"""
    annihilated = {'lin_out.bias': 'lin_out.weight', 'label_lin_layer.bias': 'label_lin_layer.weight'}

    def __init__(self, ops, sf_dim, variant, f_in=F_IN, hidden=HIDDEN):
        super().__init__()
        assert variant in ('gather', 'hadamard')
        self.ops, self.variant = ops, variant
        self.encoder = torch.nn.Linear(f_in, hidden)
        self.convs = torch.nn.ModuleList([ops.gcn(hidden, hidden), ops.gcn(hidden, hidden)])
        self.lin_out = torch.nn.Linear(hidden, hidden)
        self.bn_feats = torch.nn.BatchNorm1d(hidden)
        self.label_lin_layer = torch.nn.Linear(sf_dim, sf_dim)
        self.bn_labels = torch.nn.BatchNorm1d(sf_dim)
        self.lin = torch.nn.Linear(sf_dim + hidden, 1)

    def stack(self, x, graph):
        x = self.encoder(x)
        for conv in self.convs:
            x = x + conv(x, *_args(graph))  # the residual form: x has two consumers
        return x

    def forward(self, b, taps=None):
        h = self._stack(b.x, b.graph)
        if self.variant == 'gather':
            y = self.ops.gather(h, b.links)
            d = y[:, 0] * y[:, 1]
        else:
            d = self.ops.hadamard(h, b.links)
        if taps is not None:
            taps['stack'], taps['readout'] = h, d
        f = torch.relu(self.bn_feats(self.lin_out(d)))
        s = torch.relu(self.bn_labels(self.label_lin_layer(b.sf)))
        return self.lin(torch.cat([s, f], 1)).view(-1)


class _Seal(_Model):
    """b: z int64 [T], graph, pools"""

    def forward(self, b, taps=None):
        h = self._stack(self.z_embedding(b.z), b.graph)
        p = self.readout(h, b.pools)
        if taps is not None:
            taps['stack'], taps['readout'] = h, p
        return self.head(p).view(-1)


class SealSage(_Seal):
    def __init__(self, ops, max_z, hidden=SEAL_HIDDEN):
        super().__init__()
        self.ops = ops
        self.z_embedding = torch.nn.Embedding(max_z, hidden)
        self.convs = torch.nn.ModuleList([ops.sage(hidden, hidden), ops.sage(hidden, hidden)])
        self.lin = torch.nn.Linear(hidden, 1)

    def stack(self, h, graph):
        for conv in self.convs:
            h = torch.relu(conv(h, *_args(graph)))
        return h

    def readout(self, h, pools):
        return self.ops.center_pool(h, pools)

    def head(self, p):
        return self.lin(p)


def _mlp(a, b):
    return torch.nn.Sequential(torch.nn.Linear(a, b), torch.nn.BatchNorm1d(b), torch.nn.ReLU(), torch.nn.Linear(b, b))


class SealGin(_Seal):
    annihilated = {'convs.0.nn.0.bias': 'convs.0.nn.0.weight', 'convs.1.nn.0.bias': 'convs.1.nn.0.weight'}

    def __init__(self, ops, max_z, hidden=SEAL_HIDDEN):
        super().__init__()
        self.ops = ops
        self.z_embedding = torch.nn.Embedding(max_z, hidden)
        self.convs = torch.nn.ModuleList([ops.gin(_mlp(hidden, hidden), train_eps=True), ops.gin(_mlp(hidden, hidden), train_eps=True)])
        self.lin = torch.nn.Linear(hidden, 1)

    def stack(self, h, graph):
        for conv in self.convs:
            h = conv(h, *_args(graph))
        return h

    def readout(self, h, pools):
        return self.ops.mean_pool(h, pools)

    def head(self, p):
        return self.lin(p)


class SealDgcnn(_Seal):
    """tanh(GCNConv) x 3, the last one GCNConv(hidden, 1): a one-column product; the three outputs side by side, sort pooling to k
    rows, then Conv1d / MaxPool1d / Conv1d and two Linear"""

    def __init__(self, ops, max_z, k, hidden=SEAL_HIDDEN):
        super().__init__()
        self.ops, self.k = ops, int(k)
        self.z_embedding = torch.nn.Embedding(max_z, hidden)
        self.convs = torch.nn.ModuleList([ops.gcn(hidden, hidden), ops.gcn(hidden, hidden), ops.gcn(hidden, 1)])
        width = 2 * hidden + 1
        self.conv1 = torch.nn.Conv1d(1, 16, width, width)
        self.maxpool1d = torch.nn.MaxPool1d(2, 2)
        self.conv2 = torch.nn.Conv1d(16, 32, 5, 1)
        dense = (int((self.k - 2) / 2 + 1) - 5 + 1) * 32
        self.lin1 = torch.nn.Linear(dense, 128)
        self.lin2 = torch.nn.Linear(128, 1)

    def stack(self, h, graph):
        xs = []
        for conv in self.convs:
            h = torch.tanh(conv(h, *_args(graph)))
            xs.append(h)
        return torch.cat(xs, dim=-1)

    def readout(self, h, pools):
        return self.ops.sort_pool(h, pools)

    def head(self, p):
        x = torch.relu(self.conv1(p.unsqueeze(1)))
        x = torch.relu(self.conv2(self.maxpool1d(x)))
        return self.lin2(torch.relu(self.lin1(x.view(x.size(0), -1))))


# ---- the shared inputs --------------------------------------------------------------------------------------------------------------
HOT = 300  # the node of more than 256 endpoint slots: a hub row of the decoder's backward at the default hub_entries


def elph_inputs(seed=5):
    """gcn_restatement.planted('random') (N = 601), x float32 [N, F_IN] and about 700 links: random pairs, a self link, a duplicated
    link, both hubs (in-degree 300, out-degree 300), the node whose only edge is a loop of weight 0, and HOT in 280 slots"""
    rng = np.random.RandomState(seed)
    ei, w = gr.planted('random')
    hub_in, hub_out = gr.IN_NODES[-1], gr.OUT_NODES[-1]
    links = [tuple(p) for p in rng.randint(0, gr.N, size=(413, 2))]
    links += [(77, 77), (12, 345), (12, 345), (hub_in, hub_out), (hub_out, 3), (gr.ZERO_LOOP, 8), (9, gr.ZERO_LOOP)]
    others = rng.randint(0, gr.N, size=280)
    links += [(HOT, int(o)) if i % 2 == 0 else (int(o), HOT) for i, o in enumerate(others)]
    links = np.array(links, dtype=np.int64)[rng.permutation(len(links))]
    x = gr.features(gr.N, F_IN, seed=seed + 1)
    return types.SimpleNamespace(n=gr.N, ei=ei, w=w, x=x, links=np.ascontiguousarray(links))


def small_elph_inputs(seed=9, n=40, L=50):
    """the same shape at a reduced size (the host test): a random directed weighted graph with loops and an isolated node"""
    rng = np.random.RandomState(seed)
    ei = rng.randint(0, n - 1, size=(2, 160)).astype(np.int64)  # node n - 1 is isolated
    ei[:, :3] = [[4, 4, 7], [4, 4, 7]]                           # two explicit loops at one node, one at another
    w = rng.uniform(0.25, 2.0, size=ei.shape[1]).astype(np.float32)
    links = rng.randint(0, n, size=(L, 2)).astype(np.int64)
    links[:4] = [[3, 3], [5, 6], [5, 6], [n - 1, 2]]
    return types.SimpleNamespace(n=n, ei=ei, w=w, x=gr.features(n, F_IN, seed=seed + 1), links=links)


def subgraph_edges(rowptr, adj_ptr, nbr):
    """int64 [2, A] in batch-global node slots from a subgraph batch's arrays: source rowptr[q] + nbr, target t"""
    rowptr, adj_ptr = np.asarray(rowptr, dtype=np.int64), np.asarray(adj_ptr, dtype=np.int64)
    T = len(adj_ptr) - 1
    target = np.repeat(np.arange(T, dtype=np.int64), np.diff(adj_ptr))
    link_of = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    return np.stack([rowptr[:-1][link_of][target] + np.asarray(nbr, dtype=np.int64), target])


def clamp_z(z):
    """the subgraph labels as the models' Embedding(MAX_Z, .) takes them"""
    return z.clamp(max=MAX_Z - 1)


def labels_for(L, seed, device='cpu', dtype=torch.float32):
    return torch.from_numpy((np.random.RandomState(seed).rand(L) < 0.5).astype(np.float32)).to(device=device, dtype=dtype)


ELPH_SEED, SEAL_SEED = 41, 43


def build(make, ops, seed):
    """make(ops) from a seed, on the CPU, with every parameter that torch initialises to a constant (BatchNorm's weight and bias, a
    zero bias, GIN's eps) moved off it by a seeded amount in [-0.5, 0.5).  The GPU test loads this state into the package model, so
    the host test's stand-in run and the GPU run start from the same numbers."""
    torch.manual_seed(seed)
    model = make(ops)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for p in model.parameters():
            if p.numel() and bool((p == p.view(-1)[0]).all()):
                p.add_(torch.rand(p.shape, generator=g) - 0.5)
    return model


def copy_state(src, dst):
    """dst's state becomes a deep copy of src's (moved to dst's device and dtype)"""
    dst.load_state_dict(copy.deepcopy(src.state_dict()))
    return dst


# ---- one step, and what is compared ---------------------------------------------------------------------------------------------------
def step(model, batch, labels, input_grad=True, backwards=1):
    """forward, BCE-with-logits, backward (backwards > 1: again on the retained graph, without zero_grad).  Returns an ordered dict:
    loss, logits, 'grad <parameter>' for every parameter, 'grad x' for an ELPH batch, the gradients of the two taps -- the conv
    stack's output through register_hook, the decoded / pooled tensor through retain_grad -- and 'buffer <name>' after the step.
    A tensor that received no gradient is None."""
    model.zero_grad(set_to_none=True)
    b = copy.copy(batch)
    if getattr(batch, 'x', None) is not None:
        b.x = batch.x.detach().clone().requires_grad_(input_grad)
    taps, hooked = {}, []
    logits = model(b, taps)
    loss = F.binary_cross_entropy_with_logits(logits, labels)
    if taps['stack'].requires_grad:
        taps['stack'].register_hook(lambda g: hooked.append(g.detach().clone()))
    if taps['readout'].requires_grad:
        taps['readout'].retain_grad()
    for i in range(backwards):
        loss.backward(retain_graph=i + 1 < backwards)
    out = OrderedDict(loss=loss.detach().clone(), logits=logits.detach().clone())
    for name, p in model.named_parameters():
        out['grad ' + name] = None if p.grad is None else p.grad.detach().clone()
    if getattr(batch, 'x', None) is not None:
        out['grad x'] = None if b.x.grad is None else b.x.grad.detach().clone()
    out['tap stack'] = hooked[0] if hooked else None
    out['tap readout'] = None if taps['readout'].grad is None else taps['readout'].grad.detach().clone()
    for name, buf in model.named_buffers():
        out['buffer ' + name] = buf.detach().clone()
    return out


def sgd_steps(model, batch, seeds=LABEL_SEEDS, lr=0.05):
    """three torch.optim.SGD steps, fresh seeded labels each: per step loss, logits and every parameter after it"""
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    device = next(model.parameters()).device
    dtype = next(model.parameters()).dtype
    trail = []
    for seed in seeds:
        r = step(model, batch, labels_for(batch.num_links, seed, device, dtype))
        opt.step()
        rec = OrderedDict(loss=r['loss'], logits=r['logits'])
        for name, p in model.named_parameters():
            rec['param ' + name] = p.detach().clone()
        trail.append(rec)
    return trail


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def differing(got, want, keys=None):
    """the names (with a count) of the entries of two step records whose bits differ; [] when every compared entry is identical"""
    assert list(got) == list(want), f'the records list different tensors: {sorted(set(got) ^ set(want))}'
    bad = []
    for key in (list(got) if keys is None else keys):
        a, b = got[key], want[key]
        if a is None or b is None:
            if a is not b:
                bad.append(f'{key}: one of the two is None')
            continue
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append(f'{key}: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}')
            continue
        n = int((_bits(a) != _bits(b)).sum())
        if n:
            bad.append(f'{key}: {n} of {a.numel()} elements differ, max |difference| {float((a.cpu().double() - b.cpu().double()).abs().max()):.3e}')
    return bad


def compared_in_float64(record):
    return [k for k in record if k in ('loss', 'logits') or k.startswith('grad ')]


def error_table(model, got, r64, r32):
    """rows (name, s, e_hip, e_32, ratio, ok) for loss, logits, every parameter gradient and the input gradient (module docstring)"""
    f64 = lambda t: t.detach().cpu().double().numpy()
    rows = []
    for key in compared_in_float64(r64):
        assert got[key] is not None and r64[key] is not None and r32[key] is not None, f'{key}: no gradient'
        g, a, b = f64(got[key]), f64(r64[key]), f64(r32[key])
        s = float(np.abs(a).max())
        name = key[5:] if key.startswith('grad ') else None
        if name in model.annihilated:
            layer = float(np.abs(f64(r64['grad ' + model.annihilated[name]])).max())
            assert s <= 1e-9 * layer, f'{key}: expected an exactly-zero gradient, float64 gives {s:.3e} beside {layer:.3e}'
            s = layer
        assert s > 0, f'{key}: the float64 value is all zeros'
        e_hip, e_32 = float(np.abs(g - a).max()) / s, float(np.abs(b - a).max()) / s
        rows.append((key, s, e_hip, e_32, e_hip / e_32 if e_32 > 0 else float('inf'), e_hip <= MARGIN * e_32 + FLOOR))
    return rows


def format_table(title, rows):
    lines = [f'[model steps] {title}: e_hip = max|got - R64| / s, e_32 = max|R32 - R64| / s, s = max|R64|',
             f'  {"tensor":<34} {"s":>10} {"e_hip":>10} {"e_32":>10} {"e_hip/e_32":>10}']
    for key, s, e_hip, e_32, ratio, ok in rows:
        lines.append(f'  {key:<34} {s:10.3e} {e_hip:10.3e} {e_32:10.3e} {ratio:10.3f}{"" if ok else "   ABOVE 4 * e_32 + 2^-23"}')
    return '\n'.join(lines)


def float64_runs(make_model, source, batch, labels):
    """the plain form on the CPU with source's parameters, in float64 and in float32: (R64, R32) step records.
    make_model(ops) builds the model class; batch holds host handles and float32 CPU tensors"""
    runs, threads = [], torch.get_num_threads()
    torch.set_num_threads(1)  # (one thread: the sums of R32 have one order, so e_32 is the same number in every run on a host)
    try:
        for dtype in (torch.float64, torch.float32):
            model = make_model(plain_ops())
            model.load_state_dict({k: v.detach().cpu() for k, v in source.state_dict().items()})
            model = model.to(dtype)
            model.train(source.training)
            b = copy.copy(batch)
            for name in ('x', 'sf'):
                if getattr(batch, name, None) is not None:
                    setattr(b, name, getattr(batch, name).detach().cpu().to(dtype))
            runs.append(step(model, b, labels.detach().cpu().to(dtype)))
    finally:
        torch.set_num_threads(threads)
    return runs
