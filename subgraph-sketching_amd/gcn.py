"""A trainable GCNConv on the engine's groupings: ELPH's `feature_conv` (reference models/elph.py:131-160, 214), which train_elph
runs on the whole graph for every batch and differentiates (reference runners/train.py:188-213).

PyG is absent from this image, so its semantics are RESTATED (as in sign.py): gcn_norm with its defaults, then aggregation at the
TARGET, out[col_e] += norm_e * x[row_e] -- the transpose of torch_sparse.spmm's out[row_e] += norm_e * x[col_e] that sign.py serves.
Each product is the other's gradient with respect to x, so two kernels give both flows a backward:
  flow='target'  ss_gcn_spmm_t  (grouping by column; GCNConv)       backward: ss_sign_spmm
  flow='source'  ss_sign_spmm   (grouping by row; torch_sparse.spmm) backward: ss_gcn_spmm_t
Both accumulate every output element in one lane, in ascending edge order with the node's remaining loop last, so forward AND
backward are reproducible bit for bit (no float atomics) and equal the sequential fp32 scatter-add.

`GCNGraph` is the plan (both stable groupings, the scan words, dinv, loop_w), built once per graph; `gcn_propagate` the
differentiable product; `GCNConv` the layer with PyG's parameter names.  There is no CPU fallback.
"""
import math

import torch

from . import _native
from ._plans import _PlanCache, check_edge_list, device_edge_list, padded_rows
from ._runtime import _compute_device, _ptr, _stream
from .sign import group_ids_stable


class GCNGraph(object):
    """gcn_norm(edge_index, edge_weight, num_nodes) in the form the two product kernels read: the STABLE groupings of the edge
    indices by row and by column (both always sorted -- unlike generate_sign_features, which lets the column grouping go unsorted
    for unit weights: here its order is an accumulation order), ss_gcn_scan_edges' words, dinv and loop_w.  One host read (the
    bounds flags); ids outside [0, num_nodes) raise IndexError.  The edge list is copied: later edits of `edge_index` do not reach
    a plan.  edge_weight (default: ones) is a constant of the product, not a differentiable input.  device: where the plan lives
    (default: the edge list's GPU, or the current one for host tensors)."""
    builds = 0  # plans built so far (the layer cache's tests count them)

    def __init__(self, num_nodes, edge_index, edge_weight=None, device=None):
        n, E = check_edge_list(num_nodes, edge_index, edge_weight)
        lib = _native.lib()
        device = torch.device(device) if device is not None else _compute_device(edge_index, edge_weight)  # (host tensors: the current GPU)
        ei, self.row, self.col, self.w, no_order = device_edge_list(edge_index, edge_weight, device,
                                                                     lambda E: torch.ones(max(E, 1), dtype=torch.float32, device=device))
        self.num_nodes, self.num_edges, self.device = n, E, device
        err = torch.zeros(1, dtype=torch.int32, device=device)
        self.scan = torch.empty(lib.ss_gcn_scan_bytes(n), dtype=torch.uint8, device=device)
        _native.check(lib.ss_gcn_scan_edges(_ptr(self.row), _ptr(self.col), _ptr(self.w), E, n, _ptr(self.scan), _stream(device)),
                      'ss_gcn_scan_edges')
        self.rowptr_c, self.order_c = group_ids_stable(ei[1], n, err)
        self.rowptr_r, self.order_r = group_ids_stable(ei[0], n, err)
        if E == 0:
            self.order_c = self.order_r = no_order
        self.dinv = torch.empty(n, dtype=torch.float32, device=device)
        self.loop_w = torch.empty(n, dtype=torch.float32, device=device)
        _native.check(lib.ss_gcn_degree(_ptr(self.rowptr_c), _ptr(self.order_c), _ptr(self.row), _ptr(self.w), n, _ptr(self.scan), _ptr(self.dinv),
                                        _ptr(self.loop_w), _stream(device)), 'ss_gcn_degree')
        # (the one host read) the groupings' flag, or the scan's own word for ids outside [0, N), negative ones included
        if int((err + self.scan[4:8].view(torch.int32)).item()):
            raise IndexError('edge_index refers to nodes outside [0, num_nodes)')
        GCNGraph.builds += 1

    def product(self, x, target):
        """A^T x (target: aggregation at edge_index[1], GCNConv) or A x (aggregation at edge_index[0], torch_sparse.spmm) for
        contiguous fp32 x [N, F] on this device"""
        n, F = self.num_nodes, x.size(1)
        if F == 0:
            return torch.empty((n, F), dtype=torch.float32, device=self.device)
        lib = _native.lib()

        def run(Fp, x):
            out = torch.empty((n, Fp), dtype=torch.float32, device=self.device)
            if target:
                _native.check(lib.ss_gcn_spmm_t(_ptr(self.rowptr_c), _ptr(self.order_c), _ptr(self.row), _ptr(self.w), _ptr(self.dinv), _ptr(self.loop_w),
                                                _ptr(self.scan), n, _ptr(x), Fp, _ptr(out), _stream(self.device)), 'ss_gcn_spmm_t')
            else:
                _native.check(lib.ss_sign_spmm(_ptr(self.rowptr_r), _ptr(self.order_r), _ptr(self.col), _ptr(self.w), _ptr(self.dinv), _ptr(self.loop_w),
                                               _ptr(self.scan), n, _ptr(x), Fp, _ptr(out), _stream(self.device)), 'ss_sign_spmm')
            return out

        return padded_rows(run, F, x)


class _Propagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, graph, target):
        ctx.graph, ctx.target = graph, target  # (nothing else is saved: the product is linear in x)
        return graph.product(x.contiguous(), target)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        return ctx.graph.product(grad_out.contiguous(), not ctx.target), None, None


def gcn_propagate(x, graph, flow='target'):
    """gcn_norm(A) applied to node features x (fp32 [N, F] on the graph's device), differentiable in x.
    flow='target': out[col_e] += norm_e * x[row_e] (GCNConv, PyG's default flow); flow='source': out[row_e] += norm_e * x[col_e]
    (torch_sparse.spmm; bit for bit sign.generate_sign_features(x, ei, w, 0)).  The backward is the other flow of grad_out."""
    if flow not in ('target', 'source'):
        raise ValueError(f"flow must be 'target' or 'source', got {flow!r}")
    if not isinstance(graph, GCNGraph):
        raise ValueError('graph must be a GCNGraph')
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.size(0) != graph.num_nodes:
        raise ValueError(f'x must be a float32 tensor [{graph.num_nodes}, F]')
    if x.device != graph.device:
        raise ValueError(f'x is on {x.device}, the graph on {graph.device}: there is no CPU fallback and no silent copy')
    return _Propagate.apply(x, graph, flow == 'target')


_CACHE = _PlanCache()  # the plan of the edge_index tensor seen last, shared by every layer: the h convs of one forward do one build


class GCNConv(torch.nn.Module):
    """torch_geometric.nn.GCNConv with its defaults [PyG semantics restated]: out = gcn_norm(A)^T (x W^T) + bias.  Parameters are
    `lin.weight` [out, in] (glorot-uniform) and `bias` [out] (zeros), so a checkpoint written with PyG's layer loads.  The
    keywords of PyG's layer that change the mathematics are accepted at their defaults only."""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, add_self_loops=None, normalize=True, bias=True, **kwargs):
        super().__init__()
        given = dict(improved=(improved, (False,)), cached=(cached, (False,)), add_self_loops=(add_self_loops, (None, True)),
                     normalize=(normalize, (True,)), aggr=(kwargs.pop('aggr', 'add'), ('add',)),
                     flow=(kwargs.pop('flow', 'source_to_target'), ('source_to_target',)))
        for name, (value, allowed) in given.items():
            if not any(value is a or value == a for a in allowed):
                raise NotImplementedError(f'GCNConv({name}={value!r}) is not built here: only {name}={allowed[-1]!r}')
        if kwargs:
            raise TypeError(f'GCNConv got unexpected keywords {sorted(kwargs)}')
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.lin = torch.nn.Linear(self.in_channels, self.out_channels, bias=False)
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(self.out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        bound = math.sqrt(6.0 / (self.in_channels + self.out_channels))  # PyG's glorot
        with torch.no_grad():
            self.lin.weight.uniform_(-bound, bound)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, x, edge_index, edge_weight=None):
        """edge_index: a GCNGraph (never rebuilt), or an int64 tensor [2, E] whose plan the module-level cache keeps while the
        SAME tensor object comes back unedited; a fresh tensor of equal content rebuilds"""
        if isinstance(edge_index, GCNGraph):
            if edge_weight is not None:
                raise ValueError('a GCNGraph carries its own weights')
            graph = edge_index
        else:
            if not isinstance(x, torch.Tensor) or x.dim() != 2:
                raise ValueError('x must be a float32 tensor [N, in_channels]')
            device = x.device if x.is_cuda else None
            graph = _CACHE.get((x.size(0), device), (edge_index, edge_weight),
                               lambda: GCNGraph(x.size(0), edge_index, edge_weight, device=device))
        out = gcn_propagate(torch.nn.functional.linear(x, self.lin.weight), graph)  # PyG's order: transform, then propagate
        return out if self.bias is None else out + self.bias

    def __repr__(self):
        return f'{self.__class__.__name__}({self.in_channels}, {self.out_channels})'
