"""SAGEConv and GINConv on a sum / mean neighbour aggregation in HIP (csrc/ss_aggr.hip): the two SEAL models that
GCNConv does not serve (reference models/seal.py:116-173 SEALSAGE, :259-328 SEALGIN) and the SAGE baseline (models/gnn.py:90-113).

PyG is absent from this image, so its semantics are RESTATED (as in gcn.py): the unnormalised aggregation at the target,
out[col_e] (+)= w_e * x[row_e] -- no gcn_norm, existing self loops are ordinary entries, no loop is added.  SAGE divides by the row's
weight sum (the count for unit weights), GIN adds (1 + eps) * x_i.  Each flow's gradient with respect to x is the other flow:
  flow='target'  grouping by edge_index[1], gathering x[edge_index[0]]      backward: flow='source' of grad_out
  flow='source'  grouping by edge_index[0], gathering x[edge_index[1]]      backward: flow='target' of grad_out
The accumulation order is fixed (chunks of 256 entries, each summed sequentially in ascending edge order, the chunk sums added in
chunk order), so forward AND backward repeat bit for bit, and a row's bits do not depend on whether the row went through the
regular tier (one lane group walks the row) or the hub tier (one lane group per chunk, then a finish launch).

`AggrGraph` is the plan, `aggregate` the differentiable product, `SAGEConv` / `GINConv` the layers with PyG's parameter names.
There is no CPU fallback.
"""
import torch

from . import _native
from ._plans import _PlanCache, check_edge_list, device_edge_list, finish_hubs, list_hubs, padded_rows
from ._runtime import _compute_device, _ptr, _stream
from .sign import group_ids_stable

AGGR_CHUNK = 256  # the unit's SS_AGGR_CHUNK, which ss_aggr_chunk() returns: a plan checks that the two agree
# rows of more than this many entries go through the hub tier.  Measured (profiles/aggr_probe.txt): on the rank^-0.9 graph
# the product takes 8.6 / 9.0 / 39.9 ms without the tier and 0.28 / 0.43 / 1.64 ms at 256 (F = 128 / 256 / 1024); 256, one chunk, was
# the fastest of 256 .. 8192 at every width, and a graph without such rows never launches the tier.
DEFAULT_HUB_ENTRIES = 256


class _Side(object):
    """one grouping of a plan: the entries that arrive at every node, where their values come from, den and the hub lists"""
    __slots__ = ('rowptr', 'order', 'other', 'den', 'hub_rows', 'hub_chunk', 'chunk_hub', 'n_hubs', 'n_chunks')


class AggrGraph(object):
    """The plan of `aggregate`: both STABLE groupings of the edge indices (by edge_index[1] for flow='target', by edge_index[0] for
    flow='source'; both always sorted: the order inside a group is an accumulation order), den for both (the chunked sum of the
    weights into every node, the count for unit weights, 1 for a node without entries), and for both the rows of more than
    `hub_entries` entries with the offsets of their 256-entry chunks, listed on the device.  One host read: the bounds flags together
    with the hub and chunk totals; ids outside [0, num_nodes) raise IndexError.  The edge list is copied: later edits of `edge_index`
    do not reach a plan.  edge_weight (default: unit weights, which the kernels never gather) is a constant of the product, not a
    differentiable input.  hub_entries: None takes DEFAULT_HUB_ENTRIES.  device: where the plan lives (default: the edge list's GPU,
    or the current one for host tensors)."""
    builds = 0  # plans built so far (the layer cache's tests count them)

    def __init__(self, num_nodes, edge_index, edge_weight=None, hub_entries=None, device=None):
        n, E = check_edge_list(num_nodes, edge_index, edge_weight)
        if E >= 1 << 31:
            raise ValueError('edge lists of 2^31 edges or more are not supported')
        hub = DEFAULT_HUB_ENTRIES if hub_entries is None else hub_entries
        if isinstance(hub, bool) or not isinstance(hub, int) or hub < 1:
            raise ValueError(f'hub_entries must be a positive integer, got {hub_entries!r}')
        lib = _native.lib()
        if lib.ss_aggr_chunk() != AGGR_CHUNK:
            raise RuntimeError(f'the library sums chunks of {lib.ss_aggr_chunk()} entries, this module lists chunks of {AGGR_CHUNK}')
        device = torch.device(device) if device is not None else _compute_device(edge_index, edge_weight)  # (host tensors: the current GPU)
        ei, self.row, self.col, self.w, no_order = device_edge_list(edge_index, edge_weight, device, lambda E: None)  # (unit weights are never gathered)
        self.num_nodes, self.num_edges, self.device, self.hub_entries = n, E, device, hub
        err = torch.zeros(1, dtype=torch.int32, device=device)
        # negative ids: the groupings wrap them torch-style, PyG does not -- they are refused with the ones past the end
        bad = ((ei < 0) | (ei >= n)).any().to(torch.int64).reshape(1)
        cap = E // (hub + 1)  # a row of more than `hub` entries: there are at most this many
        sides, lists, totals = [], [], []
        for ids, other in ((self.col, self.row), (self.row, self.col)):
            s = _Side()
            s.rowptr, s.order = group_ids_stable(ids[:E], n, err)
            if E == 0:
                s.order = no_order
            s.other = other
            s.den = torch.empty(n, dtype=torch.float32, device=device)
            _native.check(lib.ss_aggr_degree(_ptr(s.rowptr), _ptr(s.order), _ptr(self.w), n, _ptr(s.den), _stream(device)), 'ss_aggr_degree')
            # the hub rows ascending and where their chunks start, without a host read
            *listed, n_hubs, n_chunks = list_hubs(s.rowptr[1:] - s.rowptr[:-1], hub, AGGR_CHUNK, cap)
            sides.append(s)
            lists.append(listed)
            totals += [n_hubs, n_chunks]
        # (the one host read) the groupings' flag and the sign test, with the four totals the hub launches are sized by
        flag, bad, h_t, c_t, h_s, c_s = torch.cat([err.to(torch.int64), bad] + totals).tolist()
        for s, listed, H, C in zip(sides, lists, (h_t, h_s), (c_t, c_s)):
            s.n_hubs, s.n_chunks = H, C
            s.hub_rows, s.hub_chunk, s.chunk_hub = finish_hubs(*listed, H, C)
        self.target, self.source = sides
        if flag or bad:  # (the plan is complete all the same: the kernels do not follow such an id)
            raise IndexError('edge_index refers to nodes outside [0, num_nodes)')
        AggrGraph.builds += 1

    @classmethod
    def from_subgraphs(cls, sg, hub_entries=None):
        """the plan of an ExactSubgraphs / SampledSubgraphs batch: its T listed nodes, the disjoint union's edge list, the arc
        multiplicities as weights (the edge_weight SEAL's layers receive)"""
        return cls(int(sg.ids.numel()), sg.edge_index(), sg.weight.to(torch.float32), hub_entries=hub_entries)

    def product(self, x, target, mean=False, root=None, root_x=None, gather_den=None):
        """one product for contiguous fp32 x [N, F] on this device.  target: aggregation at edge_index[1] (else at edge_index[0]);
        mean: divide by this side's den; root (fp32 [1] on the device) with root_x (default x): + root * root_x[i];
        gather_den (fp32 [N]): every gathered row is divided by its node's entry first"""
        n, F = self.num_nodes, x.size(1)
        if F == 0:
            return torch.empty((n, F), dtype=torch.float32, device=self.device)
        s = self.target if target else self.source
        lib, stream = _native.lib(), _stream(self.device)
        den = s.den if mean else None

        def run(Fp, x, root_x):
            if root is not None and root_x is None:
                root_x = x
            out = torch.empty((n, Fp), dtype=torch.float32, device=self.device)
            _native.check(lib.ss_aggr_rows(_ptr(s.rowptr), _ptr(s.order), _ptr(s.other), _ptr(self.w), n, self.hub_entries, _ptr(x), Fp, _ptr(gather_den),
                                           _ptr(den), _ptr(root), _ptr(root_x), _ptr(out), stream), 'ss_aggr_rows')
            if s.n_hubs:
                ws_bytes = lib.ss_aggr_workspace_bytes(s.n_chunks, Fp)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
                _native.check(lib.ss_aggr_hub_partials(_ptr(s.rowptr), _ptr(s.order), _ptr(s.other), _ptr(self.w), n, _ptr(s.hub_rows),
                                                       _ptr(s.hub_chunk), _ptr(s.chunk_hub), s.n_hubs, s.n_chunks, _ptr(x), Fp, _ptr(gather_den), _ptr(ws),
                                                       ws_bytes, stream), 'ss_aggr_hub_partials')
                _native.check(lib.ss_aggr_hub_finish(_ptr(s.hub_rows), _ptr(s.hub_chunk), s.n_hubs, s.n_chunks, n, _ptr(ws), ws_bytes, Fp, _ptr(den),
                                                     _ptr(root), _ptr(root_x), _ptr(out), stream), 'ss_aggr_hub_finish')
            return out

        return padded_rows(run, F, x, root_x if root is not None else None)  # (without a root no root row is read, or padded)


class _Aggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, root, graph, mean, target):
        x = x.contiguous()
        ctx.graph, ctx.mean, ctx.target = graph, mean, target
        ctx.has_root = root is not None
        ctx.save_for_backward(*((x, root) if ctx.has_root and root.requires_grad else (root,) if ctx.has_root else ()))
        return graph.product(x, target, mean=mean, root=None if root is None else root.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        graph, g = ctx.graph, grad_out.contiguous()
        saved = ctx.saved_tensors
        root = saved[-1] if ctx.has_root else None
        grad_x = grad_root = None
        if ctx.needs_input_grad[0]:
            # the mean: every gathered row of g is divided by the forward's den of its node, inside the gather (measured against a
            # division pass of its own, profiles/aggr_probe.txt: 4 - 14 % faster; the bits are the same either way)
            den = (graph.target if ctx.target else graph.source).den if ctx.mean else None
            grad_x = graph.product(g, not ctx.target, root=root, root_x=g, gather_den=den)
        if ctx.has_root and ctx.needs_input_grad[1]:
            grad_root = (g * saved[0]).sum().reshape(1)
        return grad_x, grad_root, None, None, None


def aggregate(x, graph, aggr='sum', flow='target', root=None):
    """The unnormalised neighbour aggregation of node features x (fp32 [N, F] on the graph's device), differentiable in x and root.
    flow='target': out[col_e] += w_e * x[row_e] (PyG's default flow); flow='source': out[row_e] += w_e * x[col_e].  aggr='sum' or
    'mean' (the sum divided by the node's den: the count of its entries for unit weights, 1 for a node without entries).
    root: None, or a float32 device tensor [1] r read on the device: out_i += r * x_i (GINConv: 1 + eps).  The backward with respect
    to x is the other flow of grad_out (mean: of grad_out / den), with the same root term applied to grad_out; with respect to
    root it is (grad_out * x).sum()."""
    if flow not in ('target', 'source'):
        raise ValueError(f"flow must be 'target' or 'source', got {flow!r}")
    if aggr not in ('sum', 'add', 'mean'):
        raise ValueError(f"aggr must be 'sum' (or 'add') or 'mean', got {aggr!r}")
    if not isinstance(graph, AggrGraph):
        raise ValueError('graph must be an AggrGraph')
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.size(0) != graph.num_nodes:
        raise ValueError(f'x must be a float32 tensor [{graph.num_nodes}, F]')
    if x.device != graph.device:
        raise ValueError(f'x is on {x.device}, the graph on {graph.device}: there is no CPU fallback and no silent copy')
    if root is not None:
        if not isinstance(root, torch.Tensor) or root.dtype != torch.float32 or root.shape != (1,):
            raise ValueError('root must be None or a float32 tensor [1]')
        if root.device != graph.device:
            raise ValueError(f'root is on {root.device}, the graph on {graph.device}: it is read on the device')
    return _Aggregate.apply(x, root, graph, aggr == 'mean', flow == 'target')


# the plan of the edge_index tensor seen last, shared by the layers of this module (gcn.py keeps its own: a GCNGraph and an AggrGraph
# of one tensor are different plans)
_CACHE = _PlanCache()


def _graph_of(layer, x, edge_index, edge_weight):
    """the plan a layer's forward runs on: an AggrGraph as it is, a subgraph batch through from_subgraphs, a tensor through the cache"""
    if isinstance(x, (tuple, list)):
        raise NotImplementedError(f'{layer}: bipartite inputs (a tuple x) are not built here')
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError('x must be a float32 tensor [N, in_channels]')
    if isinstance(edge_index, AggrGraph):
        if edge_weight is not None:
            raise ValueError('an AggrGraph carries its own weights')
        return edge_index
    if edge_weight is not None:
        raise NotImplementedError(f"{layer}: PyG's layer takes no edge_weight; multiplicities come in through an AggrGraph")
    if hasattr(edge_index, 'adj_ptr') and hasattr(edge_index, 'edge_index'):  # an ExactSubgraphs / SampledSubgraphs batch
        return AggrGraph.from_subgraphs(edge_index)
    device = x.device if x.is_cuda else None
    return _CACHE.get((x.size(0), device), (edge_index,), lambda: AggrGraph(x.size(0), edge_index, device=device))


class SAGEConv(torch.nn.Module):
    """torch_geometric.nn.SAGEConv [PyG semantics restated]: out = lin_l(aggregate(x)) + lin_r(x), the aggregation BEFORE lin_l.
    Parameters are `lin_l.weight` [out, in], `lin_l.bias` [out] (with bias) and, with root_weight, `lin_r.weight` [out, in] (no
    bias), initialised as torch.nn.Linear does, so a checkpoint written with PyG's layer loads.  aggr: 'mean', 'sum' or 'add';
    normalize=True applies F.normalize(out, p=2, dim=-1).  'max', 'lstm', project=True and bipartite inputs are not built."""

    def __init__(self, in_channels, out_channels, aggr='mean', normalize=False, root_weight=True, project=False, bias=True, **kwargs):
        super().__init__()
        if isinstance(in_channels, (tuple, list)):
            raise NotImplementedError('SAGEConv(in_channels=(a, b)): bipartite inputs are not built here')
        if aggr not in ('mean', 'sum', 'add'):
            raise NotImplementedError(f"SAGEConv(aggr={aggr!r}) is not built here: only 'mean', 'sum' and 'add'")
        if project:
            raise NotImplementedError('SAGEConv(project=True) is not built here')
        flow = kwargs.pop('flow', 'source_to_target')
        if flow != 'source_to_target':
            raise NotImplementedError(f"SAGEConv(flow={flow!r}) is not built here: only flow='source_to_target'")
        if kwargs:
            raise TypeError(f'SAGEConv got unexpected keywords {sorted(kwargs)}')
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.aggr, self.normalize, self.root_weight = 'sum' if aggr == 'add' else aggr, bool(normalize), bool(root_weight)
        self.lin_l = torch.nn.Linear(self.in_channels, self.out_channels, bias=bool(bias))
        if self.root_weight:
            self.lin_r = torch.nn.Linear(self.in_channels, self.out_channels, bias=False)

    def reset_parameters(self):
        self.lin_l.reset_parameters()
        if self.root_weight:
            self.lin_r.reset_parameters()

    def forward(self, x, edge_index, edge_weight=None):
        """edge_index: an AggrGraph (never rebuilt), an ExactSubgraphs / SampledSubgraphs batch (its plan is built from it), or an
        int64 tensor [2, E] whose plan the module-level cache keeps while the SAME tensor object comes back unedited"""
        graph = _graph_of('SAGEConv', x, edge_index, edge_weight)
        out = self.lin_l(aggregate(x, graph, self.aggr))
        if self.root_weight:
            out = out + self.lin_r(x)
        return torch.nn.functional.normalize(out, p=2.0, dim=-1) if self.normalize else out

    def __repr__(self):
        return f'{self.__class__.__name__}({self.in_channels}, {self.out_channels}, aggr={self.aggr})'


class GINConv(torch.nn.Module):
    """torch_geometric.nn.GINConv [PyG semantics restated]: out = nn(sum_j x_j + (1 + eps) * x_i).  `eps` is a buffer [1], or a
    Parameter with train_eps; it is read on the device (no host read), and its gradient is that of the root term.  State-dict keys:
    `nn.*` and `eps`."""

    def __init__(self, nn, eps=0., train_eps=False, **kwargs):
        super().__init__()
        aggr, flow = kwargs.pop('aggr', 'add'), kwargs.pop('flow', 'source_to_target')
        if aggr not in ('add', 'sum') or flow != 'source_to_target':
            raise NotImplementedError(f"GINConv(aggr={aggr!r}, flow={flow!r}) is not built here: only aggr='add', flow='source_to_target'")
        if kwargs:
            raise TypeError(f'GINConv got unexpected keywords {sorted(kwargs)}')
        self.nn = nn
        self.initial_eps = float(eps)
        if train_eps:
            self.eps = torch.nn.Parameter(torch.empty(1))
        else:
            self.register_buffer('eps', torch.empty(1))
        self.reset_parameters()

    def reset_parameters(self):
        for m in self.nn.modules():  # PyG's reset(nn): every layer that can reset itself
            if m is not self.nn and hasattr(m, 'reset_parameters'):
                m.reset_parameters()
        if hasattr(self.nn, 'reset_parameters'):
            self.nn.reset_parameters()
        with torch.no_grad():
            self.eps.fill_(self.initial_eps)

    def forward(self, x, edge_index, edge_weight=None):
        """edge_index: as for SAGEConv.forward"""
        graph = _graph_of('GINConv', x, edge_index, edge_weight)
        return self.nn(aggregate(x, graph, 'sum', root=1.0 + self.eps))

    def __repr__(self):
        return f'{self.__class__.__name__}(nn={self.nn})'
