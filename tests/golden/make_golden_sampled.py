#!/usr/bin/env python
"""Generate tests/golden/g18_seal_khop.npz by IMPORTING the modelled project's src/datasets/seal.py and calling its k_hop_subgraph.

    python tests/golden/make_golden_sampled.py --reference <checkout of the modelled project>

G18: what k_hop_subgraph(src, dst, h, A, sample_ratio=1.0, max_nodes_per_hop=None) returns on the BA-40 graph for the links of
g3_g4_ba40.npz, h = 1, 2, 3: the node list and `dists`, stored per link ascending by id and once each (for src == dst the reference lists
the root twice).  With sampling off the walk is deterministic, so this pins the WALK of tests/sampled_subgraph_restatement.py -- the joint
fringe, `visited`, the hop a node joins at -- to the reference's own; the sampling law is tested on its own.

seal.py is imported unmodified; the packages it imports at module level that the walk never touches (torch_geometric, torch_sparse) are
replaced by empty `sys.modules` stand-ins, as make_golden.py does for hashing.py.  The file holds links, ids and hops only."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import scipy.sparse as ssp

HERE = os.path.dirname(os.path.abspath(__file__))
HOPS = (1, 2, 3)


class _Anything(object):
    """a base class / a callable for names that seal.py binds at import and the walk never uses"""

    def __init__(self, *a, **k):
        pass


def install_stand_ins():
    names = {'torch_geometric': (), 'torch_geometric.data': ('Data', 'Dataset', 'InMemoryDataset'),
             'torch_geometric.utils': ('negative_sampling', 'add_self_loops', 'to_undirected'), 'torch_sparse': ('coalesce',)}
    for name, attrs in names.items():
        mod = types.ModuleType(name)
        for a in attrs:
            setattr(mod, a, _Anything)
        sys.modules[name] = mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the modelled project (its src/datasets/seal.py is imported)')
    ap.add_argument('--out', default=os.path.join(HERE, 'g18_seal_khop.npz'))
    args = ap.parse_args()
    install_stand_ins()
    sys.path.insert(0, args.reference)
    seal = importlib.import_module('src.datasets.seal')
    g = np.load(os.path.join(HERE, 'g3_g4_ba40.npz'))
    n, ei, links = int(g['num_nodes']), np.asarray(g['edge_index'], dtype=np.int64), np.asarray(g['links'], dtype=np.int64)
    A = ssp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n))
    out = {'hops': np.array(HOPS), 'links': links}
    calls = 0
    for h in HOPS:
        rowptr, ids, hops = [0], [], []
        for u, v in links.tolist():
            nodes, _, dists, _, _ = seal.k_hop_subgraph(u, v, h, A, sample_ratio=1.0, max_nodes_per_hop=None)
            calls += 1
            hop_of = {}
            for x, d in zip(nodes, dists):
                assert hop_of.setdefault(int(x), int(d)) == int(d)
            row = sorted(hop_of)
            ids += row
            hops += [hop_of[x] for x in row]
            rowptr.append(len(ids))
        out[f'h{h}_rowptr'], out[f'h{h}_ids'], out[f'h{h}_hop'] = np.array(rowptr, np.int64), np.array(ids, np.int32), np.array(hops, np.uint8)
    np.savez_compressed(args.out, **out)
    print(f'{args.out}: {calls} reference calls, {os.path.getsize(args.out)} bytes')


if __name__ == '__main__':
    main()
