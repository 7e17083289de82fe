#!/usr/bin/env python
"""Generate tests/golden/g19_lcc.npz by IMPORTING the modelled project's src/lcc.py and calling its get_largest_connected_component.

    python tests/golden/make_golden_lcc.py --reference <checkout of the modelled project>

G19: seven symmetric graphs of 12 to 300 nodes -- six of `undirected` random pairs drawn by numpy's default_rng(seed) and listed in both
directions (one of them has no edge at all), and the BA-40 graph of g3_g4_ba40.npz, which is connected.  For each: the edge_index, the
reference's largest component SORTED (the reference returns it in the iteration order of a Python set, which is not ascending), and the
number of components that share the largest size, counted from the reference's own get_component.  The reference is O(N E): N <= 300.

lcc.py is imported unmodified; torch_geometric, which it imports for two type annotations, is replaced by empty `sys.modules` stand-ins,
as make_golden_sampled.py does for seal.py, and the dataset is a SimpleNamespace.  The file holds arrays only."""
import argparse
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RANDOM = ((40, 12, 1), (40, 12, 2), (12, 0, 6), (64, 20, 3), (200, 60, 4), (300, 400, 5))  # (N, undirected random edges, seed)


class _Anything(object):
    def __init__(self, *a, **k):
        pass


def install_stand_ins():
    for name, attrs in {'torch_geometric': (), 'torch_geometric.data': ('Data', 'InMemoryDataset')}.items():
        mod = types.ModuleType(name)
        for a in attrs:
            setattr(mod, a, _Anything)
        sys.modules[name] = mod


def dataset_of(n, ei):
    return types.SimpleNamespace(data=types.SimpleNamespace(x=np.zeros((n, 1), dtype=np.float32), edge_index=types.SimpleNamespace(numpy=lambda: ei)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the modelled project (its src/lcc.py is imported)')
    ap.add_argument('--out', default=os.path.join(HERE, 'g19_lcc.npz'))
    args = ap.parse_args()
    install_stand_ins()
    sys.path.insert(0, args.reference)
    sys.path.insert(0, os.path.dirname(HERE))
    lcc = importlib.import_module('src.lcc')
    from components_restatement import symmetric_random_graph
    ba = np.load(os.path.join(HERE, 'g3_g4_ba40.npz'))
    graphs = [(n, symmetric_random_graph(n, m, seed)) for n, m, seed in RANDOM] + [(int(ba['num_nodes']), np.asarray(ba['edge_index'], dtype=np.int64))]
    out = {'num_graphs': np.array(len(graphs))}
    for k, (n, ei) in enumerate(graphs):
        ds = dataset_of(n, ei)
        best = np.sort(np.asarray(lcc.get_largest_connected_component(ds), dtype=np.int64))
        left, sizes = set(range(n)), []
        while left:  # the sizes of all components, by the reference's own walk
            comp = lcc.get_component(ds, min(left))
            sizes.append(len(comp))
            left -= comp
        assert max(sizes) == len(best)
        out[f'g{k}_num_nodes'], out[f'g{k}_edge_index'], out[f'g{k}_lcc'] = np.array(n), ei, best
        out[f'g{k}_tied'] = np.array(sizes.count(max(sizes)))
        print(f'graph {k}: N = {n}, E = {ei.shape[1]}, components = {len(sizes)}, largest = {len(best)} nodes, shared by {sizes.count(max(sizes))}')
    np.savez_compressed(args.out, **out)
    print(f'{args.out}: {os.path.getsize(args.out)} bytes')


if __name__ == '__main__':
    main()
