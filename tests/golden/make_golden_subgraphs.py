#!/usr/bin/env python
"""Generate tests/golden/g17_seal_labels.npz by IMPORTING the modelled project's src/labelling_tricks.py (torch, numpy, scipy only).

    python tests/golden/make_golden_subgraphs.py --reference <checkout of the modelled project>

G17: drnl_node_labeling / de_node_labeling / de_plus_node_labeling of the reference on the enclosing subgraphs of BA-40 links, h = 1, 2, 3,
max_dist = 1, 3, 1000.  The subgraph handed to the reference is the restated local adjacency (tests/subgraph_restatement.py) reordered so
that the roots sit at 0 and 1, as SEAL's k_hop_subgraph orders them; the labels are mapped back to the row's id order.  Links: those of
the node-list fixture (test_exact_nodes_host._ba40) without the u == v ones (outside the reference's domain), unmasked and masked, plus
every edge of the graph as a masked positive.  The file holds links, parameters, ids and labels only."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import scipy.sparse as ssp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import subgraph_restatement as sr  # noqa: E402
from test_exact_nodes_host import _ba40  # noqa: E402

HOPS, MAX_DISTS = (1, 2, 3), (1, 3, 1000)
LABELS = {'drnl': 'drnl_node_labeling', 'de': 'de_node_labeling', 'deplus': 'de_plus_node_labeling'}


def reference_labels(fn, ptr, nbr, weight, ru, rv, max_dist):
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(ptr))
    adj = ssp.csr_matrix((weight.astype(np.float64), (rows, nbr)), shape=(n, n))
    perm = np.array([ru, rv] + [i for i in range(n) if i not in (ru, rv)])
    z = fn(adj[perm, :][:, perm], 0, 1, max_dist).numpy()
    back = np.empty_like(z)
    back[perm] = z
    return back


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the modelled project (its src/labelling_tricks.py is imported)')
    ap.add_argument('--out', default=os.path.join(HERE, 'g17_seal_labels.npz'))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location('labelling_tricks', os.path.join(args.reference, 'src', 'labelling_tricks.py'))
    lt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lt)
    n, ei, fixture = _ba40()
    fixture = np.where(fixture < 0, fixture + n, fixture)
    fixture = fixture[fixture[:, 0] != fixture[:, 1]]
    out = {'hops': np.array(HOPS), 'max_dists': np.array(MAX_DISTS)}
    calls = 0
    for mask in (False, True):
        links = np.concatenate([fixture, ei.T]) if mask else fixture
        out[f'links_m{int(mask)}'] = links
        for h in HOPS:
            sub = sr.restate(n, ei, links, h, mask_target=mask)
            key = f'h{h}_m{int(mask)}'
            out[key + '_rowptr'], out[key + '_ids'] = sub.rowptr, sub.ids.astype(np.int32)
            for md in MAX_DISTS:
                for name, fn in LABELS.items():
                    z = []
                    for q in range(len(links)):
                        _, ptr, nbr, weight = sub.row(q)
                        z.append(reference_labels(getattr(lt, fn), ptr, nbr, weight, int(sub.roots[q, 0]), int(sub.roots[q, 1]), md))
                        calls += 1
                    out[f'{key}_d{md}_{name}'] = np.concatenate(z).astype(np.int32)
    np.savez_compressed(args.out, **out)
    print(f'{args.out}: {calls} reference calls, {os.path.getsize(args.out)} bytes')


if __name__ == '__main__':
    main()
