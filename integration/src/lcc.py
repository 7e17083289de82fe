"""Drop-in `src/lcc.py` for a melifluos/subgraph-sketching checkout: the reference's four function names on the MI355X engine.

Copy this file over `<reference checkout>/src/lcc.py`.  Its import site keeps working unchanged:
    from src.lcc import get_largest_connected_component, remap_edges, get_node_mapper      (src/data.py:26)
and INTEGRATION.md shows a body for data.use_lcc that needs none of them.  The engine is located as integration/src/hashing.py locates
it: an importable `subgraph_sketching_amd`, the environment variable SUBGRAPH_SKETCH_AMD_ROOT, or this file's own place in the engine's
repository.  Nothing of PyG is imported: `dataset` is anything with dataset.data.x.shape[0] and dataset.data.edge_index.

What differs from the original (subgraph_sketching_amd/components.py says why):
  * get_largest_connected_component returns the node ids ASCENDING (the original: in the iteration order of a Python set);
  * get_component treats every edge as undirected (the original follows out-edges only; the same on a symmetric edge_index);
  * both run on the device: seconds of kernel time where the original needs O(N E) interpreter steps.
"""
import importlib
import os
import sys

import numpy as np


def _load_engine():
    try:
        return importlib.import_module('subgraph_sketching_amd')
    except ImportError:
        pass
    here = os.path.dirname(os.path.abspath(__file__))
    for root in (os.environ.get('SUBGRAPH_SKETCH_AMD_ROOT'), os.path.dirname(os.path.dirname(here))):
        if root and os.path.exists(os.path.join(root, 'subgraph_sketching_amd.py')):
            if root not in sys.path:
                sys.path.insert(0, root)
            return importlib.import_module('subgraph_sketching_amd')
    raise ImportError('subgraph_sketching_amd not found: install it, or set SUBGRAPH_SKETCH_AMD_ROOT to the engine repository '
                      '(and build it once with `python __graft_entry__.py`)')


_engine = _load_engine()


def _graph(dataset):
    return int(dataset.data.x.shape[0]), dataset.data.edge_index


def get_largest_connected_component(dataset) -> np.ndarray:
    """the node ids of the largest connected component, ascending; among equally large ones the one holding the smallest node id"""
    num_nodes, edge_index = _graph(dataset)
    return _engine.connected_components(num_nodes, edge_index).largest().cpu().numpy()


def get_node_mapper(lcc: np.ndarray) -> dict:
    """old id -> new id: the position in `lcc`"""
    return {int(node): new_id for new_id, node in enumerate(np.asarray(lcc).tolist())}


def remap_edges(edges: list, mapper: dict) -> list:
    """[[row ...], [col ...]] of the (i, j) pairs in `edges`, in new ids"""
    return [[mapper[int(i)] for i, _ in edges], [mapper[int(j)] for _, j in edges]]


def get_component(dataset, start: int = 0) -> set:
    """the nodes connected to `start`"""
    num_nodes, edge_index = _graph(dataset)
    labels = _engine.connected_components(num_nodes, edge_index).labels
    return set((labels == labels[start]).nonzero().flatten().tolist())
