"""subgraph-sketching_amd -- MI355X (gfx950) engine for the ELPH/BUDDY subgraph-sketching hot path.

Import name: `subgraph_sketching_amd` (see /subgraph_sketching_amd.py; the directory keeps the project's
hyphenated name).  Public surface = the reference's src/hashing.py surface.
"""
from .hashing import (LABEL_LOOKUP, ElphHashes, HllPropagation, HopSketch, MinhashPropagation, SketchTable,
                      build_csr, load_sketches, pack_minhash, save_sketches, unpack_minhash)
from .feature_store import DeviceFeatureStore
from .head import StructureHead
from .negatives import NegativeSampler, sample_negatives
from .wedge import WedgeGraph
from .subgraphs import ExactSubgraphs
from .components import Components, InducedSubgraph, connected_components, induced_subgraph, largest_component_subgraph
from .gcn import GCNConv, GCNGraph, gcn_propagate
from .aggr import AggrGraph, GINConv, SAGEConv, aggregate
from .link_decoder import LinkBatch, link_gather, link_hadamard
from .cn_pool import CommonNeighbourBatch, common_neighbour_pool
from .graph_prep import CoalescedGraph, coalesce, coalesce_graph, is_undirected, to_undirected
from .pooling import center_pool, global_add_pool, global_mean_pool, global_sort_pool, sort_pool_k
from . import _native, hll_tables, knobs, dist, heuristics, sign, roofline, lsh, negatives, wedge, subgraphs, components, gcn, pooling, aggr, link_decoder, graph_prep, cn_pool

__all__ = ['cn_pool', 'CommonNeighbourBatch', 'common_neighbour_pool', 'graph_prep', 'CoalescedGraph', 'coalesce', 'coalesce_graph', 'is_undirected', 'to_undirected', 'link_decoder', 'LinkBatch', 'link_gather', 'link_hadamard', 'aggr', 'AggrGraph', 'aggregate', 'SAGEConv', 'GINConv', 'pooling', 'global_sort_pool', 'global_add_pool', 'global_mean_pool', 'center_pool', 'sort_pool_k', 'gcn', 'GCNConv', 'GCNGraph', 'gcn_propagate', 'components', 'Components', 'InducedSubgraph', 'connected_components', 'induced_subgraph', 'largest_component_subgraph','LABEL_LOOKUP', 'ElphHashes', 'HllPropagation', 'MinhashPropagation', 'SketchTable', 'HopSketch',
           'build_csr', 'DeviceFeatureStore', 'StructureHead', 'pack_minhash', 'unpack_minhash', 'save_sketches', 'load_sketches', 'hll_tables', 'knobs', 'dist', 'heuristics', 'sign', 'roofline', 'lsh', 'negatives', 'NegativeSampler', 'sample_negatives', 'wedge', 'WedgeGraph', 'subgraphs', 'ExactSubgraphs']
