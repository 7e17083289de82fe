"""ctypes binding of the C-ABI library (include/subgraph_sketch.h).

The HIP library is the product: there is no CPU fallback.  `lib()` raises loudly when the shared
object has not been built (run `python __graft_entry__.py` or `subgraph-sketching_amd/csrc/build.sh`).
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SS_LIB: measurement hook -- tools/ab_variant.sh loads a scratch build of the library beside the product's)
LIB_PATH = os.environ.get('SS_LIB') or os.path.join(_HERE, 'libsubgraph_sketch.so')

SS_MAX_HOPS = 3
SS_MAX_TABLE = 512
SS_FLAG_USE_ZERO_ONE = 1
SS_FLAG_FLOOR_SF = 2
SS_FLAG_MASK_TARGET = 4  # ss_exact_pairs / ss_exact_large: balls of the graph without the link's own edge
SS_CSR_ERR_BOUNDS, SS_CSR_ERR_PROTOCOL = 1, 2  # bits of a CSR build's err_flag


class HllParams(ctypes.Structure):
    """mirror of `struct ss_hll_params`"""
    _fields_ = [('p', c_int32), ('n_tbl', c_int32), ('alpha_mm', c_float), ('threshold', c_float),
                ('lc_min_zeros', c_int32), ('reserved', c_int32),
                ('raw_est', c_void_p), ('bias', c_void_p), ('lc_table', c_void_p)]


class CsrGraphStruct(ctypes.Structure):
    """mirror of `struct ss_csr_graph`"""
    _fields_ = [('rowptr', c_void_p), ('col', c_void_p), ('num_nodes', c_int64), ('n_self_loops', c_int64),
                ('n_self_loops_dev', c_void_p), ('hub_threshold', c_int32), ('reserved', c_int32),
                ('hub_rows', c_void_p), ('hub_count', c_void_p), ('mega_rows', c_void_p), ('mega_count', c_void_p),
                ('mega_scratch', c_void_p), ('row_begin', c_int64), ('row_end', c_int64),
                ('n_mirrors', c_int32), ('reserved2', c_int32), ('mirror_mh', c_void_p * 7), ('mirror_hll', c_void_p * 7),
                ('mirror_cards', c_void_p * 7), ('hub_report', c_void_p), ('report_hub_count', c_void_p), ('report_mega_count', c_void_p),
                ('symmetric_dev', c_void_p)]
    # (`reserved` is the flags word: GRAPH_HOP_TABLES below)


GRAPH_HOP_TABLES = 1  # SS_GRAPH_HOP_TABLES of include/subgraph_sketch.h


class PprGraphStruct(ctypes.Structure):
    """mirror of `struct ss_ppr_graph`"""
    _fields_ = [('rowptr', c_void_p), ('col', c_void_p), ('w', c_void_p), ('z', c_void_p), ('num_nodes', c_int64), ('nnz', c_int64),
                ('hub_rows', c_void_p), ('hub_seg', c_void_p), ('seg_hub', c_void_p), ('n_hubs', c_int64), ('n_segments', c_int64)]


class StructureHeadStruct(ctypes.Structure):
    """mirror of `struct ss_structure_head`"""
    _fields_ = [('dim', c_int32), ('normalised', c_int32), ('w1', c_void_p), ('shift', c_void_p), ('w2', c_void_p), ('bias', c_float)]


PPR_SEGMENT, PPR_MAX_COLUMNS = 256, 4096  # SS_PPR_SEGMENT / SS_PPR_MAX_COLUMNS of include/subgraph_sketch.h
ABI_VERSION = 129  # ss_version() of the library this module's struct mirrors and signatures describe
PROF_MINHASH_HOP, PROF_HLL_HOP, PROF_FIRST_HOP_MH, PROF_FIRST_HOP_HLL, PROF_PAIRS, PROF_CSR, PROF_HUB, PROF_FUSED, PROF_MINHASH_ROWS = range(9)  # SS_PROF_* tags
MEGA_DESC_WORDS = 8  # SS_MEGA_DESC_WORDS
NEG_MODES = {'uniform': 0, 'same_source': 1, 'wedge': 2}  # SS_NEG_*
NEG_MAX_TRIES = 64  # SS_NEG_MAX_TRIES
SUBGRAPH_LABELS = {'drnl': 0, 'de': 1, 'de+': 2}  # SS_SUBGRAPH_LABEL_*: the labels ss_subgraph_labels computes
SUBGRAPH_MAX_DIST = 1 << 20  # SS_SUBGRAPH_MAX_DIST
COMPONENTS_CHUNK = 2048  # SS_COMPONENTS_CHUNK: items per workgroup of the count / fill passes of ss_components_* / ss_induced_*
WEDGE_MAX_SLOTS, WEDGE_MAX_SLICES = 4096, 64  # SS_WEDGE_MAX_SLOTS; the slices ss_wedge_emit takes at most
MEGA_SLICE, MEGA_SLOT_BYTES, CSR_FINGERPRINT_BYTES, MAX_MIRRORS = 1024, 1280, 8448, 7  # SS_MEGA_SLICE / SS_MEGA_SLOT_BYTES of include/subgraph_sketch.h


# name -> (restype, argtypes); must list every symbol declared in include/subgraph_sketch.h and include/subgraph_sketch_debug.h
SIGNATURES = {
    'ss_version': (c_int32, []),
    'ss_error_string': (c_char_p, [c_int32]),
    'ss_minhash_init': (c_int32, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int32, c_void_p]),
    'ss_hll_init': (c_int32, [c_void_p, c_int64, c_int64, c_int32, c_void_p]),
    'ss_csr_workspace_bytes': (c_size_t, [c_int64, c_int64]),
    'ss_csr_build': (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ss_csr_build_cached': (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    'ss_csr_build_symmetric': (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    'ss_propagate': (c_int32, [POINTER(CsrGraphStruct), c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                               c_int32, c_void_p, c_int64, POINTER(HllParams), c_void_p]),
    'ss_minhash_hop_rows': (c_int32, [POINTER(CsrGraphStruct), c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_void_p]),
    'ss_first_hop': (c_int32, [POINTER(CsrGraphStruct), c_void_p, c_void_p, c_int32, c_void_p, c_int32,
                               c_void_p, c_void_p, c_int64, POINTER(HllParams), c_void_p]),
    'ss_fused_hop_stage': (c_int32, [POINTER(CsrGraphStruct), c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_int64, POINTER(HllParams), c_void_p]),
    'ss_hll_count': (c_int32, [c_void_p, c_int64, POINTER(HllParams), c_void_p, c_int64, c_void_p]),
    'ss_estimate_bias': (c_int32, [c_void_p, c_int64, POINTER(HllParams), c_void_p, c_int32, c_void_p]),
    'ss_pair_features': (c_int32, [c_void_p, c_int64, c_int64, c_int32, POINTER(c_void_p), c_int32, POINTER(c_void_p),
                                   c_void_p, c_int64, POINTER(HllParams), c_uint32, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p]),
    'ss_pair_features_normalised': (c_int32, [c_void_p, c_int64, c_int64, c_int32, POINTER(c_void_p), c_int32,
                                              POINTER(c_void_p), c_void_p, c_int64, POINTER(HllParams), c_uint32, c_void_p,
                                              c_void_p, c_void_p, c_void_p]),
    'ss_group_links_by_source': (c_int32, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ss_gather_links': (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    'ss_scatter_feature_rows': (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    'ss_pair_features_grouped': (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_int32, POINTER(c_void_p), c_int32, POINTER(c_void_p),
                                           c_void_p, c_int64, POINTER(HllParams), c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ss_pair_features_grouped_kernel': (c_int32, [c_int32, c_void_p, c_void_p, c_int64, c_int64, c_int32, POINTER(c_void_p), c_int32,
                                                  POINTER(c_void_p), c_void_p, c_int64, POINTER(HllParams), c_uint32, c_void_p, c_void_p,
                                                  c_void_p, c_void_p]),
    'ss_pair_scores': (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_int32, POINTER(c_void_p), c_int32, POINTER(c_void_p), c_void_p,
                                 c_int64, POINTER(HllParams), c_uint32, c_void_p, POINTER(StructureHeadStruct), c_void_p, c_void_p, c_void_p]),
    'ss_common_neighbour_scores': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                             c_void_p]),
    'ss_common_neighbour_scores_f32': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                                 c_void_p, c_void_p]),
    'ss_ppr_workspace_bytes': (c_size_t, [c_int64, c_int32, c_int64, c_int64]),
    'ss_ppr_begin': (c_int32, [POINTER(PprGraphStruct), c_void_p, c_int32, c_double, c_void_p, c_size_t, c_void_p, c_void_p]),
    'ss_ppr_iterate': (c_int32, [POINTER(PprGraphStruct), c_int32, c_int32, c_int32, c_double, c_void_p, c_size_t, c_void_p]),
    'ss_ppr_status': (c_int32, [POINTER(PprGraphStruct), c_int32, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    'ss_ppr_scores': (c_int32, [POINTER(PprGraphStruct), c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_size_t, c_void_p, c_void_p,
                                c_void_p]),
    'ss_ppr_vectors': (c_int32, [POINTER(PprGraphStruct), c_int32, c_void_p, c_size_t, c_void_p, c_void_p]),
    'ss_topk_workspace_bytes': (c_size_t, [c_int64, c_int32]),
    'ss_topk_scan': (c_int32, [c_void_p, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, POINTER(HllParams), c_void_p,
                               c_size_t, c_void_p, c_void_p]),
    'ss_topk_exclude': (c_int32, [c_void_p, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ss_topk_score_scan': (c_int32, [c_void_p, c_int32, c_int64, c_int32, POINTER(c_void_p), POINTER(c_void_p), c_int32, c_void_p, c_int64,
                                     POINTER(HllParams), c_uint32, c_void_p, POINTER(StructureHeadStruct), c_void_p, c_size_t, c_void_p,
                                     c_void_p]),
    'ss_rank_score_scan': (c_int32, [c_void_p, c_void_p, c_int32, c_int64, c_int32, POINTER(c_void_p), POINTER(c_void_p), c_int32, c_void_p,
                                     c_int64, POINTER(HllParams), c_uint32, c_void_p, POINTER(StructureHeadStruct), c_void_p, c_void_p,
                                     c_void_p]),
    'ss_lsh_band_keys': (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    'ss_lsh_count': (c_int32, [c_void_p, c_int32, c_int64, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                               c_void_p, c_void_p, c_void_p]),
    'ss_lsh_fill': (c_int32, [c_void_p, c_int32, c_int64, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                              c_void_p, c_void_p, c_void_p]),
    'ss_sample_negatives': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_int32, c_uint64,
                                      c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ss_wedge_walks': (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    'ss_wedge_fold': (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    'ss_wedge_emit': (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    'ss_exact_workspace_bytes': (c_size_t, [c_int64]),
    'ss_exact_slot_bytes': (c_size_t, [c_int64]),
    'ss_exact_pairs': (c_int32, [POINTER(CsrGraphStruct), c_void_p, c_int64, c_int64, c_int32, c_uint32, c_int32, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ss_exact_large': (c_int32, [POINTER(CsrGraphStruct), c_void_p, c_int64, c_int64, c_int32, c_uint32, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_size_t, c_int32, c_void_p, c_size_t, c_void_p]),
    'ss_exact_nodes_pairs': (c_int32, [POINTER(CsrGraphStruct), c_void_p, c_int64, c_int64, c_int32, c_uint32, c_int32, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ss_exact_nodes_large': (c_int32, [POINTER(CsrGraphStruct), c_void_p, c_int64, c_int64, c_int32, c_uint32, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_size_t, c_int32, c_void_p, c_size_t, c_void_p]),
    'ss_sampled_nodes_pairs': (c_int32, [POINTER(CsrGraphStruct), c_void_p, c_int64, c_int64, c_int32, c_int32, c_double, c_uint64, c_int32,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ss_sampled_nodes_large': (c_int32, [POINTER(CsrGraphStruct), c_void_p, c_int64, c_int64, c_int32, c_int32, c_double, c_uint64, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int32, c_void_p, c_size_t, c_void_p]),
    'ss_subgraph_adj': (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_uint32, c_int32, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ss_subgraph_labels': (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_void_p, c_void_p, c_void_p,
                                     c_void_p]),
    'ss_components_labels': (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ss_components_sizes': (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    'ss_components_roots': (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ss_components_same': (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    'ss_induced_select': (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ss_induced_mapper': (c_int32, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ss_induced_edges': (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    'ss_update_workspace_bytes': (c_size_t, [c_int64, c_int32]),
    'ss_update_mark': (c_int32, [POINTER(CsrGraphStruct), c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_void_p,
                                 c_size_t, c_void_p]),
    'ss_update_hop': (c_int32, [POINTER(CsrGraphStruct), c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                c_int32, c_void_p, c_int64, POINTER(HllParams), c_void_p, c_size_t, c_void_p]),
    'ss_masked_workspace_bytes': (c_size_t, [c_int64]),
    'ss_masked_pair_features': (c_int32, [POINTER(CsrGraphStruct), c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p, POINTER(c_void_p),
                                          c_int32, POINTER(c_void_p), c_void_p, c_int64, POINTER(HllParams), c_uint32, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ss_spmm_csr': (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_void_p]),
    'ss_csr_group_ids': (c_int32, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ss_csr_sort_workspace_bytes': (c_size_t, [c_int64]),
    'ss_csr_sort_rows': (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ss_gcn_scan_bytes': (c_size_t, [c_int64]),
    'ss_gcn_scan_edges': (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    'ss_gcn_degree': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ss_sign_spmm': (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_void_p]),
    'ss_csr_protocol_faults': (c_int32, []),
    'ss_table_digest': (c_int32, [c_void_p, c_int64, c_void_p, c_void_p]),
    'ss_pack_minhash': (c_int32, [c_void_p, c_void_p, c_int64, c_void_p]),
    'ss_unpack_minhash': (c_int32, [c_void_p, c_void_p, c_int64, c_void_p]),
    'ss_profile_enable': (c_int32, [c_uint32]),
    'ss_profile_sample': (c_int32, [c_int32]),
    'ss_debug_hub_calls': (c_int64, [c_int32]),
    'ss_debug_csr_helpers': (c_int32, [c_void_p]),
    'ss_debug_csr_protocol_faults': (c_int32, []),
    'ss_profile_read': (c_int32, [c_int32, POINTER(c_float), POINTER(c_int32)]),
    'ss_time_propagate': (c_int32, [POINTER(CsrGraphStruct), c_void_p, c_void_p, c_int32, c_void_p,
                                    c_void_p, c_int32, c_void_p, c_int64, POINTER(HllParams), c_void_p, c_int32,
                                    POINTER(c_float)]),
    'ss_time_pair_features': (c_int32, [c_void_p, c_int64, c_int64, c_int32, POINTER(c_void_p), c_int32,
                                        POINTER(c_void_p), c_void_p, c_int64, POINTER(HllParams), c_uint32, c_void_p,
                                        c_void_p, c_int32, POINTER(c_float)]),
}

_lib = None


class NativeLibraryMissing(RuntimeError):
    pass


def lib():
    """load (once) and return the ctypes handle; raises NativeLibraryMissing if it was never built"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryMissing(
                f'{LIB_PATH} not found: the HIP engine is not built. Run `python __graft_entry__.py` '
                f'(or subgraph-sketching_amd/csrc/build.sh). There is no CPU fallback.')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        if handle.ss_version() != ABI_VERSION:  # a stale in-tree build with another struct layout would corrupt launches
            raise NativeLibraryMissing(f'{LIB_PATH} is version {handle.ss_version()}, this package needs {ABI_VERSION}: '
                                       f'rebuild with `python __graft_entry__.py`')
        _lib = handle
    return _lib


def check(code, what):
    if code != 0:
        msg = lib().ss_error_string(code).decode()
        raise RuntimeError(f'{what} failed: {msg} ({code})')
