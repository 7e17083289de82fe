"""ElphHashes: the reference's class (hashing.py:48-323), same constructor, methods, attributes and errors, over the HIP engine."""
from collections import OrderedDict
import logging
import os
import weakref
from ctypes import byref, c_float, c_void_p

import numpy as np
import torch

from . import _native, exact, hll_tables, knobs
from ._runtime import (CsrProtocolFault, raise_csr_protocol_faults, _DeferredErrors, _DeviceParams, _Span, _check_sizes, _compute_device, _error_flag, _ptr, _stream, _take_error,
                       linear_counting_table, logger)
from .containers import (HopSketch, LazyMinhash, SketchTable, _packed_hll_of, _packed_minhash_of, _stamp_tables, _tag, unpack_minhash)
from .csr import _CsrCache, build_csr, group_links_by_source
from .propagation import HllPropagation, MinhashPropagation, _propagate

# reference hashing.py:22-25 -- primary key = max hops, secondary key = feature index, value = (hops from u, hops from v)
LABEL_LOOKUP = {1: {0: (1, 1), 1: (0, 1), 2: (1, 0)},
                2: {0: (1, 1), 1: (2, 1), 2: (1, 2), 3: (2, 2), 4: (0, 1), 5: (1, 0), 6: (0, 2), 7: (2, 0)},
                3: {0: (1, 1), 1: (2, 1), 2: (1, 2), 3: (2, 2), 4: (3, 1), 5: (1, 3), 6: (3, 2), 7: (2, 3), 8: (3, 3),
                    9: (0, 1), 10: (1, 0), 11: (0, 2), 12: (2, 0), 13: (0, 3), 14: (3, 0)}}


# ---- one-vs-all link candidates (ElphHashes.topk_candidates, csrc/ss_topk.hip) -----------------------------------------------------
TOPK_SENTINEL = -(1 << 63)  # the key of an ineligible candidate (v == u, excluded, out-of-range source): below every real key
_TOPK_KEY_BYTES = 1 << 31   # bound on one block's key buffer [sources, N] int64 (rows do not depend on it; not a user knob)
# ---- each link's rank among all nodes (ElphHashes.rank_links, csrc/ss_rank.hip): rows depend on neither constant ------------------------
_RANK_LAUNCH_LINKS = 8 * 65535  # links per ss_rank_score_scan launch: grid.y at the smallest block of staged links
_RANK_EXCLUDE_PAIRS = 1 << 22   # excluded (link, partner) pairs scored and compared at a time (the exclusion correction)


def _decode_topk_keys(keys):
    """(ids int64, scores float32) of ss_topk_scan keys, on keys.device: high word = monotone bits of the score as a signed int32,
    low word = 0xFFFFFFFF - id; the sentinel decodes to (-1, -inf)"""
    hi, lo = keys >> 32, keys & 0xFFFFFFFF
    m = hi + (1 << 31)                                              # the score's monotone bits as an unsigned word
    bits = torch.where(m >= (1 << 31), m - (1 << 31), 0xFFFFFFFF - m)  # its IEEE bits
    bits = bits - ((bits >> 31) << 32)                              # as a signed int32 value
    scores = bits.to(torch.int32).view(torch.float32)
    pad = keys == TOPK_SENTINEL
    return (0xFFFFFFFF - lo).masked_fill(pad, -1), scores.masked_fill(pad, float('-inf'))


def _encode_topk_keys(scores, ids):
    """the key ss_topk_key.hpp forms of (score float32, id int64), in torch (topk_links_lsh ranks scores of ss_pair_scores by it):
    signed int64 order == (score descending, id ascending), -0.0 folded into +0.0; _decode_topk_keys is its inverse"""
    bits = scores.view(torch.int32).to(torch.int64)
    bits = bits.masked_fill(bits == -(1 << 31), 0)
    hi = torch.where(bits >= 0, bits, -(1 << 31) - 1 - bits)
    return (hi << 32) | (0xFFFFFFFF - ids)


def _csr_row_keys(csr, rows, N):
    """sorted unique keys i * N + v over every v in row rows[i] of a CSR (rows: int64 ids in [0, N), duplicates allowed; the CSR's
    rows hold duplicates, unordered), or None when those rows are empty.  One host read (the size of the gather)."""
    deg = csr.rowptr[rows + 1] - csr.rowptr[rows]
    ends = torch.cumsum(deg, 0)
    total = int(ends[-1].item()) if rows.numel() else 0
    if total == 0:
        return None
    e = torch.arange(total, dtype=torch.int64, device=rows.device)
    s = torch.searchsorted(ends, e, right=True)
    v = csr.col[csr.rowptr[rows[s]] + (e - (ends[s] - deg[s]))].to(torch.int64)
    return torch.unique(s * N + v)


def _table_shape(hash_table, hop):
    """(N, P) of a hop's MinHash table without touching a device"""
    entry = hash_table[hop]
    t = entry.mh_u32 if isinstance(entry, HopSketch) else entry['minhash']
    if t.dim() != 2:
        raise ValueError(f'hop {hop} MinHash table must be 2-D, got {tuple(t.shape)}')
    return int(t.shape[0]), int(t.shape[1])


def _table_ptrs(mh, hll):
    """the two pointer arrays (one entry per hop) the link entry points take for packed MinHash / HLL tables"""
    return tuple((c_void_p * len(ts))(*[t.data_ptr() for t in ts]) for ts in (mh, hll))


def _exclude_csr(ex, N, device, strict, err):
    """(CSR with row u = {v : u -> v} of an exclude edge_index or None, negative ids wrapped; the error flag of the launches behind it)"""
    csr = None
    if ex is not None:
        ex = ex.to(device=device, dtype=torch.int64)
        ex = torch.where(ex < 0, ex + N, ex)  # (ids below -N stay negative: out of range)
        csr = build_csr(ex.flip(0), N, device, check=strict, err_flag=None if strict else err)
    return csr, (_error_flag(device) if strict else err)

class ElphHashes(object):
    """class to store hashes and retrieve subgraph features (mirror of reference hashing.py:48-323)"""
    HUB_HINT_SHAPES = 256  # graph shapes that get a hub hint word (one pinned int32 each, kept for the engine's lifetime)

    def __init__(self, args, fuse_hop_stage=None, defer_first_hop=None, defer_table_hop=None):
        """args: the reference's namespace (max_hash_hops, floor_sf, minhash_num_perm, hll_p, use_zero_one).  Extensions (keyword
        only in spirit; None = the engine's defaults): fuse_hop_stage -- hop-1 MinHash + hop-2 HLL in one launch inside
        build_hash_tables; defer_first_hop / defer_table_hop -- the deferred launches of the ELPH call sequence (minhash_prop
        records its hop, the next consumer decides how much of it runs).  The environment variables
        SS_FUSED_STAGE / SS_DEFER_TABLE_HOP only set the defaults (tests, A/B measurements)."""
        assert args.max_hash_hops in {1, 2, 3}, f'hashing is not implemented for {args.max_hash_hops} hops'
        self._defer_first_hop, self._defer_table_hop = defer_first_hop, defer_table_hop
        self.max_hops = args.max_hash_hops
        self.floor_sf = args.floor_sf  # if true set minimum sf to 0
        # minhash params (reference hashing.py:58-63)
        self._mersenne_prime = np.uint64((1 << 61) - 1)
        self._max_minhash = np.uint64((1 << 32) - 1)
        self._minhash_range = (1 << 32)
        self.minhash_seed = 1
        self.num_perm = args.minhash_num_perm
        self._csr_cache = _CsrCache(self._bounds, self._prop_hub_hint)
        self._sorted_rows_cache = None  # exact_subgraphs: the cached CSR's columns with every row sorted (subgraphs._SortedRowsCache)
        self.minhash_prop = MinhashPropagation(self._csr_cache, self._report_after_host_copy, defer_first_hop, defer_table_hop)
        # hll params (reference hashing.py:65-81)
        self.p = args.hll_p
        self.m = 1 << self.p
        self.use_zero_one = args.use_zero_one
        self.label_lookup = LABEL_LOOKUP[self.max_hops]
        self.hll_tables = hll_tables.load(self.p)
        self.hll_hashfunc = None  # datasketch's sha1 hashfunc is never used on the path (reference :71)
        self.alpha = self.hll_tables.alpha
        self.max_rank = self.hll_tables.max_rank
        assert self.max_rank == 64 - self.p, 'not using 64 bits for hll++ hashing'
        self.hll_size = self.m
        self.hll_threshold = self.hll_tables.threshold
        self.bias_vector = torch.tensor(self.hll_tables.bias, dtype=torch.float)
        self.estimate_vector = torch.tensor(self.hll_tables.raw_estimate, dtype=torch.float)
        self.hll_prop = HllPropagation(self._csr_cache, self._params, self.m, self._report_after_host_copy)
        self._dev_params = {}
        self._dev_perms = {}
        self.fuse_first_hop = True  # compute hop 1 straight from node ids when the fused kernel supports (num_perm, p)
        # hop-1 MinHash + hop-2 HLL in one launch (ss_fused_hop_stage; num_perm == 128, hll_p == 8, max_hops >= 2, unsharded build)
        self.fuse_hop_stage = (os.environ.get('SS_FUSED_STAGE', '1') != '0') if fuse_hop_stage is None else bool(fuse_hop_stage)
        # node ids outside [0, num_nodes): 'deferred' (default) = IndexError at the NEXT call into this engine or at
        # check_errors(), no host synchronisation inside a step; True = IndexError from the offending call itself (one
        # synchronising 4-byte read per CSR build / query call); False = never reported (edges dropped, NaN feature rows)
        self.strict_bounds = 'deferred'
        self._deferred = _DeferredErrors()
        # link sets of >= knobs.GROUP_LINKS_MIN pairs: 'auto' = grouped by their first node unless the list already has its runs (one
        # host read per such call), True = always grouped, False = walked as listed (no host read)
        self.group_links = 'auto'
        # skip the hub units of build_hash_tables for shapes whose earlier builds listed no hub rows (see _hub_hint)
        self.hub_hints = os.environ.get('SS_HUB_HINTS', '1') != '0'
        self._hub_words, self._hub_arena = {}, None

    # no device handles in pickled state (SURVEY.md section 8(b) threading row)
    def __getstate__(self):
        state = dict(self.__dict__)
        state['_dev_params'], state['_dev_perms'] = {}, {}
        state['_csr_cache'], state['_deferred'] = None, None
        state['_sorted_rows_cache'] = None
        state['_hub_words'], state['_hub_arena'] = {}, None
        state.pop('_tables_id', None)
        state['minhash_prop'], state['hll_prop'] = None, None
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.__dict__.setdefault('hub_hints', os.environ.get('SS_HUB_HINTS', '1') != '0')
        self.__dict__.setdefault('group_links', 'auto')
        self._hub_words, self._hub_arena = {}, None
        self._deferred = _DeferredErrors()
        self._csr_cache = _CsrCache(self._bounds, self._prop_hub_hint)
        self.minhash_prop = MinhashPropagation(self._csr_cache, self._report_after_host_copy, self.__dict__.get('_defer_first_hop'),
                                               self.__dict__.get('_defer_table_hop'))
        self.hll_prop = HllPropagation(self._csr_cache, self._params, self.m, self._report_after_host_copy)

    def _report_after_host_copy(self):
        """a result has just been copied to a CPU caller (ELPH on CPU tensors): the launches behind it are complete, so a
        deferred bounds report is final -- raise it from the offending call, as the reference's CPU indexing would"""
        if self.strict_bounds == 'deferred':
            self._deferred.raise_if_set()

    # ---- host-side helpers -------------------------------------------------------------------------
    @property
    def tables_id(self):
        """identity of the HLL++ tables in use (hll_tables.table_id), recomputed if `hll_tables` is replaced"""
        cached = self.__dict__.get('_tables_id')
        if cached is None or cached[0] is not self.hll_tables:
            cached = (self.hll_tables, hll_tables.table_id(self.hll_tables))
            self.__dict__['_tables_id'] = cached
        return cached[1]

    def _params(self, device):
        key = str(device)
        if key not in self._dev_params:
            _check_sizes(self.num_perm, self.p)
            self._dev_params[key] = _DeviceParams(self.hll_tables, device)
        return self._dev_params[key]

    def _np_bit_length(self, bits):
        """number of bits needed to represent each (non-negative) int in `bits` (reference :83-89), computed
        exactly in integer arithmetic"""
        b = np.asarray(bits).astype(np.uint64)
        n = np.zeros(b.shape, dtype=np.int64)
        for s in (32, 16, 8, 4, 2, 1):
            big = b >= (np.uint64(1) << np.uint64(s))
            n = np.where(big, n + s, n)
            b = np.where(big, b >> np.uint64(s), b)
        return (n + (b > 0)).astype(int)

    def _get_hll_rank(self, bits):
        """rank = leading zeros of `bits` seen as a (64 - p)-bit word, plus one (reference :91-104)"""
        rank = self.max_rank - self._np_bit_length(bits) + 1
        if rank.size and rank.min() <= 0:
            raise ValueError("Hash value overflow, maximum size is %d bits" % self.max_rank)
        return rank

    def _init_permutations(self, num_perm):
        """universal-hash parameters (a_j, b_j), j < num_perm, from numpy's legacy RandomState(seed): the draws
        interleave a_0, b_0, a_1, b_1, ... (reference :106-116).  uint64 [2, num_perm]."""
        gen = np.random.RandomState(self.minhash_seed)
        ab = np.empty((2, num_perm), dtype=np.uint64)
        for j in range(num_perm):
            ab[0, j] = gen.randint(1, self._mersenne_prime, dtype=np.uint64)
            ab[1, j] = gen.randint(0, self._mersenne_prime, dtype=np.uint64)
        return ab

    def _perms(self, device):
        key = str(device)
        if key not in self._dev_perms:
            ab = self._init_permutations(self.num_perm).view(np.int64)
            self._dev_perms[key] = torch.from_numpy(ab.copy()).to(device)
        return self._dev_perms[key]

    # ---- hop-0 sketches ------------------------------------------------------------------------------
    def _init_minhash_u32(self, n_nodes, device):
        _check_sizes(self.num_perm, self.p)
        ab = self._perms(device)
        out = torch.empty((n_nodes, self.num_perm), dtype=torch.int32, device=device)
        _native.check(_native.lib().ss_minhash_init(_ptr(out), 0, n_nodes, _ptr(ab[0]), _ptr(ab[1]), self.num_perm,
                                                    _stream(device)), 'ss_minhash_init')
        return out

    def _init_hll_u8(self, n_nodes, device):
        _check_sizes(self.num_perm, self.p)
        out = torch.empty((n_nodes, self.m), dtype=torch.uint8, device=device)
        _native.check(_native.lib().ss_hll_init(_ptr(out), 0, n_nodes, self.p, _stream(device)), 'ss_hll_init')
        return out

    def initialise_minhash(self, n_nodes):
        """int64 [n_nodes, num_perm] hop-0 MinHash rows (reference :118-124); lives on the HIP device"""
        device = _compute_device()
        packed = self._init_minhash_u32(n_nodes, device)
        out = unpack_minhash(packed)
        _tag(out, '_ss_u32', packed)
        # hop-0 marker: lets minhash_prop compute the first hop straight from node ids (ss_first_hop) instead of
        # gathering this table; voided by any in-place edit (version counter)
        out._ss_hop0 = (out._version, self._perms(device), self.p)
        return out

    def initialise_hll(self, n_nodes):
        """int8 [n_nodes, m] hop-0 HLL rows, one non-zero register each (reference :126-137)"""
        device = _compute_device()
        packed = self._init_hll_u8(n_nodes, device)
        out = packed.view(torch.int8)
        _tag(out, '_ss_u8', packed)
        out._ss_hop0 = (out._version, None, self.p)
        return out

    # ---- build ---------------------------------------------------------------------------------------
    def _bounds(self, device, what):
        """-> (check, err_flag) for a launch that validates node ids, after raising what an earlier deferred launch reported"""
        if self.strict_bounds == 'deferred':
            self._deferred.raise_if_set()
            return False, self._deferred.flag(device, what)
        raise_csr_protocol_faults()  # (strict / unchecked modes pass no deferred word: the library's own count still reports)
        return bool(self.strict_bounds), None

    def _prop_hub_hint(self, device, num_nodes, edge_index):
        """the same hint for the CSR of hll_prop / minhash_prop (the ELPH call sequence)"""
        return self._hub_hint(device, num_nodes, edge_index) if getattr(self, 'hub_hints', False) else None

    def _hub_hint(self, device, num_nodes, edge_index):
        """-> (pinned host word a build of this shape reports its hub + mega row count into, whether an EARLIER build of
        the shape reported none).  The word is read without synchronising -- it holds whatever the most recent COMPLETED build of
        the shape left (-1: none yet) -- and is only a hint: with it, an unskewed graph is built without hub lists (no leading hub
        workgroups in its launches; rounds 1-3: without the two hub-pass launches per hop that found nothing to do, 9 us of a 0.455 ms
        step at ogbl-collab size); if the hint is stale (another graph of the
        same shape that does have hub rows) those rows are walked by single wavefronts once -- slow, never wrong -- and the next
        build of the shape has its hub units back.  `eh.hub_hints = False` keeps them unconditionally."""
        key = (str(device), int(num_nodes), tuple(edge_index.shape), knobs.HUB_THRESHOLD)
        word = self._hub_words.get(key)
        if word is None:
            # One pinned arena for the engine's lifetime, one word per shape, NEVER handed back while the engine lives: a first-hop
            # launch still in flight stores into its word (system-scope store, csrc report_hub_rows) -- a word returned to torch's
            # pinned-memory cache could be given to somebody else by then.  More shapes than words: no hint for them.
            if self._hub_arena is None:
                self._hub_arena = torch.full((self.HUB_HINT_SHAPES,), -1, dtype=torch.int32).pin_memory()
            if len(self._hub_words) >= self.HUB_HINT_SHAPES:
                return None, False
            word = self._hub_words[key] = self._hub_arena[len(self._hub_words):len(self._hub_words) + 1]
        return word, int(word[0]) == 0

    def check_errors(self):
        """strict_bounds = 'deferred': wait for the launches issued so far and raise IndexError if any of them met a node id
        outside its num_nodes (call once after preprocessing / at the end of an epoch; every call into the engine also
        performs the non-waiting form of this check)"""
        self._deferred.raise_if_set(synchronize=True)

    def build_hash_tables(self, num_nodes, edge_index):
        """k-hop sketches of every node, k = 0..max_hops, and their HLL cardinalities (reference :139-165).
        @return: (SketchTable {k: {'hll','minhash'}}, cards float32 [num_nodes, max_hops])"""
        return self._build(num_nodes, edge_index, None)

    def _build(self, num_nodes, edge_index, shard):
        """shard = None: this process computes every row.  Otherwise (dist.sharded_build_hash_tables) an object with
        `rows` = (begin, end) owned by this rank, `padded_rows` >= num_nodes (allocation size, a multiple of the world
        size) and `gather(tensor) -> handle` / `wait(handle)`: in-place all-gather of the owned row blocks.  The two
        sketches are launched separately so that the gather of one overlaps the kernel of the other."""
        home = edge_index.device
        device = _compute_device(edge_index)
        params = self._params(device)
        # add_self_loops without num_nodes (reference :148): loops for i < max(edge_index) + 1 only; the count is
        # produced on the device by ss_csr_build and read by the propagation kernel -- no host round trip
        check, err_flag = self._bounds(device, f'build_hash_tables(num_nodes={num_nodes})')
        report, no_hubs = (None, False) if (check or not self.hub_hints) else self._hub_hint(device, num_nodes, edge_index)
        csr = build_csr(edge_index, num_nodes, device, check=check, err_flag=err_flag)
        csr.hub_report = report  # (the first-hop kernels of this build leave its hub + mega row count there)
        if no_hubs:  # an earlier build of this shape listed no hub / mega rows: no hub units (the row kernels walk every row)
            csr.has_hub_rows = False
        csr.use_inferred_self_loops = True
        rows = None if shard is None else shard.rows
        n_alloc = num_nodes if shard is None else shard.padded_rows
        cards = torch.empty((n_alloc, self.max_hops), dtype=torch.float32, device=device)
        table = SketchTable()
        h = self.max_hops
        # hop 1 from node ids: MinHash for 64 / 128 / 192 / 256 permutations at any hll_p, HLL at hll_p == 8
        fused_mh = self.fuse_first_hop and self.num_perm % 64 == 0 and self.num_perm <= 256
        fused = fused_mh and self.p == 8
        peer = shard is not None and getattr(shard, 'peer_write', False)
        if peer:  # the shard's persistent, IPC-shared tables (every rank's launches store into every rank's copy)
            mh, hll, cards = shard.tables(h, self.num_perm, self.m, device)
        else:
            mh = [torch.empty((n_alloc, self.num_perm), dtype=torch.int32, device=device) for _ in range(h)]
            hll = [torch.empty((n_alloc, self.m), dtype=torch.uint8, device=device) for _ in range(h)]
        if fused:
            # hop 1 is computed straight from node ids (ss_first_hop); the hop-0 tables (pure functions of the node id,
            # never read by get_subgraph_features) are produced only if a caller actually looks at them
            table[0] = HopSketch(None, None, home, make_packed=lambda n=num_nodes, d=device: (self._init_minhash_u32(n, d),
                                                                                            self._init_hll_u8(n, d)))
            mh_prev = hll_prev = None
        elif fused_mh:
            hll_prev = self._init_hll_u8(num_nodes, device)
            table[0] = HopSketch(None, None, home, make_packed=lambda n=num_nodes, d=device, l=hll_prev: (self._init_minhash_u32(n, d), l))
            mh_prev = None
        else:
            mh_prev = self._init_minhash_u32(num_nodes, device)  # hop 0 is replicated: a pure function of the node id
            hll_prev = self._init_hll_u8(num_nodes, device)
            table[0] = HopSketch(mh_prev, hll_prev, home)
        # (collab-like -4 %, ppa-like -5 %, citation2-like -1.2 % per step against the unfused schedule)
        if shard is None and fused and h >= 2 and self.num_perm == 128 and self.fuse_hop_stage:
            # ONE call for hops 1 and 2: hop-1 HLL first (hop-2 HLL rows need that table complete), then hop-1 MinHash + hop-2 HLL
            # in one launch (the VALU-bound first hop and the memory-bound table hop interleaved inside every wavefront,
            # csrc/ss_fused_hop.hip), then hop-2 MinHash; further hops unfused
            ab = self._perms(device)
            graph = csr.struct()
            # (the workspace of the stage's records form: 64 bytes per node, written by its HLL first hop and read by its fused kernel;
            # the library decides per call whether it is used)
            records = torch.empty((num_nodes, 16), dtype=torch.int32, device=device)
            with _Span('fused_hop_stage', device):
                _native.check(_native.lib().ss_fused_hop_stage_records(byref(graph), _ptr(ab[0]), _ptr(ab[1]), self.num_perm, _ptr(mh[0]),
                                                                       _ptr(mh[1]), self.p, _ptr(hll[0]), _ptr(cards), _ptr(hll[1]),
                                                                       _ptr(cards[:, 1]), h, byref(params.struct), _ptr(records),
                                                                       int(edge_index.shape[1]), _stream(device)), 'ss_fused_hop_stage_records')
            for k in range(3, h + 1):  # (inputs: hop k - 1 >= 2 of this build -- on a symmetric graph the rows skip their own row)
                _propagate(csr, mh[k - 2], hll[k - 2], device, cards_out=cards[:, k - 1], cards_stride=h, params=params,
                           mh_out=mh[k - 1], hll_out=hll[k - 1], hop_tables=True)
        elif shard is None:
            # (inside the library each of these calls is one launch per sketch, each hosting its hub units: measured faster than
            # two-sketch kernels -- first hop 37 + 134 us vs 184, table hop 111 + 192 us vs 326 on the bench graph)
            for k in range(1, h + 1):
                if k == 1 and fused:
                    self._first_hop(csr, device, mh[0], hll[0], cards, params)
                elif k == 1 and fused_mh:
                    self._first_hop(csr, device, mh[0], None, None, params)
                    _propagate(csr, None, hll_prev, device, cards_out=cards[:, 0], cards_stride=h, params=params, hll_out=hll[0])
                else:
                    logger.info(f"Calculating hop {k} hashes")
                    # (k >= 2: both inputs are hop k - 1 of this build; hop-0 rows are functions of the id alone: the self row stays)
                    _propagate(csr, mh_prev, hll_prev, device, cards_out=cards[:, k - 1], cards_stride=h, params=params,
                               mh_out=mh[k - 1], hll_out=hll[k - 1], hop_tables=k >= 2)
                mh_prev, hll_prev = mh[k - 1], hll[k - 1]
        elif peer:
            # peer-write: no exchange step -- the kernels store every finished row into all ranks' tables while they run
            # (csrc: mirror_* stores); a hop may start once EVERY rank's launches of the previous hop are complete
            if not (fused_mh and fused):
                raise NotImplementedError('the peer-write build is built for the default sketch shape (128 permutations, hll_p = 8)')
            for k in range(1, h + 1):
                mir_mh, mir_hll = shard.mirrors('mh', k - 1), shard.mirrors('hll', k - 1)
                none = [0] * len(mir_mh)
                if k == 1:
                    self._first_hop(csr, device, mh[0], None, None, params, rows=rows, mirrors=(mir_mh, none, none))
                    self._first_hop(csr, device, None, hll[0], cards, params, rows=rows, mirrors=(none, mir_hll, shard.mirrors('cards', 0)))
                else:
                    _propagate(csr, mh[k - 2], None, device, mh_out=mh[k - 1], rows=rows, mirrors=(mir_mh, none, none))
                    _propagate(csr, None, hll[k - 2], device, cards_out=cards[:, k - 1], cards_stride=h, params=params, hll_out=hll[k - 1],
                               rows=rows, mirrors=(none, mir_hll, shard.mirrors('cards', k - 1)))
                shard.hop_barrier()
            cards = cards[:num_nodes]
        else:
            pending_mh = pending_hll = None
            for k in range(1, h + 1):
                shard.wait(pending_mh)  # hop k-1 MinHash rows of every rank have arrived
                if k == 1 and fused_mh:
                    self._first_hop(csr, device, mh[0], None, None, params, rows=rows)
                else:
                    _propagate(csr, mh_prev, None, device, mh_out=mh[k - 1], rows=rows)
                pending_mh = shard.gather(mh[k - 1])
                shard.wait(pending_hll)
                if k == 1 and fused:
                    self._first_hop(csr, device, None, hll[0], cards, params, rows=rows)
                else:
                    _propagate(csr, None, hll_prev, device, cards_out=cards[:, k - 1], cards_stride=h, params=params,
                               hll_out=hll[k - 1], rows=rows)
                pending_hll = shard.gather(hll[k - 1])
                mh_prev, hll_prev = mh[k - 1], hll[k - 1]
            shard.wait(pending_mh)
            shard.wait(pending_hll)
            shard.wait(shard.gather(cards))
            cards = cards[:num_nodes]
        for k in range(1, h + 1):
            table[k] = HopSketch(mh[k - 1][:num_nodes], hll[k - 1][:num_nodes], home)
        if home != device:
            cards = cards.to(home)
            if self.strict_bounds == 'deferred':  # (the copy has waited for the build: the report is final, see get_subgraph_features)
                self._deferred.raise_if_set()
        return table, _stamp_tables(cards, self.tables_id)

    def _first_hop(self, csr, device, mh_out, hll_out, cards, params, rows=None, mirrors=None):
        """fused hop-0 + hop-1 (ss_first_hop) for either or both sketches"""
        ab = self._perms(device)
        graph = csr.struct(rows, mirrors)
        with _Span('first_hop_mh' if hll_out is None else ('first_hop_hll' if mh_out is None else 'first_hop'), device):
            _native.check(_native.lib().ss_first_hop(byref(graph), _ptr(ab[0]), _ptr(ab[1]), self.num_perm, _ptr(mh_out), self.p,
                                                     _ptr(hll_out), _ptr(cards) if hll_out is not None else None, self.max_hops,
                                                     byref(params.struct), _stream(device)), 'ss_first_hop')

    # ---- query ---------------------------------------------------------------------------------------
    def _resolve_tables(self, hash_table, device, rows=None):
        """packed tables of hops 1 .. max_hops; rows: the node ids the caller is going to read (a deferred LAST hop -- nobody
        else's input -- is then computed for those rows only, knobs.DEFER_TABLE_HOP)"""
        mh, hll = [], []
        for k in range(1, self.max_hops + 1):
            entry = hash_table[k]
            if isinstance(entry, HopSketch) and entry.mh_u32.device == device:
                m, l = entry.packed(device)
                mh.append(m)
                hll.append(l)
            else:
                t = entry['minhash']
                tw = None
                if rows is not None and k == self.max_hops and isinstance(t, LazyMinhash) and t.device == device:
                    tw = t.packed_for_rows(rows)
                mh.append(tw if tw is not None else _packed_minhash_of(t, device))
                hll.append(_packed_hll_of(entry['hll'], device))
        N, P = mh[0].shape
        for a, b in zip(mh, hll):
            if a.shape != (N, P) or b.shape != (N, self.m):
                raise ValueError('hash tables of different hops must have the same shape')
        return mh, hll, N, P

    def _device_cards(self, cards, N, device):
        """cards as float32 [N, >= max_hops] with unit column stride on `device`"""
        h = self.max_hops
        made_with = getattr(cards, '_ss_tables', None)
        if made_with is not None and not hll_tables.same_tables(made_with, self.tables_id):
            raise ValueError(f'cards were estimated with HLL++ tables {made_with}, this engine uses {self.tables_id}: '
                             f'a feature row would mix two bias tables (rebuild the cache or load the same tables)')
        # ELPH keeps `cards` on the CPU and the reference re-uploads it on every call (hashing.py:274): keep a device
        # twin on the tensor, invalidated by in-place edits, so repeated eval batches do not pay the copy again
        tag = getattr(cards, '_ss_cards', None)
        if cards.device == device and cards.dtype == torch.float32:
            cd = cards
        elif tag is not None and tag[0] == cards._version and tag[1].device == device:
            cd = tag[1]
        else:
            cd = cards.to(device=device, dtype=torch.float32)
            _tag(cards, '_ss_cards', cd)
        if cd.dim() != 2 or cd.size(0) != N or cd.size(1) < h:
            raise ValueError(f'cards must have shape [{N}, >= {h}], got {tuple(cd.shape)}')
        return cd if cd.stride(1) == 1 else cd.contiguous()

    def _device_degrees(self, degrees, N, device):
        """degrees (or None) as contiguous float32 [N] on `device`"""
        if degrees is None:
            return None
        dg = degrees.to(device=device, dtype=torch.float32).contiguous()
        if dg.dim() != 1 or dg.numel() != N:
            raise ValueError(f'degrees must have shape [{N}], got {tuple(dg.shape)}')
        return dg

    def _check_head(self, head, degrees):
        """what score_links and topk_links ask of their head before anything else is touched"""
        from .head import StructureHead
        if not isinstance(head, StructureHead):
            raise ValueError(f'head must be a StructureHead (StructureHead.from_module(model)), got {type(head).__name__}')
        if head.hops != self.max_hops:
            raise ValueError(f'head.dim = {head.dim} belongs to max_hash_hops = {head.hops}, this engine has max_hash_hops = {self.max_hops}')
        if head.normalised and degrees is None:
            raise ValueError('head.normalised: the head takes the degree-normalised copy of the row, give degrees')
        if degrees is not None and not head.normalised:
            raise ValueError(f'degrees given but head.dim = {head.dim} has no columns for the normalised copy (normalised=False)')

    def _flags(self, floor_sf=None):
        """the SS_FLAG_* word of a query; floor_sf: instead of self.floor_sf (DeviceFeatureStore records HashDataset's post-hoc floor)"""
        floor = self.floor_sf if floor_sf is None else floor_sf
        return (_native.SS_FLAG_USE_ZERO_ONE if self.use_zero_one else 0) | (_native.SS_FLAG_FLOOR_SF if floor else 0)

    def _send_home(self, home, *results):
        """device results on the caller's device.  A copy has waited for the launches: a deferred report is final behind it"""
        if all(r.device == home for r in results):
            return results
        results = tuple(r.to(home) for r in results)
        if self.strict_bounds == 'deferred':
            self._deferred.raise_if_set()
        return results

    def _query_inputs(self, links, hash_table, cards, degrees, floor_sf, out, out_width, what):
        """what every launch of the pair kernel takes, resolved once per call (the feature query and score_links share it);
        out_width: columns per link of a caller-supplied `out` (None: one float per link, a 1-D tensor)"""
        # where the links live, else where the packed tables already are, else cards, else the current device
        first = hash_table.get(1) if hasattr(hash_table, 'get') else None
        device = _compute_device(links, first.mh_u32 if isinstance(first, HopSketch) else None, cards)
        params = self._params(device)
        lk = links.to(device=device, dtype=torch.int64).contiguous()
        mh, hll, N, P = self._resolve_tables(hash_table, device, rows=lk)
        h = self.max_hops
        B = lk.size(0)
        cd = torch.zeros((N, h), dtype=torch.float32, device=device) if cards is None else self._device_cards(cards, N, device)
        shape = (B,) if out_width is None else (B, out_width)
        if out is not None and (out.device != device or out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous()):
            raise ValueError(f'out must be a contiguous float32 {list(shape)} tensor on {device}, got {out.dtype} {tuple(out.shape)} on {out.device}')
        mh_ptrs, hll_ptrs = _table_ptrs(mh, hll)
        flags = self._flags(floor_sf)
        strict, err = self._bounds(device, f'{what}({B} links, num_nodes={N})')
        if strict:
            err = _error_flag(device)  # (non-strict launches never touch the shared flag)
        dg = self._device_degrees(degrees, N, device)
        return device, params, lk, (mh, hll), mh_ptrs, hll_ptrs, N, P, B, cd, flags, strict, err, dg

    def _pair_kernel(self, links, hash_table, cards, want_debug=False, degrees=None, floor_sf=None, group_batch=None, out=None):
        """runs ss_pair_features for links [B,2]; returns (features [B,nf] (or [B,2nf] with degrees) on device, debug dict or None).
        group_batch: the links are first grouped by their first node and walked in that order, `group_batch` pairs per launch
        (knobs.GROUP_LINKS_MIN; same rows, in the caller's order).  out: the rows are written THERE (a contiguous float32
        [B, width] tensor on the compute device -- a slice of a larger result, dist.sharded_precompute) instead of a fresh tensor"""
        h = self.max_hops
        nf = h * (h + 2)
        width = 2 * nf if degrees is not None else nf
        device, params, lk, _tables, mh_ptrs, hll_ptrs, N, P, B, cd, flags, strict, err, dg = self._query_inputs(
            links, hash_table, cards, degrees, floor_sf, out, width, 'get_subgraph_features')
        if group_batch and not want_debug and 1 < B < (1 << 31) and N < (1 << 31):
            # a list that already has its runs (a coalesced edge list, an evaluation set listing every source's negatives together)
            # is walked as it is: grouping it again costs ~8 % and scatters the output rows.  One small reduction + ONE host read
            # per call of >= knobs.GROUP_LINKS_MIN links (0.5 ms of query and more); ElphHashes.group_links = True / False skips it.
            mode = getattr(self, 'group_links', 'auto')  # (instances pickled before the attribute existed)
            if mode == 'auto':
                mode = float((lk[1:, 0] == lk[:-1, 0]).sum().item()) < 0.5 * (B - 1)
            order = group_links_by_source(lk, N, device) if mode else None
            nf_out = width
            if out is None:
                out = torch.empty((B, nf_out), dtype=torch.float32, device=device)
            for s0 in range(0, B, group_batch):
                nb = min(group_batch, B - s0)
                lib = _native.lib()
                with _Span('pair_features', device):
                    if order is not None and B >= knobs.GROUP_GATHER_MIN:
                        # a set of gigabytes: gather the chunk's links, query the (now contiguous, grouped) chunk, scatter its rows
                        o = c_void_p(order.data_ptr() + 4 * s0)
                        lk_c = torch.empty((nb, 2), dtype=torch.int64, device=device)
                        rows_c = torch.empty((nb, nf_out), dtype=torch.float32, device=device)
                        _native.check(lib.ss_gather_links(_ptr(lk), o, nb, _ptr(lk_c), _stream(device)), 'ss_gather_links')
                        _native.check(lib.ss_pair_features_grouped(_ptr(lk_c), None, nb, N, h, mh_ptrs, P, hll_ptrs, _ptr(cd), cd.stride(0),
                                                                   byref(params.struct), flags, _ptr(dg), _ptr(rows_c), _ptr(err),
                                                                   _stream(device)), 'ss_pair_features_grouped')
                        _native.check(lib.ss_scatter_feature_rows(_ptr(rows_c), o, nb, nf_out, _ptr(out), _stream(device)), 'ss_scatter_feature_rows')
                        continue
                    if order is not None:  # every launch writes rows out[order[s0 + t]] of the ONE output tensor
                        args = (_ptr(lk), c_void_p(order.data_ptr() + 4 * s0), nb, N, h, mh_ptrs, P, hll_ptrs, _ptr(cd), cd.stride(0),
                                byref(params.struct), flags, _ptr(dg), _ptr(out), _ptr(err), _stream(device))
                    else:                  # as listed: a slice of the links and the matching slice of the output
                        args = (c_void_p(lk.data_ptr() + 16 * s0), None, nb, N, h, mh_ptrs, P, hll_ptrs, _ptr(cd), cd.stride(0),
                                byref(params.struct), flags, _ptr(dg), c_void_p(out.data_ptr() + 4 * nf_out * s0), _ptr(err), _stream(device))
                    _native.check(lib.ss_pair_features_grouped(*args), 'ss_pair_features_grouped')
            if strict and _take_error(device):
                raise IndexError(f'links refer to nodes outside [-{N}, {N})')
            return out, None
        if degrees is not None:
            if out is None:
                out = torch.empty((B, 2 * nf), dtype=torch.float32, device=device)
            with _Span('pair_features', device):
                _native.check(_native.lib().ss_pair_features_normalised(
                    _ptr(lk), B, N, h, mh_ptrs, P, hll_ptrs, _ptr(cd), cd.stride(0), byref(params.struct), flags, _ptr(dg),
                    _ptr(out), _ptr(err), _stream(device)), 'ss_pair_features_normalised')
            if strict and B > 0 and _take_error(device):
                raise IndexError(f'links refer to nodes outside [-{N}, {N})')
            return out, None
        if out is None:
            out = torch.empty((B, nf), dtype=torch.float32, device=device)
        dbg = None
        if want_debug:
            dbg = {'match': torch.empty((B, h, h), dtype=torch.int32, device=device),
                   'zeros': torch.empty((B, h, h), dtype=torch.int32, device=device),
                   'inter': torch.empty((B, h, h), dtype=torch.float32, device=device)}
        with _Span('pair_features', device):
            _native.check(_native.lib().ss_pair_features(
                _ptr(lk), B, N, h, mh_ptrs, P, hll_ptrs, _ptr(cd), cd.stride(0), byref(params.struct), flags, _ptr(out),
                _ptr(dbg['match']) if dbg else None, _ptr(dbg['zeros']) if dbg else None,
                _ptr(dbg['inter']) if dbg else None, _ptr(err), _stream(device)), 'ss_pair_features')
        if strict and B > 0 and _take_error(device):
            raise IndexError(f'links refer to nodes outside [-{N}, {N})')
        return out, dbg

    def _score_kernel(self, links, hash_table, cards, head, degrees=None, group_batch=None, out=None):
        """runs ss_pair_scores for links [B,2]: float32 [B] on the compute device.  group_batch / out: as _pair_kernel"""
        device, params, lk, _tables, mh_ptrs, hll_ptrs, N, P, B, cd, flags, strict, err, dg = self._query_inputs(
            links, hash_table, cards, degrees, None, out, None, 'score_links')
        h = self.max_hops
        hd = head._device(device)
        lib = _native.lib()
        if out is None:
            out = torch.empty((B,), dtype=torch.float32, device=device)

        def launch(lk_ptr, order_ptr, nb, out_ptr):
            _native.check(lib.ss_pair_scores(lk_ptr, order_ptr, nb, N, h, mh_ptrs, P, hll_ptrs, _ptr(cd), cd.stride(0), byref(params.struct),
                                             flags, _ptr(dg), byref(hd.struct), out_ptr, _ptr(err), _stream(device)), 'ss_pair_scores')

        if group_batch and 1 < B < (1 << 31) and N < (1 << 31):
            # the walk of get_subgraph_features over a large link set, one float per link instead of a row: grouped by first node
            # unless the list already has its runs (one host read), gathered / scattered around the launch for sets of gigabytes
            mode = getattr(self, 'group_links', 'auto')
            if mode == 'auto':
                mode = float((lk[1:, 0] == lk[:-1, 0]).sum().item()) < 0.5 * (B - 1)
            order = group_links_by_source(lk, N, device) if mode else None
            for s0 in range(0, B, group_batch):
                nb = min(group_batch, B - s0)
                with _Span('pair_scores', device):
                    if order is not None and B >= knobs.GROUP_GATHER_MIN:
                        o = c_void_p(order.data_ptr() + 4 * s0)
                        lk_c = torch.empty((nb, 2), dtype=torch.int64, device=device)
                        sc_c = torch.empty((nb,), dtype=torch.float32, device=device)
                        _native.check(lib.ss_gather_links(_ptr(lk), o, nb, _ptr(lk_c), _stream(device)), 'ss_gather_links')
                        launch(_ptr(lk_c), None, nb, _ptr(sc_c))
                        _native.check(lib.ss_scatter_feature_rows(_ptr(sc_c), o, nb, 1, _ptr(out), _stream(device)), 'ss_scatter_feature_rows')
                    elif order is not None:  # every launch writes out[order[s0 + t]] of the ONE output tensor
                        launch(_ptr(lk), c_void_p(order.data_ptr() + 4 * s0), nb, _ptr(out))
                    else:                    # as listed: a slice of the links and the matching slice of the output
                        launch(c_void_p(lk.data_ptr() + 16 * s0), None, nb, c_void_p(out.data_ptr() + 4 * s0))
        else:
            with _Span('pair_scores', device):
                launch(_ptr(lk), None, B, _ptr(out))
        if strict and B > 0 and _take_error(device):
            raise IndexError(f'links refer to nodes outside [-{N}, {N})')
        return out

    def score_links(self, links, hash_table, cards, head, degrees=None, batch_size=11000000, out=None, **unsupported):
        """one float per link: the structure-feature head of a trained model applied to the row get_subgraph_features would return,
        inside the pair kernel -- the row is never written (csrc/ss_head.hpp).  For link q

            score[q] = b2 + sum_j w2[j] * max(0, t'[j] + sum_i W'[j][i] * x_q[i]),

        x_q = exactly the row get_subgraph_features(links, hash_table, cards, degrees=degrees) holds for q (same use_zero_one /
        floor_sf flags, NaN / Inf -> 0 rule of the normalised half and negative-id wrapping).  For a model without node features,
        embeddings and RA this is its eval-mode logit; for every other model the label branch's exact share of it (INTEGRATION.md
        shows the three lines that add the rest).
        @param head: a `StructureHead` (head.py) whose dim matches max_hash_hops; head.normalised requires `degrees`, and `degrees`
               without it is a ValueError
        @param degrees: float tensor [N], as get_subgraph_features takes it
        @param batch_size: pairs per kernel launch (scores do not depend on it, bit for bit)
        @param out: optional contiguous float32 [n_links] tensor on the compute device the scores are written into
        @return: float32 [n_links] on links.device; an id outside [-N, N) gives NaN and is reported as get_subgraph_features
                 reports it, in every strict_bounds mode
        Inference only -- there are no gradients.  Out of scope (ValueError where an argument suggests otherwise): a head on the
        masked query (mask_target), lazy stores, dist.sharded_precompute.  The head inside the one-vs-all scan is topk_links.  No CPU fallback."""
        if unsupported:
            names = ', '.join(sorted(unsupported))
            raise ValueError(f'score_links does not take {names}: the head runs behind the plain query only (no mask_target, no lazy store)')
        self._check_head(head, degrees)
        if links.dim() == 1:
            links = links.unsqueeze(0)
        _native.lib()  # (NativeLibraryMissing before anything else is touched)
        n = links.size(0)
        batch_size = max(int(batch_size), 1)
        if knobs.GROUP_LINKS_MIN and n >= knobs.GROUP_LINKS_MIN and n < (1 << 31):
            scores = self._score_kernel(links, hash_table, cards, head, degrees=degrees, group_batch=batch_size, out=out)
        elif n <= batch_size:
            scores = self._score_kernel(links, hash_table, cards, head, degrees=degrees, out=out)
        elif out is not None:
            if out.dim() != 1 or out.size(0) != n or not out.is_contiguous():
                raise ValueError(f'out must be a contiguous float32 [{n}] tensor on the compute device, got {out.dtype} {tuple(out.shape)}')
            for s in range(0, n, batch_size):
                self._score_kernel(links[s:s + batch_size], hash_table, cards, head, degrees=degrees, out=out[s:s + batch_size])
            scores = out
        else:
            scores = torch.cat([self._score_kernel(links[s:s + batch_size], hash_table, cards, head, degrees=degrees)
                                for s in range(0, n, batch_size)], dim=0)
        return scores if out is not None else self._send_home(links.device, scores)[0]

    def _get_intersections(self, edge_list, hash_table):
        """set-intersection estimates jaccard * union for every (k1, k2) (reference :167-189).
        @return: {(k1, k2): float32 [n_edges]} on edge_list.device"""
        _, dbg = self._pair_kernel(edge_list, hash_table, None, want_debug=True)
        inter = dbg['inter'].to(edge_list.device)
        return {(k1, k2): inter[:, k1 - 1, k2 - 1].contiguous()
                for k1 in range(1, self.max_hops + 1) for k2 in range(1, self.max_hops + 1)}

    def topk_candidates(self, sources, hash_table, k, hops=(1, 1), exclude=None):
        """the k best link partners of every source by the engine's set-intersection estimate -- what the reference's
        sample_hard_negatives (src/data.py:262-304, unfinished) ranks by, and what full-ranking evaluation and candidate generation
        need.  The score of candidate v for source u is I[k1, k2] = J * U of u's hop-k1 and v's hop-k2 sketches (hashing.py:167-189),
        bit-identical to _get_intersections([(u, v)])[(k1, k2)] (-0.0 comes back as +0.0).
        @param sources: int64 [S] node ids (torch-style negative ids allowed), CPU or device
        @param hash_table: anything get_subgraph_features accepts
        @param k: 1 <= k <= N;  @param hops: (k1, k2), 1 <= k1, k2 <= max_hash_hops
        @param exclude: optional int64 [2, E] edge_index: every v with an edge u -> v in it is no candidate of u (nor is u itself)
        @return: (ids int64 [S, k], scores float32 [S, k]) on sources.device, ordered by score descending then id ascending; rows
                 with fewer than k eligible candidates end in id -1 / score -inf.  A row depends on its own source only.
        Ranking by a trained model's structure head instead of one raw estimate: topk_links."""
        try:
            k1, k2 = (int(x) for x in hops)
        except (TypeError, ValueError):
            raise ValueError(f'hops must be a pair (k1, k2), got {hops!r}')
        if not (1 <= k1 <= self.max_hops and 1 <= k2 <= self.max_hops):
            raise ValueError(f'hops must lie in [1, {self.max_hops}], got {(k1, k2)}')
        src, ex, N, P = self._topk_arguments(sources, hash_table, k, exclude)

        def scan(lib, sb, nb, N, P, mh, hll, params, keys, nbytes, err, stream):
            _native.check(lib.ss_topk_scan(sb, nb, N, _ptr(mh[k1 - 1]), _ptr(hll[k1 - 1]), _ptr(mh[k2 - 1]), _ptr(hll[k2 - 1]), P,
                                           byref(params.struct), _ptr(keys), nbytes, _ptr(err), stream), 'ss_topk_scan')

        return self._topk_run('topk_candidates', src, ex, hash_table, int(k), scan)

    def _topk_arguments(self, sources, hash_table, k, exclude, what='sources'):
        """what topk_candidates, topk_links and rank_links (its links, flattened: what='links') check before a device is touched:
        (sources, exclude or None, N, P)"""
        from .candidates import _check_host_ids, _id_list
        src = _id_list(sources, what)
        N, P = _table_shape(hash_table, 1)
        _check_sizes(P, self.p)
        k = int(k)
        if not 1 <= k <= N:
            raise ValueError(f'k must lie in [1, {N}], got {k}')
        ex = None
        if exclude is not None:
            ex = torch.as_tensor(exclude)
            if ex.dim() != 2 or ex.size(0) != 2 or ex.dtype.is_floating_point or ex.dtype == torch.bool:
                raise ValueError(f'exclude must be an integer [2, E] edge_index, got {ex.dtype} {tuple(ex.shape)}')
        _check_host_ids(src, N, what)  # CPU ids are checked here, as the reference's CPU indexing would; device ids are reported late (strict_bounds)
        if ex is not None and not ex.is_cuda and ex.numel() and (int(ex.min()) < -N or int(ex.max()) >= N):
            raise IndexError(f'exclude refers to nodes outside [-{N}, {N})')
        return src, ex, N, P

    def _topk_run(self, what, src, ex, hash_table, k, scan, cards=None, degrees=None):
        """the walk both one-vs-all queries share: blocks of sources bounded by _TOPK_KEY_BYTES, `scan` filling a block's keys, the
        exclude CSR, torch.topk on the unique keys, _decode_topk_keys.  cards / degrees: resolved on the compute device and handed
        to `scan` (topk_links)"""
        home = src.device
        S = src.numel()
        first = hash_table.get(1) if hasattr(hash_table, 'get') else None
        device = _compute_device(src, first.mh_u32 if isinstance(first, HopSketch) else None)
        mh, hll, N, P = self._resolve_tables(hash_table, device)
        params = self._params(device)
        extra = ()
        if cards is not None:
            extra = (self._device_cards(cards, N, device), self._device_degrees(degrees, N, device))
        lk = src.to(device=device, dtype=torch.int64).contiguous()
        strict, err = self._bounds(device, f'{what}({S} sources, num_nodes={N})')
        csr, err = _exclude_csr(ex, N, device, strict, err)
        ids = torch.empty((S, k), dtype=torch.int64, device=device)
        scores = torch.empty((S, k), dtype=torch.float32, device=device)
        blk = max(1, min(S, _TOPK_KEY_BYTES // (8 * N)))
        lib = _native.lib()
        if S:
            keys = torch.empty((blk, N), dtype=torch.int64, device=device)
            nbytes = keys.numel() * 8
        for b0 in range(0, S, blk):
            nb = min(blk, S - b0)
            sb = c_void_p(lk.data_ptr() + 8 * b0)
            with _Span('topk_scan', device):
                scan(lib, sb, nb, N, P, mh, hll, params, keys, nbytes, err, _stream(device), *extra)
            if csr is not None:
                with _Span('topk_exclude', device):
                    _native.check(lib.ss_topk_exclude(sb, nb, N, _ptr(csr.rowptr), _ptr(csr.col), _ptr(keys), nbytes, _stream(device)),
                                  'ss_topk_exclude')
            with _Span('topk_select', device):
                top = torch.topk(keys[:nb], k, dim=1, largest=True, sorted=True).values  # unique keys: no ties, deterministic
                ids[b0:b0 + nb], scores[b0:b0 + nb] = _decode_topk_keys(top)
        if strict and S and _take_error(device):
            raise IndexError(f'sources refer to nodes outside [-{N}, {N})')
        return self._send_home(home, ids, scores)

    def topk_links(self, sources, hash_table, cards, k, head, degrees=None, exclude=None):
        """the k link partners a trained model's structure head ranks highest for every source: topk_candidates' one-vs-all scan with
        score_links' score instead of one raw intersection estimate (csrc/ss_topk_head.hip) -- what full-ranking
        evaluation (MRR / Hits@K over all nodes), hard-negative mining by the model's own score and candidate generation ask for.
        The score of candidate v for source u is bit-identical to score_links([[u, v]], hash_table, cards, head, degrees=degrees)
        (u first: the row is not symmetric; -0.0 comes back as +0.0); no link list and no feature row is ever written.
        @param sources: int64 [S] node ids (torch-style negative ids allowed), CPU or device
        @param hash_table, cards, head, degrees: as score_links takes them (head.normalised requires degrees; degrees without it is
               a ValueError)
        @param k: 1 <= k <= N
        @param exclude: optional int64 [2, E] edge_index: every v with an edge u -> v in it is no candidate of u (nor is u itself)
        @return: (ids int64 [S, k], scores float32 [S, k]) on sources.device, ordered by score descending then id ascending; rows
                 with fewer than k eligible candidates end in id -1 / score -inf.  A row depends on its own source only.
        Ids outside [-N, N) are reported as topk_candidates reports them.  Non-finite scores (overflow under absurd weights) are
        outside the contract.  Inference only; out of scope: the masked query behind the scan, dist sharding.  No CPU fallback.
        The exact rank of a GIVEN link among all nodes (MRR / Hits@K at any depth, no keys): rank_links."""
        self._check_head(head, degrees)
        if cards is None:
            raise ValueError('cards must be given: the feature row needs the neighbourhood sizes build_hash_tables returns')
        src, ex, N, P = self._topk_arguments(sources, hash_table, k, exclude)
        h = self.max_hops
        flags = self._flags()

        def scan(lib, sb, nb, N, P, mh, hll, params, keys, nbytes, err, stream, cd, dg):
            hd = head._device(keys.device)
            mh_ptrs, hll_ptrs = _table_ptrs(mh, hll)
            _native.check(lib.ss_topk_score_scan(sb, nb, N, h, mh_ptrs, hll_ptrs, P, _ptr(cd), cd.stride(0), byref(params.struct), flags,
                                                 _ptr(dg), byref(hd.struct), _ptr(keys), nbytes, _ptr(err), stream), 'ss_topk_score_scan')

        return self._topk_run('topk_links', src, ex, hash_table, int(k), scan, cards=cards, degrees=degrees)

    def rank_links(self, links, hash_table, cards, head, degrees=None, exclude=None, **unsupported):
        """at which rank a trained model's structure head puts each link (u, t) among ALL link partners of u: what MRR / Hits@K of
        positive links over all nodes ask for (reference src/evaluation.py ranks a positive among sampled negatives).  With s(u, v)
        the float32 score_links([[u, v]], hash_table, cards, head, degrees=degrees) returns, bit for bit, and the candidates
        C_q = {v in [0, N) : v != u, v != t, (u -> v) not in exclude} of link q = (u, t):

            greater[q] = #{v in C_q : s(u, v) > s(u, t)},     equal[q] = #{v in C_q : s(u, v) == s(u, t)}

        (float compares: -0.0 == +0.0, as topk_links folds it).  Optimistic rank 1 + greater, pessimistic 1 + greater + equal; the
        place of t in the topk_links(u, k = N) row is greater + #{tied v < t}.  The one-vs-all scan of topk_links with two counters
        per link in registers instead of its 8 N bytes of ranking keys per source: 16 bytes per link are written, nothing is
        selected (csrc/ss_rank.hip).
        @param links: int [L, 2] (or [2]) rows (u, t), torch-style negative ids allowed, CPU or device; u == t is a link like any other
        @param hash_table, cards, head, degrees: as score_links / topk_links take them (head.normalised requires degrees; degrees
               without it is a ValueError)
        @param exclude: optional int [2, E] edge_index read as a SET of directed pairs u -> v (duplicates, self loops, negative ids
               allowed): such a v is no candidate of u.  The target is never a candidate of itself, so (u -> t) in it changes nothing
               (the filtered setting, where positives are edges)
        @return: (greater int64 [L], equal int64 [L]) on links.device.  A row depends on its own link only -- not on L, the order,
                 duplicates or how the call is split into launches.  Ids outside [-N, N), in links or exclude, are reported as
                 topk_links reports them; both counts of such a link are -1.
        Non-finite scores are outside the contract.  Inference only; out of scope: the masked query behind the scan, dist sharding,
        de-duplicating links that share a source (each link is scanned on its own).  No CPU fallback."""
        if unsupported:
            names = ', '.join(sorted(unsupported))
            raise ValueError(f'rank_links does not take {names}: the head runs behind the plain query only (no mask_target, no lazy store)')
        self._check_head(head, degrees)
        if cards is None:
            raise ValueError('cards must be given: the feature row needs the neighbourhood sizes build_hash_tables returns')
        lk = torch.as_tensor(links)
        if lk.dim() == 1:
            lk = lk.unsqueeze(0)
        if lk.dim() != 2 or lk.size(1) != 2:
            raise ValueError(f'links must be an integer [L, 2] tensor, got {lk.dtype} {tuple(lk.shape)}')
        _, ex, N, P = self._topk_arguments(lk.reshape(-1), hash_table, 1, exclude, what='links')
        home, L = lk.device, lk.size(0)
        if L == 0:
            return torch.empty(0, dtype=torch.int64, device=home), torch.empty(0, dtype=torch.int64, device=home)
        first = hash_table.get(1) if hasattr(hash_table, 'get') else None
        device = _compute_device(lk, first.mh_u32 if isinstance(first, HopSketch) else None, cards)
        mh, hll, N, P = self._resolve_tables(hash_table, device)
        params = self._params(device)
        cd, dg, hd = self._device_cards(cards, N, device), self._device_degrees(degrees, N, device), head._device(device)
        h = self.max_hops
        mh_ptrs, hll_ptrs = _table_ptrs(mh, hll)
        flags = self._flags()
        lk = lk.to(device=device, dtype=torch.int64).contiguous()
        strict, err = self._bounds(device, f'rank_links({L} links, num_nodes={N})')
        csr, err = _exclude_csr(ex, N, device, strict, err)
        lib = _native.lib()
        scores = self._pair_scores(device, N, P, mh_ptrs, hll_ptrs, cd, params, dg, hd, err)
        thr = scores(lk, torch.empty((L,), dtype=torch.float32, device=device))
        counts = torch.zeros((L, 2), dtype=torch.int64, device=device)
        for s0 in range(0, L, _RANK_LAUNCH_LINKS):
            nb = min(_RANK_LAUNCH_LINKS, L - s0)
            with _Span('rank_scan', device):
                _native.check(lib.ss_rank_score_scan(c_void_p(lk.data_ptr() + 16 * s0), c_void_p(thr.data_ptr() + 4 * s0), nb, N, h, mh_ptrs,
                                                     hll_ptrs, P, _ptr(cd), cd.stride(0), byref(params.struct), flags, _ptr(dg),
                                                     byref(hd.struct), c_void_p(counts.data_ptr() + 16 * s0), _ptr(err), _stream(device)),
                              'ss_rank_score_scan')
        wrapped = torch.where(lk < 0, lk + N, lk)
        bad = ((wrapped < 0) | (wrapped >= N)).any(dim=1)
        if csr is not None:
            with _Span('rank_exclude', device):
                self._rank_exclusion(counts, wrapped, bad, thr, csr, N, scores)
        counts.masked_fill_(bad.unsqueeze(1), -1)
        if strict and _take_error(device):
            raise IndexError(f'links refer to nodes outside [-{N}, {N})')
        return self._send_home(home, counts[:, 0].contiguous(), counts[:, 1].contiguous())

    def _pair_scores(self, device, N, P, mh_ptrs, hll_ptrs, cd, params, dg, hd, err):
        """the ONE form of s(u, v): the launch behind score_links as scores(pairs int64 [n, 2], out float32 [n]) -> out, for
        rank_links' thresholds and excluded pairs and for topk_links_lsh's candidates"""
        lib, h, flags = _native.lib(), self.max_hops, self._flags()

        def scores(pairs, out):
            with _Span('pair_scores', device):
                _native.check(lib.ss_pair_scores(_ptr(pairs), None, pairs.size(0), N, h, mh_ptrs, P, hll_ptrs, _ptr(cd), cd.stride(0),
                                                 byref(params.struct), flags, _ptr(dg), byref(hd.struct), _ptr(out), _ptr(err),
                                                 _stream(device)), 'ss_pair_scores')
            return out

        return scores

    @staticmethod
    def _rank_exclusion(counts, links, bad, thr, csr, N, scores):
        """the scan has counted every v != u, t; the excluded partners of each link's source are taken back out of counts [L, 2]:
        the set {v : u -> v in the exclude CSR} \\ {u, t} per link, s(u, v) from `scores`, compared with thr as the scan compares.
        links: wrapped ids; bad: links with an id out of range (they take no part).  Two host reads (the sizes of the two gathers)."""
        device = links.device
        u = links[:, 0].masked_fill(bad, 0)
        # the rows of the DISTINCT sources, each partner once: sorted keys source * N + v (the CSR's rows hold duplicates, unordered)
        us, of_link = torch.unique(u, return_inverse=True)
        keys = _csr_row_keys(csr, us, N)
        if keys is None:
            return
        row = torch.searchsorted(keys, torch.arange(us.numel() + 1, dtype=torch.int64, device=device) * N)
        # per link the extent of its source's row in `keys`; the pairs (link, partner) are walked flat, _RANK_EXCLUDE_PAIRS at a time
        n_q = (row[of_link + 1] - row[of_link]).masked_fill(bad, 0)
        q_ends = torch.cumsum(n_q, 0)
        pairs = int(q_ends[-1].item())
        for a in range(0, pairs, _RANK_EXCLUDE_PAIRS):
            e = torch.arange(a, min(a + _RANK_EXCLUDE_PAIRS, pairs), dtype=torch.int64, device=device)
            q = torch.searchsorted(q_ends, e, right=True)
            v = keys[row[of_link[q]] + (e - (q_ends[q] - n_q[q]))] % N
            sc = scores(torch.stack([u[q], v], dim=1).contiguous(), torch.empty((e.numel(),), dtype=torch.float32, device=device))
            candidate = (v != links[q, 0]) & (v != links[q, 1])
            hit = torch.stack([(sc > thr[q]) & candidate, (sc == thr[q]) & candidate], dim=1).to(torch.int64)
            counts.index_add_(0, q, -hit)

    def build_lsh_index(self, hash_table, hop=1, rows=4, bands=None, max_bucket=1024, _key_bits=64):
        """an LSH index by banding over the stored hop-`hop` MinHash rows (lsh.py, csrc/ss_lsh.hip): what lsh_candidates
        and topk_links_lsh look partners up in instead of scanning all N nodes per source, for the workloads that ask for many sources
        (hard-negative mining by the model's own score, candidate generation, a kNN graph).  Band j of node v is the slice
        M_hop[v][j * rows : (j + 1) * rows] of its row (`HopSketch.mh_u32`); the bucket of (j, v) is the set of nodes whose band-j slice
        equals v's, value for value.  Two nodes whose hop-`hop` neighbourhoods have Jaccard J share a band with probability about
        J^rows and one of `bands` bands with about 1 - (1 - J^rows)^bands.
        @param hash_table: anything get_subgraph_features accepts;  @param hop: 1 <= hop <= max_hash_hops
        @param rows: MinHash values per band, >= 1;  @param bands: rows * bands <= P, default P // rows
        @param max_bucket: a bucket with more members is skipped: it yields no candidates for any of its members in that band (rows
               shared by many nodes -- nodes without edges and self loop, an empty graph -- would make the query quadratic)
        @return: an `LshIndex` resident on the compute device (hop, rows, bands, num_nodes, num_perm, max_bucket, skipped_buckets int64
                 [bands], nbytes).  It keeps a view of the hop's packed table to verify slices against: after update_hash_tables (or any
                 other change of the table) it is STALE and must be rebuilt.
        Out of scope: several hops in one index (build two, merge the candidates), saving / loading, dist sharding, incremental update."""
        from . import lsh
        return lsh.build_lsh_index(self, hash_table, hop, rows, bands, max_bucket, _key_bits)

    def lsh_candidates(self, sources, index, exclude=None, min_bands=1):
        """the nodes that share a bucket of `index` with each source: v is a candidate of u iff v != u, (u -> v) is not in `exclude`
        and u, v share a non-skipped bucket in at least `min_bands` bands (exact slice equality: the index's sort key never decides).
        @param sources: int [S] node ids as topk_links takes them (torch-style negative ids wrapped, duplicates allowed, CPU or device,
               S = 0 fine; ids outside [-N, N) are reported as topk_links reports them and have no candidates)
        @param exclude: optional int [2, E] edge_index read as a set of directed pairs u -> v (duplicates, self loops, negative ids fine)
        @return: (rowptr int64 [S + 1], ids int64 [T], bands int32 [T]) on sources.device: row s is ids[rowptr[s] : rowptr[s + 1]],
                 ascending and unique, bands = in how many bands the pair shares a bucket.  A row depends on its own source only.
        The masked query and dist sharding are out of scope."""
        from . import lsh
        return lsh.lsh_candidates(self, sources, index, exclude, min_bands)

    def topk_links_lsh(self, sources, hash_table, cards, k, head, index, degrees=None, exclude=None, min_bands=1):
        """topk_links restricted to the candidates lsh_candidates(sources, index, exclude, min_bands) lists: the k of them the structure
        head ranks highest per source, scored pair by pair through the launch behind score_links -- no scan of all N nodes, no feature
        row and no [S, N] array.  Approximate by design: a partner that shares no bucket with u is never seen (tools/probe_lsh.py
        measures the recall against topk_links).
        @param sources, hash_table, cards, k, head, degrees, exclude: as topk_links takes them;  @param index: build_lsh_index(hash_table, ...)
        @return: (ids int64 [S, k], scores float32 [S, k]) on sources.device, ordered by score descending then id ascending; rows with
                 fewer than k candidates end in id -1 / score -inf.  Scores are bit-identical to score_links([[u, v]], ...) (-0.0 comes
                 back as +0.0).  A row depends on its own source only.  Ids outside [-N, N) are reported as topk_links reports them."""
        from . import lsh
        return lsh.topk_links_lsh(self, sources, hash_table, cards, k, head, index, degrees, exclude, min_bands)

    def topk_links_wedge(self, sources, hash_table, cards, k, head, graph, degrees=None, exclude=None, min_common=1, max_walks=None,
                         _lds_slots=None):
        """topk_links restricted to the EXACT two-hop candidates graph.candidates(sources, exclude, min_common, max_walks) lists -- the
        nodes that share at least min_common neighbours with the source (wedge.py, csrc/ss_wedge.hip): the k of them the
        structure head ranks highest per source, scored pair by pair through the launch behind score_links -- no scan of all N nodes,
        no feature row and no [S, N] array.  Exact on its set: unlike topk_links_lsh nothing depends on a tuning of rows / bands; a
        partner without a common neighbour is never seen.
        @param sources, hash_table, cards, k, head, degrees, exclude: as topk_links takes them
        @param graph: WedgeGraph(num_nodes, edge_index) of the tables' num_nodes;  @param min_common, max_walks: as .candidates
        @return: (ids int64 [S, k], scores float32 [S, k]) on sources.device, ordered by score descending then id ascending; rows with
                 fewer than k candidates (a skipped source: none) end in id -1 / score -inf.  Scores are bit-identical to
                 score_links([[u, v]], ...) (-0.0 comes back as +0.0).  A row depends on its own source only.  Ids outside [-N, N)
                 are reported as topk_links reports them."""
        from . import wedge
        return wedge.topk_links_wedge(self, sources, hash_table, cards, k, head, graph, degrees, exclude, min_common, max_walks, _lds_slots)

    def exact_subgraph_features(self, links, num_nodes, edge_index, batch_size=11000000, return_counts=False, mask_target=False):
        """the features get_subgraph_features would return if every estimator were exact: with the k-hop balls B_k of the graph
        build_hash_tables(num_nodes, edge_index) propagates over (its edges, flow source -> target, plus a self loop at every node
        below max(edge_index) + 1), I[k1][k2] = |B_k1(u) & B_k2(v)| replaces J * U and |B_k(u)|, |B_k(v)| replace cards[u], cards[v]
        in the same feature algebra (LABEL_LOOKUP order, use_zero_one / floor_sf as set now).  Counted by BFS on the GPU
        (exact.py, csrc/ss_exact.hip).
        @param links: int tensor [L, 2] (or [2]), torch-style negative ids wrapped; CPU or device
        @param num_nodes, edge_index: as given to build_hash_tables; edge_index CPU or device
        @param batch_size: pairs per launch (results do not depend on it)
        @param mask_target: True counts every link in the graph without its own edge (every copy of u -> v and of v -> u; self loops and
               max(edge_index) + 1 stay): the exact counterpart of get_subgraph_features(mask_target=edge_index)
        @return: float32 [L, h(h+2)] on links.device; with return_counts also int32 I [L, h, h] and int32 balls [L, 2, h] (u, v)"""
        return exact.exact_subgraph_features(self, links, num_nodes, edge_index, batch_size=batch_size, return_counts=return_counts,
                                             mask_target=mask_target)

    def exact_subgraph_nodes(self, links, num_nodes, edge_index, batch_size=11000000, mask_target=False, max_nodes=None, return_info=False):
        """WHICH nodes exact_subgraph_features counts: per link (u, v) every node x of B_h(u) | B_h(v), h = max_hash_hops, with the
        distance pair (d_u(x), d_v(x)) -- the node set of the link's enclosing subgraph with its distance-encoding labels.  The graph,
        the balls (in-edge hops; on a symmetric edge_index: hops) and the arguments are those of exact_subgraph_features, except that
        a root is always in its own ball at distance 0, also a node at or above max(edge_index) + 1, whose sketch ball is empty.  BFS
        on the GPU (exact_nodes.py, csrc/ss_exact_nodes.hip).
        @param links: int tensor [L, 2] (or [2]), torch-style negative ids wrapped; CPU or device; L = 0 fine
        @param num_nodes, edge_index: as given to build_hash_tables; duplicate edges and self-loop edges change nothing; E = 0 fine
        @param batch_size: pairs per launch (rows do not depend on it)
        @param mask_target: True lists every link in the graph without its own edge (every copy of u -> v and of v -> u), as
               exact_subgraph_features(mask_target=True) counts it
        @param max_nodes: None = no cap; otherwise a link whose union holds more than max_nodes nodes gets an EMPTY row and is
               reported in info['truncated'] (the rule max_walks is for WedgeGraph.candidates, applied to hub links)
        @return: (rowptr int64 [L + 1], ids int64 [T], dist uint8 [T, 2]) on links.device, T = rowptr[L]: row q is
                 ids[rowptr[q] : rowptr[q + 1]], ascending and unique, dist[:, 0] = d_u, dist[:, 1] = d_v.  A distance of 0 .. h is the
                 graph distance (within the ball it equals the distance in the induced subgraph).  h + 1 is a SENTINEL, not a
                 distance: it says "farther than h, or unreachable", so labels computed on the induced subgraph may differ beyond h.
                 u == v gives one ball with d_u == d_v.  A row is a function of the graph, the link and mask_target only: not of
                 the kernel tier, batch_size or the other links.  The counts of exact_subgraph_features(return_counts=True) are
                 histograms of dist: I[q, k1, k2] = #{d_u <= k1 + 1 and d_v <= k2 + 1} (for roots below max(edge_index) + 1).
                 With return_info also {'truncated': int64 indices of the capped links, 'lds_links' / 'large_links': how many links
                 each kernel tier counted}.  Argument errors as exact_subgraph_features, before any launch.  No CPU fallback."""
        from . import exact_nodes
        return exact_nodes.exact_subgraph_nodes(self, links, num_nodes, edge_index, batch_size=batch_size, mask_target=mask_target,
                                                max_nodes=max_nodes, return_info=return_info)

    def sampled_subgraph_nodes(self, links, num_nodes, edge_index, batch_size=11000000, max_nodes_per_hop=None, ratio_per_hop=1.0, seed=0,
                               max_nodes=None, return_info=False):
        """the node rows of the reference's SEAL path WITH its per-hop neighbour caps: k_hop_subgraph's sample_ratio and
        max_nodes_per_hop (src/datasets/seal.py:291-348), restated deterministically and run for a whole batch of links on the GPU
        (sampled_nodes.py, csrc/ss_sampled_nodes.hip).  Where exact_subgraph_nodes(max_nodes=...) EMPTIES the row of a
        link near a hub, this keeps a uniform sample of every hop and expands only what it kept.  One joint walk from {u, v}, h =
        max_hash_hops, over the in-arcs of edge_index (on a symmetric graph: the neighbours):
            visited = kept_0 = {u, v} (u == v: one root);  for hop = 1 .. h:
                fringe = in-neighbours(kept_{hop-1}) - visited;  visited |= fringe -- the WHOLE fringe: a node that is rejected never
                    comes back at a later hop, as in the reference
                F = |fringe|;  m = F if ratio_per_hop == 1.0 else int(ratio_per_hop * F);  with a cap m = min(m, max_nodes_per_hop)
                kept_hop = the m fringe nodes with the smallest (key, id);  stop when m == 0
            key(x) = hash_u64(hash_u64(K + 0x9E3779B97F4A7C15 * hop) ^ (x + 1)),  K = hash_u64(seed ^ hash_u64(((u << 32) | v) + 1)),
            hash_u64 = the splitmix64 finaliser of the node hashes, 64-bit wrapping, u and v after the negative-id wrap
        The target link is NOT removed during the walk (the reference walks the graph with it; removing it belongs to the adjacency,
        exact_subgraphs(mask_target=True)).  The reference samples twice (ratio, then cap) with random.sample; a uniform sample of a
        uniform sample is uniform, and so is one bottom-m selection by an independent key: the same law, one stage.
        @param links, num_nodes, edge_index, batch_size: as exact_subgraph_nodes takes them (same checks, before any launch)
        @param max_nodes_per_hop: None or an integer >= 1
        @param ratio_per_hop: a real number in (0, 1]
        @param seed: an integer in [0, 2^63)
        @param max_nodes: None = no cap; otherwise a row longer than max_nodes is EMPTY and reported in info['truncated'].  With
               max_nodes_per_hop a row never exceeds 2 + h * max_nodes_per_hop
        @return: (rowptr int64 [L + 1], ids int64 [T], hop uint8 [T]) on links.device: row q ascending and unique, hop = the hop at
                 which the node joined the walk (0 for the roots: the reference's `dists`).  A row is a function of (graph, u, v, h,
                 max_nodes_per_hop, ratio_per_hop, seed) only: not of the link's position, batch_size, the kernel tier, the knobs or
                 the other links; a link that appears twice gets the same row twice.  With return_info also {'truncated',
                 'lds_links', 'large_links' (links whose VISITED set passed the on-chip table), 'sampled_links' (links where at least
                 one hop dropped a node)}.  No CPU fallback."""
        from . import sampled_nodes
        return sampled_nodes.sampled_subgraph_nodes(self, links, num_nodes, edge_index, batch_size=batch_size, max_nodes_per_hop=max_nodes_per_hop,
                                                    ratio_per_hop=ratio_per_hop, seed=seed, max_nodes=max_nodes, return_info=return_info)

    def exact_subgraphs(self, links, num_nodes, edge_index, batch_size=11000000, mask_target=True, max_nodes=None, node_label='drnl',
                        max_dist=1000, return_info=False, *, max_nodes_per_hop=None, ratio_per_hop=1.0, seed=0):
        """the labelled enclosing subgraph of every link as one disjoint-union batch: the node rows of exact_subgraph_nodes, the
        adjacency they induce and the SEAL node labels computed INSIDE each subgraph -- the object the reference's SEAL path builds
        per link in Python (k_hop_subgraph + construct_pyg_graph + labelling_tricks.py, src/datasets/seal.py:291-389), here from HIP
        kernels (subgraphs.py, csrc/ss_subgraph.hip).
        @param links, num_nodes, edge_index, batch_size, max_nodes: as exact_subgraph_nodes takes them (same checks, before any launch)
        @param mask_target: True (default, as SEAL always does) removes the link's own edge: the distance bytes are those of
               exact_subgraph_nodes(mask_target=True) and the adjacency rows of u and v do not list each other.  The node SET does
               not depend on it.  It changes nothing for a link that is no edge, or with u == v
        @param node_label: 'drnl', 'de', 'de+' (labelling_tricks.py bit for bit), 'hop' (min of the two ball distances), 'zo'
               (hop == 0) or None.  'de': z = (d_u, d_v), the BFS depths in the induced subgraph clipped to max_dist, unreachable =
               max_dist.  'de+': d_u with v removed, d_v with u removed, the removed root's own entry 1.  'drnl': those two distances
               with the removed root's entry 0, z = 1 + min(d_u, d_v) + (d // 2)(d // 2 + d % 2 - 1), d = d_u + d_v, and 1 where
               either is 0.  These depths can exceed h + 1 and differ from the ball sentinel: that is why they are computed.
               u == v is outside the reference's domain and defined here: one root, nothing removed, d_u == d_v, 'drnl' gives the
               root 1
        @param max_dist: integer in [1, 2^20]
        @param max_nodes_per_hop, ratio_per_hop, seed: (keyword only) as sampled_subgraph_nodes takes them.  With the defaults nothing
               changes.  With a cap or a ratio < 1 the node rows are those of sampled_subgraph_nodes (the target link stays in the
               WALK; mask_target still removes it from the adjacency) and the result is a subgraphs.SampledSubgraphs: hop uint8 [T] in
               place of dist (dist is None), 'hop' and 'zo' read from it, everything else as below on those rows, info with
               'sampled_links' too
        @return: subgraphs.ExactSubgraphs on links.device: rowptr / ids / dist (exactly exact_subgraph_nodes' result), roots int32 [L, 2]
                 (local indices of u and v; (-1, -1) for a row emptied by max_nodes), adj_ptr int64 [T + 1], nbr int32 [A] (per listed
                 node the local indices of the distinct nodes of its row with an arc INTO it, ascending; self loops dropped), weight
                 int32 [A] (copies of that arc in edge_index), z (int64 [T], [T, 2] or None); helpers .edge_index(), .batch(),
                 .link(q).  With return_info .info is exact_subgraph_nodes' info.  A link's rows depend on the graph, the link,
                 mask_target, node_label and max_dist only.  No CPU fallback."""
        from . import subgraphs
        return subgraphs.exact_subgraphs(self, links, num_nodes, edge_index, batch_size=batch_size, mask_target=mask_target,
                                         max_nodes=max_nodes, node_label=node_label, max_dist=max_dist, return_info=return_info,
                                         max_nodes_per_hop=max_nodes_per_hop, ratio_per_hop=ratio_per_hop, seed=seed)

    def update_hash_tables(self, hash_table, cards, num_nodes, edge_index, added=None, removed=None, copy=False, return_info=False):
        """the tables of build_hash_tables(num_nodes, old_edge_index) brought up to date with a changed edge list WITHOUT a rebuild: a
        hop-k row depends only on the closed in-neighbourhood of its node, so hop k recomputes exactly the rows within k hops downstream
        of the targets of the changed edges (plus the rows whose implicit self loop came or went because max(edge_index) moved) and
        writes nothing else (update.py, csrc/ss_update.hip).  The reference rebuilds: build_hash_tables once per split
        (src/data.py:173-176: the test split is the training graph plus the validation edges).
        @param hash_table, cards: what build_hash_tables returned for the OLD graph (or load_sketches of a packed cache of it), on the
               compute device; hops 0 .. max_hash_hops, cards float32 [num_nodes, max_hash_hops]
        @param edge_index: int64 [2, E], the graph AFTER the change -- what a rebuild would be given
        @param added, removed: int64 [2, A] / [2, R] directed edges by which the new edge list differs from the old one (both directions
               of an undirected change); only their targets (row 1) are used; at least one must be given.  Ids outside [0, num_nodes)
               are reported as build_hash_tables reports them (strict_bounds)
        @param copy: False updates the given objects in place; True clones the tables first and leaves the inputs untouched
        @param return_info: also return {'seed_rows': int, 'dirty_rows': {k: rows recomputed at hop k}, 'row_list': {k: ...},
               'hub_list': {k: ...}} (one host read, after the last launch).  'masks' adds what the marking kernels left in the
               workspace: 'dirty_mask' {k: bool [N] device tensor, the rows hop k recomputed}, and 'rows' / 'hubs' {k: int32 device
               tensor}, the listed regular rows and the listed hub rows (in-degree above the CSR's hub threshold) in list order
        @return: (table, cards[, info]): every hop table bit-identical to build_hash_tables(num_nodes, edge_index)"""
        from . import update
        return update.update_hash_tables(self, hash_table, cards, num_nodes, edge_index, added=added, removed=removed, copy=copy,
                                         return_info=return_info)

    def get_hashval(self, x):
        return x.hashvals

    def _linearcounting(self, num_zero):
        return self.m * torch.log(self.m / num_zero)

    def _estimate_bias_or_refine(self, e, refine):
        device = _compute_device(e)
        params = self._params(device)
        x = e.to(device=device, dtype=torch.float32).contiguous()
        out = torch.empty_like(x)
        _native.check(_native.lib().ss_estimate_bias(_ptr(x), x.numel(), byref(params.struct), _ptr(out), int(refine),
                                                     _stream(device)), 'ss_estimate_bias')
        return out.to(e.device)

    def _estimate_bias(self, e):
        """mean bias of the 6 table entries nearest to each estimate (reference :197-204)"""
        return self._estimate_bias_or_refine(e, False)

    def _refine_hll_count_estimate(self, estimate):
        """subtract the bias from estimates <= 5m, in place like the reference (:206-210)"""
        refined = self._estimate_bias_or_refine(estimate, True)
        estimate.copy_(refined)
        return estimate

    def hll_count(self, regs):
        """HLL++ cardinality estimate of each register row (reference :212-232).
        @param regs: integer tensor [n, m] (or [m])  @return: float32 [n] on regs.device"""
        if regs.dim() == 1:
            regs = regs.unsqueeze(dim=0)
        if regs.size(1) != self.m:
            raise ValueError(f'expected rows of {self.m} registers, got {regs.size(1)}')
        device = _compute_device(regs)
        tag = getattr(regs, '_ss_count', None)
        if tag is not None:  # produced together with `regs` by hll_prop (same kernel arithmetic); handed out once
            regs._ss_count = None
            if tag[0] == regs._version and tag[1].device == device and tag[1].numel() == regs.size(0):
                return tag[1] if regs.device == device else tag[1].to(regs.device)
        params = self._params(device)
        packed = _packed_hll_of(regs, device)
        out = torch.empty(regs.size(0), dtype=torch.float32, device=device)
        _native.check(_native.lib().ss_hll_count(_ptr(packed), regs.size(0), byref(params.struct), _ptr(out), 1,
                                                 _stream(device)), 'ss_hll_count')
        return out if regs.device == device else out.to(regs.device)

    def _hll_merge(self, src, dst):
        if src.shape != dst.shape:
            raise ValueError('source and destination register shapes must be the same')
        return torch.maximum(src, dst)

    def hll_neighbour_merge(self, root, neighbours):
        all_regs = torch.cat([root.unsqueeze(dim=0), neighbours], dim=0)
        return torch.max(all_regs, dim=0)[0]

    def minhash_neighbour_merge(self, root, neighbours):
        all_regs = torch.cat([root.unsqueeze(dim=0), neighbours], dim=0)
        return torch.min(all_regs, dim=0)[0]

    def jaccard(self, src, dst):
        """minhash Jaccard estimate of [n_edges, num_perm] hash-value tensors (reference :247-256)"""
        if src.shape != dst.shape:
            raise ValueError('source and destination hash value shapes must be the same')
        return torch.count_nonzero(src == dst, dim=-1) / self.num_perm

    def get_subgraph_features(self, links, hash_table, cards, batch_size=11000000, degrees=None, lazy=False, out=None, mask_target=None,
                              return_debug=False):
        """structural features of node pairs: approximations of the number of nodes at distance (d_u, d_v)
        from (u, v), for the (d_u, d_v) listed in LABEL_LOOKUP[max_hops] (reference :258-323).
        @param links: int tensor [n_edges, 2] (or [2])
        @param hash_table: {hop: {'hll': [N, m], 'minhash': [N, num_perm]}} (a SketchTable or plain tensors)
        @param cards: float tensor [N, max_hops] of neighbourhood cardinality estimates
        @param batch_size: pairs per kernel launch (results do not depend on it)
        @param degrees: optional float tensor [N] (HashDataset.degrees, datasets/elph.py:74).  Extension beyond the
               reference signature: when given, BUDDY's degree-normalised copy (models/elph.py:276-293: feature /
               sqrt(d_u * d_v), NaN / Inf -> 0) is appended in the same kernel and the result is [n_edges, 2 * F].
        @param lazy: extension: return a `DeviceFeatureStore` (feature_store.py) instead of the tensor -- rows are computed on
               the GPU when a batch indexes it (runners/train.py:58-60), nothing of size [n_edges, F] is materialised
        @param out: extension: a contiguous float32 [n_edges, F] tensor ON THE COMPUTE DEVICE the rows are written into (and which
               is returned): a slice of a larger result -- dist.sharded_precompute lets every launch store straight into the block
               of the output the collective then sends from
        @param mask_target: extension (masked.py, csrc/ss_masked.hip): the edge_index [2, E] (CPU or device) that
               `hash_table` and `cards` WERE BUILT ON -- nothing can check that cheaply.  Every link is then scored as if its own edge
               were absent: link (u, v) gets the features of tables built on the graph without every copy of u -> v and of v -> u
               (self loops and max(edge_index) + 1 as in the full graph), the target-link removal of the reference's SEAL path
               (src/datasets/seal.py:338).  MinHash match counts and HLL zero counts are exact, features within the engine's fp32 bar;
               a link with u == v or with neither direction present keeps the plain query's row bit for bit.  Not combinable with
               degrees, lazy or out (ValueError).  None (default): the plain query
        @param return_debug: with mask_target only: also return {'match' int32 [L, h, h], 'zeros' int32 [L, h, h], 'row_zeros' int32
               [L, 2, h], 'masked' bool [L]} -- the integers behind every row and which links were found in the graph
        @return: float32 [n_edges, max_hops * (max_hops + 2)] on links.device"""
        if mask_target is not None:
            from . import masked
            masked.check_arguments(self, links, mask_target, batch_size, degrees=degrees, lazy=lazy, out=out)
            return masked.masked_subgraph_features(self, links, hash_table, cards, mask_target, batch_size=batch_size,
                                                   return_debug=return_debug)
        if return_debug:
            raise ValueError('return_debug belongs to the masked query: give mask_target')
        if self.max_hops not in (1, 2, 3):
            raise NotImplementedError("Only 1, 2 and 3 hop hashes are implemented")
        if links.dim() == 1:
            links = links.unsqueeze(0)
        if lazy:
            from .feature_store import DeviceFeatureStore
            return DeviceFeatureStore(self, links, hash_table, cards, degrees=degrees, batch_size=batch_size)
        n = links.size(0)
        if knobs.GROUP_LINKS_MIN and n >= knobs.GROUP_LINKS_MIN and n < (1 << 31):
            feats, _ = self._pair_kernel(links, hash_table, cards, degrees=degrees, group_batch=max(int(batch_size), 1), out=out)
        elif n <= batch_size:
            feats, _ = self._pair_kernel(links, hash_table, cards, degrees=degrees, out=out)
        elif out is not None:
            for s in range(0, n, batch_size):
                self._pair_kernel(links[s:s + batch_size], hash_table, cards, degrees=degrees, out=out[s:s + batch_size])
            feats = out
        else:
            chunks = [self._pair_kernel(links[s:s + batch_size], hash_table, cards, degrees=degrees)[0]
                      for s in range(0, n, batch_size)]
            feats = torch.cat(chunks, dim=0)
        if feats.device == links.device or out is not None:
            return feats
        out = feats.to(links.device)
        # links on another device (BUDDY keeps them on the CPU): the copy back has waited for the launches, so the deferred
        # bounds report is final and can be raised from the offending call itself -- as the reference's CPU indexing does
        if self.strict_bounds == 'deferred':
            self._deferred.raise_if_set()
        return out

