#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric on BASELINE.json's config, on N MI355X of one node.

metric   : edge-pairs/sec subgraph-feature extraction (build+query)
workload : configs[1] "ogbl-collab, BUDDY, max_hash_hops=2, batch_size=65536" as a synthetic graph of the same
           shape: N=235 868 nodes, E_und=1 179 052 uniform-random undirected edges
           (seed 1, both directions -> E_dir=2 358 104), P=128, p=8, h=2; one batch of B=65 536 node pairs per step.
step     : one pass of the whole hot path over one batch: ElphHashes.build_hash_tables (CSR build, hop 1 from node ids,
           h-1 table hops with fused cardinalities) + ElphHashes.get_subgraph_features(B pairs), i.e. what ELPH does
           per training step (reference runners/train.py:198,204) and what BUDDY does once per edge set.  Nothing is
           cached between steps.  Inputs (edge_index, links) are resident in HBM.
plain run: `bench.py --gpus N --steps K --warmup W` sets up, runs the step untimed for --settle-seconds and then W warm-up steps,
           times K steps and prints the headline line (metric, value, unit, higher_is_better, dtype, ms_per_step and the keys that
           describe the run).  --dump-outputs DIR writes what the last timed step returned (dump_outputs).  Everything below that is
           not the timed region itself -- ms_per_step_cold, the roofline (HIP events inside the timed region), latency, the sustained
           run, breakdown, kernels, secondary, cpu_baseline, and at N > 1 the build probe, weak and strong figures -- runs with --full only.
N > 1    : one process per GPU (torchrun), per-batch feature rows all-gathered over RCCL (async, on RCCL's stream,
           double-buffered, every gather completed inside the timed region).
           --scaling weak (default): every rank owns its own B pairs AND repeats the whole build (table replicated):
               the N-GPU rate is ~N x by construction -- `redundant_fraction_of_step` says how much of a rank's step is
               work every rank repeats;
           --scaling strong: ONE global batch of B pairs (BASELINE configs[3] / [4] are fixed global batches sharded across
               8 GPUs), rank r computes its contiguous slice; with --build sharded the destination rows of every hop are
               split across the ranks too (in-place all-gather per hop and sketch).  value(N) / value(1) = speed-up.
           --api buddy: one build, then --buddy-links pairs in chunks of --buddy-chunk (the reference's subgraph_feature_batch_size,
               11 M: datasets/elph.py:200-208); strong scaling shards the link set.
roofline : the dominant kernel = ss::propagate_kernel<128,256>, the MinHash table hop.  achieved = algorithmic bytes per
           launch ((E'+N)*4P + 4E + 8(N+1), subgraph_sketching_amd/roofline.py) / mean launch duration measured live in
           the timed region with HIP events recorded INSIDE the library on the launch stream (subgraph_sketch_debug.h).
           `resident` says where the gathered table lives: a table <= 256 MiB sits in the Infinity Cache and the figure
           is then a fabric rate, not an HBM rate (`unique_hbm_bytes_per_launch` is what HBM itself must deliver).
           `traffic` is null: PMC counters cannot be read from inside this process; the separately collected rocprofv3
           figure is quoted under `traffic_profiled` with the file it comes from.
step_roofline : the WHOLE step against the HBM peak: bytes of the implemented schedule / ms_per_step.
kernels  : per kernel family, HIP-event launch durations measured on extra steps after the timed region.
secondary : measured in the SAME process after the timed region (so the driver witnesses more than configs[1]): the ppa- and
           citation2-like build + query steps (uniform and power-law endpoints), the ELPH call sequence at B = 2 048 and the BUDDY
           precompute at collab size -- each with ms_per_step, the dominant kernel's fraction of the HBM peak and where its
           table lives.  --no-secondary skips it.
cpu_baseline : the oracle's C port (oracle/sketch_oracle.c, OpenMP on all host cores) timed on full steps of the same
           workload, rank 0 / N=1 only; `cpu_baseline_reference_style` = the reference's dataflow in stock torch CPU ops.
"""
import argparse
import json
import math
import os
import sys
import threading
import time
from argparse import Namespace
from ctypes import byref, c_float, c_int32

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# BASELINE.json configs as synthetic shapes.  The default -- and the only one the driver's
# plain `python bench.py` measures -- is configs[1] (collab).  buddy_links = L of the BUDDY precompute.
CONFIGS = {
    'collab': dict(n=235868, e_und=1179052, h=2, batch=65536, buddy_links=2_660_000),       # configs[1] / [2]
    'cora': dict(n=2485, e_und=3550, h=2, batch=1024, buddy_links=20_000),                    # configs[0] shape (plumbing)
    'ppa': dict(n=576289, e_und=21231931, h=2, batch=131072, buddy_links=57_600_000),         # configs[3]
    'citation2': dict(n=2927963, e_und=30387995, h=3, batch=261424, buddy_links=356_000_000),  # configs[4]
}
P, HLL_P = 128, 8
N_NODES, E_UND, H, BATCH = (CONFIGS['collab'][k] for k in ('n', 'e_und', 'h', 'batch'))  # the bench shape, for the probes under tools/


def synthetic_graph(n=N_NODES, e_und=E_UND, kind='uniform', alpha=0.5, seed=1):
    rng = np.random.RandomState(seed)
    if kind == 'uniform':
        e = rng.randint(0, n, size=(2, e_und)).astype(np.int64)
    elif kind == 'local':  # edges stay within a window of ids (ids correlated with communities / time): neighbourhoods overlap
        s = rng.randint(0, n, size=e_und).astype(np.int64)
        e = np.stack([s, (s + np.rint(rng.normal(0.0, alpha, size=e_und)).astype(np.int64)) % n])
    else:  # power-law endpoint weights w_i ~ (i+1)^-alpha (Chung-Lu style): exercises hub rows
        w = np.arange(1, n + 1, dtype=np.float64) ** -alpha
        cdf = np.cumsum(w / w.sum())
        e = np.stack([np.searchsorted(cdf, rng.random_sample(e_und)), rng.randint(0, n, size=e_und)]).astype(np.int64)
        e = np.minimum(e, n - 1)
    return np.concatenate([e, e[::-1]], axis=1)


def synthetic_links(n=N_NODES, batch=BATCH, seed=2):
    return np.random.RandomState(seed).randint(0, n, size=(batch, 2)).astype(np.int64)


def cpu_baseline(ei, links, n, h, batch):
    """oracle C port (OpenMP) on full steps; returns the cpu_baseline object and the features of the last step"""
    import subgraph_sketching_amd as ssa
    from oracle import oracle
    t = ssa.hll_tables.load(HLL_P)
    prm = oracle.HllParams(t.p, t.threshold, t.raw_estimate, t.bias, alpha=t.alpha,
                           lc_table=ssa.hashing.linear_counting_table(1 << t.p).numpy())
    cores = os.cpu_count()
    oracle.lib()
    # a bounded sample of the same workload: full steps until ~10 s of CPU time have gone by (at least 5, at most 200 steps)
    reps, t_build, t_query = 0, 0.0, 0.0
    while reps < 5 or (t_build + t_query < 10.0 and reps < 200):
        reps += 1
        t0 = time.perf_counter()
        rowptr, col = oracle.csr_build(n, ei)
        n_self = int(ei.max()) + 1
        mh, hll = oracle.minhash_init(n, P), oracle.hll_init(n, HLL_P)
        tables, cards = {0: {'minhash': mh, 'hll': hll}}, np.zeros((n, h), dtype=np.float32)
        for k in range(1, h + 1):
            mh, hll, c = oracle.propagate_csr(n, rowptr, col, n_self, mh, hll, prm)
            tables[k] = {'minhash': mh, 'hll': hll}
            cards[:, k - 1] = c
        t1 = time.perf_counter()
        feats = oracle.pair_features(links, tables, cards, h, prm)
        t2 = time.perf_counter()
        t_build += t1 - t0
        t_query += t2 - t1
    return {'value': reps * batch / (t_build + t_query), 'unit': 'pairs/s', 'cores': cores, 'kind': 'port',
            'sample': f'{reps} full steps (build N={n}, E_dir={ei.shape[1]}, h={h} + {batch} pairs each); mean '
                      f'build {t_build / reps:.2f} s, query {t_query / reps:.3f} s; C/OpenMP restatement of the reference, '
                      f'not the torch/PyG code itself'}, feats


def cpu_baseline_reference_style(ei, links, n, h, batch):
    """the reference's dataflow in stock torch CPU ops (oracle/torch_refstyle.py): materialised per-edge messages +
    scatter-amax, int64 MinHash, h^2 x 4 row gathers, argsort-based bias lookup.  One full step (all h hops + the query of
    one batch) is timed.  Calibration against the real (shimmed) reference: profiles/round2_cpu_baseline_calibration.json."""
    import subgraph_sketching_amd as ssa
    from oracle import torch_refstyle as tr
    t = ssa.hll_tables.load(HLL_P)
    raw, bias = torch.tensor(t.raw_estimate, dtype=torch.float), torch.tensor(t.bias, dtype=torch.float)
    threads = min(16, os.cpu_count())  # measured best on the 256-core GPU host (8: 3.5 s/hop, 16: 2.5, 32: 3.0, 128: 6.0)
    torch.set_num_threads(threads)
    t0 = time.perf_counter()
    mh0, hll0 = tr.init_sketches(n, P, HLL_P)  # the reference makes the hop-0 sketches on the host inside its build (hashing.py:157-158)
    tables, cards = tr.build_tables(n, torch.from_numpy(ei), h, mh0, hll0, HLL_P, t.alpha, t.threshold, raw, bias, hops_to_run=h)
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    tr.pair_intersections(torch.from_numpy(links), tables, h, P, HLL_P, t.alpha, t.threshold, raw, bias)
    t_query = time.perf_counter() - t0
    return {'value': batch / (t_build + t_query), 'unit': 'pairs/s', 'cores': threads, 'kind': 'port',
            'sample': f'reference-style torch CPU ops, 1 full step: {h}-hop build {t_build:.2f} s + '
                      f'{batch}-pair query ({t_query:.3f} s); torch threads = {torch.get_num_threads()}'}


def profiled_traffic(shape_key, family):
    """fabric bytes per launch of a kernel family on a shape, from the tracked PMC passes (profiles/pmc_traffic.json["shapes"],
    written by tools/summarise_prof.py --shape from separate rocprofv3 --pmc runs of this command), or None"""
    path = os.path.join(ROOT, 'profiles', 'pmc_traffic.json')
    if not os.path.exists(path):
        return None
    with open(path) as fh:
        entry = json.load(fh).get('shapes', {}).get(shape_key)
    if not entry or family not in entry:
        return None
    return {'bytes_per_launch': entry[family], 'file': entry.get('file', 'profiles/pmc_traffic.json')}


def shape_key(config, graph, alpha):
    return f'{config}_uniform' if graph == 'uniform' else f'{config}_{graph}{int(round(alpha * 10)):02d}'


def roofline_numbers(rf, bytes_alg, launch_ms, table_bytes, traffic):
    """fraction of the HBM peak for one kernel family, and the rate of the row-gather micro-benchmark for a table of that size beside
    it.  The bytes the fraction is taken on are the algorithmic bytes, CAPPED at the bytes the PMC passes saw crossing the fabric
    when those are fewer: a row kernel on a skewed graph reads the same source rows again and again, and the repeats are served by
    the L2 -- they are not memory traffic, and counting them gave fractions above 1.  The micro-benchmark figure
    is a reference point, NOT a ceiling (round 4 clamped a `frac_of_ceiling` at 1 when a kernel beat it by 0.3 - 0.9 %: a probe a
    kernel beats bounds nothing) -- the only fraction printed is the one of the 8 TB/s peak."""
    if not launch_ms:
        return {}
    basis, note = bytes_alg, 'algorithmic bytes'
    if traffic and traffic["bytes_per_launch"] < 0.97 * bytes_alg:  # (within 3 %: counter calibration, not repeats -- algorithmic bytes stand)
        basis, note = traffic['bytes_per_launch'], f"fabric bytes of the PMC passes ({traffic['file']}): fewer than the algorithmic bytes, repeats served by the L2"
    achieved = basis / (launch_ms * 1e-3) / 1e9
    return {'achieved_gbs': achieved, 'frac_of_hbm_peak': achieved / rf.HBM_PEAK_GBS, 'bytes_basis': note,
            'gather_probe_gbs': rf.gather_probe_gbs(table_bytes),
            'gather_probe_note': 'rate of random 512-byte-row gathers (ids read, rows gathered) from a table of this size, tools/micro/gather_ceiling.hip '
                                 '(profiles/round4_gather_ceiling.txt, id bytes counted): a reference point for this access pattern, not a bound'}


def emit(out):
    """print the ONE line.  Order: the contract's keys, then a compact summary of the secondary shapes (name -> ms_per_step, fraction of
    the HBM peak of the dominant kernel, where its table lives) -- the long objects come last, so that a reader who keeps only the
    head of the line (the driver's record does) still sees the ELPH step and the HBM-resident shapes"""
    head = ['metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'ms_per_step_cold', 'higher_is_better', 'scaling', 'vs_baseline',
            'dtype', 'data', 'settle_seconds', 'settle_steps', 'rccl_ranks', 'backend', 'build', 'build_probe_ms_per_step', 'build_fastest']
    line = {k: out[k] for k in head if k in out}
    if 'secondary' in out:
        line['secondary_summary'] = {name: ({'ms_per_step': round(row['ms_per_step'], 4),
                                             'frac': round(row['dominant_frac_of_hbm_peak'], 3) if row.get('dominant_frac_of_hbm_peak') else None,
                                             'kernel': row.get('dominant_kernel'), 'resident': row.get('resident'),
                                             'Mpairs_per_s': round(row['pairs_per_s'] / 1e6, 1)}
                                            if isinstance(row, dict) and 'ms_per_step' in row else row)
                                     for name, row in out['secondary'].items() if name != 'note'}
    for k in ('configs_3_4_strong', 'latency_one_step_ms', 'weak', 'same_work_speedup'):
        if k in out:
            line[k] = out[k]
    line.update({k: v for k, v in out.items() if k not in line})
    print(json.dumps(line), flush=True)


DUMP_MAX_BYTES = 64 << 20  # --dump-outputs: all files together
DUMP_TABLE_ROWS = 2048     # rows of every hop's MinHash / HLL table written (the same rows for every hop)


def sample_rows(n_rows, row_bytes, max_bytes, seed):
    """None (every row) when n_rows rows fit in max_bytes, else a fixed, seeded, sorted sample of row indices that fits together with
    its own float64 index"""
    if n_rows * row_bytes <= max_bytes:
        return None
    k = min(n_rows, max(1, max_bytes // (row_bytes + 8)))
    return np.sort(np.random.RandomState(seed).choice(n_rows, size=k, replace=False))


def dump_outputs(path, feats, table, cards):
    """--dump-outputs: what the last timed step handed its caller -- the feature rows of get_subgraph_features, the cardinalities and the
    per-hop MinHash / HLL tables of build_hash_tables (the reference-shaped int64 / int8 leaves) -- as DIR/<name>.npy in float32, or in
    float64 for the uint32 MinHash values (exact).  An array above its share of DUMP_MAX_BYTES is a fixed, seeded sample of its rows,
    whose indices are written beside it as <name>_rows.npy; the inputs of a run are fixed by its arguments, so two builds of the project
    can be compared file by file."""
    os.makedirs(path, exist_ok=True)
    arrays = {}

    def put(name, t, dtype, idx):
        if idx is not None:
            t = t[torch.from_numpy(idx).to(t.device)]
            arrays[f'{name}_rows'] = idx.astype(np.float64)
        arrays[name] = t.cpu().numpy().astype(dtype)

    put('features', feats, np.float32, sample_rows(feats.shape[0], 4 * feats[0].numel(), 20 << 20, 11))
    put('cards', cards, np.float32, sample_rows(cards.shape[0], 4 * cards[0].numel(), 12 << 20, 12))
    n = cards.shape[0]
    rows = np.sort(np.random.RandomState(13).choice(n, size=DUMP_TABLE_ROWS, replace=False)) if n > DUMP_TABLE_ROWS else None
    if rows is not None:
        arrays['table_rows'] = rows.astype(np.float64)
    sel = torch.from_numpy(rows if rows is not None else np.arange(n))
    for k in sorted(table):
        arrays[f'minhash_hop{k}'] = table[k]['minhash'][sel.to(table[k]['minhash'].device)].cpu().numpy().astype(np.float64)
        arrays[f'hll_hop{k}'] = table[k]['hll'][sel.to(table[k]['hll'].device)].cpu().numpy().astype(np.float32)
    total = sum(x.nbytes for x in arrays.values())
    assert total <= DUMP_MAX_BYTES, f'--dump-outputs: {total} bytes exceed {DUMP_MAX_BYTES}'
    for name, x in arrays.items():
        np.save(os.path.join(path, f'{name}.npy'), x)
    print(f'dump-outputs: {len(arrays)} arrays, {total / 2**20:.1f} MiB -> {path}', file=sys.stderr, flush=True)


def resident_label(rf, table_bytes):
    """where the gathered table lives, from the share of it the 256 MiB Infinity Cache can hold: all of it / most of it / little of it"""
    return rf.resident_label(table_bytes)


# the rows above the hub threshold are walked as hub units by leading workgroups of the row launches (csrc/ss_hub.hpp); SS_HUB_LAUNCHES=1
# brings back the launches of their own of rounds 1-3 -- the byte model follows (roofline.kernel_bytes `hosted`)
HUB_UNITS_HOSTED = os.environ.get('SS_HUB_LAUNCHES', '0') in ('', '0')


def hub_stats(ssa, ei_np, n):
    """(hub_edges, hub_rows) under the hub threshold a build of this graph uses: the rows the row kernels leave to the hub passes"""
    thr = ssa.hashing.HUB_THRESHOLD if ssa.hashing.HUB_THRESHOLD is not None else ssa.hashing.default_hub_threshold(ei_np.shape[1])
    return ssa.roofline.hub_split(np.bincount(ei_np[1], minlength=n), thr)


def secondary_case(ssa, dev, name, config, graph='uniform', alpha=0.5, api='build_query', batch=None, min_seconds=0.5, warmup=10):
    """one more shape / call style, timed after the headline's region: the same step functions, the same fences, the dominant
    kernel's HIP-event spans from inside the library; returns a small dict.  >= 10 warm-up steps, then a timed loop of at least
    `min_seconds` (5 steps after 2 warm-ups printed 0.279 ms for an ELPH step that takes 0.24: VERDICT r3 weak #7)"""
    rf, nat = ssa.roofline, ssa._native
    lib = nat.lib()
    cfg = CONFIGS[config]
    n, e_und, h = cfg['n'], cfg['e_und'], cfg['h']
    batch = batch or cfg['batch']
    e_dir = 2 * e_und
    eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=HLL_P, minhash_num_perm=P, floor_sf=False, use_zero_one=True))
    ei_np = synthetic_graph(n, e_und, graph, alpha)
    n_links = min(cfg['buddy_links'], 64 * batch) if api == 'buddy' else batch
    links = torch.from_numpy(synthetic_links(n, n_links)).to(dev)
    ei = torch.from_numpy(ei_np).to(dev)
    hub_e, hub_n = hub_stats(ssa, ei_np, n)
    del ei_np
    state = {}

    def step():
        if api == 'elph':
            loops = torch.arange(n, device=dev).repeat(2, 1)
            hei = torch.cat([ei, loops], dim=1)
            if 'mh0' not in state:
                state['mh0'], state['hll0'] = eh.initialise_minhash(n), eh.initialise_hll(n)
            table = {0: {'minhash': state['mh0'], 'hll': state['hll0']}}
            cards = torch.zeros((n, h), device=dev)
            for k in range(1, h + 1):
                table[k] = {'hll': eh.hll_prop(table[k - 1]['hll'], hei), 'minhash': eh.minhash_prop(table[k - 1]['minhash'], hei)}
                cards[:, k - 1] = eh.hll_count(table[k]['hll'])
            return eh.get_subgraph_features(links, table, cards)
        table, cards = eh.build_hash_tables(n, ei)
        return eh.get_subgraph_features(links, table, cards, batch_size=11000000)

    for _ in range(warmup):
        step()
    # dominant kernel: the MinHash table hop, except where it does not run in full (ELPH: the query's rows only) or the link
    # set dwarfs the build (BUDDY: the query)
    if api == 'buddy':
        tag, family = nat.PROF_PAIRS, 'pair_features'
    elif api == 'elph' and ssa.hashing.DEFER_TABLE_HOP and ssa.hashing.LAZY_MINHASH and h == 2:
        tag, family = nat.PROF_FUSED, 'fused_first_hop_hll_hop'
    else:
        tag, family = nat.PROF_MINHASH_HOP, 'minhash_hop'
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(3):
        step()
    torch.cuda.synchronize(dev)
    steps = max(5, int(math.ceil(min_seconds / max((time.perf_counter() - t0) / 3, 1e-6))))
    lib.ss_profile_enable(1 << tag)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    ms = 1e3 * (time.perf_counter() - t0) / steps
    dom_ms, dom_n = c_float(), c_int32()
    lib.ss_profile_read(tag, byref(dom_ms), byref(dom_n))
    lib.ss_profile_enable(0)
    eh.check_errors()
    per_launch = links.size(0) if api == 'buddy' and links.size(0) <= 11000000 else batch
    bytes_ = rf.kernel_bytes(n, e_dir + (n if api == 'elph' else 0), P, HLL_P, h, per_launch, hub_e, hub_n, HUB_UNITS_HOSTED)[family]
    survey = None
    H = ssa.hashing
    if api == 'buddy' and H.GROUP_LINKS_MIN and links.size(0) >= H.GROUP_LINKS_MIN and links.size(0) <= 11000000:
        # the precompute walks its links grouped by their first node: that node's rows are fetched once per run of pairs, not
        # once per pair -- the roofline fraction is taken on the bytes this walk has to move; the 2h-rows-per-pair figure of
        # SURVEY 8(d) (which such a walk beats by construction: 1.18 "of peak" at this size) is kept beside it
        runs = int(torch.unique(links[:, 0]).numel())
        survey = {'bytes': bytes_, 'equivalent_gbs': bytes_ / (dom_ms.value * 1e-3) / 1e9 if dom_ms.value else None,
                  'note': '2h table rows per pair (SURVEY 8(d)); the grouped walk fetches the first node\'s rows once per run, so this '
                          'many bytes are NOT moved: a rate on them is a cross-check of the walk, not a fraction of a ceiling'}
        bytes_ = rf.pair_bytes_grouped(links.size(0), runs, P, HLL_P, h)
    table_bytes = rf.gathered_table_bytes(n, family, P, HLL_P, h)
    traffic = profiled_traffic(shape_key(config, graph, alpha) + ('' if api == 'build_query' else f'_{api}'), family)
    roof = roofline_numbers(rf, bytes_, dom_ms.value, table_bytes, traffic)
    frac = roof.get('frac_of_hbm_peak')
    return {'name': name, 'config': config, 'graph': graph if graph == 'uniform' else f'{graph} (endpoint weights ~ rank^-{alpha})',
            'api': api, 'num_nodes': n, 'directed_edges': e_dir, 'max_hash_hops': h, 'pairs_per_step': links.size(0),
            'ms_per_step': ms, 'pairs_per_s': links.size(0) / (ms * 1e-3), 'steps': steps,
            'dominant_kernel': family, 'dominant_mean_launch_ms': dom_ms.value, 'dominant_launches': dom_n.value,
            'dominant_algorithmic_bytes': bytes_, 'dominant_traffic_bytes': traffic['bytes_per_launch'] if traffic else None,
            'dominant_frac_of_hbm_peak': frac, 'dominant_bytes_basis': roof.get('bytes_basis'),
            'gather_probe_gbs': roof.get('gather_probe_gbs'),
            'hub_rows': hub_n, 'hub_edge_share': hub_e / e_dir,
            'resident': resident_label(rf, table_bytes),
            'cache_resident_fraction': rf.cache_resident_fraction(table_bytes),
            **({'survey_definition': survey, 'source_runs': runs} if survey else {})}


def strong_scaling_figures(ssa, eh, dist, dev, n, h, ei, cfg, batch, world, rank, reps=3, with_peer=False):
    """after the timed region, N > 1: t(1 GPU) and t(N GPUs) of the same two jobs, max over ranks; see the call site"""
    nf = h * (h + 2)
    L = min(cfg['buddy_links'], 64 * batch)
    links_all = torch.from_numpy(synthetic_links(n, L, 2)).to(dev)  # the SAME link set on every rank
    exchange = ssa.dist.choose_exchange(dev)

    def timed(fn):
        fn()
        torch.cuda.synchronize(dev)
        dist.barrier()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize(dev)
        t = torch.tensor([(time.perf_counter() - t0) / reps], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item()) * 1e3

    def job(links, build, sharded_query):
        table, cards = build()
        if sharded_query:
            return ssa.dist.sharded_subgraph_features(lambda lk: eh.get_subgraph_features(lk, table, cards), links)
        return eh.get_subgraph_features(links, table, cards)

    replicated = lambda: eh.build_hash_tables(n, ei)
    sharded = lambda: ssa.dist.sharded_build_hash_tables(eh, n, ei)
    builds = [('replicated_build', replicated), ('sharded_build', sharded)]
    res = {'exchange': exchange, 'exchange_probe_seconds': ssa.dist.exchange_probe_times(dev), 'world': world}
    if with_peer:
        # peer-write: the ranks map each other's tables (CUDA-IPC) and store into them from inside the kernels.  PeerShard's
        # constructor asks hipDeviceCanAccessPeer for every peer and probes every mirror with a store + read-back before any kernel
        # uses it, and fails on every rank or on none -- then the figures simply lack this build.
        try:
            shard = ssa.dist.PeerShard(n, eh.max_hops, eh.num_perm, eh.m, dev)
            builds.append(('peer_write_build', lambda: ssa.dist.peer_write_build_hash_tables(eh, n, ei, shard=shard)[:2]))
        except Exception as exc:
            res['peer_write_build_unavailable'] = f'{type(exc).__name__}: {exc}'
    else:
        res['peer_write_build'] = 'not measured (over RCCL the peer-write build is opt-in: --strong-peer; see its help)'
    for name, links in (('buddy_precompute', links_all), ('build_plus_one_global_batch', links_all[:batch])):
        t1 = timed(lambda: job(links, replicated, False))
        row = {'pairs': links.size(0), 'ms_1gpu_same_work': t1}
        for bname, build in builds:
            tn = timed(lambda: job(links, build, True))
            row[bname] = {'ms': tn, 'speedup_vs_n1_same_work': t1 / tn, 'pairs_per_s': links.size(0) / (tn * 1e-3)}
        res[name] = row
    res['note'] = ('same job on 1 GPU (every rank runs all of it, no communication) vs sharded over the ranks: links cut into contiguous '
                   'slices, feature rows all-gathered; build replicated on every rank or destination rows sharded with an in-place exchange '
                   'per hop and sketch.  At ogbl-collab size the build is 0.4 ms and the exchange costs more than it saves (DESIGN 6); '
                   '--config ppa / citation2 --scaling strong --build sharded are the shapes it is for.')
    return res


def device_links(n, count, dev, seed=2):
    """`count` pairs of node ids in [0, n), a pure integer function of (seed, position) evaluated on the device: every rank of a job
    draws the SAME link set without 5.7 GB of host memory per rank (ogbl-citation2: 356 M links) and without trusting two random
    generators to agree"""
    x = torch.arange(2 * count, dtype=torch.int64, device=dev) + seed * 0x2545F491
    for mult, shift in ((0x9E3779B97F4A7C15 - (1 << 64), 29), (0xBF58476D1CE4E5B9 - (1 << 64), 32)):  # (int64 products wrap like uint64 ones)
        x = x * mult
        x = x ^ ((x >> shift) & ((1 << (64 - shift)) - 1))  # logical shift
    return torch.remainder(x & 0x7FFFFFFFFFFFFFFF, n).view(count, 2)


def configs_3_4_strong(ssa, dist, dev, world, rank, reps=2, with_peer=False, links_cap=None, only=None):
    """BASELINE configs[3] (ogbl-ppa, h = 2) and configs[4] (ogbl-citation2, h = 3) as the jobs north_star means by "8 GPUs": the BUDDY
    feature precompute of the WHOLE link set (one build_hash_tables + get_subgraph_features over every link, reference
    datasets/elph.py:200-213) on one GPU (every rank runs all of it, nothing exchanged) against the same job over the N ranks:
    destination rows of every hop sharded (exchange form of dist.choose_exchange; peer-write with --strong-peer), links sharded, and
    the feature rows handled by each gather mode of dist.sharded_precompute --
      none : every rank keeps the rows of its share (a data-parallel training loop reads its own shard);
      rank0: group rank 0 ends with the [L, F] tensor (the rank that writes the feature cache);
      all  : every rank ends with it (the reference's single-process semantics) -- (N - 1) / N of L * F * 4 bytes arrive at every rank,
             round by round under the next round's launches (LinkRounds), not as one collective after the job.
    Times are the max over ranks behind a barrier + synchronise; speedup = t(1 GPU) / t(N GPUs) of the SAME job."""
    out = {'world': world, 'reps': reps,
           'note': 'strong scaling of the BUDDY precompute at ogbl-ppa / ogbl-citation2 size (synthetic uniform graph, links a device-side integer '
                   'hash of their position -- identical on every rank); build + every link, nothing cached; speedup vs the same job on ONE GPU'}
    exchange = ssa.dist.choose_exchange(dev) if dist.get_backend() == 'nccl' else 'all_gather (host-staged: not RCCL)'
    out['exchange'] = exchange

    def timed(fn):
        fn()
        torch.cuda.synchronize(dev)
        dist.barrier()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize(dev)
        t = torch.tensor([(time.perf_counter() - t0) / reps], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item()) * 1e3

    t_start = time.perf_counter()

    def progress(msg):  # (stderr, rank 0: where a run that is cut short by the watchdog got to)
        if rank == 0 and os.environ.get('SS_BENCH_VERBOSE', '1') != '0':
            print(f'[configs_3_4_strong +{time.perf_counter() - t_start:6.1f} s] {msg}', file=sys.stderr, flush=True)

    for name in ('ppa', 'citation2'):
        if only and name not in only:
            continue
        cfg = CONFIGS[name]
        n, h = cfg['n'], cfg['h']
        nf = h * (h + 2)
        L = min(cfg['buddy_links'], links_cap) if links_cap else cfg['buddy_links']
        eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=HLL_P, minhash_num_perm=P, floor_sf=False, use_zero_one=True))
        ei = torch.from_numpy(synthetic_graph(n, cfg['e_und'])).to(dev)
        links = device_links(n, L, dev)
        row = {'config': f'BASELINE configs[{3 if name == "ppa" else 4}]: ogbl-{name}-like, h = {h}', 'links': L, 'num_nodes': n,
               'directed_edges': 2 * cfg['e_und'], 'feature_bytes': L * nf * 4,
               'bytes_received_per_rank_gather_all': (world - 1) * L * nf * 4 // world,
               'links_per_round_and_rank': ssa.dist.default_link_block(L, world)}

        def one_gpu():
            table, cards = eh.build_hash_tables(n, ei)
            return eh.get_subgraph_features(links, table, cards)
        progress(f'{name}: graph + {L} links on the device')
        row['ms_1gpu_same_work'] = timed(one_gpu)
        row['pairs_per_s_1gpu'] = L / (row['ms_1gpu_same_work'] * 1e-3)
        progress(f'{name}: one GPU {row["ms_1gpu_same_work"]:.2f} ms')
        builds = [('replicated_build', lambda: eh.build_hash_tables(n, ei)), ('sharded_build', lambda: ssa.dist.sharded_build_hash_tables(eh, n, ei))]
        shard_box = {}
        if with_peer:
            try:
                progress(f'{name}: mapping the peers\' tables (PeerShard)')
                shard_box['s'] = ssa.dist.PeerShard(n, eh.max_hops, eh.num_perm, eh.m, dev)
                progress(f'{name}: mapped')
                builds.append(('peer_write_build', lambda: ssa.dist.peer_write_build_hash_tables(eh, n, ei, shard=shard_box['s'])[:2]))
            except Exception as exc:
                row['peer_write_build_unavailable'] = f'{type(exc).__name__}: {str(exc)[:200]}'
        row['variants'] = {}
        for bname, build in builds:
            for gather in ('none', 'rank0', 'all'):
                def job():
                    table, cards = build()
                    return ssa.dist.sharded_precompute(eh, links, table, cards, gather=gather)
                try:
                    tn = timed(job)
                    row['variants'][f'{bname}+gather_{gather}'] = {'ms': tn, 'speedup_vs_1gpu_same_work': row['ms_1gpu_same_work'] / tn,
                                                                  'pairs_per_s': L / (tn * 1e-3)}
                    progress(f'{name}: {bname} + gather {gather}: {tn:.2f} ms')
                except Exception as exc:  # (deterministic failures are the same on every rank)
                    row['variants'][f'{bname}+gather_{gather}'] = {'error': f'{type(exc).__name__}: {str(exc)[:200]}'}
        ok = {k: v for k, v in row['variants'].items() if 'ms' in v}
        for gather in ('none', 'rank0', 'all'):
            cands = {k: v for k, v in ok.items() if k.endswith('gather_' + gather)}
            if cands:
                best = min(cands, key=lambda k: cands[k]['ms'])
                row[f'best_gather_{gather}'] = dict(cands[best], variant=best)
        out[name] = row
        eh.check_errors()
        del ei, links, eh, shard_box, builds
        torch.cuda.empty_cache()
    return out


SECONDARY = [
    # (name, config, graph, alpha, api, batch): BASELINE configs[3] / [4] as SURVEY 8(d) asks -- U and PL at the same N, E --,
    # configs[2] (the ELPH message-passing step at the reference's batch size), BUDDY's precompute at collab size
    ('ppa_uniform', 'ppa', 'uniform', 0.5, 'build_query', None), ('ppa_powerlaw', 'ppa', 'powerlaw', 0.5, 'build_query', None),
    ('citation2_uniform', 'citation2', 'uniform', 0.5, 'build_query', None),
    ('citation2_powerlaw', 'citation2', 'powerlaw', 0.5, 'build_query', None),
    ('collab_powerlaw05', 'collab', 'powerlaw', 0.5, 'build_query', None), ('collab_powerlaw09', 'collab', 'powerlaw', 0.9, 'build_query', None),
    ('collab_elph_b2048', 'collab', 'uniform', 0.5, 'elph', 2048), ('collab_buddy', 'collab', 'uniform', 0.5, 'buddy', None),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    # defaults: 200 timed steps of ~0.45 ms behind 20 warm-up steps -- 20 / 3 gave 0.456-0.461 ms from run to run on one box, 200 / 20 gives
    # 0.4484 / 0.4485 (clocks and caches settled; the timed region is still only 90 ms)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--time-every', type=int, default=None,
                    help='HIP events around every n-th launch of the dominant kernel inside the timed region (default: every launch up to '
                         '50 steps -- five samples were thin, VERDICT r4 #7e -- else every 4th: a timed launch costs its step ~5 us)')
    ap.add_argument('--settle-seconds', type=float, default=2.0,
                    help='run the step untimed for this long BEFORE the warm-up steps: a fresh process finds the GPU at idle clocks, and a few '
                         'milliseconds of warm-up do not bring it to the state every later step of a job runs in (reported in the line)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--config', default='collab', choices=sorted(CONFIGS), help='synthetic shape (default: BASELINE configs[1])')
    ap.add_argument('--graph', default='uniform', choices=['uniform', 'powerlaw', 'local'])
    ap.add_argument('--alpha', type=float, default=0.5, help='power-law exponent of the endpoint weights; --graph local: standard deviation of dst - src')
    ap.add_argument('--batch', type=int, default=None, help='pairs per query batch (default: the config\'s)')
    ap.add_argument('--api', default='build_query', choices=['build_query', 'elph', 'buddy'],
                    help='build_query (default, the BASELINE metric): build_hash_tables + get_subgraph_features per step; '
                         'elph: the exact call sequence of ELPH.forward (models/elph.py:186-213) + one query per step; '
                         'buddy: one build amortised over --buddy-links pairs (datasets/elph.py:200-208)')
    ap.add_argument('--buddy-chunk', type=int, default=11000000,
                    help='pairs per get_subgraph_features launch in --api buddy (default: the reference\'s --subgraph_feature_batch_size, '
                         'runners/run.py:238)')
    ap.add_argument('--buddy-links', type=int, default=None,
                    help='pairs per BUDDY precompute (default: min(the config\'s L, 64 batches)); a step = the build + all of them')
    ap.add_argument('--buddy-negs', type=int, default=0,
                    help='--api buddy: link set in evaluation style -- this many pairs per source node, listed together (ogbl-citation2: '
                         '1 000 negatives per source); 0 (default) = pairs drawn uniformly at random')
    ap.add_argument('--scaling', default='strong', choices=['weak', 'strong'],
                    help='strong (default; identical to weak at N = 1): ONE global batch / link set sharded across the ranks -- the same '
                         'job on N GPUs (BASELINE configs[3], [4], north_star); weak: every rank its own batch and a replicated build (N x '
                         'by construction) -- at N > 1 the default line carries it as the secondary key `weak`')
    ap.add_argument('--build', default='auto', choices=['auto', 'replicated', 'sharded', 'peer'],
                    help='N > 1 only. auto (default): the fastest of the three on this node, measured on a few steps before the timed '
                         'region (the line says which and prints the probe); replicated: every rank builds the whole table; sharded: destination rows split '
                         'across ranks + in-place all-gather after every hop (pays off at ogbl-ppa / citation2 sizes); peer: the same row split, '
                         'every rank\'s kernels store their rows straight into all ranks\' (IPC-mapped) tables: no exchange step')
    ap.add_argument('--sustain-seconds', type=float, default=8.0,
                    help='length of the sustained run after the timed region (0 = skip); long enough for a 5 s utilisation sampler')
    ap.add_argument('--strong-peer', action='store_true',
                    help='N > 1 over RCCL: include the peer-write build (ranks map each other\'s tables through CUDA-IPC and store into them from '
                         'inside kernels) in the build probe and the strong-scaling figures.  Opt-in there: it has only ever met processes sharing '
                         'ONE GPU, and a store through a mapping that does not work faults the process -- which would cost the run its line; the '
                         'exchange form can only hang, and the watchdog covers that.  (With the gloo test hooks it is on by default.)')
    ap.add_argument('--no-strong-peer', action='store_true', help='N > 1: leave the peer-write build out everywhere')
    ap.add_argument('--strong-timeout', type=float, default=420.0, help='N > 1: seconds the strong-scaling figures may take before the line is printed without them')
    ap.add_argument('--no-configs-3-4', action='store_true', help='N > 1: skip `configs_3_4_strong` (the ppa- / citation2-size BUDDY precomputes, strong-scaled)')
    ap.add_argument('--strong-links-cap', type=int, default=int(os.environ.get('SS_BENCH_STRONG_LINKS', '0')) or None,
                    help='N > 1: cap on the links of a `configs_3_4_strong` precompute (default: the config\'s full link set over RCCL; 1 M with the '
                         'gloo test hooks, whose gathers go through the host)')
    ap.add_argument('--no-strong', action='store_true', help='N > 1: skip the strong-scaling figures measured after the timed region')
    ap.add_argument('--no-secondary', action='store_true', help='skip the `secondary` shapes measured after the timed region')
    ap.add_argument('--no-kernel-table', action='store_true', help='skip the per-kernel HIP-event table (extra steps after the timed region)')
    ap.add_argument('--full', action='store_true',
                    help='everything beyond the headline: the cold figure, the roofline of the dominant kernel (HIP events inside the timed '
                         'region), latency, sustained run, breakdown, kernel table, secondary shapes, CPU baselines and the N > 1 build probe, '
                         'weak and strong figures.  Without it a run sets up, warms up, times --steps steps and prints the headline only')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step returned to its caller as DIR/<name>.npy (float32 / float64, '
                         'at most 64 MB: arrays larger than their share are a fixed, seeded sample of rows, whose indices go to <name>_rows.npy)')
    a = ap.parse_args()
    cfg = CONFIGS[a.config]
    n, e_und, h = cfg['n'], cfg['e_und'], cfg['h']
    batch = a.batch or cfg['batch']
    e_dir = 2 * e_und

    assert a.steps > 0 and a.warmup >= 0, '--steps must be positive and --warmup non-negative'
    if a.time_every is None:
        a.time_every = 1 if a.steps <= 50 else 4
    if a.gpus > 1 and 'RANK' not in os.environ:
        # `python3 bench.py --gpus N` by itself (the shape of the driver's N = 1 command): this process becomes the launcher -- N ranks
        # under torch.distributed.run on a free local port, rank 0 prints the one JSON line, the exit status is non-zero if any rank dies
        import socket
        import subprocess
        with socket.socket() as sock:
            sock.bind(('127.0.0.1', 0))
            port = sock.getsockname()[1]
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(a.gpus), '--master-addr', '127.0.0.1',
               '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
        sys.exit(subprocess.run(cmd, env=env).returncode)
    if os.environ.get('SS_BENCH_DUMP_AFTER'):  # debugging aid: every rank prints its Python stack to stderr after that many seconds
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ['SS_BENCH_DUMP_AFTER']), exit=False)
    launched = 'RANK' in os.environ  # under torchrun (also with one rank, so the RCCL path can be smoke-tested)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    assert torch.cuda.is_available(), 'bench.py needs MI355X GPUs'
    # test hooks (tools/two_ranks_one_gpu.sh: the N > 1 control flow on a one-GPU box): every rank on device 0, gloo instead of RCCL
    one_device = os.environ.get('SS_BENCH_SINGLE_DEVICE') == '1'
    backend = os.environ.get('SS_BENCH_BACKEND', 'nccl')
    if one_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    dist = None
    if launched:
        import torch.distributed as dist
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=dev)
        else:
            dist.init_process_group(backend)
    assert a.gpus == world, f'--gpus {a.gpus} but WORLD_SIZE={world}: launch with torchrun --nproc-per-node {a.gpus}'

    import subgraph_sketching_amd as ssa
    from subgraph_sketching_amd import roofline as rf
    nat = ssa._native
    lib = nat.lib()  # fails loudly if the HIP engine is missing
    eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=HLL_P, minhash_num_perm=P, floor_sf=False, use_zero_one=True))
    assert eh.strict_bounds == 'deferred'  # the class default: bounds errors are reported late, no host sync inside a step
    nf = h * (h + 2)

    # BUDDY: the link set is a multiple of the batch; ONE plan / one gather covers all of it (a gather per batch would cost ~30 us
    # each, several times a rank's share of a batch at 8 GPUs); strong scaling cuts the link set into contiguous slices
    buddy_links = a.buddy_links or min(cfg['buddy_links'], 64 * batch)
    buddy_batches = max(1, math.ceil(buddy_links / batch))
    pairs_planned = batch * buddy_batches if a.api == 'buddy' else batch
    plan = ssa.dist.BatchPlan(a.scaling, world, rank, pairs_planned)
    ei_np = synthetic_graph(n, e_und, a.graph, a.alpha)
    # rows (and their in-edges) the row kernels leave to the hub passes: the byte models of --full only
    hub_e, hub_n = hub_stats(ssa, ei_np, n) if a.full else (None, None)
    links_np = synthetic_links(n, pairs_planned, plan.links_seed)
    if a.api == 'buddy' and a.buddy_negs > 0:  # every source's pairs listed together
        links_np[:, 0] = np.repeat(links_np[::a.buddy_negs, 0], a.buddy_negs)[:pairs_planned]
    ei = torch.from_numpy(ei_np).to(dev)
    links = plan.local(torch.from_numpy(links_np).to(dev)).contiguous()
    gather = ssa.dist.AsyncFeatureGather(plan, nf, dev) if launched else (lambda f: f)
    peer_state = {'shard': None}
    mode = {'build': a.build if (launched and world > 1) else 'replicated'}

    def build_tables():
        if mode['build'] == 'peer':
            table, cards, peer_state['shard'] = ssa.dist.peer_write_build_hash_tables(eh, n, ei, shard=peer_state['shard'])
            return table, cards
        if mode['build'] == 'sharded':
            return ssa.dist.sharded_build_hash_tables(eh, n, ei)
        return eh.build_hash_tables(n, ei)

    stream = torch.cuda.current_stream(dev)
    phase_marks = []
    last = {}  # --dump-outputs: the tables and cardinalities of the latest step (only kept when they are to be written)

    def keep(table, cards):
        if a.dump_outputs:
            last['table'], last['cards'] = table, cards

    def step_build_query(mark=False):
        if mark:
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record(stream)
        table, cards = build_tables()
        if mark:
            e1.record(stream)
        f = eh.get_subgraph_features(links, table, cards)
        if mark:
            e2.record(stream)
            phase_marks.append((e0, e1, e2))
        gather(f)
        keep(table, cards)
        return f

    elph_state = {}

    def step_elph(mark=False):
        """what reference models/elph.py:186-213 + runners/train.py:204 execute per training step"""
        loops = torch.arange(n, device=dev).repeat(2, 1)
        hash_edge_index = torch.cat([ei, loops], dim=1)                      # add_self_loops
        if 'mh0' not in elph_state:                                          # init once (elph.py:189-192)
            elph_state['mh0'], elph_state['hll0'] = eh.initialise_minhash(n), eh.initialise_hll(n)
        table = {0: {'minhash': elph_state['mh0'], 'hll': elph_state['hll0']}}
        cards = torch.zeros((n, h), device=dev)
        for k in range(1, h + 1):
            table[k] = {'hll': eh.hll_prop(table[k - 1]['hll'], hash_edge_index),
                        'minhash': eh.minhash_prop(table[k - 1]['minhash'], hash_edge_index)}
            cards[:, k - 1] = eh.hll_count(table[k]['hll'])
        f = eh.get_subgraph_features(links, table, cards)
        gather(f)
        keep(table, cards)
        return f

    def step_buddy(mark=False):
        """one build, then this rank's share of the whole link set in chunks of --buddy-chunk pairs (datasets/elph.py:200-208:
        get_subgraph_features(links, hashes, cards, subgraph_feature_batch_size)), one gather of all feature rows"""
        table, cards = build_tables()
        f = eh.get_subgraph_features(links, table, cards, batch_size=a.buddy_chunk)
        gather(f)
        keep(table, cards)
        return f

    step = {'build_query': step_build_query, 'elph': step_elph, 'buddy': step_buddy}[a.api]
    pairs_per_step = plan.pairs_per_step  # whole job, all ranks (BUDDY: the whole link set)

    def fence():
        if launched:
            gather.drain()
        torch.cuda.synchronize(dev)
        if launched:  # (one process: the synchronisation above is the whole fence)
            dist.barrier()
            torch.cuda.synchronize(dev)

    def timed_region(steps):
        fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        fence()
        t = time.perf_counter() - t0
        if launched:
            tmax = torch.tensor([t], dtype=torch.float64, device=dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            t = float(tmax.item())
        return t

    # N > 1, --build auto: the timed region below runs with the REPLICATED build -- the one mode whose only collective is the gather of
    # the feature rows -- so that a line exists whatever the node does with the others; the row-sharded and peer-write builds are
    # timed with the same protocol AFTER it, under the watchdog of the strong-scaling figures, and the headline moves to the
    # fastest mode only if one of them beat it (`build`, `build_probe_ms_per_step` say which and by how much)
    build_probe = None
    auto_build = mode['build'] == 'auto'
    if auto_build:
        mode['build'] = 'replicated'
    sharded_build = mode['build'] in ('sharded', 'peer')

    # the driver's protocol as a fresh process meets it (its --warmup steps, then its --steps), BEFORE anything has settled: printed
    # as ms_per_step_cold beside the settled figure (VERDICT r4 #7a); --full only
    ms_per_step_cold = None
    if a.full:
        for _ in range(a.warmup):
            step()
        ms_per_step_cold = 1e3 * timed_region(a.steps) / a.steps
    # steady state: clocks, caches, allocator pools and the hub hint of this shape (disclosed as `settle_seconds`; not timed)
    settle_steps = 0
    if a.settle_seconds > 0:
        t_settle = time.perf_counter()
        while True:
            for _ in range(10):
                feats = step()
            settle_steps += 10
            torch.cuda.synchronize(dev)
            go = time.perf_counter() - t_settle < a.settle_seconds
            if launched:  # every rank runs the SAME number of steps (a step holds collectives): continue while any rank's clock says so
                flag = torch.tensor([1.0 if go else 0.0], dtype=torch.float64, device=dev)
                dist.all_reduce(flag, op=dist.ReduceOp.MAX)
                go = bool(flag.item() > 0)
            if not go:
                break
    for _ in range(a.warmup):
        feats = step()
    # HIP events around every launch of the dominant kernel, on its stream.  ELPH call sequence at h = 2 with the deferred table hop:
    # no full MinHash table hop is left in a step (the query's rows go through ss_minhash_hop_rows) -- the fused stage dominates
    elph_rows_only = a.api == 'elph' and ssa.hashing.DEFER_TABLE_HOP and ssa.hashing.LAZY_MINHASH
    dom_tag = nat.PROF_FUSED if (elph_rows_only and h == 2) else nat.PROF_MINHASH_HOP
    if a.api == 'buddy':  # the link set dwarfs the build: the query is the dominant kernel (92 % of a citation2-size precompute)
        dom_tag = nat.PROF_PAIRS
    # (every 4th launch of it: a timed launch costs its step ~5 us -- the completion signal its events are filled from --, 1 % of the step)
    # --full only: a plain run times the steps without them
    if a.full:
        lib.ss_profile_sample(a.time_every)
        lib.ss_profile_enable(0 if os.environ.get('SS_BENCH_EXP_NO_EVENTS') else 1 << dom_tag)
    fence()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        feats = step()
    fence()
    elapsed = time.perf_counter() - t0
    dom_ms, dom_n = c_float(), c_int32()
    if a.full:
        lib.ss_profile_read(dom_tag, byref(dom_ms), byref(dom_n))  # the launches of the timed region only
        lib.ss_profile_enable(0)
        lib.ss_profile_sample(1)
    if launched:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    ms_per_step = 1e3 * elapsed / a.steps
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, feats, last['table'], last['cards'])
    config_obj = {'workload': f'ogbl-{a.config}-like synthetic {a.graph} graph' + (' (BASELINE configs[1])' if a.config == 'collab' else '') +
                              ', BUDDY/ELPH hot path: step = build_hash_tables + get_subgraph_features, nothing cached across steps; '
                              'tables stay in the packed u32 / u8 layout the query reads -- the reference-shaped int64 [N, P] views of '
                              'the returned dict are lazy and are NOT materialised inside a step' +
                              ('' if a.api == 'build_query' else f' [api mode: {a.api}' + (f', {pairs_planned} links per build' + (f' ({a.buddy_negs} per source, listed together)' if a.buddy_negs else ' (uniformly random pairs)') + f', get_subgraph_features in chunks of {a.buddy_chunk} (datasets/elph.py:207-208); link sets >= {ssa.hashing.GROUP_LINKS_MIN} pairs are grouped by their first node unless they already are (hashing.GROUP_LINKS_MIN)' if a.api == 'buddy' else '')
                               + (', last-hop MinHash rows computed for the queried nodes only (hashing.DEFER_TABLE_HOP; SS_DEFER_TABLE_HOP=0: all N rows)'
                                  if a.api == 'elph' and ssa.hashing.DEFER_TABLE_HOP else '') + ']'),
                  'num_nodes': n, 'directed_edges': e_dir, 'max_hash_hops': h, 'minhash_num_perm': P, 'hll_p': HLL_P,
                  'pairs_per_step_per_gpu': links.size(0), 'global_pairs_per_step': pairs_per_step,
                  'parallelism': (f'edge batches sharded x{world} ({a.scaling} scaling), all_gather of features; sketch table ' +
                                  ((f'built row-sharded x{world}, every rank writing its rows into all ranks\' tables (peer-write, no exchange step)' if mode['build'] == 'peer' else f'built row-sharded x{world} with an in-place all_gather per hop and sketch') if sharded_build
                                   else 'replicated (every rank builds it)')),
                  'hll_tables': eh.tables_id}
    # the headline: the same keys, with the same meaning, in a plain run and in a --full one
    headline = {
        'metric': 'edge-pairs/sec subgraph-feature extraction (build+query)',
        'value': pairs_per_step * a.steps / elapsed, 'unit': 'pairs/s', 'n_gpus': world, 'steps': a.steps,
        'warmup': a.warmup, 'settle_seconds': a.settle_seconds, 'settle_steps': settle_steps, 'ms_per_step': ms_per_step,
        'higher_is_better': True, 'scaling': a.scaling,
        'rccl_ranks': (dist.get_world_size() if (launched and backend == 'nccl') else None), 'backend': (backend if launched else None),
        'build': mode['build'], 'vs_baseline': None, 'dtype': 'u32/u8 sketches, f32 estimator', 'data': 'synthetic', 'config': config_obj}
    if not a.full:
        eh.check_errors()  # the deferred bounds report of every launch so far (none expected on the synthetic workload)
        if rank == 0:
            emit(headline)
        if launched:
            dist.destroy_process_group()
        return
    # one step at a time: the latency of ONE synchronous build + query (BUDDY builds once; the headline above is a throughput -- the
    # host queues steps ahead of the GPU, so launch overhead of step i + 1 hides under the kernels of step i)
    lat = []
    for _ in range(max(a.steps, 5)):
        fence()
        t0 = time.perf_counter()
        step()
        fence()
        lat.append(1e3 * (time.perf_counter() - t0))
    latency_one_step_ms = float(np.median(lat))
    if launched:
        tl = torch.tensor([latency_one_step_ms], dtype=torch.float64, device=dev)
        dist.all_reduce(tl, op=dist.ReduceOp.MAX)
        latency_one_step_ms = float(tl.item())
    # N > 1: the weak figure beside the (strong) headline -- every rank its own batch of the config's size, the build replicated: N x
    # by construction, it measures the gather machinery
    weak = None
    if launched and world > 1 and a.scaling == 'strong' and a.api == 'build_query':
        wplan = ssa.dist.BatchPlan('weak', world, rank, pairs_planned)
        wlinks = torch.from_numpy(synthetic_links(n, pairs_planned, wplan.links_seed)).to(dev)
        wgather = ssa.dist.AsyncFeatureGather(wplan, nf, dev)

        def wstep():
            table, cards = eh.build_hash_tables(n, ei)
            wgather(eh.get_subgraph_features(wlinks, table, cards))
        for _ in range(3):
            wstep()
        wgather.drain()
        fence()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            wstep()
        wgather.drain()
        fence()
        tw = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        dist.all_reduce(tw, op=dist.ReduceOp.MAX)
        weak = {'value': wplan.pairs_per_step * a.steps / float(tw.item()), 'unit': 'pairs/s', 'ms_per_step': 1e3 * float(tw.item()) / a.steps,
                'global_pairs_per_step': wplan.pairs_per_step,
                'note': 'weak scaling: every rank its own batch, every rank repeats the whole build -- ~N x the 1-GPU rate by construction'}
        del wlinks, wgather
    eh.check_errors()  # the deferred bounds report of every launch so far (none expected on the synthetic workload)

    # ---- everything below runs AFTER the timed region ----------------------------------------------------------------
    sustained = None
    if a.sustain_seconds > 0:  # a region long enough for external samplers (the driver's gpu_busy probe) to see
        reps = max(a.steps, int(math.ceil(a.sustain_seconds * 1e3 / ms_per_step)))
        fence()
        t0 = time.perf_counter()
        for _ in range(reps):
            step()
        fence()
        sustained = {'ms_per_step': 1e3 * (time.perf_counter() - t0) / reps, 'steps': reps}
    if a.api == 'build_query':
        for _ in range(5):
            step_build_query(mark=True)
        fence()
    kernel_table = None
    if not a.no_kernel_table:
        tags = {'csr_build': nat.PROF_CSR, 'first_hop_hll': nat.PROF_FIRST_HOP_HLL, 'first_hop_minhash': nat.PROF_FIRST_HOP_MH,
                'hll_hop': nat.PROF_HLL_HOP, 'fused_first_hop_hll_hop': nat.PROF_FUSED, 'minhash_hop': nat.PROF_MINHASH_HOP, 'minhash_hop_rows': nat.PROF_MINHASH_ROWS, 'hub_passes': nat.PROF_HUB,
                'pair_features': nat.PROF_PAIRS}
        lib.ss_profile_enable(sum(1 << t for t in tags.values()))
        extra = 5
        for _ in range(extra):
            step()
        fence()
        lib.ss_profile_enable(0)
        model = rf.kernel_bytes(n, e_dir, P, HLL_P, h, min(links.size(0), batch), hub_e, hub_n, HUB_UNITS_HOSTED)
        model['hub_passes'] = (model['hub_first_hop'] + (h - 1) * model['hub_table_hop']) // h  # mean over the h launches of a step
        model['minhash_hop_rows'] = rf.minhash_rows_bytes(n, e_dir, 2 * min(links.size(0), batch), P)
        kernel_table = {}
        for name, tag in tags.items():
            ms, cnt = c_float(), c_int32()
            lib.ss_profile_read(tag, byref(ms), byref(cnt))
            if not cnt.value:
                continue
            row = {'mean_launch_ms': ms.value, 'launches_per_step': cnt.value / extra}
            if name in model and not (sharded_build and name != 'pair_features' and name != 'csr_build'):
                row['algorithmic_bytes'] = model[name]
                row['frac_of_hbm_peak'] = model[name] / (ms.value * 1e-3) / 1e9 / rf.HBM_PEAK_GBS
                tr = None if sharded_build else profiled_traffic(shape_key(a.config, a.graph, a.alpha), name)
                if tr:
                    row['traffic_bytes'] = tr['bytes_per_launch']
                    if tr["bytes_per_launch"] < 0.97 * model[name]:  # repeats served by the L2 (see roofline_numbers)
                        row['frac_of_hbm_peak'] = tr['bytes_per_launch'] / (ms.value * 1e-3) / 1e9 / rf.HBM_PEAK_GBS
                        row['bytes_basis'] = 'fabric bytes of the PMC passes'
            kernel_table[name] = row
        kernel_table['note'] = ('HIP-event brackets inside the library on the launch stream (include ~5 us of dispatch each); csr_build '
                                'spans all launches of one build; hub units (rows above the hub threshold) are hosted by the first_hop_hll and minhash_hop launches, '
                                'whose bytes include them (hub_passes: their own launches, SS_HUB_LAUNCHES=1 only)')

    # ---- roofline of the dominant kernel -----------------------------------------------------------------------------
    dom_family = {nat.PROF_FUSED: 'fused_first_hop_hll_hop', nat.PROF_PAIRS: 'pair_features'}.get(dom_tag, 'minhash_hop')
    prop_bytes = rf.kernel_bytes(n, e_dir, P, HLL_P, h, batch, hub_e, hub_n, HUB_UNITS_HOSTED)['minhash_hop']
    roof_kernel = "ss::propagate_kernel<128,256> (MinHash table hop: (E'+N)*4P + 4E + 8(N+1) bytes)"
    if dom_tag == nat.PROF_FUSED:
        prop_bytes = rf.kernel_bytes(n, e_dir, P, HLL_P, h, batch, hub_e, hub_n, HUB_UNITS_HOSTED)['fused_first_hop_hll_hop']
        roof_kernel = ("ss::fused_hop_persistent_kernel<2> (MinHash first hop + HLL table hop: 4E + 8(N+1) + N*4P + (E'+N)*M + 4N bytes; "
                       "VALU-bound first hop over the memory-bound table hop)")
    if dom_tag == nat.PROF_PAIRS:
        per_launch = min(links.size(0), a.buddy_chunk)
        H_ = ssa.hashing
        if H_.GROUP_LINKS_MIN and links.size(0) >= H_.GROUP_LINKS_MIN:  # grouped walk: the first node's rows once per run of pairs
            runs = int(torch.unique(links[:per_launch, 0]).numel())
            prop_bytes = rf.pair_bytes_grouped(per_launch, runs, P, HLL_P, h)
            roof_kernel = (f"ss::pair_features_kernel<{h},128,256> walked grouped by first node (ss_pair_features_grouped): per pair h rows + ids + "
                           f"cards + features, per run of pairs sharing a first node h rows ({runs} runs in {per_launch} pairs)")
        else:
            prop_bytes = per_launch * rf.pair_bytes(P, HLL_P, h)
            roof_kernel = f"ss::pair_features_kernel<{h},128,256> (query: 2h rows + ids + cards + features per pair)"
    if sharded_build and dom_tag != nat.PROF_PAIRS:  # each launch covers this rank's N/G destination rows and (on the uniform graph) E'/G in-edges
        prop_bytes //= world
        roof_kernel += f' / {world} ranks (row-sharded build)'
    prop_ms, prop_n = dom_ms.value, dom_n.value
    gathered = {'fused_first_hop_hll_hop': 'hll_hop'}.get(dom_family, dom_family)
    table_bytes = rf.gathered_table_bytes(n, dom_family, P, HLL_P, h)
    traffic = None if sharded_build else profiled_traffic(shape_key(a.config, a.graph, a.alpha) + ('' if a.api == 'build_query' else f'_{a.api}'), dom_family)
    roof = roofline_numbers(rf, prop_bytes, prop_ms, table_bytes, traffic)
    achieved = roof.get('achieved_gbs')
    step_bytes = rf.step_bytes_implemented(n, e_dir, P, HLL_P, h, links.size(0), hub_e, hub_n)
    step_ok = a.api == 'build_query' and not sharded_build
    out = dict(headline, ms_per_step_cold=ms_per_step_cold, latency_one_step_ms=latency_one_step_ms, build_probe_ms_per_step=build_probe)
    out.update({
        'roofline': {'kernel': roof_kernel + ('' if h > 1 else ' (not launched at h=1)') +
                               (' [elph api mode launches it per sketch: the same kernel and bytes]' if a.api == 'elph' and dom_tag != nat.PROF_FUSED else ''),
                     'bound': 'hbm', 'achieved': achieved, 'peak': rf.HBM_PEAK_GBS, 'unit': 'GB/s',
                     'frac': roof.get('frac_of_hbm_peak'),
                     # bytes per launch that crossed the fabric in the tracked PMC passes of this command (separate rocprofv3 --pmc
                     # runs, tools/prof.sh): FETCH_SIZE counts fabric requests including Infinity-Cache hits -- it shows the absence
                     # of re-reads, it is not an HBM-only byte count
                     'traffic': traffic['bytes_per_launch'] if traffic else None, 'traffic_file': traffic['file'] if traffic else None,
                     'bytes_basis': roof.get('bytes_basis'), 'gather_probe_gbs': roof.get('gather_probe_gbs'), 'gather_probe_note': roof.get('gather_probe_note'),
                     'algorithmic_bytes_per_launch': prop_bytes, 'mean_launch_ms': prop_ms, 'launches_timed': prop_n, 'launches_timed_every': a.time_every,
                     'resident': resident_label(rf, table_bytes),
                     'cache_resident_fraction': rf.cache_resident_fraction(table_bytes),
                     'hub_rows': hub_n, 'hub_edge_share': hub_e / e_dir,
                     **({'unique_hbm_bytes_per_launch': (rf.unique_bytes(n, e_dir, 'hll_hop', P, HLL_P) + n * 4 * P if dom_tag == nat.PROF_FUSED else
                                                         rf.unique_bytes(n, e_dir, 'minhash_hop', P, HLL_P) // (world if sharded_build else 1))}
                        if dom_tag != nat.PROF_PAIRS else {}),
                     'note': 'resident = infinity-cache: the gathered table fits the 256 MiB Infinity Cache, so `achieved` is a fabric + cache '
                             'rate (`gather_probe_gbs`: what random row gathers from a table of this size reach in a micro-benchmark; ~6.3 TB/s '
                             'is what HBM alone streams); mixed: the cache holds at least half of it; hbm: less -- see secondary_summary.citation2_uniform'},
    })
    if step_ok:
        out['step_roofline'] = {'bound': 'hbm', 'bytes_per_step': step_bytes, 'ms_per_step': ms_per_step,
                                'achieved': step_bytes / (ms_per_step * 1e-3) / 1e9, 'peak': rf.HBM_PEAK_GBS, 'unit': 'GB/s',
                                'frac': step_bytes / (ms_per_step * 1e-3) / 1e9 / rf.HBM_PEAK_GBS,
                                'bytes_per_step_survey_definition': rf.step_bytes_survey(n, e_dir, P, HLL_P, h, links.size(0)),
                                'note': 'bytes of the IMPLEMENTED schedule (CSR build, hop 1 from node ids without table reads, h-1 table '
                                        'hops, query) over the whole step time incl. launch gaps; the SURVEY 8(d) definition counts a table '
                                        'read for hop 1 too, which this schedule does not perform'}
    if weak:
        out['weak'] = weak
    if sustained:
        out['sustained'] = dict(sustained, pairs_per_s=pairs_per_step / (sustained['ms_per_step'] * 1e-3),
                                note='same step, run back to back for >= --sustain-seconds after the timed region')
    if phase_marks:
        build_ms = sum(s0.elapsed_time(s1) for s0, s1, _ in phase_marks) / len(phase_marks)
        query_ms = sum(s1.elapsed_time(s2) for _, s1, s2 in phase_marks) / len(phase_marks)
        out['breakdown'] = {'build_ms': build_ms, 'query_ms': query_ms,
                            'build_directed_edges_per_s': h * (e_dir + n) / (build_ms * 1e-3),  # h * E' / T_build
                            'query_pairs_per_s': links.size(0) / (query_ms * 1e-3), 'scope': 'this rank, HIP events on the launch stream',
                            'regime': 'five marked steps queued back to back behind a fence: event-to-event spans on the stream, i.e. GPU time of a '
                                      'step whose launches were queued ahead (they include the inter-kernel gaps of the stream, not host latency); '
                                      'ms_per_step is the same regime over --steps steps, latency_one_step_ms the synchronous one (a fence after '
                                      'every step: launch overhead exposed)'}
        if not sharded_build:  # what every rank repeats: the whole build
            out['redundant_fraction_of_step'] = build_ms / (build_ms + query_ms) if world > 1 else 0.0
            out['redundant_note'] = ('replicated build: every rank repeats it; under weak scaling the N-GPU rate is ~N x by construction'
                                     if world > 1 else 'single GPU: nothing is repeated')
    if kernel_table:
        out['kernels'] = kernel_table
    # ---- N > 1: strong-scaling figures beside the weak line -----------------------------------------------------
    # The timed region above is weak scaling with a replicated build: ~N x by construction.  Here the SAME job is timed on one GPU
    # (every rank runs all of it, no communication) and sharded over the N ranks, for the two jobs BASELINE names: the BUDDY
    # precompute of the config (one build + its link set) and one build + one global batch; with the build replicated and
    # row-sharded (exchange form chosen by dist.choose_exchange's micro-probe).  speedup_vs_n1_same_work = t(1 GPU) / t(N GPUs).
    if launched and world > 1 and a.api == 'build_query':
        # The figures below run collectives that the timed region does not (row exchanges, feature all-gathers).  A rank that
        # fails alone would leave the others waiting in one for ever, and the weak line above is already measured: a watchdog
        # prints it without the figures and ends the process if they take longer than --strong-timeout.
        def bail():
            if rank == 0:
                out['strong'] = {'error': f'strong-scaling figures did not finish within {a.strong_timeout:.0f} s; skipped'}
                out['cpu_baseline'] = None
                emit(out)
            os._exit(0)
        with_peer = not a.no_strong_peer and (a.strong_peer or backend != 'nccl')  # (see --strong-peer)
        watchdog = threading.Timer(a.strong_timeout, bail)
        watchdog.daemon = True
        watchdog.start()
        if auto_build:  # the other build modes on the headline's own job and protocol (see above)
            build_probe = {'replicated': ms_per_step}
            out['build_probe_ms_per_step'] = build_probe
            for cand in ['sharded'] + (['peer'] if with_peer else []):
                mode['build'] = cand
                try:
                    for _ in range(max(3, a.warmup)):
                        step()
                    t = timed_region(a.steps)
                    build_probe[cand] = 1e3 * t / a.steps
                except Exception as exc:  # (PeerShard fails on every rank or on none: no peer access, no IPC)
                    build_probe[cand] = f'unavailable: {type(exc).__name__}: {str(exc)[:200]}'
            mode['build'] = out['build']
            # the headline (value, ms_per_step, roofline, step figures) STAYS the replicated run it was measured with (a best-of-N
            # headline beside a roofline of another mode mixed two runs); the other modes are reported here and named
            timed_ok = {k: v for k, v in build_probe.items() if isinstance(v, float)}
            out['build_fastest'] = min(timed_ok, key=timed_ok.get)
        if not a.no_configs_3_4:
            try:
                # (the gloo test hooks: both ranks time-slice ONE GPU and every gather goes through the host -- a small link set, one repetition)
                cap = a.strong_links_cap or (None if backend == 'nccl' else 1_000_000)
                out['configs_3_4_strong'] = configs_3_4_strong(ssa, dist, dev, world, rank, reps=2 if backend == 'nccl' else 1, with_peer=with_peer,
                                                               links_cap=cap, only=os.environ.get('SS_BENCH_STRONG_ONLY', '').split(',') if os.environ.get('SS_BENCH_STRONG_ONLY') else None)
                out['configs_3_4_strong']['links_cap'] = cap
            except Exception as exc:
                out['configs_3_4_strong'] = {'error': f'{type(exc).__name__}: {exc}'}
        try:
            out['strong'] = ({'skipped': '--no-strong'} if a.no_strong else
                             strong_scaling_figures(ssa, eh, dist, dev, n, h, ei, cfg, batch, world, rank, with_peer=with_peer))
        except Exception as exc:  # (deterministic failures are the same on every rank; the headline line must survive)
            out['strong'] = {'error': f'{type(exc).__name__}: {exc}'}
        watchdog.cancel()
        # the honest N-GPU figure beside the weak line (whose N x is by construction): the SAME BUDDY precompute on 1 and on N GPUs,
        # best build mode (VERDICT r3 #7c)
        row = out['strong'].get('buddy_precompute') if isinstance(out['strong'], dict) else None
        if row:
            modes = {k: v['speedup_vs_n1_same_work'] for k, v in row.items() if isinstance(v, dict) and 'speedup_vs_n1_same_work' in v}
            if modes:
                best = max(modes, key=modes.get)
                out['same_work_speedup'] = {'value': modes[best], 'build': best, 'job': 'buddy_precompute', 'pairs': row['pairs'], 'n_gpus': world,
                                            'note': 't(1 GPU, whole job) / t(N GPUs, job sharded): strong scaling of the BUDDY precompute'}
    default_line = a.config == 'collab' and a.graph == 'uniform' and a.api == 'build_query' and batch == cfg['batch']
    feats_host = feats.cpu().numpy() if (rank == 0 and world == 1 and not a.no_cpu_baseline) else None
    if rank == 0 and world == 1 and not a.no_secondary and default_line:
        ei = links = feats = None  # (the headline's device tensors make room for the larger shapes)
        torch.cuda.empty_cache()
        out['secondary'] = {}
        for name, config, graph, alpha, api, b in SECONDARY:
            try:
                out['secondary'][name] = secondary_case(ssa, dev, name, config, graph, alpha, api, b)
            except Exception as exc:  # a secondary shape must never cost the headline line
                out['secondary'][name] = {'error': f'{type(exc).__name__}: {exc}'}
            torch.cuda.empty_cache()
        out['secondary']['note'] = ('same process, after the timed region and the sustained run: build + query steps of the other BASELINE '
                                    'shapes (uniform and power-law endpoints at the same N, E), the ELPH call sequence at the reference batch, '
                                    'the BUDDY precompute; dominant_frac_of_hbm_peak = algorithmic bytes of the dominant kernel (hub rows '
                                    'excluded from the row kernels\' bytes) / its mean HIP-event span / 8 TB/s')
    if rank == 0 and world == 1 and not a.no_cpu_baseline and a.config in ('collab', 'cora') and a.api == 'build_query' and batch == cfg['batch']:
        base, ofeat = cpu_baseline(ei_np, links_np, n, h, batch)
        out['cpu_baseline'] = base
        out['cpu_baseline']['max_abs_feature_diff_vs_gpu'] = float(np.abs(feats_host - ofeat).max())
        out['speedup_vs_cpu_baseline'] = out['value'] / base['value']
        if a.config == 'collab':
            out['cpu_baseline_reference_style'] = cpu_baseline_reference_style(ei_np, links_np, n, h, batch)
    elif rank == 0:
        out['cpu_baseline'] = None
    if rank == 0:
        emit(out)
    if launched:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
