"""The plans of components_planted.py without a GPU: each planted input reaches what its docstring names (which wavefront patterns
occur, where each winner sits by lane, wavefront, tile and chunk, that the stride graphs pass the cap of cc_stride_grid as the source
states it), and for each of nine WRONG kernels a numpy model answers at least one plan differently from the right kernel -- the
argument on paper that tests/test_components_planted_gpu.py and the new graphs of tests/test_components_gpu.py would fail on it."""
import re
import time

import numpy as np
import pytest

import components_planted as P
import components_restatement as restated

C, T, W = P.CHUNK, P.TILE, P.WAVE


def test_the_constants_are_the_sources():
    from subgraph_sketching_amd import _native
    assert P.CHUNK == _native.COMPONENTS_CHUNK and P.CHUNK % P.TILE == 0 and P.TILE % P.WAVE == 0
    text = open(P.UNIT).read()
    body = re.search(r'inline unsigned cc_stride_grid\(int64_t n\).*?\n\}', text, flags=re.S).group(0)
    assert f'blocks < {P.STRIDE_BLOCKS} ? blocks : {P.STRIDE_BLOCKS}' in body and 'kCcBlock' in body
    assert P.STRIDE_CAP == P.STRIDE_BLOCKS * P.TILE
    for kernel in ('cc_init_kernel', 'cc_hook_kernel', 'cc_flatten_kernel'):  # the three launches the cap bounds
        assert re.search(r'hipLaunchKernelGGL\(%s, dim3\(cc_stride_grid\(' % kernel, text)
    assert f'constexpr int kCcPeel = {P.PEEL};' in text and P.TILES == 8
    assert P.place(0) == (0, 0, 0, 0) and P.place(C + 3 * T + 2 * W + 10) == (1, 3, 2, 10) and P.place(P.N_BASE - 1) == (3, 1, 0, 0)


# ---- 1. labels --------------------------------------------------------------------------------------------------------------------------
def _waves(label):
    return [label[b:b + W] for b in range(0, len(label), W)]


def _seen(plan):
    """the wavefront patterns a label array shows, told from the labels alone"""
    seen = set()
    for w, l in enumerate(_waves(plan.label)):
        adds, rest = P.peel(l)
        kinds = len(np.unique(l))
        if len(l) == W:
            if kinds == 1:
                seen.add('one')
            if kinds == P.PEEL and not rest:
                seen.add('four')
            if kinds == P.PEEL + 1 and len(rest) == 60 and len({int(l[i]) for i in rest}) == 1:
                seen.add('five_60')
            if kinds == P.PEEL + 1 and len(rest) == 1:
                seen.add('five_1')
            if kinds == W:
                seen.add('sixty_four')
            if kinds == 2 and len(set(l[0::2])) == 1 and len(set(l[1::2])) == 1:
                seen.add('alternate')
            if kinds == 2 and [c for _, c in adds] == [W - 1, 1]:
                seen.add('leader63')
            if l[0] == w * W and l[W - 1] == w * W + W - 1:
                seen.add('fixed')
        elif len(l) == 1:
            seen.add('one live lane')
    return seen


def test_the_base_labels_show_every_pattern():
    plan = P.label_plan(P.N_BASE)
    assert plan.N == 3 * C + 257 and len(plan.names) == 101 and set(plan.names) == set(P.PATTERNS)
    assert _seen(plan) == {'one', 'four', 'five_60', 'five_1', 'sixty_four', 'alternate', 'leader63', 'fixed', 'one live lane'}
    waves = _waves(plan.label)
    # a label shared by whole wavefronts of different workgroups: each anchor
    for a in P.anchors(plan.N):
        chunks = {w * W // C for w, l in enumerate(waves) if len(l) == W and (l == a).all()}
        assert len(chunks) >= 2, (a, chunks)
    # fixed points at lane 0 and lane 63, in the first and the last tile of a chunk, in the first and the last chunk
    fixed = np.flatnonzero(plan.label == np.arange(plan.N))
    places = {P.place(x) for x in fixed}
    for chunk in (0, 3):
        assert (chunk, 0, 0, 0) in places and (chunk, 0, 0, W - 1) in places
    assert (0, P.TILES - 1, 3, 0) in places and (0, P.TILES - 1, 3, W - 1) in places and (2, P.TILES - 1, 3, W - 1) in places
    assert P.place(fixed[-1]) == (3, 1, 0, 0) and fixed[-1] == plan.N - 1  # the last chunk's last tile: one node
    assert (plan.block_roots > 0).all() and plan.block_roots.sum() == len(fixed) and plan.size.sum() == plan.N
    print('patterns:', {n: plan.names.count(n) for n in P.PATTERNS}, 'fixed points per chunk:', plan.block_roots.tolist())


def test_the_small_label_arrays_are_cut_where_n_ends():
    plans = P.label_plans()
    assert [p for p in plans if p[1] == 0] == [(P.N_BASE, 0)] + [(n, 0) for n in (C - 1, C, C + 1, 63, 64, 65)]
    for n in (C - 1, C, C + 1):
        plan = P.label_plan(n)
        assert plan.label.shape == (n,) and _seen(plan) >= {'one', 'four', 'five_60', 'five_1', 'sixty_four', 'alternate', 'leader63', 'fixed'}
        assert len(plan.block_roots) == (2 if n > C else 1)
    assert 'one live lane' in _seen(P.label_plan(C + 1)) and 'one live lane' in _seen(P.label_plan(65))
    # one wavefront shows one pattern: at 63, 64 and 65 nodes every pattern takes the first wavefront in turn
    for n in (63, 64, 65):
        assert {P.label_plan(n, first).names[0] for first in range(1, len(P.PATTERNS) + 1)} == set(P.PATTERNS)
    assert set().union(*(_seen(P.label_plan(64, first)) for first in range(1, len(P.PATTERNS) + 1))) >= set(P.PATTERNS) - {'shared'}
    for n, first in plans:
        plan = P.label_plan(n, first)
        P.check_labels(plan.label, n)
        np.testing.assert_array_equal(P.model_sizes(plan.label), plan.size)  # the peel adds up to the plain count


def test_labels_outside_the_range_are_refused_before_a_launch():
    label = P.label_plan(64).label.copy()
    for bad in (-1, 64):
        label[5] = bad
        with pytest.raises(AssertionError):
            P.check_labels(label, 64)
    case = P.roots_case('lane 31')
    with pytest.raises(AssertionError):
        P.check_block_incl(case.block_incl + 1, case.label == np.arange(case.N))


def test_wrong_peels_are_caught():
    """the leftover lanes of the peel dropped, or counted twice: size[] differs from the plain count in the base array and already in
    single wavefronts of 64 and 65 nodes; a wavefront of at most four labels cannot tell"""
    for leftover in (0, 2):
        caught = [p for p in P.label_plans() if not np.array_equal(P.model_sizes(P.label_plan(*p).label, leftover), P.label_plan(*p).size)]
        assert (P.N_BASE, 0) in caught and (C - 1, 0) in caught and any(n == 64 for n, _ in caught) and any(n == 63 for n, _ in caught)
        blind = [p for p in P.label_plans() if p not in caught]
        assert blind and all(n <= 65 for n, _ in blind)
        assert {P.label_plan(64, first).names[0] for n, first in caught if n == 64} == {'five_60', 'five_1', 'sixty_four'}
        print(f'leftover lanes add {leftover}:', len(caught), 'of', len(P.label_plans()), 'label arrays differ')


# ---- 2. roots ---------------------------------------------------------------------------------------------------------------------------
def test_every_winner_sits_where_its_name_says():
    want = {'lane 0': (0, 0, 0, 0), 'lane 31': (0, 0, 0, 31), 'lane 32': (0, 0, 0, 32), 'lane 63': (0, 0, 0, 63),
            'wavefront 1 lane 5': (0, 0, 1, 5), 'wavefront 3 lane 5': (0, 0, 3, 5), 'last tile of a chunk': (1, 7, 1, 36),
            'first tile of the last chunk': (3, 0, 1, 6), 'last node': (3, 1, 0, 0), 'tie at lanes 62 and 63': (1, 1, 1, 62),
            'tie in two wavefronts': (1, 0, 0, 10), 'tie in two workgroups': (0, 1, 3, 52), 'larger size in the earlier workgroup': (0, 1, 3, 52),
            'larger size in the later workgroup': (2, 1, 3, 52), 'size 2^31 - 1': (2, 0, 1, 13), 'survives seven later tiles': (1, 0, 1, 36),
            'chunk without a root': (2, 1, 0, 44), 'every node a root': (0, 5, 3, 28)}
    assert set(want) == set(P.ROOTS_CASES)
    for name in P.ROOTS_CASES:
        c = P.roots_case(name)
        assert P.place(c.winner) == want[name], (name, P.place(c.winner))
        assert c.label[c.winner] == c.winner and c.size[c.winner] == c.top and c.best == (c.top << 32) | (0xFFFFFFFF - c.winner)
        assert P.model_best(c) == (c.top, c.winner)
        others = c.sizes[c.roots != c.winner]
        tie = name.startswith('tie')
        assert (others == c.top).sum() == (1 if tie else 0) and (others <= c.top).all()
        if tie:
            assert c.roots[c.sizes == c.top].tolist() == sorted(x for x, _ in P.TIES[name]) and c.winner == P.TIES[name][0][0]
        # sizes are the test's, not counts; a non-root's word is larger than every root's (it must not be read) except beside 2^31 - 1
        assert (c.size[c.label != np.arange(c.N)] >= 1 << 20).all() and not np.array_equal(c.sizes, np.bincount(c.label, minlength=c.N)[c.roots])
        np.testing.assert_array_equal(P.model_compact(c.label == np.arange(c.N)), c.roots)
        print(f'{name}: winner {c.winner} (chunk, tile, wavefront, lane) = {P.place(c.winner)}, size {c.top}, {len(c.roots)} roots')
    a, b = P.TIES['tie at lanes 62 and 63']
    assert P.place(a[0])[:3] == P.place(b[0])[:3] and (P.place(a[0])[3], P.place(b[0])[3]) == (62, 63)
    a, b = P.TIES['tie in two wavefronts']
    assert P.place(a[0])[0] == P.place(b[0])[0] and P.place(a[0])[2] != P.place(b[0])[2]
    for name in ('tie in two workgroups', 'larger size in the earlier workgroup', 'larger size in the later workgroup'):
        a, b = P.TIES[name]
        assert P.place(a[0])[0] != P.place(b[0])[0]
    c = P.roots_case('size 2^31 - 1')
    assert c.top == 0x7FFFFFFF and c.best >> 63 == 0 and c.best & 0xFFFFFFFF == 0xFFFFFFFF - c.winner
    c = P.roots_case('chunk without a root')
    assert np.diff(np.concatenate([[0], c.block_incl])).tolist()[1] == 0 and (np.diff(np.concatenate([[0], c.block_incl]))[[0, 2, 3]] > 0).all()
    c = P.roots_case('every node a root')
    assert c.N == C + 1 and len(c.roots) == c.N and c.block_incl.tolist() == [C, C + 1]
    c = P.roots_case('survives seven later tiles')
    later = [c.winner + i * T for i in range(1, P.TILES)]
    assert all(c.label[x] == x and 0 < c.size[x] < c.top for x in later) and P.place(later[-1])[:2] == (1, P.TILES - 1)


def _caught(**wrong):
    return [name for name in P.ROOTS_CASES if P.model_best(P.roots_case(name), **wrong) != P.model_best(P.roots_case(name))]


def test_wrong_root_reductions_are_caught():
    half = _caught(lanes=32)  # a butterfly over 32 lanes
    assert {'lane 32', 'lane 63', 'last tile of a chunk', 'tie at lanes 62 and 63', 'chunk without a root', 'tie in two workgroups'} <= set(half)
    assert not {'lane 0', 'lane 31', 'wavefront 1 lane 5', 'wavefront 3 lane 5'} & set(half)
    first = _caught(first_tile_only=True)  # a key taken from a thread's first tile only
    assert {'last tile of a chunk', 'last node', 'tie at lanes 62 and 63', 'tie in two workgroups', 'chunk without a root', 'every node a root'} <= set(first)
    assert 'first tile of the last chunk' not in first and 'survives seven later tiles' not in first
    larger = _caught(larger_root=True)  # ties going to the larger root
    assert sorted(larger) == sorted(n for n in P.ROOTS_CASES if n.startswith('tie'))
    group0 = _caught(chunk0_only=True)  # the maximum of workgroup 0 only
    assert set(group0) == {n for n in P.ROOTS_CASES if P.place(P.roots_case(n).winner)[0] > 0}
    assert {'last node', 'first tile of the last chunk', 'larger size in the later workgroup', 'size 2^31 - 1'} <= set(group0)
    for what, names in (('32-lane butterfly', half), ('first tile only', first), ('ties to the larger root', larger), ('workgroup 0 only', group0)):
        print(f'{what}: wrong in {len(names)} of {len(P.ROOTS_CASES)} cases:', ', '.join(names))


def test_a_rank_without_the_earlier_wavefronts_is_caught():
    sets = {f'roots, {name}': P.roots_case(name).label == np.arange(P.roots_case(name).N) for name in P.ROOTS_CASES}
    sets.update({f'mask {kind}': P.mask_plan(kind).keep for kind in ('runs', 'everything')})
    sets.update({f'label {root}': P.label_plan(P.N_BASE).label == root for root, _, _ in P.select_label_cases()})
    sets.update({f'edges {kind} {E}': P.edges_case(kind, E).keep for kind, E in P.EDGE_CASES})
    caught = set()
    for what, keep in sets.items():
        np.testing.assert_array_equal(P.model_compact(keep), np.flatnonzero(keep), err_msg=what)
        if not np.array_equal(P.model_compact(keep, earlier_wavefronts=False), np.flatnonzero(keep)):
            caught.add(what)
    # a set of whole wavefronts in different tiles cannot tell: two of the four label sets are such sets
    blind = set(sets) - caught
    assert all(what.startswith('label') for what in blind) and len(blind) <= 2, blind
    print('a rank without the earlier wavefronts: wrong in', len(caught), 'of', len(sets), 'sets; not in', sorted(blind))


# ---- 3. select, mapper, edges, same -----------------------------------------------------------------------------------------------------
def test_the_select_plans():
    plan = P.label_plan(P.N_BASE)
    roots = [root for root, _, _ in P.select_label_cases()]
    assert roots == [0, C - 1, 2 * C, plan.N - 1] and [P.place(r)[:2] for r in roots] == [(0, 0), (0, 7), (2, 0), (3, 1)]
    for root, best, members in P.select_label_cases():
        assert best & 0xFFFFFFFF == 0xFFFFFFFF - root and best >> 32 > 0 and root in members and len(members) > 2 * W
        assert len({P.place(x)[0] for x in members}) >= 2
    runs = P.mask_plan('runs')
    assert set(np.unique(runs.mask)) == {0, 1, 2, 0x80, 0xFF} and runs.mask.dtype == np.uint8
    k = runs.keep
    for edge in (T, C):  # a run ends at the last position of a tile / a chunk: the next position is dropped
        assert k[edge - 1] and not k[edge] and not k[edge + 1]
    for edge in (2 * T, 2 * C):  # a run starts at the first position: the one before is dropped
        assert k[edge] and not k[edge - 1] and not k[edge - 2]
    for edge in (2 * C + T, 3 * C):  # and runs across both kinds of boundary
        assert k[edge - 1] and k[edge]
    assert k[-1] and not k[-2] and 1000 < k.sum() < 3000
    assert P.mask_plan('everything').keep.all() and set(np.unique(P.mask_plan('everything').mask)) == {1, 2, 0x80, 0xFF}
    assert not P.mask_plan('nothing').mask.any()
    # mask == 1 instead of != 0
    for kind in ('runs', 'everything'):
        m = P.mask_plan(kind)
        assert not np.array_equal(np.flatnonzero(m.mask == 1), np.flatnonzero(m.mask != 0)) and np.array_equal(m.mask != 0, m.keep)


def test_the_mapper_plans():
    sizes = {}
    for name in P.MAPPER_CASES:
        c = P.mapper_case(name)
        n = len(c.nodes)
        sizes[name] = n
        assert c.nodes.dtype == np.int64 and (c.nodes < 0).sum() >= n // 2 and (n == 1 or not (np.diff(c.nodes % c.N) > 0).all())
        assert (c.err, c.dup) == (int(name.startswith('an id')), int(name.startswith('twice')))
        listed = (c.mapper >= 0).sum()
        assert listed + sum(len(v) for v in c.twice.values()) + c.err == n
    assert [sizes[k] for k in ('1', '255', '256', '257', '5000')] == [1, 255, 256, 257, 5000]
    (x, (i, j)), = P.mapper_case('twice in a wavefront').twice.items()
    assert i // W == j // W
    (x, (i, j)), = P.mapper_case('twice 4000 apart').twice.items()
    assert j - i == 4000 and i // T != j // T
    c = P.mapper_case('twice as x and x - N')
    (x, (i, j)), = c.twice.items()
    assert c.nodes[i] == x and c.nodes[j] == x - c.N
    assert c.N in P.mapper_case('an id equal to N').nodes and -c.N - 1 in P.mapper_case('an id below -N').nodes


def test_the_edge_plans():
    assert [E for _, E in P.EDGE_CASES] == [2 * C + 300, 2 * C + 300, C - 1, C, C + 1]
    for kind, E in P.EDGE_CASES:
        c = P.edges_case(kind, E)
        k = c.keep
        assert len(k) == E and c.err == 1 and (c.src == c.N).sum() + (c.dst == c.N).sum() == 1
        assert ((c.src < 0) & (c.dst < 0) & k).sum() == 1
        # not a ranking: no select pass made this mapper
        assert set(np.unique(c.mapper[c.mapper >= 0] % 7)) == {3} and (c.mapper == -1).sum() == 334
        assert k[8 * W:9 * W].all() and not k[9 * W:10 * W].any()
        for edge in (T, C, 2 * C):
            if edge + 1 < E and not (kind == 'hole' and edge in (C, 2 * C)):
                assert k[edge - 1] and k[edge] and not k[edge - 2] and not k[edge + 1]
        if E in (C, C + 1):  # the last edge kept: at the last position of the only chunk, or alone in a second chunk
            assert k[-1] and k[C - 1] and not k[C - 2]
        per_chunk = np.diff(np.concatenate([[0], c.block_incl]))
        if kind == 'hole':
            assert per_chunk[1] == 0 and per_chunk[0] > 0 and per_chunk[2] > 0 and k[C - 1] and k[2 * C]
        # dropped edges of all three kinds
        ws, wd = restated.wrapped(c.N, c.src), restated.wrapped(c.N, c.dst)
        inside = np.concatenate([c.mapper >= 0, [False]])
        kinds = {(bool(a), bool(b)) for a, b in zip(inside[np.minimum(ws, c.N)][~k], inside[np.minimum(wd, c.N)][~k])}
        assert kinds == {(False, False), (True, False), (False, True)}
        np.testing.assert_array_equal(c.edge_ids, np.flatnonzero(k))


def test_the_same_plans():
    for L in P.SAME_L:
        c = P.same_case(L)
        assert c.links.shape == (L, 2) and c.err == 1 and c.out[100] == 0 and c.links[100, 1] == c.N
        assert 0.3 * L < c.out.sum() < 0.8 * L
        assert c.links[3].tolist() == c.links[2][::-1].tolist() and c.out[3] == c.out[2]
        assert (c.links[5] == c.links[4] - c.N).all() and c.out[5] == c.out[4]
        assert c.out[6] == 1 and c.out[7] == 1 and c.links[6, 0] == c.links[6, 1]
        signs = {(bool(u < 0), bool(v < 0)) for u, v in c.links}
        assert signs == {(False, False), (True, False), (False, True), (True, True)}


# ---- 4. the graphs for the API ----------------------------------------------------------------------------------------------------------
def _largest_root(n, ei):
    lab = restated.labels(n, ei)
    roots, sizes = restated.roots_and_sizes(lab)
    return lab, int(roots[np.argmax(sizes)]), int(sizes.max()), roots, sizes


def test_the_late_giant_and_the_ties():
    n, ei = P.late_giant()
    lab, root, size, roots, sizes = _largest_root(n, ei)
    chunk, tile, wave, lane = P.place(root)
    assert n == 3 * C + 191 + 20000 and ei.min() == 3 * C + 191 and chunk >= 3 and lane != 0 and size > 15000
    assert (lab[:3 * C + 191] == np.arange(3 * C + 191)).all()  # every lower id is isolated
    print(f'late giant: root {root} at (chunk, tile, wavefront, lane) = {(chunk, tile, wave, lane)}, {size} nodes, {len(roots)} components')
    for make, a, b in ((P.tie_across_workgroups, 5 * C + 100, 17 * C + 63), (P.tie_in_one_wavefront, 9 * C + 62, 9 * C + 63)):
        n, ei = make()
        lab, root, size, roots, sizes = _largest_root(n, ei)
        assert n == 18 * C and root == a and size == P.PATH_NODES and roots[sizes == size].tolist() == [a, b] and restated.tied(lab) == 2
        assert (sizes[sizes != size] == 1).all() and ei[0, 0] == b  # everything else is isolated; the larger ids are listed first
        print(f'{make.__name__}: roots {a} at {P.place(a)} and {b} at {P.place(b)}')
    assert P.place(5 * C + 100)[0] != P.place(17 * C + 63)[0]
    assert P.place(9 * C + 62)[:3] == P.place(9 * C + 63)[:3] and P.place(9 * C + 63)[3] == 63


def test_the_stride_graphs_pass_the_cap_and_one_trip_is_not_enough():
    """N and E of both graphs are above what one trip of a grid-stride launch covers, and a hook that made only its first trip -- the
    arcs from position STRIDE_CAP on ignored -- leaves other labels.  Prints the restatement's CPU time for the two graphs."""
    assert P.STRIDE_CAP == 4096 * 256
    for name in P.STRIDE_GRAPHS:
        n, ei = P.API_GRAPHS[name]()
        E = ei.shape[1]
        assert n == 1_100_000 and n > P.STRIDE_CAP and E > P.STRIDE_CAP and ei.nbytes < 40e6 and ei.dtype == np.int64
        t0 = time.perf_counter()
        lab = restated.labels(n, ei)
        t1 = time.perf_counter()
        restated.largest_component_subgraph(n, ei)
        t2 = time.perf_counter()
        one_trip = restated.labels(n, ei[:, :P.STRIDE_CAP])
        # the random graph lists every pair in both directions, the second direction behind the first: its arcs past the cap repeat
        # edges of the first trip, and only its N tests a second trip (init, flatten).  Shuffled, its arcs past the cap carry edges
        # of their own, as the path's do.
        assert np.array_equal(one_trip, lab) == (name == 'stride random')
        roots, sizes = restated.roots_and_sizes(lab)
        print(f'{name}: N = {n}, E = {E}, {len(roots)} components, largest {sizes.max()}; restatement: labels {t1 - t0:.2f} s, '
              f'largest_component_subgraph {t2 - t1:.2f} s; first trip only: {int((one_trip != lab).sum())} labels differ')
        if name == 'stride random shuffled':
            np.testing.assert_array_equal(lab, restated.labels(*P.stride_random()))
        if name == 'stride path':
            assert len(roots) == 1 and E == n - 1
            # a deep chain that crosses every stride boundary: consecutive path edges sit in different trips, ids all over the range
            assert np.abs(np.diff(ei[0, :1000])).mean() > n / 10
        else:
            assert sizes.max() > n // 3 and len(roots) > 1000
