"""The plan toolbox (subgraph_sketching_amd/_plans.py) on CPU tensors, without the library: the hub listing against a plain-Python
loop on planted row lengths, the identity-keyed plan cache with a counting builder, the padding of feature rows to float4 pieces."""
import gc

import pytest
import torch

from subgraph_sketching_amd import _plans

CHUNK = 256


def _hubs_by_loop(m, hub, chunk, names=None):
    rows, starts, chunk_hub = [], [0], []
    for i, entries in enumerate(m):
        if entries > hub:
            chunk_hub += [len(rows)] * (-(-entries // chunk))
            rows.append(i if names is None else names[i])
            starts.append(len(chunk_hub))
    return rows, starts, chunk_hub


def _planted(hub):
    """row lengths by case: no hub; one hub of exactly hub + 1 entries; hubs of chunk, chunk + 1 and 2 * chunk entries; hubs in the
    first and the last row; every row a hub at n = 1 and n = 5"""
    big = max(hub, CHUNK)
    return {'no hub': [0, 1, hub, hub, 1],
            'hub + 1': [1, hub + 1, 0, hub],
            'chunk multiples': [1, max(CHUNK, hub + 1), 0, max(CHUNK + 1, hub + 1), max(2 * CHUNK, hub + 1), 1],
            'first and last': [big + 7, 0, 1, hub, 3 * big + 1],
            'all hubs, n = 1': [hub + 1],
            'all hubs, n = 5': [hub + 1, 2 * big, big + 1, 4 * big + 3, hub + 2]}


@pytest.mark.parametrize('with_names', [False, True])
@pytest.mark.parametrize('hub', [1, 256])
def test_hub_listing(hub, with_names):
    for what, lengths in _planted(hub).items():
        n = len(lengths)
        m = torch.tensor(lengths, dtype=torch.int64)
        names = [1000 + 3 * i for i in range(n)] if with_names else None
        cap = sum(lengths) // (hub + 1)  # as the plans size it: a row of more than `hub` entries, there are at most this many
        rows, chunks, hub_chunk, n_hubs, n_chunks = _plans.list_hubs(m, hub, CHUNK, cap, None if names is None else torch.tensor(names, dtype=torch.int32))
        want_rows, want_starts, want_chunk_hub = _hubs_by_loop(lengths, hub, CHUNK, names)
        H, C = len(want_rows), len(want_chunk_hub)
        assert (rows.dtype, chunks.dtype, hub_chunk.dtype, n_hubs.dtype, n_chunks.dtype) == (torch.int32,) + (torch.int64,) * 4, what
        assert rows.shape == chunks.shape == hub_chunk.shape == (cap + 1,) and n_hubs.shape == n_chunks.shape == (1,), what
        assert torch.cat([n_hubs, n_chunks]).tolist() == [H, C], what
        assert rows[:H].tolist() == want_rows and hub_chunk[:H + 1].tolist() == want_starts and int(chunks[cap]) == 0, what
        hub_rows, starts, chunk_hub = _plans.finish_hubs(rows, chunks, hub_chunk, H, C)
        assert hub_rows.dtype == starts.dtype == chunk_hub.dtype == torch.int32 and hub_rows.is_contiguous(), what
        assert starts.tolist() == want_starts, what
        if H:
            assert hub_rows.tolist() == want_rows and chunk_hub.tolist() == want_chunk_hub, what
        else:  # size-1 stand-ins: the pointers must exist
            assert what == 'no hub' and hub_rows.shape == chunk_hub.shape == (1,) and starts.tolist() == [0] and chunk_hub.tolist() == [0]
        with pytest.raises(ValueError, match='the hub rows have 2\\^31 chunks or more'):
            _plans.finish_hubs(rows, chunks, hub_chunk, H, 1 << 31)


class _Builder(object):
    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return ('plan', self.calls)


def test_plan_cache():
    cache, build = _plans._PlanCache(), _Builder()
    ei, w = torch.arange(6).view(2, 3), torch.ones(3)
    first = cache.get((5, None), (ei, w), build)
    assert cache.get((5, None), (ei, w), build) is first and build.calls == 1                 # the same tensor objects hit
    assert cache.get((5, None), (ei.clone(), w), build) == ('plan', 2)                        # an equal-content fresh tensor rebuilds
    assert cache.get((5, None), (ei, w), build) == ('plan', 3) and build.calls == 3           # (one plan is kept, not two)
    ei[0, 0] = 4
    assert cache.get((5, None), (ei, w), build) == ('plan', 4)                                # an in-place edit rebuilds
    assert cache.get((6, None), (ei, w), build) == ('plan', 5)                                # a changed plain key rebuilds
    assert cache.get((6, 'cuda:1'), (ei, w), build) == ('plan', 6)
    assert cache.get((6, 'cuda:1'), (ei, w), build) == ('plan', 6)
    assert cache.get((6, 'cuda:1'), (ei, None), build) == ('plan', 7)                         # None matches only None ...
    assert cache.get((6, 'cuda:1'), (ei, None), build) == ('plan', 7)
    assert cache.get((6, 'cuda:1'), (ei, w), build) == ('plan', 8)                            # ... and a tensor does not match it
    assert cache.get((6, 'cuda:1'), (ei,), build) == ('plan', 9)                              # (another number of tensors)
    # a dead weakref rebuilds: the key of a tensor that died matches nothing, not even a new tensor at its address
    gone = torch.arange(4)
    cache.get((1,), (gone,), build)
    key = cache._key
    del gone
    gc.collect()
    assert key[1][0][0]() is None and not _plans._same(key[1][0], key[1][0]) and build.calls == 10
    fresh = torch.arange(4)
    assert cache.get((1,), (fresh,), build) == ('plan', 11)
    # an inference-mode tensor has no version counter and is cached all the same
    with torch.inference_mode():
        inf = torch.arange(6).view(2, 3)
        assert cache.get((1,), (inf,), build) == ('plan', 12) and cache.get((1,), (inf,), build) == ('plan', 12)
    assert cache.get((1,), (inf,), build) == ('plan', 12) and build.calls == 12

    def broken():
        raise ValueError('no plan')

    with pytest.raises(ValueError, match='no plan'):
        cache.get((1,), (ei,), broken)
    assert cache._key is None and cache._plan is None                                          # a build that raises leaves the cache empty
    assert cache.get((1,), (inf,), build) == ('plan', 13)
    # each module keeps its own instance
    from subgraph_sketching_amd import aggr, gcn
    assert isinstance(gcn._CACHE, _plans._PlanCache) and isinstance(aggr._CACHE, _plans._PlanCache) and gcn._CACHE is not aggr._CACHE


@pytest.mark.parametrize('F', [0, 1, 4, 5])
def test_padded_rows(F):
    x = torch.arange(3 * F, dtype=torch.float32).view(3, F) + 1
    y = -x
    seen = []

    def run(Fp, a, b, c):
        seen.append((Fp, a, b, c))
        return a + 2 * b

    out = _plans.padded_rows(run, F, x, y, None)
    Fp, a, b, c = seen[0]
    assert len(seen) == 1 and Fp == (F + 3) // 4 * 4 and c is None and a.shape == b.shape == (3, Fp)
    assert torch.equal(a[:, :F], x) and torch.equal(b[:, :F], y) and not a[:, F:].any() and not b[:, F:].any()
    assert (a is x and b is y) == (F % 4 == 0)  # whole float4 rows are passed as they are
    assert out.shape == (3, F) and torch.equal(out, x + 2 * y)
