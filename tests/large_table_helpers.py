"""What tests/test_large_tables_gpu.py and tests/test_large_tables_links_gpu.py share: the fixture object and its release pattern,
the links around the boundary rows, and the C oracle on a COMPACTED table (the distinct rows a query touches, gathered and renumbered:
every offset of the compacted table is far below 2^31).  No test lives here."""
import numpy as np
import torch

ATOL = 1e-4
GB = 1 << 30
# free device memory asked for around ONE [8 650 752, 128] four-byte table (4.43 GB) and what is made from it: the measured peak of
# the spmm case + 10 % (profiles/large_tables_tests.txt)
NEEDS_ONE_TABLE = int(1.1 * 9886710784)


class Big(object):
    """what a fixture holds; release() reports the peak of the tests that used it and drops its device tensors (building the next
    fixture and the last test release the previous one: a module-scoped fixture would otherwise live until the end of the module)"""
    table = None

    def release(self):
        if self.table is None:
            return
        peak = torch.cuda.max_memory_allocated()
        print(f'\n[large tables] fixture {self.name}: N = {self.n}, peak torch.cuda.max_memory_allocated() = {peak} bytes ({peak / GB:.2f} GiB)')
        for name in ('graph', 'blocks', 'table', 'cards', 'eh', 'cache'):
            setattr(self, name, None)
        torch.cuda.empty_cache()


LIVE = []


def release_all(dev):
    for big in LIVE:
        big.release()
    del LIVE[:]
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()


def require_free_memory(dev, need, what):
    """skip the calling test, with the byte counts, when the device has less than `need` bytes free"""
    import pytest
    free = torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f'{what} needs {need} bytes of free device memory, {free} are free')


def wrap(ids, n):
    return torch.where(ids < 0, ids + n, ids)


def compacted_oracle(big, links, degrees=None, debug=False):
    """oracle.pair_features on the distinct rows `links` touch, gathered to the host and renumbered"""
    from oracle import oracle
    ids = wrap(links.to(torch.int64), big.n)
    uniq, inv = torch.unique(ids.flatten(), return_inverse=True)
    otab = {k: {'minhash': big.table[k].mh_u32.index_select(0, uniq).cpu().numpy().view(np.uint32),
                'hll': big.table[k].hll_u8.index_select(0, uniq).cpu().numpy()} for k in (1, 2)}
    ocards = big.cards.index_select(0, uniq).cpu().numpy()
    small = inv.reshape(-1, 2).cpu().numpy()
    res = oracle.pair_features(small, otab, ocards, 2, big.prm, debug=debug)
    feats, dbg = res if debug else (res, None)
    if degrees is not None:
        feats = oracle.append_degree_normalised(feats, small, degrees.index_select(0, uniq).cpu().numpy())
    return feats, dbg


def feature_tol(ofeat):
    return dict(rtol=1e-4, atol=ATOL * max(1.0, float(np.abs(ofeat).max()) / 100))


def boundary_links(big, dev, count, seed):
    """links whose endpoints are (low, high), (high, low), (high, high) across every boundary, the boundary rows themselves, N - 1,
    the hubs, u == v, and negative ids that wrap to high rows"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    n, w = big.n, big.graph.window
    parts = []
    per = (count - 64) // (4 * len(big.bounds))
    for b in big.bounds:
        lo = torch.randint(b - w, b, (per, 2), device=dev, generator=gen)
        hi = torch.randint(b, b + w, (per, 2), device=dev, generator=gen)
        far = torch.randint(b + w, n, (per, 2), device=dev, generator=gen)
        parts += [torch.stack([lo[:, 0], hi[:, 0]], 1), torch.stack([hi[:, 1], lo[:, 1]], 1), hi, torch.stack([far[:, 0], hi[:, 0]], 1)]
        parts.append(torch.tensor([[b, b - 1], [b - 1, b], [b, b], [b + 1, b], [b, n - 1], [n - 1, b], [0, b], [b, big.graph.mega],
                                   [big.graph.hubs[0], b - 1]], device=dev))
    parts.append(torch.tensor([[n - 1, n - 1], [n - 1, 0], [n - 2, n - 1], [big.graph.mega, big.graph.hubs[1]]], device=dev))
    links = torch.cat(parts)
    fill = torch.randint(0, n, (count - links.size(0), 2), device=dev, generator=gen)
    links = torch.cat([links, fill])[:count].contiguous()
    links[::5] -= n        # torch-style negative ids: -1 is row N - 1, -(2^18) is the top boundary row (N = top + 2^18)
    links[7, 0] = links[7, 1]
    links[1] = torch.tensor([-1, -(1 << 18)], device=dev)
    return links
