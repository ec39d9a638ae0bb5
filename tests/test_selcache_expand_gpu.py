"""Expansion of selector-cache bitsets into policy-map entries on the GPU: the
three expansion kernels (count, scan, emit) against the numpy oracle and the
library's host walker, the fused cg_selcache_entries_host against
resolve.endpoint_policy_map_state, the device-pointer entry on a non-default
stream, table replacement, and cg_policymap_sync end to end through
l4_fp_kernel with its counters."""
import numpy as np
import pytest

import selcache_expand_util as X
import selcache_util as U
from cilium_amd import _native as N
from cilium_amd import resolve as R
from cilium_amd.classifier import L4_TUPLE_DTYPE, POLICY_KEY_DTYPE
from cilium_amd.policy import htons

pytestmark = pytest.mark.gpu


@pytest.fixture()
def sc(gpu):
    s = gpu.selector_cache()
    yield s
    s.destroy()


# --------------------------------------------------------- expansion alone --
@pytest.mark.parametrize("n", X.BOUNDARY_NS)
def test_gpu_expand_word_boundaries(sc, n):
    X.check_boundary(sc, n, diag_cpu=False)


def test_gpu_expand_no_rows_and_no_entries(sc):
    X.check_no_rows(sc, diag_cpu=False)


@pytest.mark.parametrize("n", X.BOUNDARY_NS)
def test_gpu_expand_ignores_padding_bits(sc, n):
    X.check_padding_ones(sc, n, diag_cpu=False)


def test_gpu_expand_many_rows(sc):
    """N = 4,099 (65 words, one past a wave's 64), 300 rows: more rows than
    one block, so the grid has many; also array for array, order included,
    against the host walker."""
    got = X.check_big(sc, diag_cpu=False)
    src, rows = X.big_case()
    want = sc.expand(X.ExpandTable(rows), src, diag_cpu=True, threads=4)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_gpu_expand_wider_than_one_round(sc):
    X.check_wide(sc, diag_cpu=False)


def test_gpu_expand_cap(sc):
    X.check_cap(sc, diag_cpu=False)


def test_gpu_expand_bad_source_index(sc):
    X.check_bad_source_index(sc, diag_cpu=False)


def _expand_dev(sc, rows, src, stream, dev, cap):
    """expand_dev into sentinel-filled tensors on `stream`; returns numpy
    (row_off, keys[cap], proxy[cap], total)."""
    import torch
    d_src = torch.from_numpy(src.view(np.int64).copy()).to(dev)
    d_off = torch.full((len(rows) + 1,), -1, dtype=torch.int64, device=dev)
    d_keys = torch.full((cap,), -1, dtype=torch.int64, device=dev)
    d_proxy = torch.full((cap,), -1, dtype=torch.int16, device=dev)
    d_total = torch.full((1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.current_stream(dev).synchronize()  # the fills, before another stream writes
    sc.expand_dev(X.ExpandTable(rows), d_src, src.shape[0], d_off, d_keys, d_proxy, cap, d_total,
                  stream=stream.cuda_stream)
    stream.synchronize()
    return (d_off.cpu().numpy().view(np.uint64), d_keys.cpu().numpy().view(POLICY_KEY_DTYPE),
            d_proxy.cpu().numpy().view(np.uint16), int(d_total.cpu().numpy()[0]))


def test_gpu_expand_dev_on_a_stream(sc):
    import torch
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    n = 130
    sc.set_identities(X.unlabelled(n))
    src, rows = X.boundary_case(n)
    want = X.oracle(src, n, sc.ids, rows)
    total = sum(len(w) for w in want)
    row_off, keys, proxy, got = _expand_dev(sc, rows, src, stream, dev, total + 7)
    assert got == total
    X.assert_entries(rows, want, row_off, keys[:total], proxy[:total])
    assert np.all(keys[total:].view(np.int64) == -1) and np.all(proxy[total:] == 0xFFFF)
    # too small a buffer: offsets and total, nothing written
    row_off2, keys, proxy, got = _expand_dev(sc, rows, src, stream, dev, total - 1)
    assert got == total and np.array_equal(row_off2, row_off)
    assert np.all(keys.view(np.int64) == -1) and np.all(proxy == 0xFFFF)


def test_gpu_expand_follows_new_identities(sc):
    """set_identities again with another N, larger and smaller: the ids
    written are the new table's."""
    for n, first in ((65, 100), (4099, 70000), (63, 9)):
        sc.set_identities(X.unlabelled(n, first))
        src = X.random_src(3, n, (0.5,), n)
        rows = [X.row_of(0, [0]), X.row_of(1, [], N.CG_EXP_ALL), X.row_of(2, [1, 2])]
        row_off, keys, _ = X.check_expand(sc, rows, src, n, diag_cpu=False)
        assert np.array_equal(keys[int(row_off[1]):int(row_off[2])]["sec_label"], np.arange(first, first + n))


# ------------------------------------------------------ against resolve.py --
@pytest.mark.parametrize("redirects", [False, True], ids=["plain", "redirects"])
@pytest.mark.parametrize("mode", X.MODES)
@pytest.mark.parametrize("case", X.STATE_CASES)
def test_gpu_entries_match_resolve(sc, case, mode, redirects):
    X.check_states(sc, case, mode, redirects, diag_cpu=False)


# -------------------------------------------- sync_policy_maps, end to end --
def _tuples(identities):
    """identities x ports {0, 80, 443, 8080} x protocols {0, 6, 17} x both
    directions x with / without the fragment flag."""
    grid = np.array(np.meshgrid(identities, [0, 80, 443, 8080], [0, 6, 17],
                                [0, N.CG_L4_F_INGRESS], [0, N.CG_L4_F_FRAGMENT], indexing="ij")).reshape(5, -1)
    t = np.zeros(grid.shape[1], L4_TUPLE_DTYPE)
    t["identity"] = grid[0]
    t["dport"] = [htons(int(p)) for p in grid[1]]
    t["proto"] = grid[2]
    t["flags"] = grid[3] | grid[4]
    t["len"] = 100
    return t


def _key(k):
    return (k.Identity, k.DestPort, k.Nexthdr, k.TrafficDirection)


def _row_key(k):
    return (int(k["sec_label"]), int(k["dport"]), int(k["protocol"]), int(k["egress"]))


def test_gpu_sync_policy_maps_end_to_end(sc, gpu):
    """Per endpoint of seed 11: a map filled by sync_policy_maps and one
    filled key by key by resolve.sync_policy_map from the oracle's dict hold
    the same entries and give the same verdicts; a re-sync keeps the
    surviving keys' counters and starts a new key at 0."""
    cache, repo = X.state_inputs(11)
    want = X.state_oracle(11, "default", True)
    sc.set_identities(cache)
    sc.set_repository(repo)
    endpoints = list(cache)
    absent = max(cache) + 1000
    tuples = _tuples(list(cache) + [absent])
    mine = [gpu.policy_map() for _ in endpoints]
    theirs = [gpu.policy_map() for _ in endpoints]
    try:
        counts = sc.sync_policy_maps(endpoints, mine, U.REDIRECTS)
        seen = set()
        for e, a, b, state, (added, deleted) in zip(endpoints, mine, theirs, want, counts):
            assert (added, deleted) == (len(state), 0)
            R.sync_policy_map(b, state)
            assert X.dump_dict(a) == X.dump_dict(b), e
            va, vb = a.verdicts(tuples), b.verdicts(tuples)
            assert np.array_equal(va, vb), e
            seen |= set(np.unique(np.sign(vb)).tolist())
        assert seen == {-1, 0, 1}, "the oracle's verdicts lack allows, drops or proxy redirects"
        # re-sync some maps with one key removed and one added
        ents = sc.endpoint_policy_map_entries(endpoints, U.REDIRECTS)
        fresh = X.raw_keys([(absent, 1, 6, 0)])
        for i in range(0, len(endpoints), 16):
            pm, (keys, proxy) = mine[i], ents[i]
            before = {_key(k): e.Packets for k, e in pm.dump_to_slice()}
            hit = [k for k, pk in before.items() if pk > 0]
            assert len(hit) >= 2, "the traffic advanced too few counters to tell"
            gone = hit[0]
            keep = np.array([_row_key(k) != gone for k in keys])
            assert pm.sync(np.concatenate([keys[keep], fresh]), np.concatenate([proxy[keep], [0]])) == (1, 1)
            after = {_key(k): e.Packets for k, e in pm.dump_to_slice()}
            new = _row_key(fresh[0])
            assert gone not in after and after[new] == 0
            assert {k: v for k, v in after.items() if k != new} == {k: v for k, v in before.items() if k != gone}
    finally:
        for m in mine + theirs:
            m.destroy()

