"""Expansion of selector-cache bitsets into policy-map entries on the CPU: the
library's host walkers (cg_diag_selcache_expand_host,
cg_diag_selcache_entries_host) against a numpy oracle and against
resolve.endpoint_policy_map_state, and cg_policymap_sync on a host handle.
The same checks run through the kernels in test_selcache_expand_gpu.py."""
import numpy as np
import pytest

import selcache_expand_util as X
from cilium_amd import _native as N
from cilium_amd.classifier import L4_TUPLE_DTYPE
from cilium_amd.policy import htons


@pytest.fixture()
def sc(host):
    s = host.selector_cache()
    yield s
    s.destroy()


@pytest.fixture()
def pm8(host):
    m = host.policy_map(8)
    yield m
    m.destroy()


# --------------------------------------------------------- expansion alone --
@pytest.mark.parametrize("n", X.BOUNDARY_NS)
def test_expand_word_boundaries(sc, n):
    X.check_boundary(sc, n, diag_cpu=True)


def test_expand_no_rows_and_no_entries(sc):
    X.check_no_rows(sc, diag_cpu=True)


@pytest.mark.parametrize("n", X.BOUNDARY_NS)
def test_expand_ignores_padding_bits(sc, n):
    X.check_padding_ones(sc, n, diag_cpu=True)


def test_expand_many_rows(sc):
    X.check_big(sc, diag_cpu=True)


def test_expand_wider_than_one_round(sc):
    X.check_wide(sc, diag_cpu=True)


def test_expand_cap(sc):
    X.check_cap(sc, diag_cpu=True)


def test_expand_bad_source_index(sc):
    X.check_bad_source_index(sc, diag_cpu=True)


def test_expand_host_handle_refuses(sc):
    """No CPU fallback: the kernel entries return CG_NO_DEVICE on a handle
    without a GPU."""
    sc.set_identities(X.unlabelled(70))
    src, rows = np.zeros((1, sc.words), np.uint64), [X.row_of(0, [0])]
    with pytest.raises(N.CiliumGPUError) as ei:
        sc.expand(X.ExpandTable(rows), src)
    assert ei.value.code == N.CG_NO_DEVICE


# ------------------------------------------------------ against resolve.py --
@pytest.mark.parametrize("redirects", [False, True], ids=["plain", "redirects"])
@pytest.mark.parametrize("mode", X.MODES)
@pytest.mark.parametrize("case", X.STATE_CASES)
def test_entries_match_resolve(sc, case, mode, redirects):
    X.check_states(sc, case, mode, redirects, diag_cpu=True)


# --------------------------------------------------------- cg_policymap_sync --
def test_sync_counts(pm8):
    keys = X.raw_keys([(10, 80, 6, 0), (11, 80, 6, 0), (12, 0, 0, 1)])
    ports = np.asarray([0, htons(15001), 0], np.uint16)
    assert pm8.sync(keys, ports) == (3, 0)
    assert X.dump_dict(pm8) == {(10, htons(80), 6, 0): 0, (11, htons(80), 6, 0): htons(15001), (12, 0, 0, 1): 0}
    assert pm8.sync(keys, ports) == (0, 0)  # identical: nothing written
    ports2 = ports.copy()
    ports2[0] = htons(15002)
    assert pm8.sync(keys, ports2) == (1, 0)  # a proxy-port change is a write
    assert X.dump_dict(pm8)[(10, htons(80), 6, 0)] == htons(15002)
    assert pm8.sync(keys[1:], ports2[1:]) == (0, 1)  # a shrink
    assert X.dump_dict(pm8) == {(11, htons(80), 6, 0): htons(15001), (12, 0, 0, 1): 0}
    more = X.raw_keys([(12, 0, 0, 1), (13, 443, 6, 1)])
    assert pm8.sync(more, np.zeros(2, np.uint16)) == (1, 1)
    assert X.dump_dict(pm8) == {(12, 0, 0, 1): 0, (13, htons(443), 6, 1): 0}
    # the table the verdict path walks follows the sync
    t = np.zeros(3, L4_TUPLE_DTYPE)
    t["identity"], t["dport"], t["proto"] = [13, 11, 12], [htons(443), htons(80), htons(9)], [6, 6, 17]
    assert pm8.eval_host_diag(t).tolist() == [0, N.CG_DROP_POLICY, 0]


def test_sync_empty_list_empties_the_map(pm8):
    assert pm8.sync(X.raw_keys([(1, 0, 0, 0), (2, 0, 0, 0)]), np.zeros(2, np.uint16)) == (2, 0)
    assert pm8.sync(X.raw_keys([]), np.zeros(0, np.uint16)) == (0, 2)
    assert len(pm8.dump_to_slice()) == 0


def test_sync_duplicate_takes_last(pm8):
    keys = X.raw_keys([(1, 80, 6, 0), (2, 80, 6, 0), (1, 80, 6, 0)])
    assert pm8.sync(keys, np.asarray([htons(1), htons(2), htons(3)], np.uint16)) == (2, 0)
    assert X.dump_dict(pm8) == {(1, htons(80), 6, 0): htons(3), (2, htons(80), 6, 0): htons(2)}


def test_sync_is_all_or_nothing(pm8):
    first = X.raw_keys([(i, 80, 6, 0) for i in range(5)])
    assert pm8.sync(first, np.arange(5, dtype=np.uint16)) == (5, 0)
    before = X.dump_dict(pm8)
    nine = X.raw_keys([(100 + i, 443, 6, 1) for i in range(9)])
    with pytest.raises(N.CiliumGPUError) as ei:
        pm8.sync(nine, np.zeros(9, np.uint16))
    assert ei.value.code == N.CG_MAP_FULL
    assert X.dump_dict(pm8) == before
    # 8 distinct keys, one of them given twice, still fit
    eight = X.raw_keys([(100 + i, 443, 6, 1) for i in range(8)] + [(103, 443, 6, 1)])
    assert pm8.sync(eight, np.zeros(9, np.uint16)) == (8, 5)
    assert len(pm8.dump_to_slice()) == 8
