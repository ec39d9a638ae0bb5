"""CIDR policy on the GPU: selcache_cidr_match_kernel held against the host
walker, against resolve.py fed cidr_labels() dicts, and against the same
prefix identities as explicit label identities through selcache_match_kernel
(the existing kernel) — as arrays, with the word the label section ends in
checked bit by bit and the padding bits zero.  Then reach and the fused
entries over a repository mixing label and CIDR rules, section replacement,
and the policy file → allocator → ipcache + selector cache → policy map →
verdicts on addresses flow (cidr_util.py holds the shared inputs)."""
import numpy as np
import pytest

import cidr_util as CU
from cilium_amd import _native as N
from cilium_amd import resolve as R
from cilium_amd.classifier import L4_TUPLE_DTYPE
from cilium_amd.selcache import unpack_rows
from selcache_expand_util import entries_to_dict
from test_cidr import _fromcidr_case, _recs, _set_raw

pytestmark = pytest.mark.gpu
KAT = CU.KAT
Sel = R.EndpointSelector.of


@pytest.fixture()
def sc(gpu):
    s = gpu.selector_cache()
    yield s
    s.destroy()


@pytest.fixture()
def sc2(gpu):
    s = gpu.selector_cache()
    yield s
    s.destroy()


@pytest.mark.parametrize("c", [0, 1, 63, 64, 65])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_gpu_shapes(sc, sc2, n, c):
    CU.check_shape(sc, sc2, n, c, 48, diag_cpu=False)


def test_gpu_big_shape(sc, sc2):
    """N = 100 ends the label section mid-word, C = 1,100 gives a second
    prefix workgroup with a ragged last wave, S = 257 a second selector chunk
    of one selector."""
    CU.check_shape(sc, sc2, 100, 1100, 257, diag_cpu=False)


def test_gpu_pool(sc, sc2):
    """The differential pool (every u32 boundary of the compare, both /0s,
    mapped prefixes, non-canonical keys, every operator) through the kernels."""
    prefixes, sels = CU.pool_prefixes(), CU.pool_selectors()
    CU.load_pair(sc, sc2, CU.LABEL_CACHE, prefixes)
    n, c = len(CU.LABEL_CACHE), len(prefixes)
    want = CU.oracle_match(sels, CU.explicit_cache(CU.LABEL_CACHE, prefixes))
    got = sc.match(sels)
    CU.check_bits(got, sc2.match(sels), want, n, c, "pool, kernel")
    assert np.array_equal(got, sc.match(sels, diag_cpu=True))


def test_gpu_reach_expand_entries(sc, sc2):
    """A repository mixing label rules and CIDR rules, L3-only and with
    toPorts, 5 endpoints: reach and expansion equal the explicit-label
    cache's, and endpoint_policy_map_entries equals
    resolve.endpoint_policy_map_state over the combined identity cache."""
    repo, full = CU.check_reach_expand_equal(sc, sc2, diag_cpu=False)
    CU.check_states(sc, repo, full, False, entries_to_dict)
    for (k1, p1), (k2, p2) in zip(sc.endpoint_policy_map_entries(CU.ENDPOINTS),
                                  sc2.endpoint_policy_map_entries(CU.ENDPOINTS)):
        assert np.array_equal(k1, k2) and np.array_equal(p1, p2)


def test_gpu_section_replacement(sc):
    labels, prefixes, sels, full, want = CU.shape_case(65, 63)
    sc.set_identities(labels)
    sc.set_repository(CU.mixed_repository())
    label_only = sc.match(sels)
    sc.set_cidr_identities(prefixes)
    assert np.array_equal(unpack_rows(sc.match(sels), 128), want)
    # the label section alone: the prefix section moves to the new boundary, the rule matrix is republished
    sc.set_identities(dict(list(labels.items())[:10]))
    moved = unpack_rows(sc.match(sels), 73)
    assert np.array_equal(moved[:, :10], want[:, :10]) and np.array_equal(moved[:, 10:], want[:, 65:])
    assert np.array_equal(sc.match(None), sc.match(None, diag_cpu=True))
    ing, eg, fl = sc.reach(list(labels)[:5])
    ing2, eg2, fl2 = sc.reach(list(labels)[:5], diag_cpu=True)
    assert np.array_equal(ing, ing2) and np.array_equal(eg, eg2) and np.array_equal(fl, fl2)
    # the prefix section alone, then none
    sc.set_identities(labels)
    sc.set_cidr_identities(dict(list(prefixes.items())[:3]))
    assert np.array_equal(unpack_rows(sc.match(sels), 68), np.hstack([want[:, :65], want[:, 65:68]]))
    # an invalid record leaves the tables as they were
    before = sc.match(sels)
    assert _set_raw(sc, [1, 2], _recs((4, 8, (10,)), (4, 33, (10,)))) == N.CG_INVALID_ARGUMENT
    assert _set_raw(sc, [1], _recs((7, 8, (10,)))) == N.CG_INVALID_ARGUMENT
    assert np.array_equal(sc.match(sels), before)
    sc.set_cidr_identities({})
    assert sc.info()["identities"] == 65 and np.array_equal(sc.match(sels), label_only)


def test_gpu_e2e(gpu):
    """toCIDRSet 10.0.0.0/8 except 10.96.0.0/12 + toPorts 80/TCP, a /32
    toCIDR without ports and an IPv6 toCIDR, enforcement always: allocator →
    ipcache + selector cache → sync_policy_maps → verdicts_via_ipcache (v4
    and v6) against the brute-force evaluation of the rule text."""
    CU.run_e2e(gpu, on_gpu=True)


@pytest.mark.parametrize("suite", KAT["from_cidr_and_labels"]["suites"], ids=lambda s: s["name"])
def test_gpu_from_cidr_and_labels(gpu, sc, suite):
    """Policies.go:840-920: fromCIDR beside a label rule, through the synced
    map and policy_can_access_ingress with the identities given; the CIDR
    rule does not admit app3's identity."""
    repo, labels, prefixes, httpd1, asserts = _fromcidr_case(suite)
    sc.set_identities(labels)
    sc.set_cidr_identities(prefixes)
    sc.set_repository(repo)
    pm = gpu.policy_map()
    sc.sync_policy_maps([httpd1], [pm])
    t = np.zeros(len(asserts), L4_TUPLE_DTYPE)
    for i, (ident, _) in enumerate(asserts):
        t[i] = (ident, 0, 1, N.CG_L4_F_INGRESS, 100)
    got = pm.verdicts(t, mode=N.CG_L4_INGRESS) >= 0
    pm.destroy()
    assert got.tolist() == [w for _, w in asserts]


def test_gpu_egress_to_world_cidr(gpu, sc):
    CU.run_egress_world(gpu, sc, on_gpu=True)
