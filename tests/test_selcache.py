"""Selector cache on the CPU: the compiled tables of cilium_amd.selcache walked
by the library's host walkers (cg_diag_selcache_*) against resolve.py —
EndpointSelector.matches, Repository.allows_{ingress,egress}_label_access,
get_rules_matching and endpoint_policy_map_state — bit for bit.  The same
checks run through the kernels in test_selcache_gpu.py."""
import numpy as np
import pytest

import selcache_util as U
from cilium_amd import _native as N
from cilium_amd import resolve as R
from cilium_amd.selcache import _SelectorTable


@pytest.fixture()
def sc(host):
    s = host.selector_cache()
    yield s
    s.destroy()


def test_operator_kat(sc):
    U.check_operator_kat(sc, diag_cpu=True)


def test_unknown_operator_rejected(sc):
    sc.set_identities({1: {"k8s:app": "a"}})
    bad = R.EndpointSelector.of(None, [("k8s:app", "Near", ("a",))])
    with pytest.raises(N.CiliumGPUError) as ei:
        sc.match([bad], diag_cpu=True)
    assert ei.value.code == N.CG_POLICY_REJECTED
    # the rule set is all or nothing: a bad selector leaves the previous one in place
    repo, cache = U.rule_can_reach_repo()
    sc.set_identities(cache)
    sc.set_repository(repo)
    before = sc.info()
    broken = R.Repository([R.Rule(R.EndpointSelector.of({"bar": ""}), [R.IngressRule([bad])])])
    with pytest.raises(N.CiliumGPUError) as ei:
        sc.set_repository(broken)
    assert ei.value.code == N.CG_POLICY_REJECTED
    assert sc.info() == before
    U.check_rule_can_reach(sc, diag_cpu=True)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_match_differential(sc, n):
    U.check_match(sc, n, diag_cpu=True)


def test_no_identities(sc):
    sc.set_identities({})
    bits = sc.match(U.random_selectors(5, 1), diag_cpu=True)
    assert bits.shape == (5, 0)
    assert sc.identities_of([R.WILDCARD], diag_cpu=True) == [[]]


@pytest.mark.parametrize("case", U.REACH, ids=lambda c: c["case"])
def test_golden_reach(sc, case):
    U.check_golden_reach(sc, case, diag_cpu=True)


def test_rule_can_reach(sc):
    U.check_rule_can_reach(sc, diag_cpu=True)


def test_empty_repository(sc):
    U.check_empty_repository(sc, diag_cpu=True)


@pytest.mark.parametrize("seed", [11, 12])
def test_reach_random(sc, seed):
    U.check_reach_random(sc, seed, diag_cpu=True)


def test_reach_follows_new_tables(sc):
    """set_identities / set_repository replace whole tables: a smaller cache
    and another repository leave nothing of the earlier ones behind."""
    U.check_reach_random(sc, 11, diag_cpu=True)
    U.check_rule_can_reach(sc, diag_cpu=True)
    U.check_match(sc, 65, diag_cpu=True)


def test_map_states_minikube(sc):
    U.check_map_states(sc, U.minikube_repo(), U.MK_CACHE, diag_cpu=True)


def test_map_states_random(sc):
    cache = U.random_identities(40, 5)
    cache[1] = {"reserved:host": ""}
    cache[5] = {"reserved:init": "", "k8s:app": "a"}
    U.check_map_states(sc, U.random_repository(12, 21, l7=True), cache, diag_cpu=True)


def test_malformed_tables_rejected(sc):
    sc.set_identities({1: {"k8s:app": "a"}})
    with pytest.raises(N.CiliumGPUError) as ei:  # an endpoint index outside the table
        sc.reach_indices(np.array([7], np.uint32), diag_cpu=True)
    assert ei.value.code == N.CG_INVALID_ARGUMENT
    out = np.zeros(4, np.uint64)
    tab = _SelectorTable([R.WILDCARD] * 3)
    # room for fewer than S * W words
    assert N.lib.cg_diag_selcache_match_host(sc.cl.h, sc.id, tab.ref(), N.ptr(out), 2, 1) == N.CG_INVALID_ARGUMENT
    assert N.lib.cg_selcache_destroy(sc.cl.h, 0xFFFF) == N.CG_NOT_FOUND


def test_host_handle_refuses(sc):
    """No CPU fallback: on a handle without a GPU match and reach return
    CG_NO_DEVICE while the tables still compile."""
    repo, cache = U.rule_can_reach_repo()
    sc.set_identities(cache)
    sc.set_repository(repo)
    with pytest.raises(N.CiliumGPUError) as ei:
        sc.match([R.WILDCARD])
    assert ei.value.code == N.CG_NO_DEVICE
    with pytest.raises(N.CiliumGPUError) as ei:
        sc.reach([10])
    assert ei.value.code == N.CG_NO_DEVICE
    with pytest.raises(N.CiliumGPUError) as ei:
        sc.endpoint_policy_map_states([10])
    assert ei.value.code == N.CG_NO_DEVICE


def test_synth_generators():
    from cilium_amd import synth
    a, b = synth.identity_cache(300, seed=3), synth.identity_cache(300, seed=3)
    assert a == b and len(a) == 300 and all(len(v) == 8 for v in a.values())
    assert {k.split(":")[0] for v in a.values() for k in v} == {"k8s", "container", "any"}
    r1, r2 = synth.label_repository(50, seed=3), synth.label_repository(50, seed=3)
    assert r1.rules == r2.rules and len(r1.rules) == 50
