"""The policy program array on a host-only handle: the slot API, the host
evaluator against the per-map evaluator, and SelectorCache.sync_policy_array."""
import numpy as np
import pytest

import l4_array_util as U
from cilium_amd import _native as N
from cilium_amd import resolve, synth
from cilium_amd.classifier import L4_TUPLE_DTYPE
from cilium_amd.policy import htons


def _code(fn, *a, **kw):
    with pytest.raises(N.CiliumGPUError) as ei:
        fn(*a, **kw)
    return ei.value.code


def test_slots_round_trip(host):
    arr = host.policy_array()
    a, b = host.policy_map(), host.policy_map()
    assert [arr.get(s) for s in (0, 5, 65535)] == [None, None, None]
    arr.set(5, a)
    arr.set_many([0, 65535, 6], [a, b, a])  # lxc_id 0 and 65535; one map in several slots
    assert [arr.get(s) for s in (0, 5, 6, 65535, 7)] == [a.id, a.id, a.id, b.id, None]
    arr.set(5, b)  # a set slot is overwritten
    arr.clear(6)
    arr.clear(7)  # clearing an empty slot is fine
    assert [arr.get(s) for s in (0, 5, 6, 65535)] == [a.id, b.id, None, b.id]
    arr.clear([0, 5, 65535])
    assert [arr.get(s) for s in (0, 5, 65535)] == [None, None, None]
    arr.set_many([], [])  # n = 0
    assert _code(arr.set, 65536, a) == N.CG_INVALID_ARGUMENT
    arr.destroy()
    a.destroy()
    b.destroy()


def test_set_is_all_or_nothing(host):
    arr = host.policy_array()
    a, b = host.policy_map(), host.policy_map()
    arr.set(3, a)
    unknown = b.id + 1000
    assert _code(arr.set_many, [3, 4, 5], [b, b.id, unknown]) == N.CG_NOT_FOUND
    assert [arr.get(s) for s in (3, 4, 5)] == [a.id, None, None]  # the earlier, valid pairs were not applied
    assert _code(arr.set_many, [4], [0]) == N.CG_NOT_FOUND  # 0 is no map id
    assert N.lib.cg_policy_array_set(host.h, arr.id, None, None, 2) == N.CG_INVALID_ARGUMENT
    arr.destroy()
    a.destroy()
    b.destroy()


def test_destroying_a_member_empties_its_slots(host):
    arr, other = host.policy_array(), host.policy_array()
    a, b = host.policy_map(), host.policy_map()
    arr.set_many([1, 2, 9], [a, b, a])
    other.set(1, a)
    a.destroy()
    assert [arr.get(s) for s in (1, 2, 9)] == [None, b.id, None]
    assert other.get(1) is None
    t = np.zeros(3, L4_TUPLE_DTYPE)
    assert arr.eval_host_diag([1, 2, 9], t).tolist() == [-140, N.CG_DROP_POLICY, -140]
    arr.destroy()
    other.destroy()
    b.destroy()


def test_destroyed_array_is_refused(host):
    arr = host.policy_array()
    pm = host.policy_map()
    arr.destroy()
    assert _code(arr.set, 1, pm) == N.CG_NOT_FOUND
    assert _code(arr.get, 1) == N.CG_NOT_FOUND
    assert _code(arr.clear, 1) == N.CG_NOT_FOUND
    assert _code(arr.destroy) == N.CG_NOT_FOUND
    assert _code(arr.eval_host_diag, [1], np.zeros(1, L4_TUPLE_DTYPE)) == N.CG_NOT_FOUND
    pm.destroy()


def test_modes_and_empty_calls(host):
    arr = host.policy_array()
    t = np.zeros(2, L4_TUPLE_DTYPE)
    for bad in (3, 4, 0x200, 0x103):
        assert _code(arr.eval_host_diag, [0, 1], t, bad) == N.CG_INVALID_ARGUMENT
        assert _code(arr.verdicts, [0, 1], t, bad) == N.CG_INVALID_ARGUMENT
    assert len(arr.eval_host_diag([], t[:0])) == 0  # n = 0
    # an array with nothing set: every slot misses, in every mode
    for mode in U.MODES:
        assert arr.eval_host_diag([0, 65535], t, mode).tolist() == [N.CG_DROP_MISSED_TAIL_CALL] * 2
    arr.destroy()


def test_host_handle_refuses_array_verdicts(host):
    """No CPU fallback, as test_host_handle_refuses_verdicts expects of the other entries."""
    arr = host.policy_array()
    pm = host.policy_map()
    pm.allow(1, 80, 6, 0, 0)
    arr.set(4, pm)
    t = np.zeros(4, L4_TUPLE_DTYPE)
    lxc = np.full(4, 4, np.uint16)
    assert _code(arr.verdicts, lxc, t) == N.CG_NO_DEVICE
    ic = host.ipcache()
    assert _code(arr.verdicts_via_ipcache, ic, np.zeros(4, np.uint32), lxc, t) == N.CG_NO_DEVICE
    assert _code(arr.verdicts_via_ipcache, ic, np.zeros((4, 16), np.uint8), lxc, t) == N.CG_NO_DEVICE
    assert _code(arr.verdicts_dev, lxc, t, 4, np.zeros(4, np.int32)) == N.CG_NO_DEVICE
    assert _code(arr.verdicts_via_ipcache_dev, ic, 4, np.zeros(4, np.uint32), lxc, t, 4,
                 np.zeros(4, np.int32)) == N.CG_NO_DEVICE
    arr.destroy()
    pm.destroy()
    ic.destroy()


@pytest.fixture(scope="module")
def world(host):
    maps = U.build_maps(host)
    arr = U.build_array(host, maps)
    yield arr, maps
    arr.destroy()
    for pm in maps:
        pm.destroy()


@pytest.mark.parametrize("mode", U.MODES)
def test_host_evaluator_matches_per_map_evaluator(world, mode):
    arr, maps = world
    lxc, t = U.tuples_round_robin()
    exp = U.expected_host(maps, lxc, t, mode)
    got = arr.eval_host_diag(lxc, t, mode)
    assert np.array_equal(got, exp)
    assert (got[lxc == U.EMPTY_SLOT] == N.CG_DROP_MISSED_TAIL_CALL).all()
    assert not (got[lxc != U.EMPTY_SLOT] == N.CG_DROP_MISSED_TAIL_CALL).any()


def test_tuples_exercise_every_path(world):
    """The shared tuple set reaches what it is meant to reach: on the big map
    all three probe kinds hit, fragments and CB_POLICY decide verdicts, and
    tables with different bucket masks are in play."""
    arr, maps = world
    lxc, t = U.tuples_round_robin()
    assert all(lxc[i] != lxc[i + 1] for i in range(len(lxc) - 1))
    big = t[lxc == 300]
    v = maps[3].eval_host_diag(big)
    keys, _, _ = U.tables()[3]
    kset = {(int(k["sec_label"]), int(k["dport"]), int(k["protocol"]), int(k["egress"])) for k in keys}
    kinds = set()
    for x in big[v >= 0]:
        eg, frag = int(x["flags"] & 1) ^ 1, bool(x["flags"] & 2)
        if not frag and (int(x["identity"]), int(x["dport"]), int(x["proto"]), eg) in kset:
            kinds.add("l4")
        elif (int(x["identity"]), 0, 0, eg) in kset:
            kinds.add("l3")
        elif not frag and (0, int(x["dport"]), int(x["proto"]), eg) in kset:
            kinds.add("wildcard")
        else:
            assert x["flags"] & N.CG_L4_F_CB_POLICY
            kinds.add("cb")
    assert kinds == {"l4", "l3", "wildcard", "cb"}
    assert (v == N.CG_DROP_FRAG_NOSUPPORT).any() and (v == N.CG_DROP_POLICY).any() and (v > 0).any()
    for m in (1, 2):  # the one-entry map and the 64-entry map hit as well
        assert (maps[m].eval_host_diag(t[lxc == {1: 1, 2: 7}[m]]) >= 0).any()
    assert (t["identity"] >= 900_000).any()


def test_sync_policy_array(host):
    idc = synth.identity_cache(200)
    repo = synth.label_repository(30)
    sc = host.selector_cache()
    sc.set_identities(idc)
    sc.set_repository(repo)
    eps = list(idc)[:3]
    arr = host.policy_array()
    mine = host.policy_map()
    mine.allow(12345, 1, 6, 0, 0)  # a stale entry the sync has to delete
    arr.set(40, mine)
    res = sc.sync_policy_array(eps, [40, 41, 65535], arr, diag_cpu=True)
    assert len(res) == 3 and res[0][1] == 1
    assert arr.get(40) == mine.id and arr.get(41) not in (None, mine.id) and arr.get(65535) is not None
    want = sc.endpoint_policy_map_states(eps, diag_cpu=True)
    from cilium_amd.classifier import PolicyMap
    for e, lxc, w in zip(eps, [40, 41, 65535], want):
        assert w == resolve.endpoint_policy_map_state(repo, idc[e], idc)
        got = {(k.Identity, k.DestPort, k.Nexthdr, k.TrafficDirection): en.ProxyPort
               for k, en in PolicyMap.attach(host, arr.get(lxc)).dump_to_slice()}
        assert got == {(k.Identity, htons(k.DestPort), k.Nexthdr, k.TrafficDirection): htons(v)
                       for k, v in w.items()}
    assert sc.sync_policy_array(eps, [40, 41, 65535], arr, diag_cpu=True) == [(0, 0)] * 3  # already in the desired state
