"""l4_array_kernel against the per-map path: verdicts and counters on twin
maps, empty slots inside a wave, hot entries, the fused ipcache forms, the
snapshot rule and the device entry."""
import threading

import numpy as np
import pytest

import l4_array_util as U
from cilium_amd import _native as N
from cilium_amd import synth
from cilium_amd.classifier import L4_TUPLE_DTYPE
from cilium_amd.policy import htons

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1000, U.N_TUPLES]


def _layout(run):
    """The shared tuples rearranged into runs of `run` tuples per endpoint
    (each position takes the next tuple drawn for its slot's table)."""
    lxc0, t0 = U.tuples_round_robin()
    if run == 1:
        return lxc0, t0
    lxc = np.array(U.SLOTS, np.uint16)[(np.arange(U.N_TUPLES) // run) % len(U.SLOTS)]
    t = np.zeros(U.N_TUPLES, L4_TUPLE_DTYPE)
    for slot in U.SLOTS:
        idx, pool = np.flatnonzero(lxc == slot), t0[lxc0 == slot]
        t[idx] = pool[np.arange(len(idx)) % len(pool)]
    return lxc, t


@pytest.fixture
def world(gpu):
    """The array over one set of maps, and a twin set with the same entries
    for the per-map route, so that the two routes' counters are independent."""
    maps, twins = U.build_maps(gpu), U.build_maps(gpu)
    arr = U.build_array(gpu, maps)
    yield arr, maps, twins
    arr.destroy()
    for pm in maps + twins:
        pm.destroy()


def _assert_counters_equal(maps, twins):
    for pm, tw in zip(maps, twins):
        assert U.counters(pm) == U.counters(tw)


# runs of 1 (round-robin: no two neighbours share a table), of 64 (aligned to
# the waves: every wave names one slot) and of 37 (waves of two or three slots)
@pytest.mark.parametrize("run", [1, 64, 37])
def test_parity_with_per_map_path(world, run):
    arr, maps, twins = world
    lxc, t = _layout(run)
    for k, n in enumerate(SIZES):
        mode = U.MODES[(k + run) % len(U.MODES)]
        got = arr.verdicts(lxc[:n], t[:n], mode)
        assert np.array_equal(got, arr.eval_host_diag(lxc[:n], t[:n], mode)), (n, mode)
        # the map in two slots: its twin is fed with both slots' tuples
        exp = U.expected_per_map(twins, lxc[:n], t[:n], mode, lambda pm, x: pm.verdicts(x, mode))
        assert np.array_equal(got, exp), (n, mode)
    _assert_counters_equal(maps, twins)
    assert any(e[5] for e in U.counters(maps[3])) and any(e[5] for e in U.counters(maps[2]))


def test_every_mode_at_full_size(world):
    arr, maps, twins = world
    lxc, t = U.tuples_round_robin()
    for mode in U.MODES:
        got = arr.verdicts(lxc, t, mode)
        assert np.array_equal(got, U.expected_host(maps, lxc, t, mode)), mode
        assert np.array_equal(got, U.expected_per_map(twins, lxc, t, mode, lambda pm, x: pm.verdicts(x, mode)))
        assert (got[lxc == U.EMPTY_SLOT] == N.CG_DROP_MISSED_TAIL_CALL).all()
    _assert_counters_equal(maps, twins)


def _exact_keys(table_index, count, egress=0):
    """`count` exact {id, port, proto} keys of a table, in the given direction."""
    keys = U.tables()[table_index][0]
    k = keys[(keys["sec_label"] != 0) & (keys["dport"] != 0) & (keys["egress"] == egress)]
    assert len(k) >= count
    return k[:count]


def _tuples_for(keys, lens):
    t = np.zeros(len(keys), L4_TUPLE_DTYPE)
    t["identity"], t["dport"], t["proto"] = keys["sec_label"], keys["dport"], keys["protocol"]
    t["flags"] = keys["egress"] ^ 1
    t["len"] = lens
    return t


def test_empty_slots_in_a_mixed_wave(world):
    arr, maps, twins = world
    t = _tuples_for(_exact_keys(3, 64), 100 + np.arange(64))
    lxc = np.where(np.arange(64) % 2 == 0, 300, U.EMPTY_SLOT).astype(np.uint16)
    for mode in (N.CG_L4_INGRESS, N.CG_L4_CAN_ACCESS | N.CG_L4_IGNORE_DROP, N.CG_L4_EGRESS | N.CG_L4_IGNORE_DROP):
        got = arr.verdicts(lxc, t, mode)
        assert (got[1::2] == N.CG_DROP_MISSED_TAIL_CALL).all()
        assert np.array_equal(got[0::2], twins[3].verdicts(t[0::2], mode))
    _assert_counters_equal(maps, twins)  # counters only from the even lanes
    # the ingress keys themselves: hit by the first two calls on the even lanes, never on the odd ones
    got = {e[:4]: (e[5], e[6]) for e in U.counters(maps[3])}
    for i in range(64):
        key = (int(t["identity"][i]), int(t["dport"][i]), int(t["proto"][i]), 0)
        assert got[key] == ((2, 2 * (100 + i)) if i % 2 == 0 else (0, 0))


def test_hot_entries_count_exactly(world):
    """Every lane of every wave adds to one entry; then 64 entries of two maps
    interleaved.  Packets and bytes are exact sums (lengths past 16 bits and
    one past 31 bits included)."""
    arr, maps, _ = world
    rng = np.random.default_rng(5)
    hot = _exact_keys(3, 1)
    lens = rng.integers(64, 1501, 4096).astype(np.uint32)
    lens[[0, 77, 4095]] = [70_000, 65_536, 0xFFFF_FFF0]
    t1 = _tuples_for(np.repeat(hot, 4096), lens)
    assert (arr.verdicts(np.full(4096, 65535, np.uint16), t1) >= 0).all()
    # 32 entries of the 64-entry map (slot 7) and 32 of the big one (slot 300), interleaved
    k2 = np.concatenate([_exact_keys(2, 16, 0), _exact_keys(2, 16, 1), _exact_keys(3, 33)[1:]])
    which = rng.integers(0, 32, 4096)
    in_big = np.arange(4096) % 2 == 1
    pick = np.where(in_big, 32 + which, which)
    lens2 = rng.integers(64, 70_000, 4096).astype(np.uint32)
    t2 = _tuples_for(k2[pick], lens2)
    lxc2 = np.where(in_big, 300, 7).astype(np.uint16)
    assert (arr.verdicts(lxc2, t2, N.CG_L4_CAN_ACCESS) >= 0).all()
    want = {(3, int(hot[0]["sec_label"]), int(hot[0]["dport"]), int(hot[0]["protocol"]), 0):
            (4096, int(lens.astype(np.uint64).sum()))}
    for j in range(64):
        sel = pick == j
        key = (2 if j < 32 else 3, int(k2[j]["sec_label"]), int(k2[j]["dport"]), int(k2[j]["protocol"]),
               int(k2[j]["egress"]))
        assert key not in want
        want[key] = (int(sel.sum()), int(lens2[sel].astype(np.uint64).sum()))
    for m in (2, 3):
        got = {(m,) + e[:4]: (e[5], e[6]) for e in U.counters(maps[m]) if e[5] or e[6]}
        assert got == {k: v for k, v in want.items() if k[0] == m and v[0]}


IPC_ENTRIES = [
    ("0.0.0.0/0", 260, 0), ("10.0.0.0/8", 261, 0), ("10.1.0.0/16", 262, 0),
    ("10.1.2.0/24", 0, 0),  # sec_label 0 shadows the /16: WORLD
    ("10.1.2.3/32", 263, 7), ("::/0", 264, 0), ("fd00::/8", 265, 0), ("fd00:1::/64", 266, 0),
    ("fd00:1::/96", 0, 0), ("fd00:1::5/128", 267, 7),
]


@pytest.mark.parametrize("mode", [N.CG_L4_INGRESS, N.CG_L4_EGRESS])
def test_fused_ipcache_forms(gpu, world, mode):
    arr, maps, _ = world
    from cilium_amd.classifier import IPCache
    rng = np.random.default_rng(3)
    ik, iv = synth.ipcache_entries(200, n_nodes=8, seed=4)
    ids = np.unique(U.tables()[3][0]["sec_label"])
    iv = iv.copy()
    iv[:, 0] = rng.choice(np.append(ids, [0, 2, 999_999]), len(iv))
    ik = np.concatenate([ik, IPCache._keys([c for c, _, _ in IPC_ENTRIES])])
    iv = np.concatenate([iv, np.array([[i, t] for _, i, t in IPC_ENTRIES], np.uint32)])
    ic = gpu.ipcache()
    ic.update(ik, iv)
    a4, a6 = synth.ipcache_addresses(1000, ik, seed=5)
    fixed4 = np.array([int.from_bytes(bytes(x), "little") for x in ([10, 1, 2, 3], [10, 1, 2, 9], [10, 1, 9, 9],
                                                                     [10, 9, 9, 9], [99, 9, 9, 9])], np.uint32)
    a4[:5] = fixed4
    a6[0] = [0xfd, 0, 0, 1] + [0] * 11 + [5]
    a6[1] = [0xfd, 0, 0, 1] + [0] * 11 + [6]
    a6[2] = [0xfe, 0x80] + [0] * 13 + [1]
    i4, i6 = ic.resolve(a4, a6)
    assert i4[:5, 0].tolist() == [263, N.CG_WORLD_ID, 262, 261, 260]
    assert i6[:3, 0].tolist() == [267, N.CG_WORLD_ID, 264]
    lxc0, t0 = U.tuples_round_robin()
    for remote, idents in ((a4, i4[:, 0]), (a6, i6[:, 0])):
        n = len(remote)
        lxc, t = lxc0[:n], t0[:n].copy()
        resolved = t.copy()
        resolved["identity"] = idents
        t["identity"] = 0xDEAD_BEEF  # the fused form must not look at it
        got = arr.verdicts_via_ipcache(ic, remote, lxc, t, mode)
        assert np.array_equal(got, arr.verdicts(lxc, resolved, mode))
        assert (got[lxc == U.EMPTY_SLOT] == N.CG_DROP_MISSED_TAIL_CALL).all() and (got >= 0).any()
    ic.destroy()


def test_snapshot_follows_updates(gpu):
    a, b = gpu.policy_map(), gpu.policy_map()
    b.allow(50, 443, 6, 0, 0)
    arr = gpu.policy_array()
    arr.set_many([10, 11, 12], [a, b, a])
    t = np.zeros(3, L4_TUPLE_DTYPE)
    t["identity"], t["dport"], t["proto"], t["len"] = [9, 50, 9], [htons(80), htons(443), htons(80)], 6, 100
    lxc = np.array([10, 11, 12], np.uint16)
    assert arr.verdicts(lxc, t).tolist() == [N.CG_DROP_POLICY, 0, N.CG_DROP_POLICY]
    a.allow(9, 80, 6, 0, 8080)  # a member map changes between two calls
    assert arr.verdicts(lxc, t).tolist() == [htons(8080), 0, htons(8080)]
    arr.clear(12)
    assert arr.verdicts(lxc, t).tolist() == [htons(8080), 0, N.CG_DROP_MISSED_TAIL_CALL]
    arr.set(12, b)
    t["identity"][2], t["dport"][2] = 50, htons(443)
    assert arr.verdicts(lxc, t).tolist() == [htons(8080), 0, 0]
    a.destroy()  # its slot is empty from now on; the others are unaffected
    assert arr.get(10) is None
    assert arr.verdicts(lxc, t).tolist() == [N.CG_DROP_MISSED_TAIL_CALL, 0, 0]
    assert [(e[5], e[6]) for e in U.counters(b)] == [(7, 700)]
    arr.destroy()
    b.destroy()


def test_concurrent_update_is_seen_whole_or_not_at_all(gpu):
    """One thread classifies 4,096 tuples of one key 50 times while another
    toggles that key's proxy port 200 times: a call sees one value throughout."""
    pm = gpu.policy_map()
    pm.allow(9, 80, 6, 0, 1111)
    arr = gpu.policy_array()
    arr.set(5, pm)
    t = np.zeros(4096, L4_TUPLE_DTYPE)
    t["identity"], t["dport"], t["proto"], t["len"] = 9, htons(80), 6, 1
    lxc = np.full(4096, 5, np.uint16)
    legal = {htons(1111), htons(2222)}
    seen, errors = [], []

    def classify():
        try:
            for _ in range(50):
                seen.append(np.unique(arr.verdicts(lxc, t)).tolist())
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    def toggle():
        try:
            for i in range(200):
                pm.allow(9, 80, 6, 0, 2222 if i % 2 == 0 else 1111)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=classify), threading.Thread(target=toggle)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors
    assert len(seen) == 50 and all(len(v) == 1 and v[0] in legal for v in seen), seen
    assert [(e[5], e[6]) for e in U.counters(pm)] == [(50 * 4096, 50 * 4096)]
    arr.destroy()
    pm.destroy()


def test_dev_entry_on_a_side_stream(world):
    torch = pytest.importorskip("torch")
    arr, maps, twins = world
    lxc, t = _layout(37)
    dev = torch.device("cuda", 0)
    d_lxc = torch.from_numpy(lxc.view(np.int16).copy()).to(dev)
    d_t = torch.from_numpy(t.view(np.uint8).reshape(-1, 12).copy()).to(dev)
    d_out = torch.full((len(t),), 9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    arr.verdicts_dev(d_lxc, d_t, len(t), d_out, stream=side.cuda_stream, mode=N.CG_L4_INGRESS)
    side.synchronize()
    got = d_out.cpu().numpy()
    exp = U.expected_per_map(twins, lxc, t, N.CG_L4_INGRESS, lambda pm, x: pm.verdicts(x, N.CG_L4_INGRESS))
    assert np.array_equal(got, exp)
    _assert_counters_equal(maps, twins)
    assert np.array_equal(arr.verdicts(lxc, t, N.CG_L4_INGRESS), got)  # the _host entry


def test_sync_policy_array_on_the_device(gpu):
    idc = synth.identity_cache(200)
    repo = synth.label_repository(30)
    sc = gpu.selector_cache()
    sc.set_identities(idc)
    sc.set_repository(repo)
    eps = list(idc)[:3]
    arr = gpu.policy_array()
    sc.sync_policy_array(eps, [3, 4, 5], arr)
    from cilium_amd.classifier import PolicyMap
    for lxc, w in zip([3, 4, 5], sc.endpoint_policy_map_states(eps)):
        got = {(k.Identity, k.DestPort, k.Nexthdr, k.TrafficDirection): en.ProxyPort
               for k, en in PolicyMap.attach(gpu, arr.get(lxc)).dump_to_slice()}
        assert got == {(k.Identity, htons(k.DestPort), k.Nexthdr, k.TrafficDirection): htons(v)
                       for k, v in w.items()}
