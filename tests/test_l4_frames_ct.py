"""The conntrack lookup of the frames route on a host-only handle: the host
evaluator (ct_walk.h over host_view()) against the route without conntrack on
an empty map, against the Python restatement of ct_lookup4/6 and the tail of
ipv{4,6}_policy, and against the hand-written cases; near-miss keys, scopes,
apply, the map API and the tables' probe chains."""
import numpy as np
import pytest

import ct_util as T
import frames_util as F
import l4_array_util as U
from cilium_amd import _native as N
from cilium_amd.classifier import CT_ENTRY_DTYPE, CT_KEY_DTYPE, CT_RECORD_DTYPE

COMBO_IDS = [("lxc" if c["lxc"] else "epmap") + "-" + ("labels" if c["lab"] else "ipcache") for c in F.COMBOS]


def _code(fn, *a, **kw):
    with pytest.raises(N.CiliumGPUError) as ei:
        fn(*a, **kw)
    return ei.value.code


@pytest.fixture(scope="module")
def world(host):
    maps = U.build_maps(host)
    arr = U.build_array(host, maps)
    ep, ipc = F.build_endpoints(host), F.build_ipcache(host)
    yield arr, maps, ep, ipc
    for x in (arr, ep, ipc, *maps):
        x.destroy()


@pytest.fixture
def golden(host):
    arr, pm, ct, raw, off, kw, cases = T.golden_world(host)
    yield arr, pm, ct, raw, off, kw, cases
    for x in (arr, pm, ct):
        x.destroy()


# ------------------------------------------------------------ empty map ----
@pytest.mark.parametrize("ci", range(4), ids=COMBO_IDS)
def test_empty_map_equals_the_route_without_conntrack(host, world, ci):
    arr, maps, ep, ipc = world
    raw, off, pkt_len, labels, lxc = F.shared_frames()
    a, _ = F.resolver_args(F.COMBOS[ci], ep, ipc, lxc, labels)
    ct = host.conntrack_map()
    for ignore_drop in (False, True):
        v0, i0 = arr.frame_eval_host_diag(raw, off, pkt_len=pkt_len, ignore_drop=ignore_drop, info=True, **a)
        v, info, rec = arr.frame_eval_host_diag(raw, off, pkt_len=pkt_len, ignore_drop=ignore_drop, info=True,
                                                conntrack=ct, **a)
        assert np.array_equal(v, v0) and info.tobytes() == i0.tobytes()
        done = (info["t"]["flags"] & N.CG_L4_F_INGRESS) != 0
        create = done & (v >= 0)
        assert create.any() and (~done).any()
        assert (rec["op"][create] == T.OP_CREATE).all() and (rec["op"][~create] == T.OP_NONE).all()
        assert (rec["state"][done] == N.CG_CT_STATE_NEW).all()
        assert rec[~done].tobytes() == bytes(64 * int((~done).sum()))  # state none: an all-zero record
    ct.destroy()


# ------------------------------------------------- evaluator = oracle ----
@pytest.mark.parametrize("ci", range(4), ids=COMBO_IDS)
def test_host_evaluator_equals_the_oracle(host, world, ci):
    arr, maps, ep, ipc = world
    raw, off, pkt_len, labels, lxc = F.shared_frames()
    a, _ = F.resolver_args(F.COMBOS[ci], ep, ipc, lxc, labels)
    items, values = T.shared_table(ci)
    ct = T.build_map(host, items, values)
    for ignore_drop in (False, True):
        v, info, rec = arr.frame_eval_host_diag(raw, off, pkt_len=pkt_len, ignore_drop=ignore_drop, info=True,
                                                conntrack=ct, **a)
        ev, einfo, erec, _ = T.shared_expected(ci, ignore_drop)
        bad = np.flatnonzero(v != ev)
        assert not len(bad), (bad[:5], v[bad[:5]], ev[bad[:5]])
        assert np.array_equal(info, einfo)
        T.assert_records_equal(rec, erec, COMBO_IDS[ci])
    # about a quarter each reply, established and new among the frames that reach the lookup; related and none too
    ev, _, erec, _ = T.shared_expected(ci, False)
    n_done = int((erec["state"] != 0).sum())
    share = {s: int((erec["state"] == s).sum()) / n_done for s in range(1, 5)}
    assert share[N.CG_CT_STATE_REPLY] > 0.2 and share[N.CG_CT_STATE_ESTABLISHED] > 0.2, share
    assert share[N.CG_CT_STATE_NEW] > 0.2 and share[N.CG_CT_STATE_RELATED] > 0.002, share
    assert (erec["state"] == 0).sum() > len(erec) // 20
    assert {T.OP_NONE, T.OP_CREATE, T.OP_DELETE} == set(erec["op"].tolist())
    assert (erec["rev_nat_index"] != 0).any() and (erec["loopback"] != 0).any()
    est = erec["state"] == N.CG_CT_STATE_ESTABLISHED
    assert (est & (ev >= 0)).any() and (est & (ev < 0)).any()  # allowed and denied (the proxy port: the hand-written cases)
    ct.destroy()


def test_global_map_looks_up_scope_zero(host, world):
    arr, maps, ep, ipc = world
    raw, off, pkt_len, labels, lxc = F.shared_frames()
    a, _ = F.resolver_args(F.COMBOS[0], ep, ipc, lxc, labels)
    items, values = T.shared_table(0, True)
    ct = T.build_map(host, items, values, global_map=True)
    v, info, rec = arr.frame_eval_host_diag(raw, off, pkt_len=pkt_len, info=True, conntrack=ct, **a)
    ev, _, erec, _ = T.shared_expected(0, False, True)
    assert np.array_equal(v, ev)
    T.assert_records_equal(rec, erec, "global")
    assert (rec["key"]["scope"] == 0).all() and (rec["state"] >= N.CG_CT_STATE_ESTABLISHED).any()
    k = T.keys_array(items[:1])
    k["scope"] = 3
    assert _code(ct.update, k) == N.CG_INVALID_ARGUMENT  # a global map holds scope 0 only
    ct.destroy()


# ------------------------------------------------------ golden cases ----
def test_hand_written_cases(golden):
    arr, pm, ct, raw, off, kw, cases = golden
    assert len(cases) == 13
    v, info, rec = arr.frame_eval_host_diag(raw, off, info=True, conntrack=ct, **kw)
    T.check_golden(cases, v, rec)
    # the oracle reads the same cases the same way
    g = T.load_golden()
    table = {(k.Identity, k.DestPort, k.Nexthdr, k.TrafficDirection): e.ProxyPort for k, e in pm.dump_to_slice()}
    items = [T.golden_item(e) for c in cases for e in c["entries"]]
    ev, _, erec, _ = T.evaluate(F.split(raw, off), {g["slot"]: (0, table)}, T.ctmap_of(items), **kw)
    assert np.array_equal(v, ev)
    T.assert_records_equal(rec, erec, "golden")


# ---------------------------------------------------------- near misses ----
def _run(arr, raw, off, ct, kw):
    return arr.frame_eval_host_diag(raw, off, info=True, conntrack=ct, **kw)


def test_near_miss_keys_all_miss(host):
    T.near_miss_check(host, _run)


# --------------------------------------------------------------- scope ----
def test_scope_separates_endpoints(host, world):
    arr, maps, ep, ipc = world
    g = T.load_golden()
    f = bytes.fromhex(g["frames"][0]["hex"])
    raw, off = F.join([f, f])
    kw = dict(lxc_ids=[7, 300], src_labels=[1, 1])
    item = T.entry_for(f, "reply", 7)
    ct = T.build_map(host, [item])
    _, _, rec = arr.frame_eval_host_diag(raw, off, info=True, conntrack=ct, **kw)
    assert rec["state"].tolist() == [N.CG_CT_STATE_REPLY, N.CG_CT_STATE_NEW]
    assert rec["key"]["scope"].tolist() == [7, 300]
    ct.destroy()
    ct = T.build_map(host, [(0,) + item[1:]], global_map=True)
    v, _, rec = arr.frame_eval_host_diag(raw, off, info=True, conntrack=ct, **kw)
    assert rec["state"].tolist() == [N.CG_CT_STATE_REPLY] * 2 and v.tolist() == [0, 0]
    ct.destroy()


# --------------------------------------------------------------- apply ----
def _tcp4(src, sport, dport, flags=0x02, dst="10.0.0.5"):
    import ipaddress
    import struct
    ip = struct.pack(">BBHHHBBH", 0x45, 0, 40, 0, 0x4000, 64, 6, 0) + ipaddress.ip_address(src).packed + \
        ipaddress.ip_address(dst).packed
    return bytes(12) + b"\x08\x00" + ip + struct.pack(">HHIIBBHHH", sport, dport, 1, 0, 0x50, flags, 1000, 0, 0)


def _icmp4_unreach(src, dst="10.0.0.5"):
    import ipaddress
    import struct
    ip = struct.pack(">BBHHHBBH", 0x45, 0, 56, 0, 0x4000, 64, 1, 0) + ipaddress.ip_address(src).packed + \
        ipaddress.ip_address(dst).packed
    return bytes(12) + b"\x08\x00" + ip + bytes([3, 1]) + bytes(34)


def test_apply_makes_two_calls_behave_like_the_datapath(host):
    pm, arr, ct = host.policy_map(), host.policy_array(), host.conntrack_map()
    pm.allow(1000, 80, 6, 0, 0)
    arr.set(5, pm)
    syn, err = _tcp4("10.1.0.9", 33000, 80), _icmp4_unreach("10.1.0.9")
    raw, off = F.join([syn, err])
    kw = dict(lxc_ids=[5, 5], src_labels=[1000, 1000], pkt_len=[74, 90])
    call = lambda: arr.frame_eval_host_diag(raw, off, info=True, conntrack=ct, **kw)
    v, info, rec = call()
    assert v.tolist() == [0, F.DROP_POLICY] and rec["state"].tolist() == [N.CG_CT_STATE_NEW] * 2
    assert rec["op"].tolist() == [T.OP_CREATE, T.OP_NONE]
    assert ct.apply(rec, pkt_len=kw["pkt_len"], src_labels=info["t"]["identity"]).tolist() == [0, 0]
    # the flow's key and its ICMP related key, both in the TCP map (conntrack.h:722, :756-769)
    keys, vals = ct.dump()
    assert len(keys) == 2 and keys["kind"].tolist() == [N.CG_CT_MAP_TCP] * 2
    flow = keys["nexthdr"] == 6
    assert keys["flags"][flow].tolist() == [T.TUPLE_F_IN] and keys["flags"][~flow].tolist() == [T.TUPLE_F_IN | 2]
    assert keys["nexthdr"][~flow].tolist() == [1] and keys["dport"][~flow].tolist() == [0]
    assert vals["rx_packets"].tolist() == [1, 1] and vals["rx_bytes"].tolist() == [74, 74]
    assert vals["src_sec_id"].tolist() == [1000, 1000]
    assert vals["flags"][~flow].tolist() == [N.CG_CT_E_SEEN_NON_SYN] and vals["flags"][flow].tolist() == [0]
    # the same frame is now ESTABLISHED; the ICMP error is looked up in the ANY map and stays NEW
    v, info, rec = call()
    assert rec["state"].tolist() == [N.CG_CT_STATE_ESTABLISHED, N.CG_CT_STATE_NEW]
    assert v.tolist() == [0, F.DROP_POLICY] and rec["op"].tolist() == [T.OP_NONE, T.OP_NONE]
    # a UDP flow's related key lives in the ANY map, where the ICMP error finds it
    rel = T.entry_for(err, "reply", 5)
    assert rel[1] == T.KIND_ANY and rel[3]["flags"] == T.TUPLE_F_RELATED
    ct.update(T.keys_array([rel]))
    assert call()[2]["state"].tolist() == [N.CG_CT_STATE_ESTABLISHED, N.CG_CT_STATE_RELATED]
    ct.delete(T.keys_array([rel]))
    # the policy changes and denies: DROP_POLICY + DELETE, and after apply the frame reads NEW
    pm.delete(1000, 80, 6, 0)
    v, info, rec = call()
    assert v.tolist() == [F.DROP_POLICY] * 2 and rec["op"].tolist() == [T.OP_DELETE, T.OP_NONE]
    assert rec["key"][0] == keys[flow][0]
    assert ct.apply(rec).tolist() == [0, 0]
    assert ct.apply(rec).tolist() == [0, 0]  # a key already gone is not an error
    v, info, rec = call()
    assert rec["state"].tolist() == [N.CG_CT_STATE_NEW] * 2 and rec["op"].tolist() == [T.OP_NONE] * 2
    assert len(ct.dump()[0]) == 1  # the related key stays until the agent's GC, as in the reference
    for x in (arr, pm, ct):
        x.destroy()


def test_apply_duplicates_and_a_full_map(host):
    pm, arr = host.policy_map(), host.policy_array()
    pm.allow(1000, 80, 6, 0, 0)
    arr.set(5, pm)
    flows = [_tcp4("10.1.0.9", 33000 + i, 80) for i in range(4)]
    frames = [flows[0], flows[0], flows[1], flows[2], flows[1], flows[3]]
    raw, off = F.join(frames)
    n = len(frames)
    kw = dict(lxc_ids=[5] * n, src_labels=[1000] * n)
    plen = np.arange(100, 100 + n, dtype=np.uint32)
    # room for all: duplicate CREATEs leave one pair per flow (the related key is shared by the four flows)
    ct = host.conntrack_map()
    v, info, rec = arr.frame_eval_host_diag(raw, off, info=True, conntrack=ct, **kw)
    assert rec["op"].tolist() == [T.OP_CREATE] * n  # within one call every packet of a new flow reads NEW
    assert ct.apply(rec, pkt_len=plen, src_labels=info["t"]["identity"]).tolist() == [0] * n
    oracle = {}
    assert T.apply(oracle, rec, plen, info["t"]["identity"], 1 << 20).tolist() == [0] * n
    keys, vals = ct.dump()
    assert len(keys) == 5 == len(oracle)
    got = {(int(k["scope"]), int(k["kind"]), T.tuple_bytes(T.record_tuple({"key": k}))):
           (int(e["rx_packets"]), int(e["rx_bytes"]), int(e["src_sec_id"]), int(e["flags"])) for k, e in zip(keys, vals)}
    assert got == {k: (e["rx_packets"], e["rx_bytes"], e["src_sec_id"], e["flags"]) for k, e in oracle.items()}
    ct.destroy()
    # max_entries = 3: flow 0 and the related key, then flow 1; flow 2 and 3 do not fit
    ct = host.conntrack_map(max_entries=3)
    assert ct.max_entries == 3
    _, info, rec = arr.frame_eval_host_diag(raw, off, info=True, conntrack=ct, **kw)
    res = ct.apply(rec, pkt_len=plen, src_labels=info["t"]["identity"])
    oracle = {}
    assert np.array_equal(res, T.apply(oracle, rec, plen, info["t"]["identity"], 3))
    assert res.tolist() == [0, 0, 0, N.CG_DROP_CT_CREATE_FAILED, 0, N.CG_DROP_CT_CREATE_FAILED]
    keys, _ = ct.dump()
    assert len(keys) == 3 and sorted(keys["sport"].tolist()) == sorted(
        [0] + [int(rec["key"]["sport"][i]) for i in (0, 2)])
    # a frame that needs two new keys when one fits writes neither
    ct2 = host.conntrack_map(max_entries=1)
    assert ct2.apply(rec[:1]).tolist() == [N.CG_DROP_CT_CREATE_FAILED] and len(ct2.dump()[0]) == 0
    for x in (arr, pm, ct, ct2):
        x.destroy()


# ------------------------------------------------------------- map API ----
def test_map_api_round_trip(host):
    ct = host.conntrack_map(max_entries=6)
    K = ct.key
    keys = [K("10.0.0.5", "10.1.0.9", 0x5000, 0x1234, 6, 1, scope=7),
            K("10.0.0.5", "10.1.0.9", 0x5000, 0x1234, 6, 1, scope=3),
            K("10.0.0.5", "10.1.0.9", 0, 0, 1, 3, scope=3, kind=N.CG_CT_MAP_TCP),
            K("10.0.0.5", "10.1.0.9", 0, 0, 1, 3, scope=3),
            K("fd00::5", "fd01::9", 0x5000, 0x1234, 6, 1, scope=3),
            K("10.0.0.4", "10.1.0.9", 0x5000, 0x1234, 6, 1, scope=3)]
    vals = np.zeros(6, CT_ENTRY_DTYPE)
    vals["rev_nat_index"] = np.arange(6) + 10
    vals["lifetime"], vals["rx_packets"], vals["src_sec_id"], vals["flags"] = 77, np.arange(6), 1000, 0x19
    ct.update(keys, vals)
    for k, v in zip(keys, vals):
        assert ct.lookup(k).tobytes() == v.tobytes()
    assert ct.lookup(K("10.0.0.5", "10.1.0.9", 0x5000, 0x1234, 6, 0, scope=3)) is None
    # dump: (scope, kind, family, tuple bytes)
    dk, dv = ct.dump()
    # scope 3 first: its TCP map, IPv4 by tuple bytes (10.0.0.4; then 10.0.0.5 with dport bytes 00 00 before 00 50),
    # then IPv6; its ANY map; scope 7 last
    order = [5, 2, 1, 4, 3, 0]
    assert [dk[j].tobytes() for j in range(6)] == [keys[i][0].tobytes() for i in order]
    assert [int(x) for x in dv["rev_nat_index"]] == [10 + i for i in order]
    # update past max_entries changes nothing; an overwrite of existing keys still fits
    more = [K("10.0.0.9", "10.1.0.9", 1, 2, 17, 0), keys[0]]
    v2 = np.zeros(2, CT_ENTRY_DTYPE)
    v2["rev_nat_index"] = 99
    assert _code(ct.update, more, v2) == N.CG_MAP_FULL
    assert ct.dump()[0].tobytes() == dk.tobytes() and ct.dump()[1].tobytes() == dv.tobytes()
    ct.update([keys[0]], v2[:1])
    assert int(ct.lookup(keys[0])["rev_nat_index"]) == 99
    # delete: all or nothing
    assert _code(ct.delete, [keys[1], more[0]]) == N.CG_NOT_FOUND and len(ct.dump()[0]) == 6
    ct.delete([keys[1], keys[2]])
    assert ct.lookup(keys[1]) is None and ct.lookup(keys[3]) is not None and len(ct.dump()[0]) == 4
    # argument checks
    bad = K("10.0.0.5", "10.1.0.9", 1, 2, 6, 0)
    bad["family"] = 5
    assert _code(ct.update, bad) == N.CG_INVALID_ADDRESS
    bad = K("10.0.0.5", "10.1.0.9", 1, 2, 6, 8)
    assert _code(ct.update, bad) == N.CG_INVALID_ARGUMENT
    bad = K("10.0.0.5", "10.1.0.9", 1, 2, 6, 0, kind=2)
    assert _code(ct.update, bad) == N.CG_INVALID_ARGUMENT
    assert len(ct.dump()[0]) == 4
    ct.destroy()
    assert _code(ct.dump) == N.CG_NOT_FOUND
    assert CT_KEY_DTYPE.itemsize == 44 and CT_RECORD_DTYPE.itemsize == 64


# -------------------------------------------------------- probe chains ----
def test_probe_chains(host):
    T.probe_chain_check(host, _run)
