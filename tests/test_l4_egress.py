"""The from-container program of the frames route on a host-only handle: the
shared batch proven on the Python oracle alone, the host evaluator
(egress_walk.h over host_view()) against the oracle and the hand-written
cases, argument validation, the endpoint headers' API, apply of egress
records, and the round trips through the shared conntrack map."""
import collections

import numpy as np
import pytest

import ct_util as T
import egress_util as E
import frames_util as F
import l4_array_util as U
from cilium_amd import _native as N
from cilium_amd.classifier import CT_RECORD_DTYPE

SIZES = [1, 63, 64, 65, 1000, U.N_TUPLES]


def _code(fn, *a, **kw):
    with pytest.raises(N.CiliumGPUError) as ei:
        fn(*a, **kw)
    return ei.value.code


@pytest.fixture(scope="module")
def world(host):
    maps = U.build_maps(host)
    arr = E.build_array(host, maps)
    ipc = F.build_ipcache(host)
    yield arr, maps, ipc
    for x in (arr, ipc, *maps):
        x.destroy()


# ------------------------------------------ the inputs, on the oracle ----
def test_shared_batch_covers_the_program_on_the_oracle_alone():
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    frames = F.split(raw, off)
    assert len(frames) == U.N_TUPLES and set((off[:-1] % 16).tolist()) == set(range(16))
    assert (pkt_len > 0xFFFF).any()
    v, info, rec, _, hits = E.shared_expected(0, False)
    seen = collections.Counter(v.tolist())
    for code in E.ALL_CODES:
        assert seen[code] > 0, code
    assert any(x > 0 for x in seen), "a proxy port"
    # -3 three ways: ARP, neighbour solicitation, echo to the router
    answered = [f for f, x in zip(frames, v) if x == E.ANSWERED]
    arp = sum(f[12:14] == b"\x08\x06" for f in answered)
    ns = sum(f[12:14] == b"\x86\xdd" and f[54] == 135 for f in answered)
    echo = sum(f[12:14] == b"\x86\xdd" and f[54] == 128 for f in answered)
    assert arp and ns and echo and arp + ns + echo == len(answered)
    done = (info["t"]["flags"] & N.CG_L4_F_WALKED) != 0
    assert done.sum() * 2 >= len(frames)
    states = collections.Counter(rec["state"][done].tolist())
    for s in (N.CG_CT_STATE_NEW, N.CG_CT_STATE_ESTABLISHED, N.CG_CT_STATE_REPLY, N.CG_CT_STATE_RELATED):
        assert states[s] * 50 >= done.sum(), (s, states)
    assert not rec["state"][~done].any() and hits
    # every special slot is used: no IPv4, each NO_* flag, no header, no map
    assert set(lxc.tolist()) == set(E.SLOT_MAP) | {E.EMPTY_SLOT}


# -------------------------------------------------- evaluator = oracle ----
@pytest.mark.parametrize("with_ct", [False, True], ids=["no-ct", "ct"])
@pytest.mark.parametrize("ci", range(2), ids=E.COMBO_IDS)
def test_host_evaluator_equals_the_oracle(host, world, ci, with_ct):
    arr, maps, ipc = world
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    ct = T.build_map(host, *E.shared_table()) if with_ct else None
    for k, n in enumerate(SIZES):
        first = 0 if n == U.N_TUPLES else 5 * k  # windows that do not start at 0
        sl = slice(first, first + n)
        a, _ = E.resolver_args(E.COMBOS[ci], ipc, labels, sl)
        ignore_drop = k % 2 == 1
        res = arr.frame_egress_eval_host_diag(raw, off[first:first + n + 1], lxc_ids=lxc[sl], pkt_len=pkt_len[sl],
                                              ignore_drop=ignore_drop, info=True, l4_off=True, conntrack=ct, **a)
        ev, einfo, erec, el4, _ = E.shared_expected(ci, ignore_drop, with_ct)
        bad = np.flatnonzero(res[0] != ev[sl])
        assert not len(bad), (n, bad[:5], res[0][bad[:5]], ev[sl][bad[:5]])
        assert np.array_equal(res[1], einfo[sl]), (n, np.flatnonzero(res[1] != einfo[sl])[:5])
        assert np.array_equal(res[-1], el4[sl]), n
        if with_ct:
            T.assert_records_equal(res[2], erec[sl], f"n={n}")
    if ct is not None:
        ct.destroy()


def test_global_map_looks_up_scope_zero(host, world):
    arr, maps, ipc = world
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    ct = T.build_map(host, *E.shared_table(True), global_map=True)
    v, info, rec = arr.frame_egress_eval_host_diag(raw, off, lxc_ids=lxc, dst_labels=labels, pkt_len=pkt_len, info=True,
                                                   conntrack=ct)
    ev, einfo, erec, _, _ = E.shared_expected(0, False, True, True)
    assert np.array_equal(v, ev) and np.array_equal(info, einfo)
    T.assert_records_equal(rec, erec, "global")
    assert not rec["key"]["scope"].any() and (rec["state"] >= N.CG_CT_STATE_REPLY).any()
    ct.destroy()


def test_empty_map_equals_no_map(host, world):
    arr, maps, ipc = world
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    ct = host.conntrack_map()
    kw = dict(lxc_ids=lxc, dst_labels=labels, pkt_len=pkt_len)
    v0, i0 = arr.frame_egress_eval_host_diag(raw, off, info=True, **kw)
    v, info, rec = arr.frame_egress_eval_host_diag(raw, off, info=True, conntrack=ct, **kw)
    assert np.array_equal(v, v0) and info.tobytes() == i0.tobytes()
    done = (info["t"]["flags"] & N.CG_L4_F_WALKED) != 0
    assert (rec["state"][done] == N.CG_CT_STATE_NEW).all() and rec[~done].tobytes() == bytes(64 * int((~done).sum()))
    assert (rec["op"][done & (v >= 0)] == T.OP_CREATE).all() and not rec["op"][~(done & (v >= 0))].any()
    assert (rec["pad0"][done] == 1).all()
    ct.destroy()


def test_hand_written_cases(host):
    arr, pm, ct, raw, off, lxc, labels, g = E.kat_world(host)
    st, hd, ctmap = E.kat_oracle_world(g)
    frames = F.split(raw, off)
    for ignore_drop in (False, True):
        v, info, rec = arr.frame_egress_eval_host_diag(raw, off, lxc_ids=lxc, dst_labels=labels, info=True,
                                                       ignore_drop=ignore_drop, conntrack=ct)
        E.check_kat(g, v, rec, ignore_drop)
        ev, einfo, erec, _, _ = E.evaluate(frames, st, hd, lxc_ids=lxc, dst_labels=labels, ctmap=ctmap,
                                           ignore_drop=ignore_drop)
        assert np.array_equal(v, ev) and np.array_equal(info, einfo)
        T.assert_records_equal(rec, erec, "kat")
    # the fragment that egress judges with its ports takes the fragment path on ingress
    i = next(i for i, c in enumerate(g["frames"]) if c.get("ingress_fragment"))
    one, o = F.join([frames[i]])
    slot = int(lxc[i])
    vi, ii = arr.frame_eval_host_diag(one, o, lxc_ids=[slot], src_labels=[2001], info=True)
    assert ii["t"]["flags"][0] == N.CG_L4_F_INGRESS | N.CG_L4_F_FRAGMENT and vi[0] == F.DROP_POLICY
    ve, ie = arr.frame_egress_eval_host_diag(one, o, lxc_ids=[slot], dst_labels=[2000], info=True)
    assert ie["t"]["flags"][0] == N.CG_L4_F_WALKED and ve[0] == 0
    for x in (arr, pm, ct):
        x.destroy()


# ---------------------------------------------------------- arguments ----
def test_argument_validation(host, world):
    arr, maps, ipc = world
    raw, off = F.join([bytes(64)] * 2)
    lib, h = N.lib, host.h
    p = N.ptr
    lxc, lab, out = np.zeros(2, np.uint16), np.zeros(2, np.uint32), np.zeros(2, np.int32)
    rec = np.zeros(2, CT_RECORD_DTYPE)
    ct = host.conntrack_map()

    def call(mode=N.CG_L4_EGRESS, lxc_=lxc, lab_=lab, ipc_id=0, ct_id=0, rec_=None):
        return lib.cg_diag_l4_frames_egress_eval_host(h, arr.id, mode, p(raw), p(off), 2, p(lxc_), p(lab_), ipc_id, None,
                                                      ct_id, p(out), None, p(rec_), None)

    assert call() == 0 and call(N.CG_L4_EGRESS | N.CG_L4_IGNORE_DROP) == 0
    for mode in (N.CG_L4_INGRESS, N.CG_L4_CAN_ACCESS, N.CG_L4_EGRESS | 0x200, N.CG_L4_INGRESS | N.CG_L4_IGNORE_DROP, 3):
        assert call(mode) == N.CG_INVALID_ARGUMENT, mode
    assert call(lxc_=None) == N.CG_INVALID_ARGUMENT  # lxc_ids is mandatory
    assert call(ipc_id=ipc.id) == N.CG_INVALID_ARGUMENT  # both resolvers
    assert call(lab_=None) == N.CG_INVALID_ARGUMENT  # neither
    assert call(lab_=None, ipc_id=ipc.id) == 0
    assert call(rec_=rec) == N.CG_INVALID_ARGUMENT  # records without a conntrack map
    assert call(ct_id=ct.id, rec_=rec) == 0 and call(ct_id=ct.id) == 0
    assert call(ct_id=ct.id + 1000) == N.CG_NOT_FOUND
    # the device entries check the same before they ask for a device
    args = (h, arr.id, N.CG_L4_INGRESS, p(raw), p(off), 2, p(lxc), p(lab), 0, None, 0, p(out), None, None)
    assert lib.cg_l4_frames_egress_verdicts_host(*args) == N.CG_INVALID_ARGUMENT
    assert lib.cg_l4_frames_egress_verdicts_dev(*args, None) == N.CG_INVALID_ARGUMENT
    args = (h, arr.id, N.CG_L4_EGRESS, p(raw), p(off), 2, p(lxc), p(lab), 0, None, 0, p(out), None, p(rec))
    assert lib.cg_l4_frames_egress_verdicts_host(*args) == N.CG_INVALID_ARGUMENT
    # the existing ingress entries still refuse the egress mode
    assert lib.cg_diag_l4_frames_eval_host(h, arr.id, N.CG_L4_EGRESS, p(raw), p(off), 2, p(lxc), 0, p(lab), 0, None,
                                           p(out), None, None) == N.CG_INVALID_ARGUMENT
    # frame conventions: a backwards range is an empty frame, pkt_len NULL counts the frame's length
    f = E.ip4(E.headers()[0], "10.1.2.3", 6, E.tcp(1, 2))
    blob, o = F.join([f, f])
    o2 = np.array([o[1], o[0], o[2]], np.uint64)  # window [o[1], o[2]); frame 0 runs backwards
    v, info = arr.frame_egress_eval_host_diag(blob, o2, lxc_ids=[0, 0], dst_labels=[1, 1], info=True)
    assert v[0] == F.DROP_INVALID and info["t"]["len"].tolist() == [0, len(f)]
    ct.destroy()


# ------------------------------------------------------------- headers ----
def test_headers_set_get_clear(host):
    pm, arr = host.policy_map(), host.policy_array()
    assert arr.get_header(3) is None
    arr.set_header(3, mac="0a:00:00:00:00:03", node_mac=E.NODE_MAC, ipv4="10.0.0.3", ipv6="fd00::3",
                   router_ip6="fd00::1", seclabel=77, verify_dmac=False)
    h = arr.get_header(3)
    assert bytes(h["lxc_mac"]) == E.mac("0a:00:00:00:00:03") and bytes(h["node_mac"]) == E.NODE_MAC
    assert bytes(h["ipv4"]) == bytes([10, 0, 0, 3]) and h["seclabel"] == 77
    assert h["flags"] == N.CG_EPH_F_IPV4 | N.CG_EPH_F_NO_DMAC
    assert arr.get(3) is None  # the header did not fill the slot
    # all or nothing: one bad record (unknown flag bits, a non-zero pad) leaves every header as it was
    two = np.concatenate([E.header_record(E.HEADER_SPECS[0]), E.header_record(E.HEADER_SPECS[1])])
    for field, value in (("flags", 0x10), ("flags", 0x80000000), ("pad", 1)):
        bad = two.copy()
        bad[field][1] = value
        assert _code(arr.set_headers, [4, 3], bad) == N.CG_INVALID_ARGUMENT
        assert arr.get_header(4) is None and arr.get_header(3).tobytes() == h.tobytes()
    assert _code(arr.set_headers, [70000], two[:1]) == N.CG_INVALID_ARGUMENT
    arr.set_headers([4, 3], two)
    assert arr.get_header(4).tobytes() == two[0].tobytes() and arr.get_header(3).tobytes() == two[1].tobytes()
    assert arr.get_header(3)["flags"] == 0  # no IPv4
    # a header survives set / clear of the slot's map and the map's destruction
    arr.set(4, pm)
    arr.clear(4)
    assert arr.get_header(4).tobytes() == two[0].tobytes() and arr.get(4) is None
    arr.set(4, pm)
    f = E.ip4(E.headers()[0], "10.1.2.3", 6, E.tcp(1, 2))
    raw, off = F.join([f])
    run = lambda: int(arr.frame_egress_eval_host_diag(raw, off, lxc_ids=[4], dst_labels=[1])[0])
    assert run() == F.DROP_POLICY
    arr.clear_header([4, 9])  # clearing a slot that has none is not an error
    assert arr.get_header(4) is None and run() == E.NO_HEADER and arr.get(4) == pm.id
    arr.set_headers([4], two[:1])
    pm.destroy()
    assert arr.get(4) is None and arr.get_header(4) is not None and run() == F.DROP_MISSED_TAIL_CALL
    arr.destroy()


# --------------------------------------------------------------- apply ----
def test_apply_of_egress_records(host):
    pm, arr, hd = E.egress_world(host)
    frames = [E.ip4(hd, "10.1.0.1", 6, E.tcp(40000, 80)), E.ip6(hd, "fd01::1", 6, E.tcp(40000, 80)),
              E.ip4(hd, "10.1.0.1", 6, E.tcp(40000, 80)), E.ip4(hd, "10.1.0.2", 6, E.tcp(40000, 81))]
    raw, off = F.join(frames)
    plen = np.array([100, 70_000, 300, 400], np.uint32)
    ct = host.conntrack_map()
    v, info, rec = arr.frame_egress_eval_host_diag(raw, off, lxc_ids=[5] * 4, dst_labels=[2000] * 4, pkt_len=plen,
                                                   info=True, conntrack=ct)
    assert v.tolist() == [0, 0, 0, F.DROP_POLICY] and rec["op"].tolist() == [1, 1, 1, 0]
    assert (rec["pad0"] == 1).all() and (rec["pad2"][:, 0] == 4242).all() and not rec["pad2"][:, 1].any()
    oracle = {}
    exp = E.apply(oracle, rec, plen, np.full(4, 999, np.uint32), ct.max_entries)
    got = ct.apply(rec, plen, np.full(4, 999, np.uint32))  # src_labels is ignored for egress records
    assert got.tolist() == exp.tolist() == [0] * 4
    assert E.dump_got(ct) == E.dump_of(oracle) and len(oracle) == 4  # the duplicate CREATE left one pair
    keys, vals = ct.dump()
    assert (vals["tx_packets"] == 1).all() and not vals["rx_packets"].any() and not vals["rx_bytes"].any()
    assert (vals["src_sec_id"] == 4242).all()
    assert sorted(vals["tx_bytes"].tolist()) == [300, 300, 70_000, 70_000]  # the later duplicate overwrote the first
    assert sorted(keys["flags"].tolist()) == [0, 0, 2, 2]  # TUPLE_F_OUT after the reversal, and the related keys
    # a second pass reads ESTABLISHED and asks for nothing
    v2, _, rec2 = arr.frame_egress_eval_host_diag(raw, off, lxc_ids=[5] * 4, dst_labels=[2000] * 4, info=True,
                                                  conntrack=ct)
    assert rec2["state"].tolist() == [2, 2, 2, 1] and not rec2["op"].any()
    # a full map: neither key is written
    small = host.conntrack_map(max_entries=3)
    assert small.apply(rec[:2], plen[:2]).tolist() == [0, N.CG_DROP_CT_CREATE_FAILED] and len(small.dump()[0]) == 2
    for x in (ct, small, arr, pm):
        x.destroy()


def test_ingress_records_apply_as_before(host):
    """dir 0 records take the existing path: the dump equals ct_util.apply's, field for field."""
    raw, off, pkt_len, labels, lxc = F.shared_frames()
    maps = U.build_maps(host)
    arr = U.build_array(host, maps)
    items, values = T.shared_table(0)
    ct = T.build_map(host, items, values)
    v, info, rec = arr.frame_eval_host_diag(raw, off, lxc_ids=lxc, src_labels=labels, pkt_len=pkt_len, info=True,
                                            conntrack=ct)
    assert not rec["pad0"].any() and not rec["pad2"].any() and (rec["op"] == T.OP_CREATE).any()
    oracle = T.ctmap_of(items, values)
    for d in oracle.values():
        d["flags"] = N.CG_CT_E_LB_LOOPBACK if d.pop("loopback", 0) else 0
        d.pop("rev_nat_index", None)
    exp = T.apply(oracle, rec, pkt_len, labels, ct.max_entries)
    assert ct.apply(rec, pkt_len, labels).tolist() == exp.tolist()
    assert E.dump_got(ct) == E.dump_of(oracle)
    _, vals = ct.dump()
    assert not vals["tx_packets"].any() and vals["rx_packets"].any()
    for x in (ct, arr, *maps):
        x.destroy()


# ---------------------------------------------------------- round trips ----
def test_round_trips_on_the_host_evaluators(host):
    E.check_round_trips(host,
                      lambda arr, raw, off, **kw: arr.frame_egress_eval_host_diag(raw, off, info=True, **kw),
                      lambda arr, raw, off, **kw: arr.frame_eval_host_diag(raw, off, info=True, **kw))
