"""l4_frames_kernel<IngressProg> with conntrack against the host evaluator and
the Python oracle at every size and resolver combination, policy counters
against a twin array on the route without conntrack, the empty map against
the kernel without the lookup, the
hand-written cases, probe chains and near-miss keys on the device, a mixed
wave, the map's snapshot and the device entry."""
import numpy as np
import pytest

import ct_util as T
import frames_util as F
import l4_array_util as U
from cilium_amd import _native as N
from cilium_amd.classifier import CT_RECORD_DTYPE, FRAME_INFO_DTYPE

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1000, U.N_TUPLES]
COMBO_IDS = [("lxc" if c["lxc"] else "epmap") + "-" + ("labels" if c["lab"] else "ipcache") for c in F.COMBOS]


@pytest.fixture
def world(gpu):
    maps, twins = U.build_maps(gpu), U.build_maps(gpu)
    arr, twin_arr = U.build_array(gpu, maps), U.build_array(gpu, twins)
    ep, ipc = F.build_endpoints(gpu), F.build_ipcache(gpu)
    yield arr, maps, twins, twin_arr, ep, ipc
    for x in (arr, twin_arr, ep, ipc, *maps, *twins):
        x.destroy()


def _run(arr, raw, off, ct, kw):
    return arr.frame_verdicts(raw, off, info=True, conntrack=ct, **kw)


def _assert_counters_equal(maps, twins):
    for pm, tw in zip(maps, twins):
        assert U.counters(pm) == U.counters(tw)


@pytest.mark.parametrize("ci", range(4), ids=COMBO_IDS)
def test_kernel_equals_host_evaluator_and_oracle(gpu, world, ci):
    arr, maps, twins, twin_arr, ep, ipc = world
    raw, off, pkt_len, labels, lxc = F.shared_frames()
    assert set((off[:-1] % 16).tolist()) == set(range(16))  # frame starts of every alignment
    items, values = T.shared_table(ci)
    ct = T.build_map(gpu, items, values)
    replies_hit = 0
    for k, n in enumerate(SIZES):
        first = 0 if n == U.N_TUPLES else 5 * k  # a window that does not start at 0 for the smaller sizes
        sl = slice(first, first + n)
        o = off[first:first + n + 1]
        a, _ = F.resolver_args(F.COMBOS[ci], ep, ipc, lxc, labels, sl)
        ignore_drop = k % 2 == 1
        v, info, rec = arr.frame_verdicts(raw, o, pkt_len=pkt_len[sl], ignore_drop=ignore_drop, info=True,
                                          conntrack=ct, **a)
        hv, hinfo, hrec = arr.frame_eval_host_diag(raw, o, pkt_len=pkt_len[sl], ignore_drop=ignore_drop, info=True,
                                                   conntrack=ct, **a)
        ev, einfo, erec, _ = T.shared_expected(ci, ignore_drop)
        assert np.array_equal(v, hv), (n, np.flatnonzero(v != hv)[:5])
        assert info.tobytes() == hinfo.tobytes() and rec.tobytes() == hrec.tobytes(), n
        assert np.array_equal(v, ev[sl]) and np.array_equal(info, einfo[sl]), n
        T.assert_records_equal(rec, erec[sl], f"n={n}")
        # the twin array on the route without conntrack sees the same frames: its counters are the yardstick
        tv = twin_arr.frame_verdicts(raw, o, pkt_len=pkt_len[sl], ignore_drop=ignore_drop, **a)
        reply = rec["state"] >= N.CG_CT_STATE_REPLY
        assert np.array_equal(tv[~reply], v[~reply]) and (v[reply] == 0).all()
        replies_hit += int((tv[reply] >= 0).sum()) if not ignore_drop else 0
    _assert_counters_equal(maps, twins)  # replies still count
    assert replies_hit > 0 and any(e[5] for e in U.counters(maps[3]))
    ct.destroy()


def test_empty_map_equals_the_existing_kernel(gpu, world):
    arr, maps, twins, twin_arr, ep, ipc = world
    raw, off, pkt_len, labels, lxc = F.shared_frames()
    ct = gpu.conntrack_map()
    for ci, combo in enumerate(F.COMBOS):
        a, _ = F.resolver_args(combo, ep, ipc, lxc, labels)
        v, info, rec = arr.frame_verdicts(raw, off, pkt_len=pkt_len, info=True, conntrack=ct, **a)
        v0, info0 = twin_arr.frame_verdicts(raw, off, pkt_len=pkt_len, info=True, **a)
        assert np.array_equal(v, v0) and info.tobytes() == info0.tobytes(), COMBO_IDS[ci]
        done = (info["t"]["flags"] & N.CG_L4_F_INGRESS) != 0
        assert (rec["op"][done & (v >= 0)] == T.OP_CREATE).all() and (rec["op"][~(done & (v >= 0))] == 0).all()
        assert (rec["state"][done] == N.CG_CT_STATE_NEW).all() and not rec["state"][~done].any()
        # without records; the twin runs a second time too, so that the counters stay comparable
        assert np.array_equal(arr.frame_verdicts(raw, off, pkt_len=pkt_len, conntrack=ct, **a), v)
        assert np.array_equal(twin_arr.frame_verdicts(raw, off, pkt_len=pkt_len, **a), v)
    _assert_counters_equal(maps, twins)
    ct.destroy()


def test_hand_written_cases_as_one_batch(gpu):
    arr, pm, ct, raw, off, kw, cases = T.golden_world(gpu)
    v, info, rec = arr.frame_verdicts(raw, off, info=True, conntrack=ct, **kw)
    T.check_golden(cases, v, rec)
    hv, hinfo, hrec = arr.frame_eval_host_diag(raw, off, info=True, conntrack=ct, **kw)
    assert np.array_equal(v, hv) and rec.tobytes() == hrec.tobytes()
    for x in (arr, pm, ct):
        x.destroy()


def test_probe_chains_on_the_device(gpu):
    T.probe_chain_check(gpu, _run)


def test_near_miss_keys_on_the_device(gpu):
    T.near_miss_check(gpu, _run)


def test_mixed_wave(gpu, world, run=None):
    """One 64-frame wave: reply, established (allowed and denied), new
    (allowed and denied), related, walk errors, an empty slot and a foreign
    address, with exact verdicts, states and ops."""
    arr, maps, twins, twin_arr, ep, ipc = world
    keys = U.tables()[3][0]
    table = F.slot_tables()[300][1]
    l3_only = {key[0] for key in table if key[1] == 0 and key[2] == 0}  # identities allowed on every port
    k = next(x for x in keys[(keys["sec_label"] != 0) & (keys["dport"] != 0) & (keys["egress"] == 0) &
                             (keys["protocol"] == 6)] if int(x["sec_label"]) not in l3_only)
    label, port = int(k["sec_label"]), int.from_bytes(int(k["dport"]).to_bytes(2, "little"), "big")
    policy = F.policy_can_access_ingress(F.slot_tables()[300][1], label, int(k["dport"]), 6, False, False)[0]
    denied_port = next(p for p in range(20000, 20100) if F.policy_can_access_ingress(
        F.slot_tables()[300][1], label, int.from_bytes(p.to_bytes(2, "big"), "little"), 6, False, False)[0] < 0)
    g = T.load_golden()
    by_name = {c["name"]: bytes.fromhex(c["hex"]) for c in g["frames"]}

    def to(frame, dst):
        f = bytearray(frame)
        f[30:34] = bytes(int(x) for x in dst.split("."))
        return bytes(f)

    def tcp(src, sport, dport):
        return to(T.frame_for_key(dict(family=4, nexthdr=6, saddr=bytes(int(x) for x in src.split(".")),
                                       daddr=bytes(4), dport=int.from_bytes(sport.to_bytes(2, "big"), "little"),
                                       sport=int.from_bytes(dport.to_bytes(2, "big"), "little"))), "10.0.0.14")

    icmp_err = to(by_name["ICMP dest-unreach with the related key in the ANY map is related"], "10.0.0.14")
    kinds = [
        ("reply", tcp("10.1.0.1", 443, denied_port), 0, N.CG_CT_STATE_REPLY, T.OP_NONE),
        ("established allowed", tcp("10.1.0.2", 40000, port), policy, N.CG_CT_STATE_ESTABLISHED, T.OP_NONE),
        ("established denied", tcp("10.1.0.3", 40000, denied_port), F.DROP_POLICY, N.CG_CT_STATE_ESTABLISHED,
         T.OP_DELETE),
        ("new allowed", tcp("10.1.0.4", 40000, port), policy, N.CG_CT_STATE_NEW, T.OP_CREATE),
        ("new denied", tcp("10.1.0.5", 40000, denied_port), F.DROP_POLICY, N.CG_CT_STATE_NEW, T.OP_NONE),
        ("related", icmp_err, 0, N.CG_CT_STATE_RELATED, T.OP_NONE),
        ("short", tcp("10.1.0.6", 1, 2)[:40], F.DROP_CT_INVALID_HDR, 0, T.OP_NONE),
        ("unknown proto", bytes(bytearray(tcp("10.1.0.7", 1, 2))[:23] + b"\x2f" + tcp("10.1.0.7", 1, 2)[24:]),
         F.DROP_CT_UNKNOWN_PROTO, 0, T.OP_NONE),
        ("empty slot", to(tcp("10.1.0.1", 443, denied_port), "10.0.0.12"), F.DROP_MISSED_TAIL_CALL, 0, T.OP_NONE),
        ("foreign", to(tcp("10.1.0.1", 443, denied_port), "192.0.2.1"), F.NOT_LOCAL, 0, T.OP_NONE),
    ]
    assert policy >= 0
    items = [T.entry_for(kinds[0][1], "reply", 300), T.entry_for(kinds[1][1], "established", 300),
             T.entry_for(kinds[2][1], "established", 300), T.entry_for(icmp_err, "reply", 300),
             # the reply's key under the empty slot's and another endpoint's scope: never looked up
             T.entry_for(kinds[0][1], "reply", U.EMPTY_SLOT), T.entry_for(kinds[3][1], "established", 7)]
    ct = T.build_map(gpu, items)
    rng = np.random.default_rng(6)
    pick = rng.integers(0, len(kinds), 64)
    pick[:len(kinds)] = np.arange(len(kinds))
    frames = [kinds[p][1] + b"\0" * int(x) for p, x in zip(pick, rng.integers(0, 3, 64))]
    frames = [f if kinds[p][0] != "short" else kinds[p][1] for f, p in zip(frames, pick)]
    raw, off = F.join(frames)
    plen = rng.integers(64, 70_000, 64).astype(np.uint32)
    run = run or arr.frame_verdicts
    v, info, rec = run(raw, off, endpoints=ep, src_labels=np.full(64, label), pkt_len=plen, info=True, conntrack=ct)
    for j, (name, _, verdict, state, op) in enumerate(kinds):
        sel = pick == j
        assert v[sel].tolist() == [verdict] * int(sel.sum()), name
        assert rec["state"][sel].tolist() == [state] * int(sel.sum()), name
        assert rec["op"][sel].tolist() == [op] * int(sel.sum()), name
    # the hot entry counted every TCP frame to its port, the reply's denied port counted nothing
    hot = np.isin(pick, (1, 3))
    got = {e[:4]: (e[5], e[6]) for e in U.counters(maps[3]) if e[5] or e[6]}
    assert got == {(label, int(k["dport"]), 6, 0): (int(hot.sum()), int(plen[hot].astype(np.uint64).sum()))}
    ct.destroy()


def test_map_update_between_two_calls(gpu, world):
    arr, maps, twins, twin_arr, ep, ipc = world
    g = T.load_golden()
    f = bytes.fromhex(g["frames"][0]["hex"])
    raw, off = F.join([f] * 3)
    kw = dict(lxc_ids=[300] * 3, src_labels=[1] * 3)
    ct = gpu.conntrack_map()
    call = lambda: arr.frame_verdicts(raw, off, info=True, conntrack=ct, **kw)[2]["state"].tolist()
    assert call() == [N.CG_CT_STATE_NEW] * 3
    est = T.keys_array([T.entry_for(f, "established", 300)])
    ct.update(est)
    assert call() == [N.CG_CT_STATE_ESTABLISHED] * 3
    rep = T.keys_array([T.entry_for(f, "reply", 300)])
    ct.update(rep)
    assert call() == [N.CG_CT_STATE_REPLY] * 3  # the reply takes precedence
    ct.delete(rep)
    assert call() == [N.CG_CT_STATE_ESTABLISHED] * 3
    ct.delete(est)
    assert call() == [N.CG_CT_STATE_NEW] * 3
    ct.destroy()


def test_dev_entry_on_a_side_stream(gpu, world):
    torch = pytest.importorskip("torch")
    arr, maps, twins, twin_arr, ep, ipc = world
    raw, off, pkt_len, labels, lxc = F.shared_frames()
    items, values = T.shared_table(3)
    ct = T.build_map(gpu, items, values)
    n = U.N_TUPLES
    dev = torch.device("cuda", 0)
    lead = 3  # the blob does not start at the allocation's start, nor the window at offset 0
    d_raw = torch.from_numpy(np.concatenate([np.full(lead, 0xEE, np.uint8), raw])).to(dev)
    d_off = torch.from_numpy((off + np.uint64(lead)).view(np.int64).copy()).to(dev)
    d_len = torch.from_numpy(pkt_len.view(np.int32).copy()).to(dev)
    d_out = torch.full((n,), 9, dtype=torch.int32, device=dev)
    d_info = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    d_rec = torch.full((n, 64), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    arr.frame_verdicts_dev(d_raw, d_off, n, d_out, endpoints=ep, ipcache=ipc, d_pkt_len=d_len, d_info=d_info,
                           stream=side.cuda_stream, conntrack=ct, d_records=d_rec)
    side.synchronize()
    got, info = d_out.cpu().numpy(), d_info.cpu().numpy().view(FRAME_INFO_DTYPE).reshape(-1)
    rec = d_rec.cpu().numpy().view(CT_RECORD_DTYPE).reshape(-1)
    hv, hinfo, hrec = arr.frame_eval_host_diag(raw, off, endpoints=ep, ipcache=ipc, pkt_len=pkt_len, info=True,
                                               conntrack=ct)
    assert np.array_equal(got, hv) and info.tobytes() == hinfo.tobytes()
    assert rec.tobytes() == hrec.tobytes()
    assert np.array_equal(got, T.shared_expected(3, False)[0])
    twin_arr.frame_verdicts(raw, off, endpoints=ep, ipcache=ipc, pkt_len=pkt_len)
    _assert_counters_equal(maps, twins)
    ct.destroy()
