"""l4_frames_kernel<EgressProg> against the host evaluator and the Python oracle
at every size and resolver combination, with and without conntrack; policy
counters against a twin array driven with the oracle's tuples through
cg_l4_array_verdicts_* in CG_L4_EGRESS mode; the empty map, the hand-written
cases, the round trips through the shared conntrack map, a mixed wave, header
and map updates between calls, the device entry, and a batch larger than the
resident grid."""
import numpy as np
import pytest

import ct_util as T
import egress_util as E
import frames_util as F
import l4_array_util as U
from cilium_amd import _native as N
from cilium_amd.classifier import CT_RECORD_DTYPE, FRAME_INFO_DTYPE

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1000, U.N_TUPLES]


@pytest.fixture
def world(gpu):
    maps, twins = U.build_maps(gpu), U.build_maps(gpu)
    arr, twin_arr = E.build_array(gpu, maps), E.build_array(gpu, twins)
    ipc = F.build_ipcache(gpu)
    yield arr, maps, twins, twin_arr, ipc
    for x in (arr, twin_arr, ipc, *maps, *twins):
        x.destroy()


def _assert_counters_equal(maps, twins):
    for pm, tw in zip(maps, twins):
        assert U.counters(pm) == U.counters(tw)


@pytest.mark.parametrize("with_ct", [False, True], ids=["no-ct", "ct"])
@pytest.mark.parametrize("ci", range(2), ids=E.COMBO_IDS)
def test_kernel_equals_host_evaluator_and_oracle(gpu, world, ci, with_ct):
    arr, maps, twins, twin_arr, ipc = world
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    ct = T.build_map(gpu, *E.shared_table()) if with_ct else None
    for k, n in enumerate(SIZES):
        first = 0 if n == U.N_TUPLES else 5 * k  # a window that does not start at 0 for the smaller sizes
        sl = slice(first, first + n)
        o = off[first:first + n + 1]
        a, _ = E.resolver_args(E.COMBOS[ci], ipc, labels, sl)
        ignore_drop = k % 2 == 1
        kw = dict(lxc_ids=lxc[sl], pkt_len=pkt_len[sl], ignore_drop=ignore_drop, info=True, conntrack=ct, **a)
        got = arr.frame_egress_verdicts(raw, o, **kw)
        host = arr.frame_egress_eval_host_diag(raw, o, **kw)
        ev, einfo, erec, _, _ = E.shared_expected(ci, ignore_drop, with_ct)
        assert np.array_equal(got[0], host[0]), (n, np.flatnonzero(got[0] != host[0])[:5])
        assert got[1].tobytes() == host[1].tobytes(), n
        assert np.array_equal(got[0], ev[sl]) and np.array_equal(got[1], einfo[sl]), n
        if with_ct:
            assert got[2].tobytes() == host[2].tobytes(), n
            T.assert_records_equal(got[2], erec[sl], f"n={n}")
        # the twin array sees the tuples the oracle extracts, through the tuple kernel in egress mode
        t, done = E.extracted_tuples(einfo[sl])
        if not done.any():
            continue
        tv = twin_arr.verdicts(lxc[sl][done], t, mode=N.CG_L4_EGRESS | (N.CG_L4_IGNORE_DROP if ignore_drop else 0))
        if with_ct:
            reply = erec[sl]["state"][done] >= N.CG_CT_STATE_REPLY
            assert np.array_equal(tv[~reply], got[0][done][~reply]) and not got[0][done][reply].any()
        else:
            assert np.array_equal(tv, got[0][done])
    _assert_counters_equal(maps, twins)
    assert any(e[5] for e in U.counters(maps[3])) and any(e[6] > 70_000 for e in U.counters(maps[3]))
    if ct is not None:
        ct.destroy()


def test_empty_map_equals_no_map(gpu, world):
    arr, maps, twins, twin_arr, ipc = world
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    ct = gpu.conntrack_map()
    for ci, combo in enumerate(E.COMBOS):
        a, _ = E.resolver_args(combo, ipc, labels)
        kw = dict(lxc_ids=lxc, pkt_len=pkt_len, info=True, **a)
        v, info, rec = arr.frame_egress_verdicts(raw, off, conntrack=ct, **kw)
        v0, info0 = twin_arr.frame_egress_verdicts(raw, off, **kw)
        assert np.array_equal(v, v0) and info.tobytes() == info0.tobytes(), ci
        done = (info["t"]["flags"] & N.CG_L4_F_WALKED) != 0
        assert (rec["op"][done & (v >= 0)] == T.OP_CREATE).all() and not rec["op"][~(done & (v >= 0))].any()
        assert (rec["state"][done] == N.CG_CT_STATE_NEW).all() and not rec["state"][~done].any()
        # without info and records
        assert np.array_equal(arr.frame_egress_verdicts(raw, off, lxc_ids=lxc, pkt_len=pkt_len, conntrack=ct, **a), v)
        assert np.array_equal(twin_arr.frame_egress_verdicts(raw, off, lxc_ids=lxc, pkt_len=pkt_len, **a), v)
    _assert_counters_equal(maps, twins)
    ct.destroy()


def test_hand_written_cases_as_one_batch(gpu):
    arr, pm, ct, raw, off, lxc, labels, g = E.kat_world(gpu)
    for ignore_drop in (False, True):
        kw = dict(lxc_ids=lxc, dst_labels=labels, info=True, ignore_drop=ignore_drop, conntrack=ct)
        v, info, rec = arr.frame_egress_verdicts(raw, off, **kw)
        E.check_kat(g, v, rec, ignore_drop)
        hv, hinfo, hrec = arr.frame_egress_eval_host_diag(raw, off, **kw)
        assert np.array_equal(v, hv) and info.tobytes() == hinfo.tobytes() and rec.tobytes() == hrec.tobytes()
    for x in (arr, pm, ct):
        x.destroy()


def test_round_trips_on_the_device(gpu):
    E.check_round_trips(gpu,
                        lambda arr, raw, off, **kw: arr.frame_egress_verdicts(raw, off, info=True, **kw),
                        lambda arr, raw, off, **kw: arr.frame_verdicts(raw, off, info=True, **kw))


def test_mixed_wave(gpu):
    """One 64-frame wave in which neighbouring lanes leave the program at
    different steps: the hand-written cases, shuffled, with exact verdicts,
    states and ops per lane."""
    arr, pm, ct, raw, off, lxc, labels, g = E.kat_world(gpu)
    frames = F.split(raw, off)
    assert len({(c["verdict"], c["state"], c["op"]) for c in g["frames"]}) >= 16
    rng = np.random.default_rng(8)
    pick = np.concatenate([rng.permutation(len(frames)), rng.integers(0, len(frames), 64)])[:64]
    assert len(frames) <= 64
    wave, o = F.join([frames[p] for p in pick])
    plen = rng.integers(64, 70_000, 64).astype(np.uint32)
    v, info, rec = arr.frame_egress_verdicts(wave, o, lxc_ids=lxc[pick], dst_labels=labels[pick], pkt_len=plen,
                                             info=True, conntrack=ct)
    for lane, p in enumerate(pick):
        c = g["frames"][p]
        got = (int(v[lane]), T.STATE_NAMES[int(rec["state"][lane])], int(rec["op"][lane]))
        assert got == (c["verdict"], c["state"], {"none": 0, "create": 1, "delete": 2}[c["op"]]), (lane, c["name"])
    # counters: every lane that hit an entry counted its own pkt_len
    st, hd, ctmap = E.kat_oracle_world(g)
    _, _, _, _, hits = E.evaluate([frames[p] for p in pick], st, hd, lxc_ids=lxc[pick], dst_labels=labels[pick],
                                  pkt_len=plen, ctmap=ctmap)
    got = {e[:4]: (e[5], e[6]) for e in U.counters(pm) if e[5] or e[6]}
    assert got == {key: tuple(c) for (_, key), c in hits.items()} and len(got) >= 3
    for x in (arr, pm, ct):
        x.destroy()


def test_header_and_map_updates_between_calls(gpu):
    pm, arr, hd = E.egress_world(gpu)
    f = E.ip4(hd, "10.1.0.1", 6, E.tcp(40000, 80))
    raw, off = F.join([f] * 3)
    ct = gpu.conntrack_map()
    kw = dict(lxc_ids=[5] * 3, dst_labels=[2000] * 3, info=True, conntrack=ct)

    def call():
        v, _, rec = arr.frame_egress_verdicts(raw, off, **kw)
        return v.tolist(), rec["state"].tolist(), rec["pad2"][:, 0].tolist()

    assert call() == ([0] * 3, [N.CG_CT_STATE_NEW] * 3, [4242] * 3)
    # a new MAC and seclabel: the old frames fail the SMAC test as a whole batch
    spec = dict(node_mac=E.NODE_MAC, ipv4="10.0.0.5", ipv6="fd00::5", router_ip6=E.ROUTER_IP6)
    arr.set_header(5, mac="0a:00:00:00:00:55", seclabel=7, **spec)
    assert call()[0] == [E.DROP_INVALID_SMAC] * 3
    arr.set_header(5, mac="0a:00:00:00:00:05", seclabel=7, **spec)
    assert call() == ([0] * 3, [N.CG_CT_STATE_NEW] * 3, [7] * 3)
    arr.clear_header(5)
    assert call()[0] == [E.NO_HEADER] * 3
    arr.set_header(5, mac="0a:00:00:00:00:05", seclabel=8, **spec)
    # the conntrack map: an established key, then the reply key, then neither
    hdr8 = dict(hd, seclabel=8)
    t = E.from_container(f, hdr8)["tuple"]
    est = T.keys_array([(5, 0, 4, T.tuple_reverse(t))])
    rep = T.keys_array([(5, 0, 4, t)])
    ct.update(est)
    assert call()[1] == [N.CG_CT_STATE_ESTABLISHED] * 3
    ct.update(rep)
    assert call()[1] == [N.CG_CT_STATE_REPLY] * 3
    ct.delete(rep)
    ct.delete(est)
    assert call() == ([0] * 3, [N.CG_CT_STATE_NEW] * 3, [8] * 3)
    for x in (ct, arr, pm):
        x.destroy()


def test_dev_entry_on_a_side_stream(gpu, world):
    torch = pytest.importorskip("torch")
    arr, maps, twins, twin_arr, ipc = world
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    ct = T.build_map(gpu, *E.shared_table())
    n = U.N_TUPLES
    dev = torch.device("cuda", 0)
    lead = 3  # the blob does not start at the allocation's start, nor the window at offset 0
    d_raw = torch.from_numpy(np.concatenate([np.full(lead, 0xEE, np.uint8), raw])).to(dev)
    d_off = torch.from_numpy((off + np.uint64(lead)).view(np.int64).copy()).to(dev)
    d_len = torch.from_numpy(pkt_len.view(np.int32).copy()).to(dev)
    d_lxc = torch.from_numpy(lxc.view(np.int16).copy()).to(dev)
    d_out = torch.full((n,), 9, dtype=torch.int32, device=dev)
    d_info = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    d_rec = torch.full((n, 64), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    arr.frame_egress_verdicts_dev(d_raw, d_off, n, d_out, d_lxc_ids=d_lxc, ipcache=ipc, d_pkt_len=d_len, d_info=d_info,
                                  stream=side.cuda_stream, conntrack=ct, d_records=d_rec)
    side.synchronize()
    got, info = d_out.cpu().numpy(), d_info.cpu().numpy().view(FRAME_INFO_DTYPE).reshape(-1)
    rec = d_rec.cpu().numpy().view(CT_RECORD_DTYPE).reshape(-1)
    hv, hinfo, hrec = arr.frame_egress_eval_host_diag(raw, off, lxc_ids=lxc, ipcache=ipc, pkt_len=pkt_len, info=True,
                                                      conntrack=ct)
    assert np.array_equal(got, hv) and info.tobytes() == hinfo.tobytes() and rec.tobytes() == hrec.tobytes()
    assert np.array_equal(got, E.shared_expected(1, False)[0])
    # without a conntrack map the records buffer is refused, and left alone
    d_rec.fill_(0xCD)
    with pytest.raises(N.CiliumGPUError) as ei:
        arr.frame_egress_verdicts_dev(d_raw, d_off, n, d_out, d_lxc_ids=d_lxc, ipcache=ipc, d_records=d_rec)
    assert ei.value.code == N.CG_INVALID_ARGUMENT
    arr.frame_egress_verdicts_dev(d_raw, d_off, n, d_out, d_lxc_ids=d_lxc, ipcache=ipc, d_pkt_len=d_len,
                                  stream=side.cuda_stream)
    side.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), E.shared_expected(1, False, False)[0])
    assert (d_rec.cpu().numpy() == 0xCD).all()
    ct.destroy()


@pytest.mark.parametrize("with_ct", [False, True], ids=["no-ct", "ct"])
def test_more_frames_than_the_resident_grid(gpu, world, with_ct):
    """2^20 + 65 frames, the shared blob tiled: the grid-stride loop runs a
    second trip in every lane, and the last trip is ragged."""
    arr, maps, twins, twin_arr, ipc = world
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    n = (1 << 20) + 65
    reps = -(-n // U.N_TUPLES)
    size = int(off[-1])
    big_raw = np.tile(raw[:size], reps)
    big_off = (off[None, :-1] + (np.arange(reps, dtype=np.uint64) * np.uint64(size))[:, None]).reshape(-1)
    big_off = np.append(big_off, np.uint64(reps * size))[:n + 1]
    idx = np.arange(n) % U.N_TUPLES
    ct = T.build_map(gpu, *E.shared_table()) if with_ct else None
    kw = dict(lxc_ids=lxc[idx], dst_labels=labels[idx], pkt_len=pkt_len[idx], info=True, conntrack=ct)
    got = arr.frame_egress_verdicts(big_raw, big_off, **kw)
    host = arr.frame_egress_eval_host_diag(big_raw, big_off, **kw)
    ev, einfo, erec, _, _ = E.shared_expected(0, False, with_ct)
    assert np.array_equal(got[0], host[0]) and got[1].tobytes() == host[1].tobytes()
    assert np.array_equal(got[0], ev[idx]) and np.array_equal(got[1], einfo[idx])
    if with_ct:
        assert got[2].tobytes() == host[2].tobytes() and got[2].tobytes() == erec[idx].tobytes()
        ct.destroy()
