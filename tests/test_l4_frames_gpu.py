"""l4_frames_kernel<IngressProg> against the host evaluator and against the
array kernel on the tuples it extracted, counters entry for entry on twin maps; the
hand-written frames; truncation checked by value; large frames; a mixed wave
with exact counter sums; pkt_len; the endpoint map's snapshot; the device entry."""
import numpy as np
import pytest

import frames_util as F
import l4_array_util as U
from cilium_amd import _native as N
from cilium_amd.classifier import FRAME_INFO_DTYPE

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1000, U.N_TUPLES]
INGRESS = N.CG_L4_INGRESS


@pytest.fixture
def world(gpu):
    """The array over one set of maps, a twin set for the tuple route, the
    endpoint map and the ipcache."""
    maps, twins = U.build_maps(gpu), U.build_maps(gpu)
    arr, twin_arr = U.build_array(gpu, maps), U.build_array(gpu, twins)
    ep, ipc = F.build_endpoints(gpu), F.build_ipcache(gpu)
    yield arr, maps, twins, twin_arr, ep, ipc
    for x in (arr, twin_arr, ep, ipc, *maps, *twins):
        x.destroy()


def _assert_counters_equal(maps, twins):
    for pm, tw in zip(maps, twins):
        assert U.counters(pm) == U.counters(tw)


def _kat(name):
    return bytes.fromhex(next(k["hex"] for k in F.load_kat()["frames"] if k["name"] == name))


def _to4(frame, addr):
    f = bytearray(frame)
    f[30:34] = bytes(int(x) for x in addr.split("."))
    return bytes(f)


@pytest.mark.parametrize("combo", F.COMBOS, ids=lambda c: ("lxc" if c["lxc"] else "epmap") + "-" +
                         ("labels" if c["lab"] else "ipcache"))
def test_kernel_equals_host_evaluator_and_tuple_route(world, combo):
    arr, maps, twins, twin_arr, ep, ipc = world
    raw, off, pkt_len, labels, lxc = F.shared_frames()
    assert set((off[:-1] % 16).tolist()) == set(range(16))  # frame starts of every alignment
    for k, n in enumerate(SIZES):
        # a window that does not start at 0 for the smaller sizes
        first = 0 if n == U.N_TUPLES else 5 * k
        sl = slice(first, first + n)
        o = off[first:first + n + 1]
        a, _ = F.resolver_args(combo, ep, ipc, lxc, labels, sl)
        ignore_drop = k % 2 == 1
        mode = INGRESS | (N.CG_L4_IGNORE_DROP if ignore_drop else 0)
        v, info = arr.frame_verdicts(raw, o, pkt_len=pkt_len[sl], ignore_drop=ignore_drop, info=True, **a)
        hv, hinfo = arr.frame_eval_host_diag(raw, o, pkt_len=pkt_len[sl], ignore_drop=ignore_drop, info=True, **a)
        assert np.array_equal(v, hv), (n, np.flatnonzero(v != hv)[:5])
        assert np.array_equal(info, hinfo), (n, np.flatnonzero(info != hinfo)[:5])
        ran = info["t"]["flags"] != 0  # the walk completed: the verdict is the policy's
        assert np.array_equal(v[ran], twin_arr.verdicts(info["lxc_id"][ran], info["t"][ran], mode)), n
    _assert_counters_equal(maps, twins)
    assert any(e[5] for e in U.counters(maps[3])) and any(e[5] for e in U.counters(maps[2]))


def test_known_answers_as_one_batch(gpu):
    kat = F.load_kat()["frames"]
    raw, off = F.join([bytes.fromhex(k["hex"]) for k in kat])
    pm, arr = F.build_kat_map(gpu), gpu.policy_array()
    arr.set(F.KAT_SLOT, pm)
    n = len(kat)
    v, info = arr.frame_verdicts(raw, off, lxc_ids=np.full(n, F.KAT_SLOT), src_labels=np.full(n, F.KAT_LABEL),
                                 info=True)
    for i, k in enumerate(kat):
        got = dict(verdict=int(v[i]), dport=int(info["t"]["dport"][i]), proto=int(info["t"]["proto"][i]),
                   fragment=bool(info["t"]["flags"][i] & N.CG_L4_F_FRAGMENT), family=int(info["family"][i]))
        assert got == {f: k[f] for f in got}, k["name"]
    arr.destroy()
    pm.destroy()


def test_truncation_is_checked_by_value(gpu):
    """A frame that ends two bytes into its TCP header, followed by a frame
    whose first bytes would complete it to an allowed port: the bytes are
    there to be read, and the walk must not read them."""
    pm, arr = F.build_kat_map(gpu), gpu.policy_array()
    arr.set(F.KAT_SLOT, pm)
    tcp80 = _kat("IPv4 TCP port 80")
    cut = tcp80[:36]  # l4_off = 34: the source port only
    follower = tcp80[36:] + b"\0" * 40  # its first two bytes are 00 50, then the rest of a TCP header
    udp = _kat("UDP of l4_off+4 bytes")
    frames = [cut, follower, udp[:37], udp[37:] + b"\0" * 30, tcp80[:47], tcp80[47:] + b"\0" * 20, tcp80, tcp80[:13]]
    raw, off = F.join(frames)
    assert raw[int(off[1]):int(off[1]) + 2].tolist() == [0x00, 0x50]
    n = len(frames)
    kw = dict(lxc_ids=np.full(n, F.KAT_SLOT), src_labels=np.full(n, F.KAT_LABEL))
    v = arr.frame_verdicts(raw, off, **kw)
    assert np.array_equal(v, arr.frame_eval_host_diag(raw, off, **kw))
    assert v[[0, 2, 4]].tolist() == [F.DROP_CT_INVALID_HDR] * 3
    assert v[6] == 0 and v[7] == F.DROP_INVALID  # 13 bytes, the blob's last
    # the 13-byte frame in front of bytes that would make it a whole allowed packet
    raw2, off2 = F.join([tcp80[:13], tcp80[13:], tcp80])
    v2 = arr.frame_verdicts(raw2, off2, lxc_ids=[F.KAT_SLOT] * 3, src_labels=[F.KAT_LABEL] * 3)
    assert v2[0] == F.DROP_INVALID and v2[2] == 0
    assert [(e[5], e[6]) for e in U.counters(pm) if e[5]] == [(2, 2 * len(tcp80))]
    arr.destroy()
    pm.destroy()


def test_large_frames(world):
    arr, maps, twins, twin_arr, ep, ipc = world
    rng = np.random.default_rng(8)
    # 257 full-size frames: IPv4 TCP to port 80 padded to 1,400..1,514 bytes
    tcp = _to4(_kat("IPv4 TCP port 80"), "10.0.0.14")  # slot 300
    big = [tcp + bytes(rng.integers(0, 256, int(rng.integers(1400, 1515)) - len(tcp), dtype=np.uint8))
           for _ in range(257)]
    # and the 6.2 KB extension-header frame among short ones
    mixed = [tcp, _kat("IPv6 three headers of hdrlen 255"), tcp[:20], _kat("IPv6 TCP port 80"), b"", tcp] * 11
    for frames in (big, mixed):
        raw, off = F.join(frames)
        n = len(frames)
        kw = dict(lxc_ids=np.full(n, 300), src_labels=np.full(n, 900_001))
        v, info = arr.frame_verdicts(raw, off, info=True, **kw)
        hv, hinfo = arr.frame_eval_host_diag(raw, off, info=True, **kw)
        assert np.array_equal(v, hv) and np.array_equal(info, hinfo)
        ran = info["t"]["flags"] != 0
        assert ran.sum() >= n // 2
        assert np.array_equal(v[ran], twin_arr.verdicts(info["lxc_id"][ran], info["t"][ran], INGRESS))
    assert info["t"]["len"][1] == 6218 and info["t"]["proto"][1] == 6
    _assert_counters_equal(maps, twins)


def test_mixed_wave_counts_exactly(world):
    """64 frames: IPv4 and IPv6 to a hot entry, empty slots, foreign
    addresses and the host among them; packets and bytes are exact sums."""
    arr, maps, twins, twin_arr, ep, ipc = world
    keys = U.tables()[3][0]
    k = keys[(keys["sec_label"] != 0) & (keys["dport"] != 0) & (keys["egress"] == 0) & (keys["protocol"] == 6)][0]
    port = bytes([int(k["dport"]) & 0xFF, int(k["dport"]) >> 8])

    def with_port(f, l4_off):
        f = bytearray(f)
        f[l4_off + 2:l4_off + 4] = port
        return bytes(f)

    v4 = with_port(_kat("IPv4 TCP port 80"), 34)
    v6 = bytearray(with_port(_kat("IPv6 TCP port 80"), 54))
    v6[38:54] = bytes.fromhex("fd00000000000000000000000000000e")  # fd00::e: slot 300
    kinds = [_to4(v4, "10.0.0.14"), bytes(v6), _to4(v4, "10.0.0.12"), _to4(v4, "192.0.2.1"), _to4(v4, "10.0.0.1")]
    want_code = [None, None, F.DROP_MISSED_TAIL_CALL, F.NOT_LOCAL, F.TO_HOST]
    rng = np.random.default_rng(4)
    pick = rng.integers(0, len(kinds), 64)
    pick[:5] = np.arange(5)
    pad = rng.integers(0, 40, 64)
    frames = [kinds[p] + b"\0" * int(x) for p, x in zip(pick, pad)]
    raw, off = F.join(frames)
    plen = rng.integers(64, 70_000, 64).astype(np.uint32)
    plen[0] = 0xFFFF_FFF0
    label = int(k["sec_label"])
    v = arr.frame_verdicts(raw, off, endpoints=ep, src_labels=np.full(64, label), pkt_len=plen)
    hot = pick <= 1
    assert (v[hot] >= 0).all() and hot.sum() >= 10
    for j in (2, 3, 4):
        assert (v[pick == j] == want_code[j]).all()
    got = {e[:4]: (e[5], e[6]) for e in U.counters(maps[3]) if e[5] or e[6]}
    assert got == {(label, int(k["dport"]), 6, 0): (int(hot.sum()), int(plen[hot].astype(np.uint64).sum()))}
    for m in (0, 1, 2):
        assert not any(e[5] or e[6] for e in U.counters(maps[m]))


def test_pkt_len_given_against_defaulted(world):
    arr, maps, twins, twin_arr, ep, ipc = world
    raw, off, pkt_len, labels, lxc = F.shared_frames()
    n = 1000
    o = off[:n + 1]
    kw = dict(endpoints=ep, ipcache=ipc)
    v1, i1 = arr.frame_verdicts(raw, o, info=True, **kw)  # maps: bytes = frame lengths
    v2, i2 = twin_arr.frame_verdicts(raw, o, pkt_len=pkt_len[:n], info=True, **kw)  # twins: bytes = pkt_len
    assert np.array_equal(v1, v2)
    flen = np.diff(o.astype(np.int64))
    assert np.array_equal(i1["t"]["len"], flen) and np.array_equal(i2["t"]["len"], pkt_len[:n])
    a = {(m,) + e[:4]: (e[5], e[6]) for m, pm in enumerate(maps) for e in U.counters(pm) if e[5]}
    b = {(m,) + e[:4]: (e[5], e[6]) for m, pm in enumerate(twins) for e in U.counters(pm) if e[5]}
    assert a and a.keys() == b.keys() and all(a[key][0] == b[key][0] for key in a)
    _, _, _, hits = F.evaluate(F.split(raw, o), F.slot_tables(), endpoints=F.endpoints_dict(), ipcache=F.ipcache_fn)
    _, _, _, hits_p = F.evaluate(F.split(raw, o), F.slot_tables(), endpoints=F.endpoints_dict(),
                                 ipcache=F.ipcache_fn, pkt_len=pkt_len[:n])
    assert a == {(mi,) + key: tuple(c) for (mi, key), c in hits.items()}
    assert b == {(mi,) + key: tuple(c) for (mi, key), c in hits_p.items()}
    assert sum(c[1] for c in b.values()) > sum(c[1] for c in a.values())


def test_endpoint_map_update_between_two_calls(gpu, world):
    arr, maps, twins, twin_arr, _, ipc = world
    ep = gpu.endpoint_map()
    frames = [_to4(_kat("IPv4 TCP port 80"), "10.0.0.15")] * 3
    raw, off = F.join(frames)
    call = lambda: arr.frame_verdicts(raw, off, endpoints=ep, src_labels=[0, 0, 0]).tolist()
    assert call() == [F.NOT_LOCAL] * 3
    ep.write_endpoint("10.0.0.15", U.EMPTY_SLOT)
    assert call() == [F.DROP_MISSED_TAIL_CALL] * 3
    ep.write_endpoint("10.0.0.15", 300)
    policy = F.policy_can_access_ingress(F.slot_tables()[300][1], 0, 0x5000, 6, False, False)[0]
    assert call() == [policy] * 3
    ep.write_endpoint("10.0.0.15", 300, host=True)
    assert call() == [F.TO_HOST] * 3
    ep.delete_entry("10.0.0.15")
    assert call() == [F.NOT_LOCAL] * 3
    ep.destroy()


def test_dev_entry_on_a_side_stream(world):
    torch = pytest.importorskip("torch")
    arr, maps, twins, twin_arr, ep, ipc = world
    raw, off, pkt_len, labels, lxc = F.shared_frames()
    n = U.N_TUPLES
    dev = torch.device("cuda", 0)
    lead = 3  # the blob does not start at the allocation's start, nor the window at offset 0
    d_raw = torch.from_numpy(np.concatenate([np.full(lead, 0xEE, np.uint8), raw])).to(dev)
    d_off = torch.from_numpy((off + np.uint64(lead)).view(np.int64).copy()).to(dev)
    d_len = torch.from_numpy(pkt_len.view(np.int32).copy()).to(dev)
    d_out = torch.full((n,), 9, dtype=torch.int32, device=dev)
    d_info = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    arr.frame_verdicts_dev(d_raw, d_off, n, d_out, endpoints=ep, ipcache=ipc, d_pkt_len=d_len, d_info=d_info,
                           stream=side.cuda_stream)
    side.synchronize()
    got, info = d_out.cpu().numpy(), d_info.cpu().numpy().view(FRAME_INFO_DTYPE).reshape(-1)
    hv, hinfo = arr.frame_eval_host_diag(raw, off, endpoints=ep, ipcache=ipc, pkt_len=pkt_len, info=True)
    assert np.array_equal(got, hv) and np.array_equal(info, hinfo)
    assert np.array_equal(twin_arr.frame_verdicts(raw, off, endpoints=ep, ipcache=ipc, pkt_len=pkt_len), got)
    _assert_counters_equal(maps, twins)
