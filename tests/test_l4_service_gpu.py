"""l4_frames_kernel<EgressSvcProg> against the host evaluator (byte for byte)
and the Python oracle at every window size, with a given hash and with NULL;
the hand-written cases as one batch and shuffled into one wave; an empty map
equal to the call without services; the round trips; a service-map update
between two calls; the device entry on a side stream with poisoned buffers;
policy counters against a twin array driven with the oracle's translated
tuples."""
import numpy as np
import pytest

import ct_util as T
import egress_util as E
import frames_util as F
import l4_array_util as U
import service_util as S
from cilium_amd import _native as N
from cilium_amd.classifier import CT_RECORD_DTYPE, FRAME_INFO_DTYPE, LB_XLATE_DTYPE
from cilium_amd.policy import htons

pytestmark = [pytest.mark.gpu, pytest.mark.run_last]


@pytest.fixture
def world(gpu):
    maps, twins = U.build_maps(gpu), U.build_maps(gpu)
    arr, twin_arr = E.build_array(gpu, maps), E.build_array(gpu, twins)
    ipc = F.build_ipcache(gpu)
    ct = S.build_ct(gpu, *S.shared_table())
    svc = S.build_service_map(gpu, S.shared_world())
    yield arr, maps, twins, twin_arr, ipc, ct, svc
    for x in (svc, ct, arr, twin_arr, ipc, *maps, *twins):
        x.destroy()


@pytest.mark.parametrize("with_hash", [True, False], ids=["hash", "null-hash"])
def test_kernel_equals_host_evaluator_and_oracle(gpu, world, with_hash):
    arr, maps, twins, twin_arr, ipc, ct, svc = world
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    h = S.shared_hash() if with_hash else None
    for k, (first, n) in enumerate(S.WINDOWS):
        sl = slice(first, first + n)
        ignore_drop = k % 2 == 1
        kw = dict(lxc_ids=lxc[sl], ipcache=ipc, pkt_len=pkt_len[sl], info=True, conntrack=ct, services=svc,
                  hash=None if h is None else h[sl], xlate=True, ignore_drop=ignore_drop)
        o = off[first:first + n + 1]
        got = arr.frame_egress_verdicts(raw, o, **kw)
        host = arr.frame_egress_eval_host_diag(raw, o, **kw)
        exp = S.shared_expected(with_hash, ignore_drop)
        S.assert_same(got, host, what=f"n={n} host: ")
        S.assert_same(got, exp[:5], sl, f"n={n} oracle: ")
        # the twin array sees the translated tuples the oracle extracts, through the tuple kernel in egress mode
        t, done = E.extracted_tuples(exp[1][sl])
        if done.any():
            twin_arr.verdicts(lxc[sl][done], t, mode=N.CG_L4_EGRESS | (N.CG_L4_IGNORE_DROP if ignore_drop else 0))
    for pm, tw in zip(maps, twins):
        assert U.counters(pm) == U.counters(tw)
    assert any(e[5] for e in U.counters(maps[3]))


def test_hand_written_cases_as_one_batch(gpu):
    arr, pm, ipc, ct, svc, raw, off, lxc, hashes, g = S.kat_setup(gpu)
    kw = dict(lxc_ids=lxc, ipcache=ipc, info=True, conntrack=ct, services=svc, hash=hashes, xlate=True)
    got = arr.frame_egress_verdicts(raw, off, **kw)
    S.check_kat(g, *got)
    S.assert_same(got, arr.frame_egress_eval_host_diag(raw, off, **kw))
    for x in (svc, ct, ipc, arr, pm):
        x.destroy()


def test_mixed_wave(gpu):
    """One 64-frame wave in which neighbouring lanes leave the program at
    different steps: the hand-written cases, shuffled, each lane with its own
    expectation."""
    arr, pm, ipc, ct, svc, raw, off, lxc, hashes, g = S.kat_setup(gpu)
    frames = F.split(raw, off)
    rng = np.random.default_rng(8)
    pick = np.concatenate([rng.permutation(len(frames)), rng.integers(0, len(frames), 64)])[:64]
    assert len({(c["expect"]["verdict"], c["expect"]["xlate"]["status"], c["expect"]["srec"]["state"])
                for c in g["frames"]}) >= 8
    wave, o = F.join([frames[p] for p in pick])
    v, info, rec, srec, xl = arr.frame_egress_verdicts(wave, o, lxc_ids=lxc[pick], ipcache=ipc, info=True, conntrack=ct,
                                                       services=svc, hash=hashes[pick], xlate=True)
    for lane, p in enumerate(pick):
        S.check_kat_case(g["frames"][p], v[lane], info[lane], rec[lane], srec[lane], xl[lane])
    for x in (svc, ct, ipc, arr, pm):
        x.destroy()


def test_empty_service_map_equals_no_services(gpu, world):
    arr, maps, twins, twin_arr, ipc, _, _ = world
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    ct = T.build_map(gpu, *E.shared_table())
    empty = gpu.service_map()
    kw = dict(lxc_ids=lxc, ipcache=ipc, pkt_len=pkt_len, info=True, conntrack=ct)
    v0, i0, r0 = twin_arr.frame_egress_verdicts(raw, off, **kw)
    v, i, r, sr, x = arr.frame_egress_verdicts(raw, off, services=empty, xlate=True, **kw)
    assert np.array_equal(v, v0) and i.tobytes() == i0.tobytes() and r.tobytes() == r0.tobytes()
    assert sr.tobytes() == bytes(64 * len(sr)) and set(x["status"].tolist()) == {S.NONE, S.MISS}
    for pm, tw in zip(maps, twins):
        assert U.counters(pm) == U.counters(tw)
    empty.destroy()
    ct.destroy()


def test_round_trips_on_the_device(gpu):
    S.check_round_trips(gpu,
                        lambda arr, raw, off, **kw: arr.frame_egress_verdicts(raw, off, info=True, xlate=True, **kw),
                        lambda arr, raw, off, **kw: arr.frame_verdicts(raw, off, info=True, **kw))


def test_service_map_update_between_calls(gpu):
    pm, arr, hd = E.egress_world(gpu, ports=((2000, 8080, 6, 1, 0), (2000, 9090, 6, 1, 0)))
    ct, ipc, svc = gpu.conntrack_map(), gpu.ipcache(), gpu.service_map()
    ipc.upsert("10.2.0.0/16", 2000)
    raw, off = F.join([E.ip4(hd, "10.96.0.1", 6, E.tcp(40000 + i, 80)) for i in range(130)])
    kw = dict(lxc_ids=[5] * 130, ipcache=ipc, conntrack=ct, services=svc, xlate=True)

    def call():
        v, x = arr.frame_egress_verdicts(raw, off, **kw)
        return set(v.tolist()), set(x["status"].tolist()), {S._addr(a, 4) for a in x["daddr"]}, set(x["dport"].tolist())

    assert call() == ({N.CG_DROP_POLICY}, {S.MISS}, {"0.0.0.0"}, {0})
    svc.update_service(("10.96.0.1", 80), [("10.2.0.1", 8080)], True, 5)
    assert call() == ({0}, {S.TRANSLATED}, {"10.2.0.1"}, {htons(8080)})
    # the whole service changes in one update of the slave: no frame sees half of it
    svc.update([svc.key("10.96.0.1", htons(80), 1)], [svc.value("10.2.0.9", htons(9090), 0, 5)])
    assert call() == ({0}, {S.TRANSLATED}, {"10.2.0.9"}, {htons(9090)})
    svc.update_service(("10.96.0.1", 80), [], True, 5)
    assert call() == ({N.CG_DROP_POLICY}, {S.MISS}, {"0.0.0.0"}, {0})
    for o in (svc, ct, ipc, arr, pm):
        o.destroy()


def test_dev_entry_on_a_side_stream(gpu, world):
    torch = pytest.importorskip("torch")
    arr, maps, twins, twin_arr, ipc, ct, svc = world
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    n = U.N_TUPLES
    dev = torch.device("cuda", 0)
    lead = 3  # the blob does not start at the allocation's start, nor the window at offset 0
    d_raw = torch.from_numpy(np.concatenate([np.full(lead, 0xEE, np.uint8), raw])).to(dev)
    d_off = torch.from_numpy((off + np.uint64(lead)).view(np.int64).copy()).to(dev)
    d_len = torch.from_numpy(pkt_len.view(np.int32).copy()).to(dev)
    d_lxc = torch.from_numpy(lxc.view(np.int16).copy()).to(dev)
    d_hash = torch.from_numpy(S.shared_hash().view(np.int32).copy()).to(dev)
    d_out = torch.full((n,), 9, dtype=torch.int32, device=dev)
    d_info = torch.full((n, 16), 0xAB, dtype=torch.uint8, device=dev)
    d_rec, d_srec = (torch.full((n, 64), 0xAB, dtype=torch.uint8, device=dev) for _ in range(2))
    d_xl = torch.full((n, 48), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    kw = dict(d_lxc_ids=d_lxc, ipcache=ipc, d_pkt_len=d_len, stream=side.cuda_stream, conntrack=ct, services=svc,
              d_hash=d_hash)
    arr.frame_egress_verdicts_dev(d_raw, d_off, n, d_out, d_info=d_info, d_records=d_rec, d_svc_records=d_srec,
                                  d_xlate=d_xl, **kw)
    side.synchronize()
    got = (d_out.cpu().numpy(), d_info.cpu().numpy().view(FRAME_INFO_DTYPE).reshape(-1),
           d_rec.cpu().numpy().view(CT_RECORD_DTYPE).reshape(-1), d_srec.cpu().numpy().view(CT_RECORD_DTYPE).reshape(-1),
           d_xl.cpu().numpy().view(LB_XLATE_DTYPE).reshape(-1))
    S.assert_same(got, S.shared_expected(True)[:5])
    # optional outputs not asked for are left untouched
    for t in (d_info, d_rec, d_srec, d_xl):
        t.fill_(0xCD)
    d_out.fill_(9)
    arr.frame_egress_verdicts_dev(d_raw, d_off, n, d_out, **kw)
    side.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), got[0])
    assert all((t.cpu().numpy() == 0xCD).all() for t in (d_info, d_rec, d_srec, d_xl))
    # without a conntrack map the call is refused and nothing is written
    d_out.fill_(9)
    with pytest.raises(N.CiliumGPUError) as ei:
        arr.frame_egress_verdicts_dev(d_raw, d_off, n, d_out, d_lxc_ids=d_lxc, ipcache=ipc, services=svc)
    assert ei.value.code == N.CG_INVALID_ARGUMENT and (d_out.cpu().numpy() == 9).all()
