"""Throughput of the three non-north-star verdict kernels at their BASELINE
configs, one JSON line each (bench.py covers config 5, the 10K-rule HTTP set):

* L4 policymap (config 2): 16K-entry table, 100M tuples
* CIDR prefilter (config 3): 1M mixed v4/v6 prefixes, 1B addresses
* Kafka (config 4): 1K rules, 100M requests
* ipcache: 512K-entry IP → identity map, 1B addresses
* L4 with ipcache identities: config 2's map, identities resolved in-kernel
* proxylib r2d2: 512 r2d2 rules over 64 ports, ~100M requests
  on the HTTP kernel
* selcache (opt-in, --paths selcache): selector x identity matching and L3
  reach, 65,536 identities, a 10,000-rule repository, 256 endpoints, and the
  expansion of those bitsets into policy-map entries
* selcache_cidr (opt-in, --paths selcache_cidr): the selector cache's prefix
  section — 262,144 prefix identities beside 65,536 label identities, the
  10,000-rule repository plus 1,024 cidr: selectors — against the host walker
  and against the same prefixes as explicit label identities
* l4_array (opt-in, --paths l4_array): the policy program array — 256 maps of
  config 2's table mix, 100M tuples that each name their endpoint, against
  the per-map route (pre-grouped launches; sort + launches + scatter from
  host data) and the single-map figure
* l4_frames (opt-in, --paths l4_frames): L4 verdicts from raw Ethernet frames
  — 2^24 frames snapped to 96 B over 256 endpoints, endpoint and source
  identity resolved on the device — against the tuple route on pre-extracted
  tuples and against host extraction + upload + that route; with a conntrack
  map; and the egress program (l4_frames_kernel<EgressProg>) on an egress batch of
  the same shape, with and without conntrack and records, as ratios to the
  ingress kernels of the same run; and that program over a synthetic service
  map (l4_frames_kernel<EgressSvcProg>), on the batch as it is and with a quarter
  of its frames snapped to VIPs, as ratios to the egress kernel with records

Inputs are resident in HBM before timing; kernels are timed with HIP events
on their stream.  Each line carries the kernel's HBM roofline (algorithmic
bytes: packed input + output per item) and the CPU oracle timed on a sample.
Distinct synthetic items are generated on the host and tiled on the device
to the config's count; verdicts of the first copy are checked against the
oracle before timing.

    python tools/bench_paths.py [--paths l4,lpm,kafka] [--steps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0


def tile_dev(torch, host: np.ndarray, reps: int, dev):
    """Device array of `reps` back-to-back copies of host (doubling copies)."""
    raw = host.reshape(-1).view(np.uint8)
    d = torch.empty(raw.nbytes * reps, dtype=torch.uint8, device=dev)
    d[:raw.nbytes].copy_(torch.from_numpy(raw))
    done = 1
    while done < reps:
        k = min(done, reps - done)
        d[done * raw.nbytes:(done + k) * raw.nbytes].copy_(d[:k * raw.nbytes])
        done += k
    return d


PREWARM_S = 0.3  # --prewarm-seconds


def timed(torch, stream, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    # untimed launches for PREWARM_S, so the timed ones start at the clocks
    # the GPU holds (a few warm-up launches leave it ~4% slow: bench.py)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < PREWARM_S:
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
    ev = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        ev.append((a, b))
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev) / steps * 1e-3


def cpu_rate(fn, items, seconds):
    if seconds <= 0:
        return None
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        fn()
        n += items
    return n / (time.perf_counter() - t0)


def cpu_rate_mt(fn, chunks, threads, seconds):
    """cpu_rate over `threads` host threads: fn(chunk) on every chunk per
    round (fn must release the GIL, as the ctypes oracle calls do)."""
    if seconds <= 0:
        return None
    from concurrent.futures import ThreadPoolExecutor
    items = sum(len(c) for c in chunks)
    with ThreadPoolExecutor(threads) as ex:
        t0, n = time.perf_counter(), 0
        while time.perf_counter() - t0 < seconds:
            list(ex.map(fn, chunks))
            n += items
        return n / (time.perf_counter() - t0)


def line(metric, n, sec, bytes_per_item, kernel, cpu, cpu_sample, threads, extra):
    achieved = n * bytes_per_item / sec / 1e9
    return {"metric": metric, "value": n / sec, "unit": "verdicts/s", "n_gpus": 1, "ms_per_launch": sec * 1e3,
            "items_per_launch": n, "higher_is_better": True, "data": "synthetic",
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBPS, "kernel": kernel, "bytes_per_item": bytes_per_item},
            "cpu_baseline": {"value": cpu, "unit": "verdicts/s", "cores": threads, "kind": "port",
                             "sample": cpu_sample}, **extra}


def bench_l4(torch, dev, stream, cl, args, threads):
    import oracle
    from cilium_amd import synth
    keys, ports = synth.l4_table()
    pm = cl.policy_map()
    pm.allow_keys(keys, ports)
    D, reps = 10_000_000, 10
    tup = synth.l4_tuples(D, keys)
    got = pm.verdicts(tup[:2_000_000])
    exp, _, _ = oracle.l4(keys, ports, tup[:2_000_000])
    assert np.array_equal(got, exp), "L4 verdicts differ from the oracle"
    d_t = tile_dev(torch, tup, reps, dev)
    n = D * reps
    d_o = torch.empty(n, dtype=torch.int32, device=dev)
    sec = timed(torch, stream, lambda: pm.verdicts_dev(d_t, n, d_o, stream=stream.cuda_stream), args.steps, 2)
    chunks = [tup[i * 250_000:(i + 1) * 250_000] for i in range(threads)]
    cpu = cpu_rate_mt(lambda c: oracle.l4(keys, ports, c), chunks, threads, args.cpu_seconds)
    cpu1 = cpu_rate(lambda: oracle.l4(keys, ports, chunks[0]), len(chunks[0]), min(args.cpu_seconds, 2.0))
    kern = "l4_fp_kernel"  # a 16,384-entry map's fingerprints + counters fit LDS
    return line("L4 policymap verdicts/s (__policy_can_access), config 2", n, sec, 16, kern, cpu,
                f"{threads} x 250K tuples of the same workload, {threads} threads (single-core: {cpu1:.4g}/s)"
                if cpu else "", threads,
                {"config": {"workload": "BASELINE config 2: 16,384-entry policy map, 100M tuples",
                            "entries": int(len(keys)), "tuples": n}})


def _l4_table_mix(rng, n_entries=16384, n_ids=16384):
    """synth.l4_table's mix (70% {id,port,proto,dir}, 20% {id,0,0,dir}, 10%
    {0,port,proto,dir}; 20% of the entries redirect) drawn with array
    operations, so that 256 tables take seconds."""
    from cilium_amd.classifier import POLICY_KEY_DTYPE
    m = n_entries * 5 // 4
    ids = np.concatenate([np.arange(1, 6), 256 + np.arange(n_ids)]).astype(np.uint32)
    r = rng.random(m)
    k = np.zeros(m, POLICY_KEY_DTYPE)
    port = rng.integers(1, 65536, m).astype(np.uint16)
    k["sec_label"] = np.where(r < 0.9, ids[rng.integers(0, len(ids), m)], 0)
    k["dport"] = np.where((r < 0.7) | (r >= 0.9), (port & 0xFF) << 8 | port >> 8, 0)
    k["protocol"] = np.where(k["dport"] != 0, np.where(rng.random(m) < 0.5, 6, 17), 0)
    k["egress"] = rng.integers(0, 2, m)
    _, first = np.unique(k.view(np.uint64), return_index=True)
    k = k[np.sort(first)[:n_entries]]
    assert len(k) == n_entries
    p = np.where(rng.random(n_entries) < 0.8, 0, rng.integers(10000, 11000, n_entries)).astype(np.uint16)
    return k, ((p & 0xFF) << 8 | p >> 8).astype(np.uint16)


def _l4_array_tuples(rng, lxc_map, tports, n_ids=16384):
    """synth.l4_tuples' recipe with each tuple's table ports taken from its
    own endpoint's table (tports[map]): identity uniform over the ids + 10
    unknown, dport 50% a table port (Zipf s=1.1) / 50% uniform, proto and dir
    50/50, fragment 1%, CB_POLICY 1%, len 64-1500."""
    from cilium_amd.classifier import L4_TUPLE_DTYPE
    n = len(lxc_map)
    t = np.zeros(n, L4_TUPLE_DTYPE)
    ids = np.concatenate([np.arange(1, 6), 256 + np.arange(n_ids), 900000 + np.arange(10)]).astype(np.uint32)
    t["identity"] = ids[rng.integers(0, len(ids), n)]
    z = np.minimum(rng.zipf(1.1, n) - 1, tports.shape[1] - 1)
    uni = rng.integers(1, 65536, n).astype(np.uint16)
    t["dport"] = np.where(rng.random(n) < 0.5, tports[lxc_map, z], (uni & 0xFF) << 8 | uni >> 8)
    t["proto"] = np.where(rng.random(n) < 0.5, 6, 17)
    t["flags"] = ((rng.random(n) < 0.5).astype(np.uint8) | (rng.random(n) < 0.01).astype(np.uint8) << 1 |
                  (rng.random(n) < 0.01).astype(np.uint8) << 2)
    t["len"] = rng.integers(64, 1501, n)
    return t


def bench_l4_array(torch, dev, stream, cl, args, threads):
    """The policy program array: 256 endpoints' maps (config 2's table mix,
    each drawn with its own seed), config 2's tuples tiled to 100M, every
    tuple naming its endpoint — uniformly per tuple, or in runs of geometric
    length (mean 64).  Checked against cg_diag_l4_array_eval_host before
    timing.  Beside the array kernel: the per-map route in the same process
    (the tuples pre-grouped by endpoint, 256 cg_l4_policy_verdicts_dev
    launches; and its wall time from ungrouped host data, with the host
    argsort and the scatter back), and bench_l4's single-map figure."""
    from cilium_amd import _native as N
    E, D = 256, args.array_tuples
    n = min(100_000_000, 2 * D)  # the first copy and the start of a second
    mode = N.CG_L4_INGRESS
    rng = np.random.default_rng(0xA77A)
    maps, tports = [], []
    for e in range(E):
        keys, ports = _l4_table_mix(np.random.default_rng(1000 + e))
        pm = cl.policy_map()
        pm.allow_keys(keys, ports)
        maps.append(pm)
        tports.append(keys["dport"][keys["dport"] != 0])
    tports = np.stack([p[:min(len(q) for q in tports)] for p in tports])
    slots = (np.arange(E) * 257).astype(np.uint16)  # 0, 257, ..., 65535
    arr = cl.policy_array()
    arr.set_many(slots, maps)
    runs = rng.geometric(1.0 / 64, D // 32)
    mixes = {"uniform": rng.integers(0, E, D).astype(np.uint16),
             "runs64": np.repeat(rng.integers(0, E, len(runs)).astype(np.uint16), runs)[:D]}
    assert len(mixes["runs64"]) == D
    d_o = torch.empty(n, dtype=torch.int32, device=dev)
    res, cpu = {}, None
    for name, which in mixes.items():
        tup = _l4_array_tuples(rng, which, tports)
        lxc = slots[which]
        d_t = torch.empty(n * 12, dtype=torch.uint8, device=dev)
        d_t[:D * 12].copy_(torch.from_numpy(tup.view(np.uint8)))
        d_t[D * 12:].copy_(d_t[:(n - D) * 12])
        d_l = torch.empty(n, dtype=torch.int16, device=dev)
        d_l[:D].copy_(torch.from_numpy(lxc.view(np.int16)))
        d_l[D:].copy_(d_l[:n - D])
        # the check: the first copy against the host evaluator
        arr.verdicts_dev(d_l, d_t, D, d_o, stream=stream.cuda_stream, mode=mode)
        stream.synchronize()
        t0 = time.perf_counter()
        want = arr.eval_host_diag(lxc, tup, mode)
        cpu = cpu or D / (time.perf_counter() - t0)
        assert np.array_equal(d_o[:D].cpu().numpy(), want), "array verdicts differ from the host evaluator"
        sec = timed(torch, stream,
                    lambda: arr.verdicts_dev(d_l, d_t, n, d_o, stream=stream.cuda_stream, mode=mode), args.steps, 2)
        r = res[name] = {"kernel_ms": sec * 1e3, "Gtuples_s": n / sec / 1e9,
                         "roofline_frac": n * 18 / sec / 1e9 / HBM_PEAK_GBPS,
                         "hit_frac": float((want >= 0).mean())}
        # the per-map route, kernels only: grouped on the device beforehand
        order = torch.argsort(d_l.to(torch.int32) & 0xFFFF, stable=True)
        g_t = d_t.view(n, 12)[order].contiguous()
        counts = np.bincount(which, minlength=E).astype(np.int64) * (n // D)
        counts += np.bincount(which[:n - D * (n // D)], minlength=E)
        del order
        offs = np.concatenate([[0], np.cumsum(counts)])
        g_o = torch.empty(n, dtype=torch.int32, device=dev)

        def per_map(g_t=g_t, g_o=g_o, offs=offs):
            for e in range(E):
                a, b = int(offs[e]), int(offs[e + 1])
                maps[e].verdicts_dev(g_t[a:b], b - a, g_o[a:b], stream=stream.cuda_stream, mode=mode)
        sec_pm = timed(torch, stream, per_map, args.steps, 1)
        r["per_map_grouped"] = {"kernel_ms": sec_pm * 1e3, "Gtuples_s": n / sec_pm / 1e9, "launches": E}
        del g_t, g_o
        # the per-map route from ungrouped host data: what a caller of the
        # single-map entries has to do (sort, 256 calls, scatter back)
        t0 = time.perf_counter()
        h_order = np.argsort(lxc, kind="stable")
        h_t = tup[h_order]
        h_offs = np.concatenate([[0], np.cumsum(np.bincount(which, minlength=E))])
        dd_t = torch.from_numpy(h_t.view(np.uint8)).to(dev)
        dd_o = torch.empty(D, dtype=torch.int32, device=dev)
        for e in range(E):
            a, b = int(h_offs[e]), int(h_offs[e + 1])
            maps[e].verdicts_dev(dd_t[a * 12:b * 12], b - a, dd_o[a:b], stream=stream.cuda_stream, mode=mode)
        stream.synchronize()
        back = np.empty(D, np.int32)
        back[h_order] = dd_o.cpu().numpy()
        wall_pm = time.perf_counter() - t0
        assert np.array_equal(back, want), "the per-map route differs from the host evaluator"
        t0 = time.perf_counter()
        dd_t = torch.from_numpy(tup.view(np.uint8)).to(dev)
        dd_l = torch.from_numpy(lxc.view(np.int16)).to(dev)
        arr.verdicts_dev(dd_l, dd_t, D, dd_o, stream=stream.cuda_stream, mode=mode)
        stream.synchronize()
        back = dd_o.cpu().numpy()
        wall_arr = time.perf_counter() - t0
        r["from_host_data"] = {"tuples": D, "per_map_wall_s": wall_pm, "array_wall_s": wall_arr}
        del d_t, d_l, dd_t, dd_l, dd_o
    ceiling = bench_l4(torch, dev, stream, cl, argparse.Namespace(**{**vars(args), "cpu_seconds": 0}), threads)
    u = res["uniform"]
    return line("L4 verdicts/s across 256 endpoints (l4_array_kernel: the policy program array, endpoint ids "
                "uniform per tuple)", n, u["kernel_ms"] * 1e-3, 18, "l4_array_kernel", cpu,
                "cg_diag_l4_array_eval_host over the first copy, one thread", 1,
                {"config": {"workload": "256 policy maps of config 2's 16,384-entry mix, config 2's tuples",
                            "maps": E, "distinct_tuples": D, "tuples": n},
                 "mixes": res, "single_map_ceiling_Gtuples_s": ceiling["value"] / 1e9})


def _bench_l4_frames_ct(torch, dev, stream, cl, args, arr, kw, raw, off, plen, d_raw, d_off, d_len, d_out, D, n,
                        sec_plain):
    """l4_frames_kernel<IngressProg> with conntrack on bench_l4_frames' batch, against a global
    conntrack map of at least 2^20 keys derived from the frames: of the TCP /
    UDP frames whose walk completes a third get their reply key (the tuple as
    loaded), a third their established key (the reversed tuple), a third
    none; random keys fill the table up to 2^20.  Checked against
    cg_diag_l4_frames_ct_eval_host over the first copy; timed with and
    without the 64-byte records."""
    from cilium_amd import _native as N
    from cilium_amd.classifier import CT_KEY_DTYPE, CT_RECORD_DTYPE
    _, winfo, l4o = arr.frame_eval_host_diag(raw, off, pkt_len=plen, info=True, l4_off=True, **kw)
    proto = winfo["t"]["proto"]
    sel = np.flatnonzero((winfo["t"]["flags"] != 0) & ((proto == 6) | (proto == 17)))
    sel = sel[sel % 3 != 2]
    b = off[:-1].astype(np.int64)[sel]
    fam = winfo["family"][sel]
    keys = np.zeros(len(sel), CT_KEY_DTYPE)
    for f, so, do, size in ((4, 26, 30, 4), (6, 22, 38, 16)):
        m = fam == f
        keys["saddr"][m, :size] = raw[b[m][:, None] + np.arange(so, so + size)]
        keys["daddr"][m, :size] = raw[b[m][:, None] + np.arange(do, do + size)]
    p = b + l4o[sel]
    keys["dport"] = raw[p].astype(np.uint16) | raw[p + 1].astype(np.uint16) << 8
    keys["sport"] = raw[p + 2].astype(np.uint16) | raw[p + 3].astype(np.uint16) << 8
    keys["nexthdr"], keys["family"] = proto[sel], fam
    keys["kind"] = np.where(proto[sel] == 6, N.CG_CT_MAP_TCP, N.CG_CT_MAP_ANY)
    est = sel % 3 == 1  # the reversed tuple: addresses and ports swapped, TUPLE_F_IN
    rev = keys[est].copy()
    rev["daddr"], rev["saddr"] = keys["saddr"][est], keys["daddr"][est]
    rev["dport"], rev["sport"], rev["flags"] = keys["sport"][est], keys["dport"][est], N.CG_TUPLE_F_IN
    keys[est] = rev
    keys = np.unique(keys)
    target = 1 << 20
    if len(keys) < target:
        rng = np.random.default_rng(0xC7)
        fill = np.zeros(target - len(keys), CT_KEY_DTYPE)
        fill["daddr"][:, :4], fill["saddr"][:, :4] = rng.integers(0, 256, (len(fill), 4)), [172, 31, 0, 0]
        fill["sport"], fill["nexthdr"], fill["family"] = rng.integers(0, 65536, len(fill)), 6, 4
        fill["dport"] = np.arange(len(fill)) & 0xFFFF
        keys = np.unique(np.concatenate([keys, fill]))
    ct = cl.conntrack_map(max_entries=max(2 * len(keys), target), global_map=True)
    ct.update(keys)
    d_rec = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    arr.frame_verdicts_dev(d_raw, d_off, D, d_out, d_pkt_len=d_len, stream=stream.cuda_stream, conntrack=ct,
                           d_records=d_rec, **kw)
    stream.synchronize()
    want, _, wrec = arr.frame_eval_host_diag(raw, off, pkt_len=plen, info=True, conntrack=ct, **kw)
    assert np.array_equal(d_out[:D].cpu().numpy(), want), "conntrack frame verdicts differ from the host evaluator"
    assert d_rec[:D].cpu().numpy().tobytes() == wrec.tobytes(), "conntrack records differ from the host evaluator"
    sec_rec = timed(torch, stream, lambda: arr.frame_verdicts_dev(
        d_raw, d_off, n, d_out, d_pkt_len=d_len, stream=stream.cuda_stream, conntrack=ct, d_records=d_rec, **kw),
        args.steps, 2)
    del d_rec
    sec = timed(torch, stream, lambda: arr.frame_verdicts_dev(
        d_raw, d_off, n, d_out, d_pkt_len=d_len, stream=stream.cuda_stream, conntrack=ct, **kw), args.steps, 2)
    done = wrec["state"] != 0
    info = ct.table_info()
    ct.destroy()
    return {"kernel": "l4_frames_kernel<IngressProg<ep, ipc, ct>>", "table_keys": int(len(keys)),
            "table_buckets": {"v4": info[4][0], "v6": info[6][0]}, "table_probe_bound": {"v4": info[4][1], "v6": info[6][1]},
            "table_bytes": 128 * (info[4][0] + info[6][0]),
            "state_frac_of_looked_up": {name: float((wrec["state"][done] == s).mean()) for s, name in
                                        ((1, "new"), (2, "established"), (3, "reply"), (4, "related"))},
            "looked_up_frac": float(done.mean()),
            "kernel_ms": sec * 1e3, "Gframes_s": n / sec / 1e9, "over_no_conntrack": sec / sec_plain,
            "with_records": {"kernel_ms": sec_rec * 1e3, "Gframes_s": n / sec_rec / 1e9,
                             "over_no_conntrack": sec_rec / sec_plain}}


def _bench_l4_frames_services(torch, dev, stream, cl, args, arr, ct, kw, hkw, raw, off, winfo, l4o, d_off, d_out, D, n,
                              reps, sec_egress_rec):
    """l4_frames_kernel<EgressSvcProg> on _bench_l4_frames_egress' batch and conntrack
    map, over a synthetic service map: 4,096 IPv4 L3 services and 1,024 IPv6
    ones of four backends each (backends drawn from the batch's own
    destinations, so the ipcache knows them), every second one rewriting the
    port.  Two batches: the egress batch as it is, where no frame hits a
    service, and the same frames with a quarter of the TCP / UDP / ICMP frames
    that reach the policy snapped to a VIP.  Each is checked against
    cg_diag_l4_frames_egress_svc_eval_host over the first copy, then timed
    three ways: verdicts only, plus records, plus service records and
    translation records.  The ratios are to l4_frames_kernel<EgressProg<ipc,
    ct>> with records in this same run."""
    from cilium_amd.classifier import CT_RECORD_DTYPE, LB_XLATE_DTYPE
    rng = np.random.default_rng(0x5C)
    svc = cl.service_map(ipv4_loopback="169.254.42.1")
    walked = np.flatnonzero(winfo["t"]["flags"] != 0)
    b = off[:-1].astype(np.int64)
    fam = winfo["family"]
    w4, w6 = walked[fam[walked] == 4], walked[fam[walked] == 6]
    be4 = np.unique(raw[b[w4][:, None] + np.arange(30, 34)], axis=0)
    be6 = np.unique(raw[b[w6][:, None] + np.arange(38, 54)], axis=0)
    keys, vals = [], []
    vips = {4: [], 6: []}
    for f, nsvc, pool in ((4, 4096, be4), (6, 1024, be6)):
        for i in range(nsvc):
            vip = bytes([198, 18, i >> 8, i & 255]) if f == 4 else bytes([0xfd, 0x96] + [0] * 12 + [i >> 8, i & 255])
            vips[f].append(vip)
            keys.append(svc.key(vip, 0, 0))
            vals.append(svc.value(None, 0, 4, 0, 0))
            for s_ in range(1, 5):
                keys.append(svc.key(vip, 0, s_))
                port = 0 if i % 2 else int(rng.integers(1024, 65535))
                vals.append(svc.value(bytes(pool[rng.integers(0, len(pool))]), port, 0, 1 + (i & 0x3FFF), 0))
    svc.update(keys, vals)
    svc.update_revnat(np.arange(1, 4097), vips[4], np.zeros(4096, np.uint16))
    d_rec, d_srec = (torch.empty((n, 64), dtype=torch.uint8, device=dev) for _ in range(2))
    d_xl = torch.empty((n, 48), dtype=torch.uint8, device=dev)
    out = {"kernel": "l4_frames_kernel<EgressSvcProg>", "services": {"v4": 4096, "v6": 1024, "backends_each": 4},
           "yardstick": "l4_frames_kernel<EgressProg<ipc, ct>> with records, this run",
           "yardstick_kernel_ms": sec_egress_rec * 1e3}
    snapped = raw.copy()
    pick = walked[rng.random(len(walked)) < 0.25]
    for f, do, size in ((4, 30, 4), (6, 38, 16)):
        m = pick[fam[pick] == f]
        choice = np.array([list(v) for v in vips[f]], np.uint8)[rng.integers(0, len(vips[f]), len(m))]
        snapped[b[m][:, None] + np.arange(do, do + size)] = choice
    for name, blob_ in (("no_service_hit", raw), ("quarter_snapped_to_vips", snapped)):
        d_raw = tile_dev(torch, blob_, reps, dev)
        call = lambda **extra: arr.frame_egress_verdicts_dev(d_raw, d_off, n, d_out, conntrack=ct, services=svc,  # noqa: E731
                                                             **extra, **kw)
        arr.frame_egress_verdicts_dev(d_raw, d_off, D, d_out, conntrack=ct, services=svc, d_records=d_rec,
                                      d_svc_records=d_srec, d_xlate=d_xl, **kw)
        stream.synchronize()
        want, _, wrec, wsrec, wxl = arr.frame_egress_eval_host_diag(blob_, off, info=True, conntrack=ct, services=svc,
                                                                    xlate=True, **hkw)
        assert np.array_equal(d_out[:D].cpu().numpy(), want), "service verdicts differ from the host evaluator"
        assert d_rec[:D].cpu().numpy().tobytes() == wrec.tobytes(), "service route: records differ"
        assert d_srec[:D].cpu().numpy().tobytes() == wsrec.tobytes(), "service route: service records differ"
        assert d_xl[:D].cpu().numpy().tobytes() == wxl.tobytes(), "service route: translation records differ"
        sec_v = timed(torch, stream, lambda: call(), args.steps, 2)
        sec_r = timed(torch, stream, lambda: call(d_records=d_rec), args.steps, 2)
        sec_a = timed(torch, stream, lambda: call(d_records=d_rec, d_svc_records=d_srec, d_xlate=d_xl), args.steps, 2)
        ran = wsrec["state"] != 0
        out[name] = {
            "service_hit_frac": float(np.isin(wxl["status"], (2, 3)).mean()),
            "translated_frac": float((wxl["status"] == 2).mean()), "no_service_frac": float((wxl["status"] == 3).mean()),
            "service_state_frac": {k_: float((wsrec["state"][ran] == s_).mean()) if ran.any() else 0.0
                                   for s_, k_ in ((1, "new"), (3, "reply"), (4, "related"))},
            "egress_state_frac": {k_: float((wrec["state"][wrec["state"] != 0] == s_).mean())
                                  for s_, k_ in ((1, "new"), (2, "established"), (3, "reply"), (4, "related"))},
            "verdicts_only": {"kernel_ms": sec_v * 1e3, "Gframes_s": n / sec_v / 1e9},
            "with_records": {"kernel_ms": sec_r * 1e3, "Gframes_s": n / sec_r / 1e9,
                             "over_egress_ct_records_same_run": sec_r / sec_egress_rec},
            "with_records_svc_records_xlate": {"kernel_ms": sec_a * 1e3, "Gframes_s": n / sec_a / 1e9,
                                               "over_egress_ct_records_same_run": sec_a / sec_egress_rec}}
        del d_raw
    svc.destroy()
    return out


def _bench_l4_frames_egress(torch, dev, stream, cl, args, maps, slots, ipc, s4, s6, tports, D, n, reps, sec_in,
                            sec_in_ct, sec_in_ct_rec):
    """l4_frames_kernel<EgressProg> on an egress batch of the ingress line's shape:
    the same 256 maps (config 2's mix holds egress keys) in an array whose
    slots carry endpoint headers, the same ipcache resolving destinations,
    frames of synth.l4_egress_frames snapped to 96 bytes, tiled to 2^24.
    Checked against cg_diag_l4_frames_egress_eval_host over the first copy;
    timed without conntrack and, against a global map derived as
    _bench_l4_frames_ct derives it, with and without records.  The ratios
    are to the ingress kernels' times of this same run.  → (the services
    object of _bench_l4_frames_services on this batch, the egress object)."""
    from cilium_amd import _native as N
    from cilium_amd import synth
    from cilium_amd.classifier import CT_KEY_DTYPE, FRAME_INFO_DTYPE
    E = len(maps)
    arr = cl.policy_array()
    arr.set_many(slots, maps)
    hdrs = np.concatenate([arr.header(mac=bytes([0x0a, 0, 0, 0, e >> 8, e & 255]), node_mac="02:00:00:00:00:01",
                                      ipv4=bytes([10, 200, e >> 4, e & 15]), ipv6=bytes([0xfd] + [0] * 14 + [e]),
                                      router_ip6="fd00::ffff", seclabel=256 + e) for e in range(E)])
    arr.set_headers(slots, hdrs)
    chunks = [synth.l4_egress_frames(D // 4, slots, hdrs, s4.view(np.uint8).reshape(-1, 4), s6, np.concatenate(tports),
                                     seed=200 + c, min_len=64, max_len=1500, snap=96) for c in range(4)]
    raw = np.concatenate([c[0] for c in chunks])
    lens = np.concatenate([np.diff(c[1].astype(np.int64)) for c in chunks])
    off = np.zeros(D + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    plen = np.concatenate([c[2] for c in chunks])
    lxc = np.concatenate([c[3] for c in chunks])
    blob = len(raw)
    d_raw = tile_dev(torch, raw, reps, dev)
    d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_off[:D + 1].copy_(torch.from_numpy(off.view(np.int64)))
    for r in range(1, reps):
        d_off[r * D + 1:(r + 1) * D + 1].copy_(d_off[1:D + 1] + r * blob)
    d_len = tile_dev(torch, plen, reps, dev).view(torch.int32)
    d_lxc = tile_dev(torch, lxc, reps, dev).view(torch.int16)
    d_out = torch.empty(n, dtype=torch.int32, device=dev)
    d_info = torch.empty((D, 16), dtype=torch.uint8, device=dev)
    kw = dict(d_lxc_ids=d_lxc, ipcache=ipc, d_pkt_len=d_len, stream=stream.cuda_stream)
    hkw = dict(lxc_ids=lxc, ipcache=ipc, pkt_len=plen)
    arr.frame_egress_verdicts_dev(d_raw, d_off, D, d_out, d_info=d_info, **kw)
    stream.synchronize()
    want, winfo, l4o = arr.frame_egress_eval_host_diag(raw, off, info=True, l4_off=True, **hkw)
    assert np.array_equal(d_out[:D].cpu().numpy(), want), "egress frame verdicts differ from the host evaluator"
    assert np.array_equal(d_info.cpu().numpy().view(FRAME_INFO_DTYPE).reshape(-1), winfo), "egress frame info differs"
    del d_info
    sec = timed(torch, stream, lambda: arr.frame_egress_verdicts_dev(d_raw, d_off, n, d_out, **kw), args.steps, 2)
    # the conntrack table: a third of the TCP / UDP frames that reach the policy get their reply key (the tuple as
    # loaded, TUPLE_F_IN), a third their established key (reversed, TUPLE_F_OUT); random keys fill up to 2^20
    proto = winfo["t"]["proto"]
    sel = np.flatnonzero((winfo["t"]["flags"] != 0) & ((proto == 6) | (proto == 17)))
    sel = sel[sel % 3 != 2]
    b = off[:-1].astype(np.int64)[sel]
    fam = winfo["family"][sel]
    keys = np.zeros(len(sel), CT_KEY_DTYPE)
    for f, so, do, size in ((4, 26, 30, 4), (6, 22, 38, 16)):
        m = fam == f
        keys["saddr"][m, :size] = raw[b[m][:, None] + np.arange(so, so + size)]
        keys["daddr"][m, :size] = raw[b[m][:, None] + np.arange(do, do + size)]
    p = b + l4o[sel]
    keys["dport"] = raw[p].astype(np.uint16) | raw[p + 1].astype(np.uint16) << 8
    keys["sport"] = raw[p + 2].astype(np.uint16) | raw[p + 3].astype(np.uint16) << 8
    keys["nexthdr"], keys["family"], keys["flags"] = proto[sel], fam, N.CG_TUPLE_F_IN
    keys["kind"] = np.where(proto[sel] == 6, N.CG_CT_MAP_TCP, N.CG_CT_MAP_ANY)
    est = sel % 3 == 1
    rev = keys[est].copy()
    rev["daddr"], rev["saddr"] = keys["saddr"][est], keys["daddr"][est]
    rev["dport"], rev["sport"], rev["flags"] = keys["sport"][est], keys["dport"][est], N.CG_TUPLE_F_OUT
    keys[est] = rev
    keys = np.unique(keys)
    target = 1 << 20
    if len(keys) < target:
        rng = np.random.default_rng(0xC8)
        fill = np.zeros(target - len(keys), CT_KEY_DTYPE)
        fill["daddr"][:, :4], fill["saddr"][:, :4] = rng.integers(0, 256, (len(fill), 4)), [172, 31, 0, 0]
        fill["sport"], fill["nexthdr"], fill["family"] = rng.integers(0, 65536, len(fill)), 6, 4
        fill["dport"] = np.arange(len(fill)) & 0xFFFF
        keys = np.unique(np.concatenate([keys, fill]))
    ct = cl.conntrack_map(max_entries=max(2 * len(keys), target), global_map=True)
    ct.update(keys)
    d_rec = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    arr.frame_egress_verdicts_dev(d_raw, d_off, D, d_out, conntrack=ct, d_records=d_rec, **kw)
    stream.synchronize()
    cwant, _, wrec = arr.frame_egress_eval_host_diag(raw, off, info=True, conntrack=ct, **hkw)
    assert np.array_equal(d_out[:D].cpu().numpy(), cwant), "egress conntrack verdicts differ from the host evaluator"
    assert d_rec[:D].cpu().numpy().tobytes() == wrec.tobytes(), "egress conntrack records differ"
    sec_rec = timed(torch, stream, lambda: arr.frame_egress_verdicts_dev(d_raw, d_off, n, d_out, conntrack=ct,
                                                                         d_records=d_rec, **kw), args.steps, 2)
    del d_rec
    sec_ct = timed(torch, stream, lambda: arr.frame_egress_verdicts_dev(d_raw, d_off, n, d_out, conntrack=ct, **kw),
                   args.steps, 2)
    done = wrec["state"] != 0
    del d_raw
    svc_res = _bench_l4_frames_services(torch, dev, stream, cl, args, arr, ct, kw, hkw, raw, off, winfo, l4o, d_off,
                                        d_out, D, n, reps, sec_rec)
    ct.destroy()
    arr.destroy()
    return svc_res, {"kernel": "l4_frames_kernel<EgressProg>", "frames": n, "distinct_frames": D, "blob_bytes_per_frame": blob / D,
            "policy_verdict_frac": float((winfo["t"]["flags"] != 0).mean()), "allowed_frac": float((want >= 0).mean()),
            "source_check_drop_frac": float(np.isin(want, (-130, -131, -132)).mean()),
            "no_conntrack": {"kernel_ms": sec * 1e3, "Gframes_s": n / sec / 1e9, "over_ingress_same_run": sec / sec_in},
            "with_conntrack": {"kernel_ms": sec_ct * 1e3, "Gframes_s": n / sec_ct / 1e9,
                               "over_ingress_ct_same_run": sec_ct / sec_in_ct, "table_keys": int(len(keys)),
                               "state_frac_of_looked_up": {name: float((wrec["state"][done] == s).mean()) for s, name in
                                                           ((1, "new"), (2, "established"), (3, "reply"),
                                                            (4, "related"))}},
            "with_conntrack_and_records": {"kernel_ms": sec_rec * 1e3, "Gframes_s": n / sec_rec / 1e9,
                                           "over_ingress_ct_records_same_run": sec_rec / sec_in_ct_rec}}


def bench_l4_frames(torch, dev, stream, cl, args, threads):
    """L4 verdicts from raw frames: 256 endpoints' maps (config 2's table mix)
    behind an endpoint map, a 64K-entry ipcache, Ethernet frames snapped to 96
    bytes (about 80% IPv4 TCP/UDP, 15% IPv6 with a twentieth of those carrying
    extension headers, 5% ICMP, other protocols, non-IP or truncated), tiled to
    2^24 on the device.  Checked against cg_diag_l4_frames_eval_host over the
    first copy before timing.  Beside the frames kernel, on the same packets:
    (a) cg_l4_array_verdicts_ipcache_dev over the tuples extracted beforehand
    (the frames whose walk completes, one call per family): strictly less
    work, a ceiling; (b) what a caller does without this path, from host
    data: header extraction on the host (numpy over the plain IPv4 and IPv6
    frames; the few with extension headers are left out of its timing),
    upload, those calls, download — against blob upload, one call, download."""
    from cilium_amd import _native as N
    from cilium_amd import synth
    from cilium_amd.classifier import FRAME_INFO_DTYPE, L4_TUPLE_DTYPE
    E, D, n = 256, args.frames, 1 << 24
    reps = max(1, n // D)
    n = D * reps
    rng = np.random.default_rng(0xF4A5)
    maps, tports = [], []
    for e in range(E):
        keys, ports = _l4_table_mix(np.random.default_rng(1000 + e))
        pm = cl.policy_map()
        pm.allow_keys(keys, ports)
        maps.append(pm)
        tports.append(keys["dport"][keys["dport"] != 0][:4096])
    slots = (np.arange(E) * 257).astype(np.uint16)
    arr = cl.policy_array()
    arr.set_many(slots, maps)
    ep4 = np.stack([np.full(E, 10), np.full(E, 200), np.arange(E) >> 4, np.arange(E) & 15], 1).astype(np.uint8)
    ep6 = np.zeros((E, 16), np.uint8)
    ep6[:, 0], ep6[:, 15] = 0xfd, np.arange(E)
    ep = cl.endpoint_map()
    ep.write_endpoints([".".join(map(str, a)) for a in ep4], slots)
    ep.write_endpoints(["fd00::%x" % e if e else "fd00::" for e in range(E)], slots)
    ik, iv = synth.ipcache_entries(65536, n_nodes=512)
    iv = iv.copy()
    iv[:, 0] = np.where(iv[:, 0] == 0, 0, 256 + rng.integers(0, 16384, len(iv)))
    ipc = cl.ipcache()
    ipc.update(ik, iv)
    s4, s6 = synth.ipcache_addresses(8192, ik, seed=9)
    chunks = [synth.l4_frames(D // 4, ep4, ep6, s4.view(np.uint8).reshape(-1, 4), s6, np.concatenate(tports),
                              seed=100 + c, min_len=64, max_len=1500, snap=96) for c in range(4)]
    raw = np.concatenate([c[0] for c in chunks])
    lens = np.concatenate([np.diff(c[1].astype(np.int64)) for c in chunks])
    off = np.zeros(D + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    plen = np.concatenate([c[2] for c in chunks])
    blob = len(raw)
    d_raw = tile_dev(torch, raw, reps, dev)
    d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_off[:D + 1].copy_(torch.from_numpy(off.view(np.int64)))
    for r in range(1, reps):
        d_off[r * D + 1:(r + 1) * D + 1].copy_(d_off[1:D + 1] + r * blob)
    d_len = tile_dev(torch, plen, reps, dev).view(torch.int32)
    d_out = torch.empty(n, dtype=torch.int32, device=dev)
    d_info = torch.empty((D, 16), dtype=torch.uint8, device=dev)
    kw = dict(endpoints=ep, ipcache=ipc)
    arr.frame_verdicts_dev(d_raw, d_off, D, d_out, d_pkt_len=d_len, d_info=d_info, stream=stream.cuda_stream, **kw)
    stream.synchronize()
    t0 = time.perf_counter()
    want, winfo = arr.frame_eval_host_diag(raw, off, pkt_len=plen, info=True, **kw)
    cpu = D / (time.perf_counter() - t0)
    assert np.array_equal(d_out[:D].cpu().numpy(), want), "frame verdicts differ from the host evaluator"
    assert np.array_equal(d_info.cpu().numpy().view(FRAME_INFO_DTYPE).reshape(-1), winfo), "frame info differs"
    del d_info
    sec = timed(torch, stream, lambda: arr.frame_verdicts_dev(d_raw, d_off, n, d_out, d_pkt_len=d_len,
                                                              stream=stream.cuda_stream, **kw), args.steps, 2)
    ct_res = _bench_l4_frames_ct(torch, dev, stream, cl, args, arr, kw, raw, off, plen, d_raw, d_off, d_len, d_out, D,
                                 n, sec)
    # (a) the tuple route over pre-extracted tuples, kernels only
    ran = winfo["t"]["flags"] != 0
    fam4 = ran & (winfo["family"] == 4)
    fam6 = ran & (winfo["family"] == 6)
    start = off[:-1].astype(np.int64)
    sa4 = raw[start[fam4][:, None] + np.arange(26, 30)].copy().view(np.uint32).reshape(-1)
    sa6 = raw[start[fam6][:, None] + np.arange(22, 38)].copy()
    calls = []
    for fam, sel, addrs in ((4, fam4, sa4), (6, fam6, sa6)):
        m = int(sel.sum())
        d_a = tile_dev(torch, addrs, reps, dev)
        d_t = tile_dev(torch, np.ascontiguousarray(winfo["t"][sel]), reps, dev)
        d_l = tile_dev(torch, np.ascontiguousarray(winfo["lxc_id"][sel]), reps, dev).view(torch.int16)
        d_o = torch.empty(m * reps, dtype=torch.int32, device=dev)
        arr.verdicts_via_ipcache_dev(ipc, fam, d_a, d_l, d_t, m, d_o, stream=stream.cuda_stream, mode=N.CG_L4_INGRESS)
        stream.synchronize()
        assert np.array_equal(d_o[:m].cpu().numpy(), want[sel]), "the tuple route differs on the extracted tuples"
        calls.append((fam, d_a, d_l, d_t, m * reps, d_o))

    def tuple_route():
        for fam, d_a, d_l, d_t, m, d_o in calls:
            arr.verdicts_via_ipcache_dev(ipc, fam, d_a, d_l, d_t, m, d_o, stream=stream.cuda_stream,
                                         mode=N.CG_L4_INGRESS)
    sec_a = timed(torch, stream, tuple_route, args.steps, 2)
    n_a = sum(c[4] for c in calls)
    del calls
    # (b) from host data, D frames: host extraction + upload + the tuple calls + download, against the frames call
    lut = {bytes(a): s for a, s in zip(ep4, slots)}
    lut.update({bytes(a): s for a, s in zip(ep6, slots)})

    def extract():
        et = raw[np.minimum(start + 12, blob - 1)].astype(np.uint16) << 8 | raw[np.minimum(start + 13, blob - 1)]
        out = []
        for fam, code, amin in ((4, 0x0800, 34), (6, 0x86DD, 54)):
            idx = np.flatnonzero((et == code) & (lens >= amin + 14))
            b = start[idx]
            if fam == 4:
                l4 = 14 + (raw[b + 14] & 0xF).astype(np.int64) * 4
                proto, frag = raw[b + 23], ((raw[b + 20] & 0xBF) | raw[b + 21]) != 0
                sa = raw[b[:, None] + np.arange(26, 30)].copy().view(np.uint32).reshape(-1)
                da = raw[b[:, None] + np.arange(30, 34)]
            else:
                l4 = np.full(len(idx), 54, np.int64)
                proto, frag = raw[b + 20], np.zeros(len(idx), bool)
                sa = raw[b[:, None] + np.arange(22, 38)].copy()
                da = raw[b[:, None] + np.arange(38, 54)]
            ok = np.isin(proto, (6, 17)) & (l4 + 14 <= lens[idx])
            idx, b, l4, sa, da = idx[ok], b[ok], l4[ok], sa[ok], da[ok]
            t = np.zeros(len(idx), L4_TUPLE_DTYPE)
            t["dport"] = raw[b + l4 + 2].astype(np.uint16) | raw[b + l4 + 3].astype(np.uint16) << 8
            t["proto"], t["flags"], t["len"] = proto[ok], 1 | frag[ok].astype(np.uint8) << 1, plen[idx]
            key = da.view(f"V{da.shape[1]}").reshape(-1)
            uniq, inv = np.unique(key, return_inverse=True)
            lx = np.array([lut.get(u.tobytes(), 1) for u in uniq], np.uint16)[inv]  # slot 1 is empty
            out.append((fam, idx, sa, lx, t))
        return out

    t0 = time.perf_counter()
    parts = extract()
    t_extract = time.perf_counter() - t0
    back = np.full(D, 0, np.int32)
    for fam, idx, sa, lx, t in parts:
        dd = [torch.from_numpy(x.view(np.uint8).reshape(-1)).to(dev) for x in (sa, lx, t)]
        dd_o = torch.empty(len(idx), dtype=torch.int32, device=dev)
        arr.verdicts_via_ipcache_dev(ipc, fam, dd[0], dd[1], dd[2], len(idx), dd_o, stream=stream.cuda_stream,
                                     mode=N.CG_L4_INGRESS)
        stream.synchronize()
        back[idx] = dd_o.cpu().numpy()
    wall_b = time.perf_counter() - t0
    plain = np.concatenate([p[1] for p in parts])
    local = want[plain] != N.CG_FRAME_NOT_LOCAL
    assert np.array_equal(back[plain][local], want[plain][local]), "host extraction differs from the frames path"
    t0 = time.perf_counter()
    dd = [torch.from_numpy(x).to(dev) for x in (raw, off.view(np.int64), plen.view(np.int32))]
    dd_o = torch.empty(D, dtype=torch.int32, device=dev)
    arr.frame_verdicts_dev(dd[0], dd[1], D, dd_o, d_pkt_len=dd[2], stream=stream.cuda_stream, **kw)
    stream.synchronize()
    dd_o.cpu().numpy()
    wall_f = time.perf_counter() - t0
    del dd, dd_o, d_raw, d_off, d_len, d_out
    svc_res, eg_res = _bench_l4_frames_egress(torch, dev, stream, cl, args, maps, slots, ipc, s4, s6, tports, D, n, reps, sec,
                                              ct_res["kernel_ms"] * 1e-3,
                                              ct_res["with_records"]["kernel_ms"] * 1e-3)
    per_frame = blob / D + 8 + 4
    return line("L4 verdicts/s from raw frames across 256 endpoints (l4_frames_kernel: header walk, endpoint map, "
                "ipcache, policy program array)", n, sec, per_frame + 4, "l4_frames_kernel<IngressProg<ep, ipc>>", cpu,
                "cg_diag_l4_frames_eval_host over the first copy, one thread", 1,
                {"config": {"workload": "256 policy maps of config 2's mix, frames snapped to 96 B", "maps": E,
                            "distinct_frames": D, "frames": n, "blob_bytes_per_frame": blob / D,
                            "policy_verdict_frac": float(ran.mean()), "allowed_frac": float((want >= 0).mean())},
                 "kernel_ms": sec * 1e3, "Gframes_s": n / sec / 1e9,
                 "algorithmic_bytes_per_frame_in": per_frame,
                 "with_conntrack": ct_res,
                 "egress": eg_res,
                 "services": svc_res,
                 "tuple_route_ceiling": {"kernel_ms": sec_a * 1e3, "tuples": n_a, "Gtuples_s": n_a / sec_a / 1e9},
                 "from_host_data": {"frames": D, "host_extract_s": t_extract, "tuple_route_wall_s": wall_b,
                                    "frames_wall_s": wall_f, "frames_left_unparsed": int(D - len(plain))}})


def bench_lpm(torch, dev, stream, cl, args, threads):
    import oracle
    from cilium_amd import synth
    pfx = synth.lpm_prefixes()
    pf = cl.prefilter(dyn4=True, dyn6=True, max_lpm=1 << 21)
    pf.insert(0, pfx)
    D, reps = 100_000_000, 10
    v4, v6, ep4, ep6 = synth.lpm_addresses(D, pfx)
    pf.set_endpoints(ep4, ep6)
    g4, g6 = pf.verdicts(v4[:1_000_000], v6[:400_000])
    o4, o6 = oracle.prefilter(pf.config, pfx, ep4, ep6, v4[:1_000_000], v6[:400_000], nthreads=threads)
    assert np.array_equal(g4, o4) and np.array_equal(g6, o6), "prefilter verdicts differ from the oracle"
    d4 = tile_dev(torch, v4, reps, dev)
    d6 = tile_dev(torch, v6, reps, dev)
    n4, n6 = len(v4) * reps, len(v6) * reps
    o4d = torch.empty(n4, dtype=torch.uint8, device=dev)
    o6d = torch.empty(n6, dtype=torch.uint8, device=dev)
    sec = timed(torch, stream, lambda: pf.verdicts_dev(d4, n4, o4d, d6, n6, o6d, stream=stream.cuda_stream),
                args.steps, 2)
    bpi = (n4 * 9 + n6 * 33) / (n4 + n6)
    s4, s6 = v4[:700_000], v6[:300_000]
    cpu = cpu_rate(lambda: oracle.prefilter(pf.config, pfx, ep4, ep6, s4, s6, nthreads=threads), 1_000_000,
                   args.cpu_seconds)
    return line("XDP prefilter verdicts/s (check_v4/check_v6), config 3", n4 + n6, sec, bpi, "lpm_kernel", cpu,
                f"1M addresses (70% v4) of the same workload, {threads} threads", threads,
                {"config": {"workload": "BASELINE config 3: 1M mixed v4/v6 prefixes, 1B addresses",
                            "prefixes": int(len(pfx)), "addresses": n4 + n6}})


def bench_kafka(torch, dev, stream, cl, args, threads):
    import oracle
    from cilium_amd import synth
    pols, info = synth.kafka_policy()
    cl.update_kafka_policy(pols)
    D, reps = 1_000_000, 100
    rq = synth.kafka_requests(D, info)
    reqs, arena = cl.pack_kafka(**rq)
    got = cl.kafka_verdicts(reqs[:200_000], arena)
    sub = {k: v[:200_000] for k, v in rq.items()}
    orc = oracle.KafkaOracle(pols)
    assert np.array_equal(got, orc.eval(**sub, nthreads=threads)), "Kafka verdicts differ from the oracle"
    d_r = tile_dev(torch, reqs, reps, dev)
    d_a = torch.from_numpy(arena).to(dev)
    n = D * reps
    d_o = torch.empty(n, dtype=torch.uint8, device=dev)
    sec = timed(torch, stream, lambda: cl.kafka_verdicts_dev(d_r, n, d_a, d_o, stream=stream.cuda_stream),
                args.steps, 2)
    # the split layout (cg_kafka_verdicts_split_dev): 16-byte heads, 48-byte
    # topic tails read only by the requests that need them
    raw = reqs.view(np.uint8).reshape(D, 64)
    d_h = tile_dev(torch, np.ascontiguousarray(raw[:, :16]), reps, dev)
    d_t = tile_dev(torch, np.ascontiguousarray(raw[:, 16:]), reps, dev)
    del d_r
    sec_split = timed(torch, stream, lambda: cl.kafka_verdicts_split_dev(d_h, d_t, n, d_a, d_o,
                                                                         stream=stream.cuda_stream), args.steps, 2)
    got_split = d_o[:200_000].cpu().numpy()
    assert np.array_equal(got_split, got), "split-layout Kafka verdicts differ"
    cpu = cpu_rate(lambda: orc.eval(**sub, nthreads=threads), 200_000, args.cpu_seconds)
    return line("Kafka verdicts/s (kafkaRedirect.canAccess → MatchesRule), config 4", n, sec_split, 17,
                "kafka_kernel (split heads/topics)", cpu, f"200K requests of the same workload, {threads} threads",
                threads, {"config": {"workload": "BASELINE config 4: 1K Kafka rules, 100M requests", "requests": n,
                                     "layout": "16-B heads + 48-B topic tails (algorithmic bytes: head + verdict)"},
                          "records_64b": {"value": n / sec, "ms": sec * 1e3, "bytes_per_item": 65}})


def kafka_wire_pool(D: int, info: dict, seed: int = 0x4B, codec_frac: float = 0.0):
    """D distinct wire requests of config 4's mix (apiKey / version / topics /
    clientID as synth.kafka_requests draws them); codec_frac of the produce
    requests carry their message sets compressed (gzip or snappy, one
    member / block each: what the device inflates by itself)."""
    from cilium_amd import kafka_requests as K
    from cilium_amd import synth
    rq = synth.kafka_requests(D, info, seed=seed)
    rng = np.random.default_rng(seed)
    reqs, codecs = [], []
    for i in range(D):
        codec = K.CODEC_NONE
        if int(rq["api_key"][i]) == K.PRODUCE and rng.random() < codec_frac:
            codec = K.CODEC_GZIP if rng.random() < 0.5 else K.CODEC_SNAPPY
        codecs.append(codec)
        reqs.append(K.encode(int(rq["api_key"][i]), int(rq["api_version"][i]), rq["client_id"][i], rq["topics"][i],
                             rng, codec=codec))
    return reqs, dict(rq, codec=codecs)


def bench_kafka_wire(torch, dev, stream, cl, args, threads, codec_frac: float = 0.0):
    """Config 4's request mix as wire bytes: kafka_decode_kernel (ReadRequest
    + the optiopay decoders, CRC-32 of every produce message), with
    codec_frac > 0 kafka_inflate_kernel for the compressed sets (gzip /
    snappy decoded on the device, their inner sets parsed), then
    kafka_kernel, per request."""
    import ctypes as C
    from oracle import kafka_wire_ref as R
    from cilium_amd import _native as N
    from cilium_amd import kafka_requests as K
    from cilium_amd import synth
    pols, info = synth.kafka_policy()
    cl.update_kafka_policy(pols)
    D, reps = 65_536, 256
    pool, rq = kafka_wire_pool(D, info, codec_frac=codec_frac)
    if os.environ.get("CILIUM_BENCH_KAFKA_SORTED"):
        # the same requests grouped by (apiKey, version): what a wave decodes
        # when its lanes take one code path (the divergence A/B)
        order = np.lexsort((np.asarray(rq["api_version"]), np.asarray(rq["api_key"])))
        pool = [pool[i] for i in order]
        rq = {k: (v[order] if isinstance(v, np.ndarray) else [v[i] for i in order]) for k, v in rq.items()}
    if codec_frac:
        # copies per call within the 64 MiB per-call inflate arena (each
        # compressed set reserves its decoded size, at most its request's
        # bytes here: a few short messages), so nothing waits for the host
        # for want of room
        zbytes = sum(len(r) for r, z in zip(pool, rq["codec"]) if z)
        reps = max(1, min(256, int((48 << 20) / max(1, zbytes))))
    raw, off = K.concat(pool)
    red = np.zeros(D, np.uint16)
    rem = np.asarray(rq["remote"], np.uint32)
    v = cl.kafka_verdicts_raw(raw[: int(off[4096])], off[:4097], red[:4096], rem[:4096])
    want = cl.kafka_verdicts(*cl.pack_kafka(**{k: x[:4096] for k, x in rq.items() if k != "codec"}))
    assert np.array_equal(v, want), "raw-bytes Kafka verdicts differ from the field-packed path"
    tot = int(off[-1])
    d_raw = tile_dev(torch, raw, reps, dev)
    offs = torch.from_numpy(off[:-1].view(np.int64).copy()).to(dev)
    d_off = (offs.unsqueeze(0) + torch.arange(reps, device=dev, dtype=torch.int64).unsqueeze(1) * tot).reshape(-1)
    d_off = torch.cat([d_off, torch.tensor([tot * reps], dtype=torch.int64, device=dev)])
    n = D * reps
    d_red = torch.zeros(n, dtype=torch.int16, device=dev)
    d_rem = torch.from_numpy(rem.view(np.int32)).to(dev).repeat(reps)
    d_reqs = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    cap = tot * reps // 2 + 16
    d_a = torch.empty(cap, dtype=torch.int32, device=dev)
    d_o = torch.empty(n, dtype=torch.uint8, device=dev)
    ss = stream.cuda_stream

    def decode():
        cl.kafka_decode_dev(d_raw, d_off, n, d_red, d_rem, d_reqs, d_a, cap, d_st, stream=ss)

    def both():
        decode()
        cl.kafka_verdicts_dev(d_reqs, n, d_a, d_o, stream=ss)
    i0, d0 = C.c_uint64(), C.c_uint64()
    N.check(N.lib.cg_kafka_decode_stats(cl.h, C.byref(i0), C.byref(d0)))
    sec = timed(torch, stream, decode, args.steps, 2)
    i1, d1 = C.c_uint64(), C.c_uint64()
    N.check(N.lib.cg_kafka_decode_stats(cl.h, C.byref(i1), C.byref(d1)))
    calls = args.steps + 2
    inflated, deferred = (i1.value - i0.value) / calls, (d1.value - d0.value) / calls
    sec2 = timed(torch, stream, both, args.steps, 1)
    # copies carry their original's verdict
    orig = d_o[:D].clone()
    assert bool((d_o.view(reps, D) == orig.unsqueeze(0)).all()), "copies' verdicts differ"
    assert np.array_equal(orig.cpu().numpy(), cl.kafka_verdicts_raw(raw, off, red, rem))
    bpi = tot / D + 8 + 2 + 4 + 64 + 1
    sample = pool[:20_000]
    cpu = cpu_rate(lambda: [R.decode(r) for r in sample], len(sample), args.cpu_seconds)
    kern = "kafka_decode_kernel + kafka_inflate_kernel" if codec_frac else "kafka_decode_kernel"
    mix = (f"{int(codec_frac * 100)}% of produce requests with gzip / snappy sets" if codec_frac
           else "uncompressed wire bytes")
    out = line(f"Kafka wire decode requests/s (ReadRequest on raw bytes), config 4 mix, {mix}", n, sec, bpi,
               kern, cpu, "20K requests of the same mix through oracle/kafka_wire_ref.decode, "
               "1 thread (pure Python)", 1,
               {"config": {"workload": f"BASELINE config 4 request mix as wire bytes, {mix} "
                           f"({tot / D:.1f} B/request avg), 1K rules", "requests": n},
                "per_call": {"payloads_inflated_on_device": inflated, "requests_finished_by_host": deferred},
                "decode_plus_verdict": {"value": n / sec2, "ms_per_launch": sec2 * 1e3}})
    return out


def bench_http_host(torch, dev, stream, cl, args, threads):
    """Config 5 through the host entry points: cg_http_pack (CPU, the
    packer: field extraction, program lookup, class coding, tile layout) and
    cg_http_verdicts_host (pinned staging → H2D → http_kernel → D2H →
    request order).  The kernel-only rate is bench.py's line."""
    import oracle
    from cilium_amd import _native as N
    from cilium_amd import synth
    pols, info = synth.http10k_rules()
    cl.update_http_policy(pols)
    n = 4_000_000
    rq = synth.http10k_requests(n, info, distinct=200_000)
    t_pack = []
    for _ in range(3):
        t0 = time.perf_counter()
        b = cl.pack_http(**rq)
        t_pack.append(time.perf_counter() - t0)
    got = cl.http_verdicts(b)  # warm
    t_e2e = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = cl.http_verdicts(b)
        t_e2e.append(time.perf_counter() - t0)
    sub = {k: v[:50_000] for k, v in rq.items() if k not in ("hdr_blob", "hdr_off")}
    sub["hdr_off"] = rq["hdr_off"][:50_001]
    sub["hdr_blob"] = rq["hdr_blob"]
    assert np.array_equal(got[:50_000], oracle.HttpOracle(pols).eval(**sub, nthreads=threads)), \
        "host-path verdicts differ from the oracle"
    tp, te = min(t_pack), min(t_e2e)
    batch_bytes = b.used_bytes() + int(b.arena.nbytes)
    hdr_bytes = int(rq["hdr_off"][-1])
    return {"metric": "HTTP host path, config 5: cg_http_pack + cg_http_verdicts_host", "value": n / (tp + te),
            "unit": "verdicts/s", "n_gpus": 1, "higher_is_better": True, "data": "synthetic",
            "pack": {"value": n / tp, "unit": "requests/s",
                     "cores": int(N.lib.cg_http_pack_threads()),
                     "header_MBps": hdr_bytes / tp / 1e6,
                     "ms": tp * 1e3},
            "verdicts_host": {"value": n / te, "unit": "verdicts/s", "ms": te * 1e3,
                              "batch_bytes": batch_bytes, "staged_GBps": batch_bytes / te / 1e9,
                              "pcie_peak_GBps": 63.0,
                              "note": "pinned staging memcpy + H2D + kernel + D2H + request-order scatter"},
            "config": {"workload": "BASELINE config 5 (10K-rule HTTP) requests through the host entry points",
                       "requests": n, "header_bytes": hdr_bytes}}


def bench_http_raw(torch, dev, stream, cl, args, threads):
    """Config 5 requests as raw HTTP/1 heads resident in HBM →
    cg_http_verdicts_raw_dev: the codec step, program lookup, packing and the
    verdicts all on the GPU (kernels_http_raw.hip + http_kernel), one call
    per step (the device-layout sequence, the default, only enqueues; with
    CILIUM_GPU_RAW_LAYOUT=host in the environment the round-3 sequence runs
    instead, which synchronizes its stream for a host layout step)."""
    import oracle  # noqa: F401  (the check below uses the host path)
    from cilium_amd import synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_http_parse import _blob, _raw_requests
    pols, info = synth.http10k_rules()
    cl.update_http_policy(pols)
    D, reps = 65_536, 1_900
    rq = synth.http10k_requests(D, info, seed=synth.SEED ^ 0x4A1)
    raws = _raw_requests(rq)
    blob, off = _blob(raws)
    args_ = (rq["policy"], rq["ingress"], rq["port"], rq["remote"])
    want = cl.http_verdicts(cl.pack_http_raw(*args_, blob, off))
    tot = int(off[-1])
    d_raw = tile_dev(torch, blob[:tot], reps, dev)
    base = torch.arange(reps, dtype=torch.int64, device=dev).unsqueeze(1) * tot
    d_off = torch.cat([(torch.from_numpy(off[:-1].astype(np.int64)).to(dev).unsqueeze(0) + base).reshape(-1),
                       torch.tensor([tot * reps], dtype=torch.int64, device=dev)])
    rep = lambda a, dt: tile_dev(torch, np.asarray(a).astype(dt), reps, dev)
    d_pol, d_ing, d_port, d_rem = rep(args_[0], np.uint32), rep(args_[1], np.uint8), rep(args_[2], np.uint16), \
        rep(args_[3], np.uint32)
    n = D * reps
    d_out = torch.zeros(n, dtype=torch.uint8, device=dev)
    run = lambda: cl.http_verdicts_raw_dev(d_raw, d_off, n, d_pol, d_ing, d_port, d_rem, d_out,
                                           stream=stream.cuda_stream)
    sec = timed(torch, stream, run, args.steps, 1)
    got = d_out.view(reps, D)
    if not os.environ.get("CG_EXP_NOCHECK"):  # set only for measuring-device variants (tools/exp_paths.sh)
        assert bool((got == torch.from_numpy(want).to(dev).unsqueeze(0)).all()), "raw-path verdicts differ from host path"
    bpi = tot / D + 4 + 1 + 2 + 4 + 8 + 1  # head bytes, policy/ingress/port/remote, offset, verdict
    return line("HTTP/1 raw heads → verdicts/s on the GPU (codec step + packing + http_kernel), config 5", n, sec,
                bpi, ("raw_scan+raw_rank+raw_build+http_kernel" if os.environ.get("CILIUM_GPU_RAW_LAYOUT") == "host"
                      else "raw_scan_dl+raw_pad+raw_seal+http_kernel<raw>+raw_walk"), None, "", threads,
                {"config": {"workload": f"BASELINE config 5 requests as raw HTTP/1 heads ({tot / D:.1f} B/head avg), "
                            "10K rules", "requests": n},
                 "request_gbps": n * (tot / D) / sec / 1e9})


def bench_http_fields(torch, dev, stream, cl, args, threads):
    """Config 5 requests as parsed header lists (cg_http_pack's input, the
    header map Envoy's filter sees) → verdicts with the grouping, sorting and
    packing on the GPU (kernels_http_raw.hip list mode + http_kernel):
    * device entry: 124.5M lists resident in HBM, cg_http_verdicts_fields_dev,
      HIP-event timed;
    * host entry: 8M lists in host memory, cg_http_verdicts_fields_host
      (pinned staging on 2 workers, H2D, kernels, D2H), wall clock, against
      the host packer path (cg_http_pack + cg_http_verdicts_host) on the same
      lists."""
    import oracle
    from cilium_amd import synth
    pols, info = synth.http10k_rules()
    cl.update_http_policy(pols)
    D, reps = 1 << 20, 119
    rq = synth.http10k_requests_fast(D, info, seed=synth.SEED ^ 0xF1E1D)
    blob, off = rq["hdr_blob"], rq["hdr_off"]
    args_ = (rq["policy"], rq["ingress"], rq["port"], rq["remote"])
    want = cl.http_verdicts(cl.pack_http(*args_, blob, off))
    k = 20_000
    exp = oracle.HttpOracle(pols).eval(*(np.asarray(a)[:k] for a in args_), blob, off[:k + 1], nthreads=threads)
    assert np.array_equal(want[:k], exp), "host-path verdicts differ from the oracle"
    tot = int(off[-1])
    d_blob = tile_dev(torch, np.asarray(blob[:tot]), reps, dev)
    base = torch.arange(reps, dtype=torch.int64, device=dev).unsqueeze(1) * tot
    d_off = torch.cat([(torch.from_numpy(off[:-1].astype(np.int64)).to(dev).unsqueeze(0) + base).reshape(-1),
                       torch.tensor([tot * reps], dtype=torch.int64, device=dev)])
    rep = lambda a, dt: tile_dev(torch, np.asarray(a).astype(dt), reps, dev)
    d_pol, d_ing, d_port, d_rem = rep(args_[0], np.uint32), rep(args_[1], np.uint8), rep(args_[2], np.uint16), \
        rep(args_[3], np.uint32)
    n = D * reps
    d_out = torch.zeros(n, dtype=torch.uint8, device=dev)
    run = lambda: cl.http_verdicts_fields_dev(d_blob, d_off, n, d_pol, d_ing, d_port, d_rem, d_out,
                                              stream=stream.cuda_stream)
    sec = timed(torch, stream, run, args.steps, 1)
    assert bool((d_out.view(reps, D) == torch.from_numpy(want).to(dev).unsqueeze(0)).all()), \
        "device list-path verdicts differ from the host path"
    del d_blob, d_off, d_pol, d_ing, d_port, d_rem, d_out
    torch.cuda.empty_cache()
    # host entry on 8M lists (8 distinct 1M pools)
    H = 8 * D
    hq = synth.http10k_requests_fast(H, info, seed=synth.SEED ^ 0x8E1D)
    hargs = (hq["policy"], hq["ingress"], hq["port"], hq["remote"], hq["hdr_blob"], hq["hdr_off"])
    got = cl.http_verdicts_fields(*hargs)  # warm (pinned buffers, workers)
    t_host = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = cl.http_verdicts_fields(*hargs)
        t_host.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    ref = cl.http_verdicts(cl.pack_http(*hargs))
    t_pack_path = time.perf_counter() - t0
    assert np.array_equal(got, ref), "host-entry list-path verdicts differ from the host packer path"
    th = min(t_host)
    hbytes = int(hq["hdr_off"][-1])
    bpi = tot / D + 4 + 1 + 2 + 4 + 8 + 1  # list bytes, policy/ingress/port/remote, offset, verdict
    return line("HTTP header lists → verdicts/s, packing on the GPU (cg_http_verdicts_fields_dev), config 5", n, sec,
                bpi, ("raw_scan(lists)+raw_rank+raw_build+http_kernel" if os.environ.get("CILIUM_GPU_RAW_LAYOUT") == "host"
                      else "raw_scan_dl(lists)+raw_pad+raw_seal+http_kernel<raw>+raw_walk"), None, "", threads,
                {"config": {"workload": f"BASELINE config 5 requests as header lists ({tot / D:.1f} B/list avg), "
                            "10K rules, 1M distinct tiled", "requests": n},
                 "host_entry": {"value": H / th, "unit": "verdicts/s", "ms": th * 1e3, "requests": H,
                                "list_bytes": hbytes, "staged_GBps": (hbytes + 19 * H) / th / 1e9,
                                "note": "cg_http_verdicts_fields_host: lists in host memory, pinned staging on 2 "
                                        "workers, H2D, kernels, D2H (PCIe-inclusive)"},
                 "host_packer_path": {"value": H / t_pack_path, "unit": "verdicts/s", "ms": t_pack_path * 1e3,
                                      "note": "cg_http_pack (CPU) + cg_http_verdicts_host on the same lists"}})


def bench_ipcache(torch, dev, stream, cl, args, threads):
    import oracle
    from cilium_amd import synth
    k, v = synth.ipcache_entries()
    ic = cl.ipcache()
    ic.update(k, v)
    D, reps = 100_000_000, 10
    a4, a6 = synth.ipcache_addresses(D, k)
    g4, g6 = ic.resolve(a4[:1_000_000], a6[:400_000])
    o4, o6 = oracle.ipcache(k, v, a4[:1_000_000], a6[:400_000], nthreads=threads)
    assert np.array_equal(g4, o4) and np.array_equal(g6, o6), "ipcache results differ from the oracle"
    d4 = tile_dev(torch, a4, reps, dev)
    d6 = tile_dev(torch, a6, reps, dev)
    n4, n6 = len(a4) * reps, len(a6) * reps
    o4d = torch.empty(n4 * 2, dtype=torch.int32, device=dev)
    o6d = torch.empty(n6 * 2, dtype=torch.int32, device=dev)
    sec = timed(torch, stream, lambda: ic.resolve_dev(d4, n4, o4d, d6, n6, o6d, stream=stream.cuda_stream),
                args.steps, 2)
    bpi = (n4 * 12 + n6 * 24) / (n4 + n6)  # address in + {identity, tunnel} out
    s4, s6 = a4[:5_600_000], a6[:2_400_000]
    cpu = cpu_rate(lambda: oracle.ipcache(k, v, s4, s6, nthreads=threads), 8_000_000, args.cpu_seconds)
    return line("ipcache lookups/s (lookup_ip{4,6}_remote_endpoint → identity, tunnel)", n4 + n6, sec, bpi,
                "ipcache_kernel", cpu,
                f"8M addresses (70% v4) of the same workload per call (incl. the oracle's map build), {threads} threads",
                threads, {"config": {"workload": "SURVEY 8(f) row 1: 512K-entry ipcache (MaxEntries), 1B addresses",
                                     "entries": int(len(k)), "addresses": n4 + n6}})


def r2d2_workload(n: int, seed: int = 0xC111A):
    """64 ports x 8 r2d2 rules (cmd and/or an unanchored file regex; a third
    of the rules restricted to 4 of 64 remote identities); requests half
    crafted to hit a random rule, half random."""
    rng = np.random.default_rng(seed)
    ports, rules_of = [], {}
    for pi in range(64):
        port = 7000 + pi
        rules = []
        for ri in range(8):
            k = pi * 8 + ri
            kind = ri % 4
            rule = {}
            if kind != 3:
                rule["cmd"] = ["READ", "WRITE", "READ"][kind]
            if kind == 0:
                rule["file"] = f"^/svc{k}/[a-z]+"
            elif kind == 1:
                rule["file"] = f"data{k}\\.(csv|json)$"
            elif kind == 3:
                rule["file"] = f"tmp{k}"
            r = {"l7_proto": "r2d2", "l7_rules": {"l7_rules": [{"rule": rule}]}}
            if ri % 3 == 0:
                r["remote_policies"] = [int(x) for x in rng.choice(64, 4, replace=False) + 256]
            rules.append(r)
            rules_of[(port, ri)] = (rule, r.get("remote_policies"))
        ports.append({"port": port, "rules": rules})
    pols = [{"name": "r2d2-bench", "ingress_per_port_policies": ports}]
    reqs = []
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)
    for i in range(n):
        pi, ri = int(rng.integers(0, 64)), int(rng.integers(0, 8))
        port = 7000 + pi
        rule, rem = rules_of[(port, ri)]
        word = letters[rng.integers(0, 26, int(rng.integers(3, 12)))].tobytes()
        k = pi * 8 + ri
        if rng.random() < 0.5:
            cmd = rule.get("cmd", "READ").encode()
            f = {0: b"/svc%d/" % k + word, 1: b"x/data%d.json" % k, 2: word, 3: b"a/tmp%d/" % k + word}[ri % 4]
            remote = rem[0] if rem else 256 + int(rng.integers(0, 64))
        else:
            cmd = [b"READ", b"WRITE", b"HALT", b"RESET"][int(rng.integers(0, 4))]
            f = b"/svc%d/" % int(rng.integers(0, 512)) + word
            remote = 256 + int(rng.integers(0, 64))
        reqs.append((port, remote, cmd, f))
    return pols, reqs


def bench_l4ipc(torch, dev, stream, cl, args, threads):
    """Config 2's policy map with each tuple's identity resolved from its
    remote IPv4 address through the 475K-entry ipcache in the same kernel."""
    import oracle
    from cilium_amd import synth
    keys, ports = synth.l4_table()
    pm = cl.policy_map()
    pm.allow_keys(keys, ports)
    ik, iv = synth.ipcache_entries()
    rng = np.random.default_rng(5)
    iv = iv.copy()
    iv[:, 0] = rng.choice(np.append(np.unique(keys["sec_label"]), [0, 999_999]), len(iv))
    ic = cl.ipcache()
    ic.update(ik, iv)
    D, reps = 10_000_000, 10
    a4, _ = synth.ipcache_addresses(int(D / 0.7) + 1, ik)
    a4 = a4[:D]
    tup = synth.l4_tuples(D, keys)
    got = pm.verdicts_via_ipcache(ic, a4[:1_000_000], tup[:1_000_000])
    exp, _, _ = oracle.l4_egress_via_ipcache(keys, ports, ik, iv, a4[:1_000_000], tup[:1_000_000])
    assert np.array_equal(got, exp), "ipcache+L4 verdicts differ from the oracle (policy_can_egress4)"
    d_t = tile_dev(torch, tup, reps, dev)
    d_a = tile_dev(torch, a4, reps, dev)
    n = D * reps
    d_o = torch.empty(n, dtype=torch.int32, device=dev)
    from cilium_amd import _native as N

    def run():
        N.check(N.lib.cg_l4_verdicts_ipcache_dev(cl.h, pm.id, ic.id, d_a.data_ptr(), d_t.data_ptr(), n,
                                                 d_o.data_ptr(), stream.cuda_stream))
    sec = timed(torch, stream, run, args.steps, 2)
    sa, st = a4[:1_000_000], tup[:1_000_000]

    def cpu_leg():
        r4, _ = oracle.ipcache(ik, iv, sa, np.zeros((0, 16), np.uint8), nthreads=threads)
        tt = st.copy()
        tt["identity"] = r4[:, 0]
        oracle.l4(keys, ports, tt, oracle.L4_EGRESS)
    cpu = cpu_rate(cpu_leg, len(st), args.cpu_seconds)
    return line("L4 verdicts/s with ipcache identities (bpf_lxc.c:509-527), config 2 map + 475K-entry ipcache", n,
                sec, 20, "l4_fp_kernel<ipcache>", cpu,
                f"1M tuples of the same workload: oracle ipcache ({threads} threads, incl. its map build) then "
                "oracle.l4 (1 thread)", threads,
                {"config": {"workload": "BASELINE config 2 map, 100M tuples, identities from a 512K-draw ipcache",
                            "tuples": n}})


def bench_proxylib(torch, dev, stream, cl, args, threads):
    from bench import replicate_batch
    from cilium_amd.proxylib import ProxylibPolicy
    from oracle.proxylib_ref import ProxylibOracle
    D, reps = 262_144, 400
    pols, reqs = r2d2_workload(D)
    pl = ProxylibPolicy(cl)
    pl.update(pols)
    pidx = pl.index("r2d2-bench")
    args_ = ([pidx] * D, [1] * D, [r[0] for r in reqs], [r[1] for r in reqs], [r[2] for r in reqs],
             [r[3] for r in reqs])
    b = pl.pack(*args_)
    o = ProxylibOracle(pols)
    chk = 20_000
    got = cl.http_verdicts(b)[:chk]
    exp = [int(o.matches("r2d2-bench", True, r[0], r[1], r[2], r[3])) for r in reqs[:chk]]
    assert got.tolist() == exp, "proxylib verdicts differ from the oracle"
    d_batch, nslots, _, data_bytes = replicate_batch(b, reps, dev, torch)
    d_arena = torch.from_numpy(b.arena).to(dev)
    d_out = torch.zeros(nslots, dtype=torch.uint8, device=dev)
    n = D * reps
    sec = timed(torch, stream, lambda: cl.http_verdicts_dev(d_batch, nslots, d_arena, d_out,
                                                            stream=stream.cuda_stream), args.steps, 2)
    bpi = data_bytes / n + 1
    sample = reqs[:20_000]
    cpu = cpu_rate(lambda: [o.matches("r2d2-bench", True, r[0], r[1], r[2], r[3]) for r in sample], len(sample),
                   args.cpu_seconds)
    return line("proxylib r2d2 verdicts/s (PolicyInstance.Matches + r2d2 rules) on http_kernel", n, sec, bpi,
                "http_kernel", cpu, "20K requests of the same workload, 1 thread (pure-Python oracle)", 1,
                {"config": {"workload": "SURVEY 8(f) row 4: 512 r2d2 rules over 64 ports, 104.9M requests",
                            "requests": n, "allow_fraction": float(np.mean(exp))}})


def _proxylib_fields_bench(torch, dev, stream, cl, pols, name, fields, remotes, ports, want, metric, workload, cpu,
                           cpu_sample, reps):
    """Requests given as their proxylib parser's fields (ProxylibPolicy.
    pack_fields: the escaped values http_kernel walks), replicated to
    `reps` copies of each program group on the device; verdicts of the
    distinct requests equal `want` (the oracle's)."""
    from bench import replicate_batch
    from cilium_amd.proxylib import ProxylibPolicy
    pl = ProxylibPolicy(cl)
    pl.update(pols)
    pidx = pl.index(name)
    D = len(fields)
    b = pl.pack_fields([pidx] * D, [1] * D, ports, remotes, fields)
    got = cl.http_verdicts(b)
    assert got.tolist() == list(want), f"{name}: verdicts differ from the oracle"
    d_batch, nslots, _, data_bytes = replicate_batch(b, reps, dev, torch)
    d_arena = torch.from_numpy(np.concatenate([b.arena.view(np.uint8), np.zeros(16, np.uint8)])).to(dev)
    d_out = torch.zeros(nslots, dtype=torch.uint8, device=dev)
    n = D * reps
    sec = timed(torch, stream, lambda: cl.http_verdicts_dev(d_batch, nslots, d_arena, d_out,
                                                            stream=stream.cuda_stream), 5, 2)
    return line(metric, n, sec, data_bytes / n + 1, "http_kernel", cpu, cpu_sample, 1,
                {"config": {"workload": workload, "requests": n, "allow_fraction": float(np.mean(want))}})


def bench_memcache(torch, dev, stream, cl, args, threads):
    """memcache (proxylib/memcached): 64 ports x 8 rules (a text command set
    with keyExact / keyPrefix / keyRegex, or a binary opcode); requests are
    the parser's MemcacheMeta (command or opcode, keys) as fields.  Oracle:
    oracle/memcache_ref.py Rule.matches (parser.go:46-100), any rule of the
    port (PolicyInstance.Matches)."""
    from oracle.memcache_ref import Meta, Rule
    from cilium_amd.proxylib import memcache_request
    rng = np.random.default_rng(0x3CAC)
    ports, rules_of = [], {}
    for pi in range(64):
        rules = []
        for ri in range(8):
            k = pi * 8 + ri
            rule = [{"command": "get", "keyExact": f"user{k}"}, {"command": "set", "keyPrefix": f"cache{k}/"},
                    {"command": "writeGroup", "keyRegex": f"^sess{k}-[0-9]+$"}, {"command": "delete"}][ri % 4]
            rules.append(rule)
        rules_of[7000 + pi] = [Rule(r) for r in rules]
        ports.append({"port": 7000 + pi, "rules": [{"l7_proto": "memcache", "l7_rules": {"l7_rules": [
            {"rule": r} for r in rules]}}]})
    pols = [{"name": "memcache-bench", "ingress_per_port_policies": ports}]
    D = 131_072
    fields, prt, rem, want = [], [], [], []
    for i in range(D):
        pi = int(rng.integers(0, 64))
        k = pi * 8 + int(rng.integers(0, 8))
        cmd = [b"get", b"gets", b"set", b"add", b"delete", b"incr"][int(rng.integers(0, 6))]
        nk = int(rng.integers(1, 4))
        good = rng.random() < 0.5
        keys = [(b"user%d" % k if cmd in (b"get", b"gets") else b"cache%d/x%d" % (k, j) if cmd in (b"set", b"add")
                 else b"sess%d-%d" % (k, j)) if good else b"k%d" % int(rng.integers(0, 1000)) for j in range(nk)]
        m = Meta(cmd, 0, keys)
        fields.append(memcache_request(cmd, 0, keys))
        prt.append(7000 + pi)
        rem.append(1)
        want.append(int(any(r.matches(m) for r in rules_of[7000 + pi])))
    sample = list(zip(fields[:20_000], prt[:20_000]))

    def cpu_fn():
        for f, p in sample:
            m = Meta(f[0][1][1:], 0, [x for x in bytes(f[1][1]).split(b"\x03\x14") if x])
            any(r.matches(m) for r in rules_of[p])
    cpu = cpu_rate(cpu_fn, len(sample), args.cpu_seconds)
    return _proxylib_fields_bench(torch, dev, stream, cl, pols, "memcache-bench", fields, rem, prt, want,
                                  "proxylib memcache verdicts/s (memcached Rule.Matches) on http_kernel",
                                  "SURVEY 8(f) row 4: 512 memcache rules over 64 ports, requests as MemcacheMeta "
                                  "fields", cpu, "20K requests, 1 thread (pure-Python oracle)", 400)


def bench_cassandra(torch, dev, stream, cl, args, threads):
    """cassandra (proxylib/cassandra): 64 ports x 8 rules (query_action /
    query_table regexes); requests are the parser's paths
    "/opcode/action/table" as fields.  Oracle: oracle/proxylib_ref.py
    (CassandraRule.Matches, cassandraparser.go:73-89)."""
    from oracle.proxylib_ref import ProxylibOracle
    from cilium_amd.proxylib import cassandra_request
    rng = np.random.default_rng(0xCA55)
    ports = []
    for pi in range(64):
        rules = []
        for ri in range(8):
            k = pi * 8 + ri
            rules.append([{"query_action": "select", "query_table": f"ks{k}\\.t[0-9]+"},
                          {"query_action": "insert", "query_table": f"^ks{k}\\."},
                          {"query_table": f"audit{k}$"}, {"query_action": "update"}][ri % 4])
        ports.append({"port": 7000 + pi, "rules": [{"l7_proto": "cassandra", "l7_rules": {"l7_rules": [
            {"rule": r} for r in rules]}}]})
    pols = [{"name": "cassandra-bench", "ingress_per_port_policies": ports}]
    o = ProxylibOracle(pols)
    D = 131_072
    fields, prt, rem, want, paths = [], [], [], [], []
    for i in range(D):
        pi = int(rng.integers(0, 64))
        k = pi * 8 + int(rng.integers(0, 8))
        act = [b"select", b"insert", b"update", b"delete", b"truncate"][int(rng.integers(0, 5))]
        tab = [b"ks%d.t%d" % (k, int(rng.integers(0, 9))), b"ks%d.x" % k, b"audit%d" % k,
               b"other%d.t" % int(rng.integers(0, 999))][int(rng.integers(0, 4))]
        path = b"/query/" + act + b"/" + tab
        paths.append(path)
        fields.append(cassandra_request(path))
        prt.append(7000 + pi)
        rem.append(1)
        want.append(int(o.matches_path("cassandra-bench", True, 7000 + pi, 1, path)))
    sample = list(zip(paths[:20_000], prt[:20_000]))
    cpu = cpu_rate(lambda: [o.matches_path("cassandra-bench", True, p, 1, x) for x, p in sample], len(sample),
                   args.cpu_seconds)
    return _proxylib_fields_bench(torch, dev, stream, cl, pols, "cassandra-bench", fields, rem, prt, want,
                                  "proxylib cassandra verdicts/s (CassandraRule.Matches) on http_kernel",
                                  "SURVEY 8(f) row 4: 512 cassandra rules over 64 ports, requests as "
                                  "/opcode/action/table paths", cpu, "20K requests, 1 thread (pure-Python oracle)",
                                  400)


def bench_selcache_expand(torch, dev, stream, sc, repo, eps, rule_m, args, threads):
    """Expansion of the bench's bitsets into policy-map entries: per endpoint
    its two L3 rows (the ingress / egress reach rows) and L4_ROWS rows over
    two rule selectors each, drawn from the POOL rule selectors whose sets are
    nearest L4_SET identities (a policy map holds at most 16,384 entries, so
    L4 rows are sparse).  Checked against the host walker (cg_diag_selcache_entries_host
    on `threads` threads, also the CPU leg), then timed: HIP events around
    the three expansion kernels over a device source matrix, and the fused
    call's wall time with its copy back.  The parent commit's
    endpoint_policy_map_states runs on a sample of endpoints (its own L4 rows:
    the repository's resolved filters) and is extrapolated."""
    from cilium_amd.classifier import POLICY_KEY_DTYPE
    from cilium_amd.policy import htons
    from cilium_amd.selcache import ExpandTable
    POOL, L4_ROWS, L4_SET = 64, 4, 1024
    E, W = len(eps), sc.words
    rng = np.random.default_rng(0xE7)
    sels = sc.compile_repository(repo)[0]
    bits_of_byte = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.uint8)
    pop = bits_of_byte[np.ascontiguousarray(rule_m).view(np.uint8)].sum(axis=1, dtype=np.int64)
    order = [int(i) for i in np.argsort(np.abs(pop - L4_SET), kind="stable")[:POOL]]
    pool = [sels[i] for i in order]
    S = len(pool)
    rows = []
    for n in range(E):
        for k in range(L4_ROWS):
            rows.append((htons(80 + k), 6, k & 1, htons(15001) if k == 0 else 0, 0,
                         [int(x) for x in rng.choice(S, 2, replace=False)]))
        rows.append((0, 0, 0, 0, 0, [S + n]))
        rows.append((0, 0, 1, 0, 0, [S + E + n]))
    table = ExpandTable(rows)
    R = len(rows)
    # ---- the fused call, checked against the host walker
    sc.entries(pool, eps, table)  # sizes the entry buffers
    fused = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = sc.entries(pool, eps, table)
        fused.append(time.perf_counter() - t0)
    sc.entries(pool, eps[:1], ExpandTable(rows[:1]), diag_cpu=True, threads=threads)  # the walker's own M, not timed
    t0 = time.perf_counter()
    want = sc.entries(pool, eps, table, diag_cpu=True, threads=threads)
    walker_s = time.perf_counter() - t0
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), "selcache expand differs from the host walker"
    total = len(got[1])
    # ---- the three kernels over a device source matrix
    d_src = torch.empty((S + 2 * E) * W, dtype=torch.int64, device=dev)
    d_ep = torch.from_numpy(eps.view(np.int32)).to(dev)
    d_fl = torch.empty(E, dtype=torch.uint8, device=dev)
    d_off = torch.empty(R + 1, dtype=torch.int64, device=dev)
    d_keys = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    d_proxy = torch.empty(max(total, 1), dtype=torch.int16, device=dev)
    d_total = torch.empty(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    sc.match_dev(pool, d_src[:S * W], stream=stream.cuda_stream)
    sc.reach_dev(d_ep, E, d_src[S * W:(S + E) * W], d_src[(S + E) * W:], d_fl, stream=stream.cuda_stream)
    expand_s = timed(torch, stream, lambda: sc.expand_dev(table, d_src, S + 2 * E, d_off, d_keys, d_proxy, total,
                                                          d_total, stream=stream.cuda_stream), args.steps, 2)
    assert int(d_total.cpu().numpy()[0]) == total
    assert np.array_equal(d_keys.cpu().numpy().view(POLICY_KEY_DTYPE)[:total], want[1])
    assert np.array_equal(d_proxy.cpu().numpy().view(np.uint16)[:total], want[2])
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), want[0])
    # ---- the parent's path on a sample of endpoints, extrapolated
    parent = None
    if args.cpu_seconds > 0:
        sample = [int(sc.ids[e]) for e in eps[:2]]
        t0 = time.perf_counter()
        states = sc.endpoint_policy_map_states(sample)
        parent_s = time.perf_counter() - t0
        parent = {"kind": "extrapolated from a sample of endpoints (its own L4 rows: the repository's filters)",
                  "sample_endpoints": len(sample), "sample_s": parent_s, "sample_entries": sum(map(len, states)),
                  "all_endpoints_s_extrapolated": parent_s * E / len(sample)}
    fused_s = sorted(fused)[1]
    out_bytes = total * 10 + (R + 1) * 8
    return {"kernels": ["selcache_expand_count_kernel", "selcache_expand_scan_kernel", "selcache_expand_emit_kernel"],
            "rows": R, "l4_rows_per_endpoint": L4_ROWS, "l4_selector_pool": S, "entries": total,
            "kernels_ms": expand_s * 1e3, "entries_per_s": total / expand_s,
            "output_bytes": out_bytes, "output_gbps": out_bytes / expand_s / 1e9,
            "fused_call_wall_ms": fused_s * 1e3, "fused_call": "match + reach + expand + copy back, median of 3",
            "host_walker_ms": walker_s * 1e3, "host_walker_threads": threads,
            "kernels_over_host_walker": walker_s / expand_s, "fused_over_host_walker": walker_s / fused_s,
            "parent_endpoint_policy_map_states": parent}


def bench_selcache(torch, dev, stream, cl, args, threads):
    """The selector cache at regeneration scale: 65,536 identities of 8
    labels, a 10,000-rule label repository, 256 endpoints.  Both kernels are
    checked against the library's host walker of the same compiled tables
    (cg_diag_selcache_*_host on `threads` threads — that run is also the CPU
    leg), then timed on the stream; bench_selcache_expand adds the expansion
    into policy-map entries.  resolve.py (the Python restatement the
    tables are pinned to) is timed on a sample of cells and extrapolated."""
    from cilium_amd import synth
    N_IDS, N_RULES, E = 65536, 10000, 256
    cache = synth.identity_cache(N_IDS)
    repo = synth.label_repository(N_RULES)
    sc = cl.selector_cache()
    sc.set_identities(cache)
    sc.set_repository(repo)
    info = sc.info()
    S, W = info["selectors"], info["words"]
    rng = np.random.default_rng(0x5E1)
    eps = np.sort(rng.choice(N_IDS, E, replace=False)).astype(np.uint32)
    # ---- check, and the host walker's time on the same tables
    got_m = sc.match(None)
    t0 = time.perf_counter()
    want_m = sc.match(None, diag_cpu=True, threads=threads)
    cpu_match_s = time.perf_counter() - t0
    assert np.array_equal(got_m, want_m), "selcache match differs from the host walker"
    got_r = sc.reach_indices(eps)
    sc.reach_indices(eps[:1], diag_cpu=True, threads=threads)  # builds the walker's own M (not timed below)
    t0 = time.perf_counter()
    want_r = sc.reach_indices(eps, diag_cpu=True, threads=threads)
    cpu_reach_s = time.perf_counter() - t0
    assert all(np.array_equal(a, b) for a, b in zip(got_r, want_r)), "selcache reach differs from the host walker"
    # ---- kernels
    d_m = torch.empty(S * W, dtype=torch.int64, device=dev)
    d_ep = torch.from_numpy(eps.view(np.int32)).to(dev)
    d_ing = torch.empty(E * W, dtype=torch.int64, device=dev)
    d_eg = torch.empty(E * W, dtype=torch.int64, device=dev)
    d_fl = torch.empty(E, dtype=torch.uint8, device=dev)
    match_s = timed(torch, stream, lambda: sc.match_dev(None, d_m, stream=stream.cuda_stream), args.steps, 2)
    reach_s = timed(torch, stream, lambda: sc.reach_dev(d_ep, E, d_ing, d_eg, d_fl, stream=stream.cuda_stream),
                    args.steps, 2)
    assert np.array_equal(d_m.cpu().numpy().view(np.uint64).reshape(S, W), want_m)
    # ---- resolve.py on a sample, extrapolated
    py_match = py_reach = None
    if args.cpu_seconds > 0:
        sels = sc.compile_repository(repo)[0]
        labels = list(cache.values())
        ss, ii = rng.integers(0, S, 100_000), rng.integers(0, N_IDS, 100_000)
        t0 = time.perf_counter()
        for a, b in zip(ss, ii):
            sels[a].matches(labels[b])
        py_match = len(ss) / (time.perf_counter() - t0)
        t0, k = time.perf_counter(), 0
        while time.perf_counter() - t0 < min(args.cpu_seconds, 5.0):
            me, peer = labels[int(eps[k % E])], labels[int(rng.integers(0, N_IDS))]
            repo.allows_ingress_label_access(peer, me)
            repo.allows_egress_label_access(me, peer)
            k += 1
        py_reach = 2 * k / (time.perf_counter() - t0)
    expand = bench_selcache_expand(torch, dev, stream, sc, repo, eps, want_m, args, threads)
    cells, rcells = S * N_IDS, 2 * E * N_IDS
    ident_bytes = N_IDS * 8 * 16 + (N_IDS + 1) * 4
    out = line("selector x identity cells/s (selcache_match_kernel: EndpointSelector.Matches over the identity cache)",
               cells, match_s, (S * W * 8 + ident_bytes) / cells, "selcache_match_kernel", cells / cpu_match_s,
               f"the same tables walked by cg_diag_selcache_match_host on {threads} threads, one full pass", threads,
               {"unit": "cells/s",
                "config": {"workload": "65,536 identities x 8 labels, 10,000-rule label repository, 256 endpoints",
                           "identities": N_IDS, "rules": N_RULES, "selectors": S, "endpoints": E},
                "match": {"kernel_ms": match_s * 1e3, "gcells_per_s": cells / match_s / 1e9,
                          "output_bytes": S * W * 8, "output_gbps": S * W * 8 / match_s / 1e9,
                          "output_frac_of_hbm_peak": S * W * 8 / match_s / 1e9 / HBM_PEAK_GBPS,
                          "host_walker_ms": cpu_match_s * 1e3, "host_walker_threads": threads,
                          "gpu_over_host_walker": cpu_match_s / match_s},
                "reach": {"kernel": "selcache_reach_kernel", "kernel_ms": reach_s * 1e3,
                          "gcells_per_s": rcells / reach_s / 1e9, "output_bytes": 2 * E * W * 8 + E,
                          "output_gbps": (2 * E * W * 8 + E) / reach_s / 1e9,
                          "output_frac_of_hbm_peak": (2 * E * W * 8 + E) / reach_s / 1e9 / HBM_PEAK_GBPS,
                          "host_walker_ms": cpu_reach_s * 1e3, "host_walker_threads": threads,
                          "gpu_over_host_walker": cpu_reach_s / reach_s},
                "expand": expand,
                "python_resolve": {"kind": "extrapolated from a sample (single thread)",
                                   "match_cells_per_s": py_match, "match_sample_cells": 100_000,
                                   "match_full_s_extrapolated": cells / py_match if py_match else None,
                                   "reach_cells_per_s": py_reach,
                                   "reach_full_s_extrapolated": rcells / py_reach if py_reach else None}})
    sc.destroy()
    return out


def bench_selcache_cidr(torch, dev, stream, cl, args, threads):
    """The prefix section at the ipcache's scale: 65,536 label identities of
    8 labels, 262,144 prefix identities (the ipcache bench's /32-heavy mix),
    the 10,000-rule label repository plus 128 egress rules carrying 1,024
    distinct cidr: selectors.  Three things, measured in one run:
    selcache_cidr_match_kernel (a cache holding only the prefix section, so
    no other kernel runs between the events), the host walker on the same
    tables, and the same prefix identities as explicit label identities
    through selcache_match_kernel — what the library could do before the
    prefix section existed — with that table's device bytes and the host
    seconds of cg_selcache_set_identities.  The native results are checked
    against the host walker and, array for array, against the explicit-label
    cache's before timing."""
    from cilium_amd import _native as N
    from cilium_amd import cidr as CIDR
    from cilium_amd import resolve as R
    from cilium_amd import synth
    from cilium_amd.selcache import _strings
    N_IDS, N_PFX, N_RULES, N_CSEL = 65536, 262144, 10000, 1024
    cache = synth.identity_cache(N_IDS)
    keys, _ = synth.ipcache_entries(int(N_PFX * 1.05))
    keys = keys[:N_PFX]
    assert len(keys) == N_PFX
    nets = [CIDR.Net(bytes(k["addr"][:4 if k["family"] == 4 else 16]), int(k["prefixlen"])) for k in keys]
    prefixes = {200_000 + i: n for i, n in enumerate(nets)}
    # 1,024 distinct cidr: selectors: ancestors of the prefix identities at mixed lengths
    rng = np.random.default_rng(0xC1D2)
    anc: dict[str, None] = {}
    while len(anc) < N_CSEL:
        n = nets[int(rng.integers(0, N_PFX))]
        lo = 8 if n.family == 4 else 32
        m = int(rng.integers(min(lo, n.ones), n.ones + 1))
        if m:
            anc[CIDR.Net(CIDR._mask(n.ip, CIDR.cidr_mask(m, n.bits)), m).text()] = None
    anc_l = list(anc)
    repo = synth.label_repository(N_RULES)
    repo.add_list([R.Rule(R.EndpointSelector.of({"k8s:cidr-bench": str(i)}), [],
                          [R.EgressRule(ToCIDR=anc_l[8 * i:8 * i + 8])]) for i in range(N_CSEL // 8)])
    # ---- native: the prefix section alone (the new kernel's own time), then both sections
    only = cl.selector_cache()
    only.set_cidr_identities(prefixes)
    only.set_repository(repo)
    S, Wc = only.info()["selectors"], only.info()["words"]
    got = only.match(None)
    t0 = time.perf_counter()
    want = only.match(None, diag_cpu=True, threads=threads)
    walker_s = time.perf_counter() - t0
    assert np.array_equal(got, want), "selcache cidr match differs from the host walker"
    d_c = torch.empty(S * Wc, dtype=torch.int64, device=dev)
    cidr_s = timed(torch, stream, lambda: only.match_dev(None, d_c, stream=stream.cuda_stream), args.steps, 2)
    assert np.array_equal(d_c.cpu().numpy().view(np.uint64).reshape(S, Wc), want)
    both = cl.selector_cache()
    both.set_identities(cache)
    both.set_cidr_identities(prefixes)
    both.set_repository(repo)
    Wb = both.info()["words"]
    got_b = both.match(None)
    assert np.array_equal(got_b, both.match(None, diag_cpu=True, threads=threads))
    assert np.array_equal(got_b[:, N_IDS // 64:], want)  # N_IDS is a multiple of 64: the prefix words are the same
    d_b = torch.empty(S * Wb, dtype=torch.int64, device=dev)
    both_s = timed(torch, stream, lambda: both.match_dev(None, d_b, stream=stream.cuda_stream), args.steps, 2)
    both.destroy()
    # ---- the same prefix identities as explicit labels
    t0 = time.perf_counter()
    ids = np.fromiter(prefixes, np.uint32, N_PFX)
    lab_off = np.zeros(N_PFX + 1, np.uint32)
    lkeys: list = []
    for i, n in enumerate(nets):
        lkeys.extend(CIDR.cidr_labels(n))
        lab_off[i + 1] = len(lkeys)
    kb, ko = _strings(lkeys)
    vb, vo = _strings([""] * len(lkeys))
    build_s = time.perf_counter() - t0
    exp = cl.selector_cache()
    t0 = time.perf_counter()
    N.check(N.lib.cg_selcache_set_identities(cl.h, exp.id, N.ptr(ids), N_PFX, N.ptr(lab_off), N.ptr(kb), N.ptr(ko),
                                             N.ptr(vb), N.ptr(vo)))
    set_ident_s = time.perf_counter() - t0
    n_labels = len(lkeys)
    del lkeys, kb, ko, vb, vo
    exp.ids, exp.words = ids, Wc
    exp.set_repository(repo)
    t0 = time.perf_counter()
    got_e = exp.match(None)  # the first call publishes: interning the rule set against 9M labels' dictionary, upload
    publish_s = time.perf_counter() - t0
    assert np.array_equal(got_e, want), "the explicit-label cache differs from the prefix section"
    d_e = torch.empty(S * Wc, dtype=torch.int64, device=dev)
    exp_s = timed(torch, stream, lambda: exp.match_dev(None, d_e, stream=stream.cuda_stream), args.steps, 2)
    exp.destroy()
    t0 = time.perf_counter()
    only.set_cidr_identities(prefixes)
    only.match(None)
    native_set_s = time.perf_counter() - t0
    only.destroy()
    cells = S * N_PFX
    native_bytes, explicit_bytes = N_PFX * 24, n_labels * 16 + (N_PFX + 1) * 4
    return line("selector x prefix-identity cells/s (selcache_cidr_match_kernel: selectors over the prefix section)",
                cells, cidr_s, (S * Wc * 8 + native_bytes) / cells, "selcache_cidr_match_kernel", cells / walker_s,
                f"the same tables walked by cg_diag_selcache_match_host on {threads} threads, one full pass", threads,
                {"unit": "cells/s",
                 "config": {"workload": "262,144 prefix identities (ipcache mix), 10,000-rule repository + 1,024 cidr: "
                                        "selectors; 65,536 label identities x 8 labels for the two-section launch",
                            "prefix_identities": N_PFX, "label_identities": N_IDS, "selectors": S,
                            "cidr_selectors": N_CSEL},
                 "native": {"kernel_ms": cidr_s * 1e3, "gcells_per_s": cells / cidr_s / 1e9,
                            "identity_table_bytes": native_bytes, "host_walker_ms": walker_s * 1e3,
                            "host_walker_threads": threads, "gpu_over_host_walker": walker_s / cidr_s,
                            "set_and_publish_s": native_set_s,
                            "both_sections_kernels_ms": both_s * 1e3},
                 "explicit_labels": {"kernel": "selcache_match_kernel", "kernel_ms": exp_s * 1e3,
                                     "labels": n_labels, "identity_table_bytes": explicit_bytes,
                                     "set_identities_s": set_ident_s, "publish_s": publish_s,
                                     "python_label_build_s": build_s,
                                     "explicit_over_native_time": exp_s / cidr_s,
                                     "explicit_over_native_bytes": explicit_bytes / native_bytes}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", default="l4,lpm,kafka,ipcache,proxylib,l4ipc")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--cpu-seconds", type=float, default=5.0)
    ap.add_argument("--prewarm-seconds", type=float, default=0.3)
    ap.add_argument("--array-tuples", type=int, default=1 << 26, help="l4_array: distinct tuples before tiling")
    ap.add_argument("--frames", type=int, default=1 << 22, help="l4_frames: distinct frames before tiling to 2^24")
    args = ap.parse_args()
    global PREWARM_S
    PREWARM_S = args.prewarm_seconds
    import torch
    from cilium_amd.classifier import Classifier
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    cl = Classifier(device=0)
    threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or min(16, os.cpu_count() or 1)
    fns = {"l4": bench_l4, "lpm": bench_lpm, "kafka": bench_kafka, "ipcache": bench_ipcache,
           "proxylib": bench_proxylib, "l4ipc": bench_l4ipc, "kafkawire": bench_kafka_wire, "httphost": bench_http_host, "httpraw": bench_http_raw,
           "httpfields": bench_http_fields, "memcache": bench_memcache, "cassandra": bench_cassandra,
           "kafkawirez": lambda *a: bench_kafka_wire(*a, codec_frac=0.5), "selcache": bench_selcache,
           "selcache_cidr": bench_selcache_cidr, "l4_array": bench_l4_array, "l4_frames": bench_l4_frames}
    for p in args.paths.split(","):
        print(json.dumps(fns[p](torch, dev, stream, cl, args, threads)), flush=True)
    cl.close()


if __name__ == "__main__":
    main()
