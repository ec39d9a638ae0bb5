"""The kernels' counters, element for element.

Verdicts are compared bit-exact with the oracle everywhere else; here the
second output of each kernel is: HTTP {allowed, denied} per program and hits
per rule, the stale-batch count, Kafka {allowed, denied} per redirect, L4
{packets, bytes} per entry, prefilter {drop, pass}.  Every expected vector
comes from the oracle's verdicts and from values the inputs carry
(counters_util.py, pinned on the CPU by test_counters.py), never from the
kernel under test, so a count that lands on the neighbouring program,
redirect or entry fails even though every sum stays the same."""
import random

import numpy as np
import pytest

import oracle
from cilium_amd import _native as N
from cilium_amd import synth
from cilium_amd.classifier import L4_TUPLE_DTYPE
from counters_util import (batch_header, chunk_table, expected_program_counters, kafka_redirect_counters,
                           l4_entry_counters, program_counters, program_of_requests)
from test_cpu_differential import ID_SETS, _kafka_edge_policy, _rand_policy, _rand_requests, all_matcher_case
from test_http_raw_dl_gpu import _big_program_policy
from test_http_raw_layouts_gpu import _blob, _raw_requests, _vary
from test_http_raw_layouts_gpu import _oracle as _raw_oracle
from test_ipcache import _ipc_l4_case
from test_rule_counters import _oracle_counts

pytestmark = pytest.mark.gpu

K_DEAL_RUN = 4  # kernels_http.hip kDealRun


def _programs(cl):
    return cl.read_counters(N.CG_CTR_HTTP_PROGRAMS)


def _http_counters_case(cl, pols, rq, nthreads=8):
    """Install, pack, run from zeroed counters: verdicts equal the oracle's and
    the per-program vector equals the helper's, built from the oracle's."""
    cl.update_http_policy(pols)
    nprogs = cl.http_policy_stats()["programs"]
    b = cl.pack_http(**rq)
    want_v = oracle.HttpOracle(pols).eval(**rq, nthreads=nthreads)
    want_c = expected_program_counters(b, want_v, nprogs)
    cl.reset_counters()
    got_v = cl.http_verdicts(b)
    got_c = _programs(cl)
    assert np.array_equal(got_v, want_v)
    assert np.array_equal(got_c, want_c), (got_c.tolist(), want_c.tolist())
    return b, want_v, want_c


# ------------------------------------------------ 2. HTTP, per program ----
@pytest.mark.parametrize("ids", sorted(ID_SETS))
@pytest.mark.parametrize("seed", range(100, 106))
def test_http_program_counters_random(gpu, seed, ids):
    """Allow-all programs, both special programs and malformed records."""
    rng = random.Random(seed)
    pols = _rand_policy(rng, ids=ID_SETS[ids])
    rq = _rand_requests(rng, 3000, len(pols), ids=ID_SETS[ids])
    b, v, c = _http_counters_case(gpu, pols, rq)
    assert c.sum() < len(v)  # some requests are counted nowhere
    assert np.count_nonzero(c.reshape(-1, 2).sum(1)) >= 2  # more than one program counts


@pytest.mark.parametrize("seed", range(4))
def test_http_program_counters_all_matchers(gpu, seed):
    """10-16 programs, some of several parts, one beyond LDS (seed 3): the
    one-part walker, http_tiles and http_kernel_global add to one vector."""
    pols, rq, _ = all_matcher_case(seed, 4000)
    _http_counters_case(gpu, pols, rq)


def test_http_all_matcher_cases_reach_both_kernels(gpu):
    stats = []
    for seed in range(4):
        gpu.update_http_policy(all_matcher_case(seed, 1)[0])
        stats.append(gpu.http_policy_stats())
    print([{k: int(s[k]) for k in ("programs", "parts", "lds_programs", "max_program_cells")} for s in stats])
    assert any(s["lds_programs"] < s["programs"] for s in stats)  # http_kernel_global has work
    assert any(s["parts"] > s["programs"] for s in stats)         # the several-part walker too


_http10k = {}


def _http10k_case(cl):
    """The 10K-rule set and 300,000 requests, the oracle's verdicts: built
    once, shared, never modified.  (The policy is installed by each test.)"""
    if not _http10k:
        pols, info = synth.http10k_rules()
        rq = synth.http10k_requests(300_000, info, distinct=100_000)
        v = oracle.HttpOracle(pols).eval(**rq, nthreads=16)
        v.setflags(write=False)
        _http10k.update(pols=pols, rq=rq, v=v)
    return _http10k["pols"], _http10k["rq"], _http10k["v"]


def _install_10k(cl):
    pols, rq, v = _http10k_case(cl)
    cl.update_http_policy(pols)
    nprogs = cl.http_policy_stats()["programs"]
    b = cl.pack_http(**rq)
    return b, v, nprogs, expected_program_counters(b, v, nprogs)


def test_http_program_counters_10k(gpu):
    """64 programs over more than 64 chunks: a workgroup's run of kDealRun
    chunks crosses program boundaries, so flush_counts runs on prog != cur
    with counts in flight."""
    b, v, nprogs, want = _install_10k(gpu)
    ct = chunk_table(b)
    changes = int((ct[1:, 0] != ct[:-1, 0]).sum())
    runs = [ct[i:i + K_DEAL_RUN, 0] for i in range(0, len(ct), K_DEAL_RUN)]
    crossing = sum(len(set(r.tolist())) > 1 for r in runs)
    print(f"programs {nprogs}, chunks {len(ct)}, program changes {changes}, "
          f"deal runs {len(runs)} of which {crossing} cross a program boundary")
    assert nprogs == 64 and len(ct) > 64
    assert changes >= nprogs - 1 and crossing > len(runs) // 2
    gpu.reset_counters()
    got_v = gpu.http_verdicts(b)
    got = _programs(gpu)
    assert np.array_equal(got_v, v)
    assert np.array_equal(got, want), np.nonzero(got != want)[0].tolist()
    assert (want.reshape(-1, 2) > 0).all()  # every program allows some and denies some


def test_http_program_counters_10k_rules_variant(gpu):
    """cg_http_verdicts_rules_*: the rule-output variant leaves the same counters."""
    b, v, nprogs, want = _install_10k(gpu)
    gpu.reset_counters()
    got_v, rule = gpu.http_verdicts_rules(b)
    got = _programs(gpu)
    hits = gpu.http_rule_hits()
    assert np.array_equal(got_v, v)
    assert np.array_equal(got, want), np.nonzero(got != want)[0].tolist()
    # its per-request rules, counted, are its per-rule counters
    attributed = rule[rule != 0xFFFFFFFF]
    assert np.array_equal(hits, np.bincount(attributed, minlength=len(hits)).astype(np.uint64))


_raw10k = {}


@pytest.mark.parametrize("layout", ["device", "host"])
def test_http_program_counters_raw_heads(gpu, monkeypatch, layout):
    """Raw heads through both cg_http_verdicts_raw sequences: a request's
    program depends on policy, direction, port and whether its head parsed,
    so it is the one cg_http_pack gives the same request (pack_http_raw)."""
    pols, info = synth.http10k_rules()
    gpu.update_http_policy(pols)
    nprogs = gpu.http_policy_stats()["programs"]
    if not _raw10k:
        rq = synth.http10k_requests(30_000, info, seed=171)
        raws = _vary(_raw_requests(rq), np.random.default_rng(172))
        args = (rq["policy"], rq["ingress"], rq["port"], rq["remote"])
        v = _raw_oracle(pols, *args, raws)
        v.setflags(write=False)
        _raw10k.update(args=args, blob=_blob(raws), v=v)
    args, (blob, off), v = _raw10k["args"], _raw10k["blob"], _raw10k["v"]
    rprog, rcnt = program_of_requests(gpu.pack_http_raw(*args, blob, off), nprogs)
    want = program_counters(rprog, rcnt, v, nprogs)
    assert 0 < (~rcnt).sum() < len(v) // 4  # heads the codec rejects are counted nowhere
    monkeypatch.setenv("CILIUM_GPU_RAW_LAYOUT", layout)
    gpu.reset_counters()
    got_v = gpu.http_verdicts_raw(*args, blob, off)
    got = _programs(gpu)
    assert np.array_equal(got_v, v)
    assert np.array_equal(got, want), np.nonzero(got != want)[0].tolist()


# --------------------------- 3. rule hits beyond kLdsRuleHits per program ----
def _word_requests(groups, n=6000, seed=5):
    """n requests "/<word>/<j>", request i on groups[i % len(groups)] = (port,
    words): half draw from the port's first 40 words (equal hits in long runs
    inside a tile), half from all of them; 30% with the word's last letter
    spoiled; every ninth from remote 5, which no rule selects."""
    rng = np.random.default_rng(seed)
    lists, ports = [], []
    for i in range(n):
        port, words = groups[i % len(groups)]
        w = words[int(rng.integers(0, min(40, len(words)) if rng.random() < 0.5 else len(words)))]
        if rng.random() < 0.3:
            w = w[:-1] + "_"
        lists.append(b":method\0GET\0:path\0/%s/%d\0" % (w.encode(), i))
        ports.append(port)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return dict(policy=np.zeros(n, np.uint32), ingress=np.ones(n, np.uint8), port=np.array(ports, np.uint16),
                remote=np.where(np.arange(n) % 9 == 8, 5, 7).astype(np.uint32),
                hdr_blob=np.frombuffer(b"".join(lists), np.uint8).copy(), hdr_off=off)


def _rule_hits_case(cl, pols, rq):
    cl.update_http_policy(pols)
    nprogs = cl.http_policy_stats()["programs"]
    info = cl.http_rule_info()
    b = cl.pack_http(**rq)
    want_v, _, want_hits = _oracle_counts(pols, rq, info)
    want_c = expected_program_counters(b, want_v, nprogs)
    cl.reset_counters()
    got_v = cl.http_verdicts(b)
    got_hits, got_c = cl.http_rule_hits(), _programs(cl)
    assert np.array_equal(got_v, want_v)
    assert np.array_equal(got_hits, want_hits), np.nonzero(got_hits != want_hits)[0].tolist()[:16]
    assert np.array_equal(got_c, want_c), (got_c.tolist(), want_c.tolist())
    return info, want_hits, want_v


@pytest.mark.parametrize("n_rules", [512, 513, 600, 734])
def test_rule_hits_of_big_programs(gpu, n_rules):
    """512 rules: the last size counted in the workgroup's LDS; 513 and 600:
    an LDS program whose hits go to global memory (count_hits' other branch,
    which flush_counts skips); 734: walked by http_kernel_global, which has
    no LDS hit counters at all."""
    pols, words = _big_program_policy(n_rules)
    gpu.update_http_policy(pols)
    st = gpu.http_policy_stats()
    print(n_rules, {k: int(st[k]) for k in ("programs", "parts", "lds_programs", "max_program_cells", "rules")})
    assert st["programs"] == 1 and st["rules"] == n_rules
    assert st["lds_programs"] == (0 if n_rules == 734 else 1), st
    info, hits, v = _rule_hits_case(gpu, pols, _word_requests([(80, words)]))
    print(f"rules hit {np.count_nonzero(hits)}, most hits on one rule {int(hits.max())}, allowed {v.mean():.3f}")
    assert np.count_nonzero(hits) > n_rules // 2 and hits.max() >= 30  # many rules, and long runs on a few
    assert 0.3 < v.mean() < 0.8


def test_rule_hits_lds_counters_skipped_between_programs(gpu):
    """Three programs of one policy in one launch, 600 / 10 / 513 rules on
    ports 80 / 81 / 82: the workgroup's LDS hit counters are passed over,
    used and flushed, and passed over again as the program changes."""
    sizes = {80: 600, 81: 10, 82: 513}
    words = {port: _big_program_policy(k, seed=port)[1] for port, k in sizes.items()}
    pols = [{"name": "three", "policy": 1, "ingress_per_port_policies": [
        {"port": port, "rules": [{"remote_policies": [7], "http_rules": {"http_rules": [
            {"headers": [{"name": ":path", "regex_match": "/" + w + ".*"}]} for w in ws]}}]}
        for port, ws in words.items()]}]
    gpu.update_http_policy(pols)
    st = gpu.http_policy_stats()
    print({k: int(st[k]) for k in ("programs", "parts", "lds_programs", "max_program_cells", "rules")})
    assert st["programs"] == 3 == st["lds_programs"] and st["rules"] == sum(sizes.values())
    rq = _word_requests([(port, ws) for port, ws in words.items()])
    info, hits, v = _rule_hits_case(gpu, pols, rq)
    for port, k in sizes.items():
        mine = hits[info["port"] == port]
        assert len(mine) == k and np.count_nonzero(mine) >= min(k, 40) // 2, (port, np.count_nonzero(mine))


# ------------------------------------------------- 4. the stale-batch path ----
def test_stale_batch_denied_and_counted(gpu):
    """A batch packed against the previous snapshot, and a batch whose tiles
    pass the nslots it is given: http_chunks refuses both by design, denies
    every slot it was given and adds one to the stale count, nothing else."""
    import torch
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    pols = synth.starwars_policy()
    rq = synth.starwars_requests(3000, seed=41)
    want_v = oracle.HttpOracle(pols).eval(**rq)
    gpu.update_http_policy(pols)
    old = gpu.pack_http(**rq)
    d_batch, d_arena = torch.from_numpy(old.batch).to(dev), torch.from_numpy(old.arena).to(dev)
    gpu.update_http_policy(pols)  # the same policy again: a new snapshot, a new epoch
    nprogs = gpu.http_policy_stats()["programs"]
    gpu.reset_counters()
    for launches in (1, 2):
        d_out = torch.full((old.nslots,), 7, dtype=torch.uint8, device=dev)
        gpu.http_verdicts_dev(d_batch, old.nslots, d_arena, d_out, stream=s)
        torch.cuda.synchronize()
        assert not d_out.cpu().numpy().any()
        allv = gpu.read_counters(N.CG_CTR_HTTP_ALLREDUCE)
        assert len(_programs(gpu)) == 2 * nprogs and len(allv) == 2 * nprogs + 1 + len(gpu.http_rule_hits())
        assert int(allv[2 * nprogs]) == launches
        assert not _programs(gpu).any() and not gpu.http_rule_hits().any()
    # repacked against the new snapshot: verdicts and counters as ever, the stale count stays
    new = gpu.pack_http(**rq)
    assert batch_header(new)["epoch"] != batch_header(old)["epoch"]
    assert np.array_equal(gpu.http_verdicts(new), want_v)
    assert np.array_equal(_programs(gpu), expected_program_counters(new, want_v, nprogs))
    assert int(gpu.read_counters(N.CG_CTR_HTTP_ALLREDUCE)[2 * nprogs]) == 2
    # a fresh batch given 64 slots fewer than its tiles hold
    before = gpu.read_counters(N.CG_CTR_HTTP_ALLREDUCE).copy()
    assert new.nslots > 128
    d_batch, d_arena = torch.from_numpy(new.batch).to(dev), torch.from_numpy(new.arena).to(dev)
    d_out = torch.full((new.nslots,), 7, dtype=torch.uint8, device=dev)
    gpu.http_verdicts_dev(d_batch, new.nslots - 64, d_arena, d_out, stream=s)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert not out[:new.nslots - 64].any() and (out[new.nslots - 64:] == 7).all()
    after = gpu.read_counters(N.CG_CTR_HTTP_ALLREDUCE)
    want = before.copy()
    want[2 * nprogs] += 1
    assert int(want[2 * nprogs]) == 3 and np.array_equal(after, want)


# ------------------------------------------------ 5. Kafka, per redirect ----
KAFKA_D = 49_999  # coprime to the 1,024 requests of a block iteration
_kafka = {}


def _kafka_case(seed):
    """Policy and requests of test_kafka_edge_parity (two redirects; requests
    name redirects {0, 0, 1, 2}, 2 being unknown; topic counts include 14),
    KAFKA_D of them, and the oracle's verdicts: built once per seed."""
    if seed not in _kafka:
        rng = random.Random(seed)
        pols, topics, clients = _kafka_edge_policy(rng)
        n = KAFKA_D
        rq = dict(redirect=[rng.choice([0, 0, 1, 2]) for _ in range(n)],
                  remote=[rng.choice([0, 7, 8, 9, 10, 11]) for _ in range(n)],
                  api_key=[rng.choice([0, 1, 3, 10, 12, 18, 37, -1, 40, 63, 64, 1000]) for _ in range(n)],
                  api_version=[rng.choice([0, 1, 5, 63, 64, 100, -1, 32767, -32768]) for _ in range(n)],
                  kind=[rng.choice([0, 1, 2, 3]) for _ in range(n)],
                  client_id=[rng.choice(clients + ["zz"]).encode() for _ in range(n)],
                  topics=[[rng.choice(topics + ["nope"]).encode() for _ in range(rng.choice([0, 0, 1, 2, 3, 14]))]
                          for _ in range(n)])
        v = oracle.KafkaOracle(pols).eval(**rq, nthreads=8)
        v.setflags(write=False)
        red = np.array(rq["redirect"], np.int64)
        want = kafka_redirect_counters(red, v, len(pols))
        # both redirects count (seeds 1 and 2 deny nothing on redirect 0), the unknown redirect would
        # be seen if counted, and denied requests that carry topics (the kernel's slow queue) are a
        # good part of the batch
        nt = np.array([len(t) for t in rq["topics"]])
        assert (want[0::2] > 0).all() and want[3] > 0 and int(want.sum()) == int((red < 2).sum()) < n
        assert 0.05 < ((v == 0) & (nt > 0) & (red < 2)).mean() < 0.6
        _kafka[seed] = (pols, rq, v, red, want)
    return _kafka[seed]


def _kafka_pack(cl, seed):
    pols, rq, v, red, want = _kafka_case(seed)
    cl.update_kafka_policy(pols)
    reqs, arena = cl.pack_kafka(**rq)
    assert len(cl.read_counters(N.CG_CTR_KAFKA)) == 4
    return reqs, arena, v, red, want


@pytest.mark.parametrize("seed", range(6))
def test_kafka_redirect_counters_host_staged(gpu, seed):
    """Request order as generated: the lanes of a wave hold mixed redirects
    (KfCount::add flushes as a lane's redirect changes; the non-uniform tail)."""
    reqs, arena, v, red, want = _kafka_pack(gpu, seed)
    gpu.reset_counters()
    got_v = gpu.kafka_verdicts(reqs, arena)
    got = gpu.read_counters(N.CG_CTR_KAFKA)
    assert np.array_equal(got_v, v)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())


@pytest.mark.parametrize("seed", range(6))
def test_kafka_redirect_counters_sorted_by_redirect(gpu, seed):
    """The same requests sorted by redirect: waves are uniform (the wave
    reduction), slow-path requests still drain on other lanes."""
    reqs, arena, v, red, want = _kafka_pack(gpu, seed)
    perm = np.argsort(red, kind="stable")
    gpu.reset_counters()
    got_v = gpu.kafka_verdicts(np.ascontiguousarray(reqs[perm]), arena)
    got = gpu.read_counters(N.CG_CTR_KAFKA)
    assert np.array_equal(got_v, v[perm])
    assert np.array_equal(got, want), (got.tolist(), want.tolist())


def _kafka_device_arrays(reqs, arena, rep=1):
    import torch
    dev = torch.device("cuda", 0)
    raw = np.ascontiguousarray(reqs).view(np.uint8).reshape(len(reqs), 64)
    d_reqs = torch.from_numpy(raw).to(dev)
    if rep > 1:
        d_reqs = d_reqs.repeat(rep, 1).contiguous()
    d_arena = torch.from_numpy(arena if len(arena) else np.zeros(1, np.uint32)).to(dev)
    d_out = torch.full((len(reqs) * rep,), 9, dtype=torch.uint8, device=dev)
    return d_reqs, d_arena, d_out


@pytest.mark.parametrize("seed", range(6))
def test_kafka_redirect_counters_device_layouts(gpu, seed):
    """cg_kafka_verdicts_dev and cg_kafka_verdicts_split_dev."""
    import torch
    reqs, arena, v, red, want = _kafka_pack(gpu, seed)
    d_reqs, d_arena, d_out = _kafka_device_arrays(reqs, arena)
    s = torch.cuda.current_stream().cuda_stream
    n = len(reqs)
    gpu.reset_counters()
    gpu.kafka_verdicts_dev(d_reqs, n, d_arena, d_out, stream=s)
    torch.cuda.synchronize()
    got = gpu.read_counters(N.CG_CTR_KAFKA)
    assert np.array_equal(d_out.cpu().numpy(), v)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    d_heads, d_topics = d_reqs[:, :16].contiguous(), d_reqs[:, 16:].contiguous()
    d_out.fill_(9)
    gpu.reset_counters()
    gpu.kafka_verdicts_split_dev(d_heads, d_topics, n, d_arena, d_out, stream=s)
    torch.cuda.synchronize()
    got = gpu.read_counters(N.CG_CTR_KAFKA)
    assert np.array_equal(d_out.cpu().numpy(), v)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())


@pytest.mark.parametrize("seed", range(2))
def test_kafka_redirect_counters_grid_stride_trips(gpu, seed):
    """The records 160 times over on the device, about 8.0 M of them: at
    least three grid-stride trips of kafka_kernel for up to 8 resident blocks
    per CU, no two with the same lane assignment (KAFKA_D is coprime to the
    1,024 requests per block iteration).  Counters carried across trips."""
    import torch
    rep = 160
    reqs, arena, v, red, want = _kafka_pack(gpu, seed)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert KAFKA_D * rep > 3 * cus * 8 * 1024, (cus, KAFKA_D * rep)
    d_reqs, d_arena, d_out = _kafka_device_arrays(reqs, arena, rep)
    gpu.reset_counters()
    gpu.kafka_verdicts_dev(d_reqs, len(reqs) * rep, d_arena, d_out, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = gpu.read_counters(N.CG_CTR_KAFKA)
    d_want = torch.from_numpy(v.copy()).to(d_out.device)
    assert bool((d_out.view(rep, len(reqs)) == d_want).all())
    assert np.array_equal(got, want * np.uint64(rep)), (got.tolist(), (want * np.uint64(rep)).tolist())


# ---------------------------------------------------- 6. L4, per entry ----
L4_EDGE_LENS = np.array([0, 1, 65535, 65536, 65537, 2 ** 32 - 1], np.uint32)  # either side of l4_count's split


def _l4_all_counters(pm, keys, pk, by):
    gpk, gby = l4_entry_counters(pm, keys)
    assert np.array_equal(gpk, pk), np.nonzero(gpk != pk)[0].tolist()[:16]
    assert np.array_equal(gby, by), np.nonzero(gby != by)[0].tolist()[:16]


@pytest.mark.parametrize("max_entries", [0, 65536])  # l4_fp_kernel's LDS counters, l4_kernel's global atomics
def test_l4_entry_counters_boundary_lengths(gpu, max_entries):
    keys, ports = synth.l4_table(n_entries=1000, n_ids=500)
    tuples = synth.l4_tuples(200_000, keys, n_ids=500, seed=61)
    by_position = tuples.copy()
    by_position["len"] = L4_EDGE_LENS[np.arange(len(tuples)) % len(L4_EDGE_LENS)]
    by_key = tuples.copy()  # an identity's entries see one length only: some, nothing but length 0
    by_key["len"] = L4_EDGE_LENS[tuples["identity"] % len(L4_EDGE_LENS)]
    for t in (by_position, by_key):
        pm = gpu.policy_map(max_entries=max_entries)
        pm.allow_keys(keys, ports)
        exp, pk, by = oracle.l4(keys, ports, t)
        assert by.dtype == np.uint64 and int(by.max()) > 2 ** 32
        if t is by_key:
            assert ((pk > 0) & (by == 0)).any() and ((pk > 0) & (by > 0)).any()
        assert np.array_equal(pm.verdicts(t), exp)
        _l4_all_counters(pm, keys, pk, by)
        pm.destroy()


@pytest.mark.parametrize("max_entries", [0, 65536])
def test_l4_entry_counters_one_hot_entry(gpu, max_entries):
    """200,000 tuples of length 65,535 on one entry: the largest length the
    packed LDS word takes, every atomic on one address."""
    keys, ports = synth.l4_table(n_entries=1000, n_ids=500)
    j = int(np.nonzero((keys["sec_label"] != 0) & (keys["dport"] != 0))[0][0])
    k = keys[j]
    t = np.zeros(200_000, L4_TUPLE_DTYPE)
    t["identity"], t["dport"], t["proto"] = k["sec_label"], k["dport"], k["protocol"]
    t["flags"] = 0 if k["egress"] else 1
    t["len"] = 65535
    exp, pk, by = oracle.l4(keys, ports, t)
    assert int(pk[j]) == len(t) == int(pk.sum()) and int(by[j]) == len(t) * 65535
    pm = gpu.policy_map(max_entries=max_entries)
    pm.allow_keys(keys, ports)
    assert np.array_equal(pm.verdicts(t), exp)
    _l4_all_counters(pm, keys, pk, by)
    pm.destroy()


_ipc = {}


def _ipc_case(n_entries, family, n):
    """_ipc_l4_case with at least n tuples of the family (the builder splits
    its addresses 70/30 between the families), cached."""
    key = (n_entries, family)
    if key not in _ipc:
        share = 0.7 if family == 4 else 0.3
        _ipc[key] = _ipc_l4_case(n_entries, int(n / share) + 8, 63, family)
    assert len(_ipc[key][4]) >= n
    return _ipc[key]


def _via_ipcache(cl, pm, ic, case, n):
    """The case's first n tuples through verdicts_via_ipcache from zeroed
    counters: verdicts and every entry's counters against the oracle."""
    keys, ports, ik, iv, remote, tuples = case[:6]
    remote, tuples = np.ascontiguousarray(remote[:n]), np.ascontiguousarray(tuples[:n])
    exp, pk, by = oracle.l4_egress_via_ipcache(keys, ports, ik, iv, remote, tuples)
    cl.reset_counters()
    assert np.array_equal(pm.verdicts_via_ipcache(ic, remote, tuples), exp)
    _l4_all_counters(pm, keys, pk, by)
    return pk


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("family", [0, 4, 6])
def test_l4_kernel_second_trip(gpu, family):
    """l4_kernel<0/4/6> (65,536-entry map: global fingerprints and counters)
    launches at most cus * 8 blocks of 256 threads: 4,097 tuples more send 17
    blocks on a second trip, one of them with a single tuple."""
    n = _cus() * 8 * 256 + 4097
    case = _ipc_case(65536, family or 4, n)
    keys, ports, ik, iv, remote, tuples = case[:6]
    pm = gpu.policy_map(max_entries=65536)
    pm.allow_keys(keys, ports)
    print(f"cus {_cus()}, n {n}")
    if family:
        ic = gpu.ipcache()
        ic.update(ik, iv)
        pk = _via_ipcache(gpu, pm, ic, case, n)
        ic.destroy()
    else:
        t = np.ascontiguousarray(tuples[:n])
        exp, pk, by = oracle.l4(keys, ports, t)
        assert np.array_equal(pm.verdicts(t), exp)
        _l4_all_counters(pm, keys, pk, by)
    assert np.count_nonzero(pk) > 500
    pm.destroy()


@pytest.mark.parametrize("family", [4, 6])
def test_l4_fp_kernel_second_trip(gpu, family):
    """l4_fp_kernel<4/6> (2,048 entries: fingerprints and counters in LDS)
    launches at most cus blocks of 4,096 tuples: one tuple more gives block 0
    a second trip of a single tuple; cus * 4096 fits exactly; a single tuple
    is one block whose other lanes re-read it."""
    cus = _cus()
    case = _ipc_case(2048, family, cus * 4096 + 1)
    keys, ports, ik, iv = case[:4]
    pm = gpu.policy_map(max_entries=16384)
    pm.allow_keys(keys, ports)
    ic = gpu.ipcache()
    ic.update(ik, iv)
    print(f"cus {cus}, n {cus * 4096 + 1}, {cus * 4096}, 1")
    for n in (cus * 4096 + 1, cus * 4096, 1):
        pk = _via_ipcache(gpu, pm, ic, case, n)
        assert int(pk.sum()) <= n
    ic.destroy()
    pm.destroy()


# -------------------------------------------- 7. prefilter, small sizes ----
def test_prefilter_counters_small_sizes(gpu):
    from test_cpu_differential import dense_prefilter_case
    pfx, v4, v6, ep4, ep6 = dense_prefilter_case(0, n=100_003)
    pf = gpu.prefilter(dyn4=True, dyn6=True, max_lpm=1 << 20)
    pf.insert(0, pfx)
    pf.set_endpoints(ep4, ep6)
    for n4, n6 in ((1, 0), (0, 1), (63, 65), (257, 1), (100_003, 50_001)):
        a4, a6 = np.ascontiguousarray(v4[:n4]), np.ascontiguousarray(v6[:n6])
        o4, o6 = oracle.prefilter(pf.config, pfx, ep4, ep6, a4, a6)
        before = gpu.read_counters(N.CG_CTR_PREFILTER, pf.id).copy()
        if not len(before):  # a prefilter's counters exist from its first run on
            before = np.zeros(2, np.uint64)
        g4, g6 = pf.verdicts(a4, a6)
        delta = gpu.read_counters(N.CG_CTR_PREFILTER, pf.id) - before
        assert np.array_equal(g4, o4) and np.array_equal(g6, o6), (n4, n6)
        o = np.concatenate([o4, o6])
        assert delta.tolist() == [int((o == 1).sum()), int((o == 2).sum())], (n4, n6, delta.tolist())
        assert int(delta.sum()) == n4 + n6
    big = np.concatenate(oracle.prefilter(pf.config, pfx, ep4, ep6, v4, v6[:50_001]))
    assert (big == 1).any() and (big == 2).any()
    pf.destroy()
