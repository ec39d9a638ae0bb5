"""counters_util on the CPU: the program the helper reads out of a packed
batch for every request is the program whose rules the host walker
attributes the request to, and the expected per-program vector adds up to
the oracle's totals.  test_counters_gpu.py then holds the kernels' counters
against these helpers element for element."""
import random

import numpy as np
import pytest

import oracle
from cilium_amd import synth
from counters_util import (F_MALFORMED, NO_REQ, batch_header, chunk_table, expected_program_counters, flags_of_slots,
                           kafka_redirect_counters, program_counters, program_of_requests, program_of_slots,
                           rule_groups)
from test_cpu_differential import ID_SETS, _rand_policy, _rand_requests, all_matcher_case

NO_RULE = 0xFFFFFFFF


def _check_helper(host, pols, rq, nthreads=4):
    """The three properties that pin the helper; returns what it saw."""
    host.update_http_policy(pols)
    b = host.pack_http(**rq)
    nprogs = host.http_policy_stats()["programs"]
    v = oracle.HttpOracle(pols).eval(**rq, nthreads=nthreads)
    rprog, rcnt = program_of_requests(b, nprogs)
    exp = expected_program_counters(b, v, nprogs)
    assert exp.dtype == np.uint64 and len(exp) == 2 * nprogs
    assert int(exp.sum()) == int(rcnt.sum())
    assert int(exp[0::2].sum()) == int(v[rcnt].sum())
    # uncounted requests: malformed ones (denied) and those of the special programs ("unknown
    # policy" denies, "no policy for the port" allows what is not malformed)
    order = b.order[:b.nslots]
    bad = np.zeros(b.n, bool)
    bad[order[order != NO_REQ]] = (flags_of_slots(b)[order != NO_REQ] & F_MALFORMED) != 0
    special = rprog >= nprogs
    assert set(np.unique(rprog[special]).tolist()) <= {0xFFFFFFFE, 0xFFFFFFFF}
    assert np.array_equal(rcnt, ~special & ~bad)
    assert np.array_equal(v[~rcnt].astype(bool), (rprog[~rcnt] == 0xFFFFFFFE) & ~bad[~rcnt])
    # the host walker's first matching rule lies in the rule range of the helper's program
    info = host.http_rule_info()
    rule = host.http_rules_host_diag(b)
    hit = rule != NO_RULE
    assert not (hit & ~rcnt).any()  # only counted requests are attributed
    if hit.any():
        group = rule_groups(info)
        ri = info[rule[hit]]
        assert np.array_equal(ri["policy"], rq["policy"][hit])
        assert np.array_equal(ri["ingress"], rq["ingress"][hit])
        assert np.all((ri["port"] == rq["port"][hit]) | (ri["port"] == 0))
        pairs = set(zip(rprog[hit].tolist(), group[rule[hit]].tolist()))
        assert len({p for p, _ in pairs}) == len(pairs) == len({g for _, g in pairs}), \
            "programs and rule ranges are not one to one"
    return b, rprog, rcnt, exp


@pytest.mark.parametrize("ids", sorted(ID_SETS))
@pytest.mark.parametrize("seed", range(100, 106))
def test_helper_random_policies(host, seed, ids):
    rng = random.Random(seed)
    pols = _rand_policy(rng, ids=ID_SETS[ids])
    rq = _rand_requests(rng, 3000, len(pols), ids=ID_SETS[ids])
    b, rprog, rcnt, _ = _check_helper(host, pols, rq)
    # both special programs and malformed records are present: none of them is counted
    assert {0xFFFFFFFE, 0xFFFFFFFF} <= set(np.unique(rprog).tolist())
    assert (~rcnt & (rprog < 0xFFFFFFFE)).any()  # malformed, under a real program
    prog, counted = program_of_slots(b, host.http_policy_stats()["programs"])
    assert len(prog) == b.nslots and int(counted.sum()) == int(rcnt.sum())  # padding slots are not counted


@pytest.mark.parametrize("seed", range(4))
def test_helper_all_matchers(host, seed):
    pols, rq, _ = all_matcher_case(seed, 4000)
    _check_helper(host, pols, rq)


def test_helper_10k(host):
    pols, info = synth.http10k_rules()
    rq = synth.http10k_requests(20_000, info)
    b, rprog, rcnt, exp = _check_helper(host, pols, rq)
    ct = chunk_table(b)
    assert len(ct) == batch_header(b)["nchunks"] and len(np.unique(ct[:, 0])) == 64
    assert rcnt.all() and (exp.reshape(-1, 2).sum(1) > 0).all()  # every program sees requests


def test_program_counters_places_each_count():
    """One request per (program, verdict) cell lands in that cell only."""
    nprogs = 5
    for p in range(nprogs):
        for v in (0, 1):
            got = program_counters(np.array([p, p], np.uint32), np.array([True, False]), np.array([v, v]), nprogs)
            want = np.zeros(2 * nprogs, np.uint64)
            want[2 * p + (1 - v)] = 1
            assert np.array_equal(got, want)


def test_kafka_redirect_counters_places_each_count():
    got = kafka_redirect_counters([0, 1, 1, 2, 0, 65535], [1, 0, 1, 1, 0, 1], 2)
    assert got.tolist() == [1, 1, 1, 1] and got.dtype == np.uint64
    assert kafka_redirect_counters([1, 1, 3], [1, 1, 1], 3).tolist() == [0, 0, 2, 0, 0, 0]
