"""Selector cache on the GPU: selcache_match_kernel and selcache_reach_kernel
against resolve.py (the checks of test_selcache.py through the kernels), one
larger shape that crosses wave, workgroup and selector-chunk tiling against
the library's host walker, the device-pointer entries on a non-default
stream, and table replacement."""
import numpy as np
import pytest

import selcache_util as U
from cilium_amd import resolve as R
from cilium_amd.selcache import unpack_rows

pytestmark = pytest.mark.gpu


@pytest.fixture()
def sc(gpu):
    s = gpu.selector_cache()
    yield s
    s.destroy()


def test_gpu_operator_kat(sc):
    U.check_operator_kat(sc, diag_cpu=False)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_gpu_match_differential(sc, n):
    U.check_match(sc, n, diag_cpu=False)


@pytest.mark.parametrize("case", U.REACH, ids=lambda c: c["case"])
def test_gpu_golden_reach(sc, case):
    U.check_golden_reach(sc, case, diag_cpu=False)


def test_gpu_rule_can_reach(sc):
    U.check_rule_can_reach(sc, diag_cpu=False)


def test_gpu_empty_repository(sc):
    U.check_empty_repository(sc, diag_cpu=False)


@pytest.mark.parametrize("seed", [11, 12])
def test_gpu_reach_random(sc, seed):
    U.check_reach_random(sc, seed, diag_cpu=False)


def test_gpu_map_states_minikube(sc):
    U.check_map_states(sc, U.minikube_repo(), U.MK_CACHE, diag_cpu=False)


# N = 4,099 identities: 65 words, 5 workgroups of 1,024 lanes, the last with
# 3 live lanes in its only live wave; S = 1,031 selectors: several selector
# chunks with a ragged last one; E = 67 endpoints.
BIG_N, BIG_S, BIG_E, BIG_RULES = 4099, 1031, 67, 40


@pytest.fixture(scope="module")
def big():
    cache = U.random_identities(BIG_N, 77)
    sels = U.random_selectors(BIG_S, 78)
    repo = U.random_repository(BIG_RULES, 79)
    rng = np.random.default_rng(80)
    endpoints = [int(e) for e in rng.choice(list(cache), BIG_E, replace=False)]
    return cache, sels, repo, endpoints


def test_gpu_big_shape(sc, big):
    cache, sels, repo, endpoints = big
    sc.set_identities(cache)
    sc.set_repository(repo)
    bits = sc.match(sels)
    assert bits.shape == (BIG_S, 65)
    assert np.array_equal(bits, sc.match(sels, diag_cpu=True, threads=8))
    assert not np.any(bits[:, -1] >> np.uint64(BIG_N % 64))
    # resolve.py on a seeded sample of 20,000 cells
    got = unpack_rows(bits, BIG_N)
    rng = np.random.default_rng(81)
    ss, ii = rng.integers(0, BIG_S, 20000), rng.integers(0, BIG_N, 20000)
    labels = list(cache.values())
    want = np.array([sels[s].matches(labels[i]) for s, i in zip(ss, ii)])
    U.assert_two_sided(want, "sampled match cells")
    assert np.array_equal(got[ss, ii], want)
    # the rule set's own selectors (sels = NULL) and reach, against the host walker
    assert np.array_equal(sc.match(None), sc.match(None, diag_cpu=True, threads=8))
    g = sc.reach(endpoints)
    h = sc.reach(endpoints, diag_cpu=True)
    for a, b in zip(g, h):
        assert np.array_equal(a, b)
    U.assert_two_sided(unpack_rows(g[0], BIG_N), "ingress reach")
    # and resolve.py on a sample of reach cells
    ing, eg = unpack_rows(g[0], BIG_N), unpack_rows(g[1], BIG_N)
    for a, b in zip(rng.integers(0, BIG_E, 300), rng.integers(0, BIG_N, 300)):
        me, peer = cache[endpoints[a]], labels[b]
        assert ing[a, b] == repo.allows_ingress_label_access(peer, me)
        assert eg[a, b] == repo.allows_egress_label_access(me, peer)
    for a in range(BIG_E):
        i_on, e_on = repo.get_rules_matching(cache[endpoints[a]])
        assert g[2][a] == int(i_on) | (int(e_on) << 1)


def test_gpu_dev_entries_on_a_stream(sc, gpu):
    import torch
    cache, sels, want = U.match_case(130)
    rcache, repo, rwant = U.reach_case(11)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        sc.set_identities(cache)
        W = sc.words
        d_bits = torch.full((len(sels) * W,), -1, dtype=torch.int64, device=dev)
        sc.match_dev(sels, d_bits, stream=stream.cuda_stream)
        stream.synchronize()
        bits = d_bits.cpu().numpy().view(np.uint64).reshape(len(sels), W)
        assert np.array_equal(unpack_rows(bits, 130), want)
        assert not np.any(bits[:, -1] >> np.uint64(130 % 64))

        sc.set_identities(rcache)
        sc.set_repository(repo)
        E, W = len(rcache), sc.words
        d_ep = torch.arange(E, dtype=torch.int32, device=dev)
        d_ing = torch.full((E * W,), -1, dtype=torch.int64, device=dev)
        d_eg = torch.full((E * W,), -1, dtype=torch.int64, device=dev)
        d_fl = torch.full((E,), 9, dtype=torch.uint8, device=dev)
        sc.reach_dev(d_ep, E, d_ing, d_eg, d_fl, stream=stream.cuda_stream)
        # the rule set's selectors, into a device matrix
        S = sc.info()["selectors"]
        d_m = torch.full((S * W,), -1, dtype=torch.int64, device=dev)
        sc.match_dev(None, d_m, stream=stream.cuda_stream)
        stream.synchronize()
    n = len(rcache)
    assert np.array_equal(unpack_rows(d_ing.cpu().numpy().view(np.uint64).reshape(E, W), n), rwant[0])
    assert np.array_equal(unpack_rows(d_eg.cpu().numpy().view(np.uint64).reshape(E, W), n), rwant[1])
    assert np.array_equal(d_fl.cpu().numpy(), rwant[2])
    assert np.array_equal(d_m.cpu().numpy().view(np.uint64).reshape(S, W), sc.match(None, diag_cpu=True))


def test_gpu_results_follow_new_tables(sc):
    """set_identities again with another N: every result has the new table's
    shape and content, whichever was larger."""
    for n in (130, 65, 130, 1):
        U.check_match(sc, n, diag_cpu=False)
    U.check_reach_random(sc, 12, diag_cpu=False)
    U.check_rule_can_reach(sc, diag_cpu=False)  # 4 identities after 132
    U.check_reach_random(sc, 11, diag_cpu=False)


def test_gpu_identities_of_matches_resolve(sc):
    cache, sels, _ = U.match_case(130)
    sc.set_identities(cache)
    assert sc.identities_of(sels) == [R.get_security_identities(cache, s) for s in sels]
