"""Shared inputs and checks of test_selcache_expand.py (host walkers,
diag_cpu=True) and test_selcache_expand_gpu.py (kernels): expansion of bitset
rows into policy-map entries against a numpy oracle, the fused
endpoint_policy_map_entries against resolve.endpoint_policy_map_state, and
PolicyMap.sync.  Every comparison is exact.  Oracles are computed once per
shape / seed and shared."""
import functools

import numpy as np

import selcache_util as U
from cilium_amd import _native as N
from cilium_amd import resolve as R
from cilium_amd.classifier import POLICY_KEY_DTYPE
from cilium_amd.policy import PolicyKey, htons
from cilium_amd.selcache import ExpandTable, unpack_rows

# kExpSpan of kernels_selcache.hip: the words of a row one emit round of a
# block covers, one per lane of its 1,024 lanes.  WIDE_N identities need more
# than one round (64 * 1,024 + 65 = 65,601: the second round holds one full
# word and a last word with a single valid bit).
SPAN = 1024
WIDE_N = 64 * SPAN + 65
BOUNDARY_NS = [1, 63, 64, 65, 130]
BIG_N, BIG_ROWS = 4099, 300  # 65 words: one past a wave's 64
PROTOS = (6, 17, 1, 132)
SENTINEL = 0xA5


def unlabelled(n, first_id=5000):
    """n identities without labels: expansion never looks at labels."""
    return {first_id + i: {} for i in range(n)}


def pack_rows(rows: np.ndarray) -> np.ndarray:
    """bool[rows][n] → u64[rows][W], the inverse of unpack_rows."""
    r, n = rows.shape
    w = (n + 63) // 64
    padded = np.zeros((r, w * 64), np.uint8)
    padded[:, :n] = rows
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(r, w).astype(np.uint64)


def random_src(rows, n, densities, seed):
    """src[rows][W]: row r has density densities[r % len]."""
    rng = np.random.default_rng(seed)
    dens = np.asarray([densities[r % len(densities)] for r in range(rows)])[:, None]
    return pack_rows(rng.random((rows, n)) < dens)


def row_of(r, sources, flags=0):
    """Row r with a key template and proxy port of its own, so an entry
    written under the wrong row is seen."""
    return (htons(1000 + r), PROTOS[r % 4], r & 1, htons(20000 + r), flags, list(sources))


def oracle(src, n, ids, rows):
    """Per row the identity numbers it must emit, in order."""
    out = []
    for _, _, _, _, flags, sources in rows:
        if flags & N.CG_EXP_ALL:
            out.append(ids.copy())
            continue
        acc = np.zeros((1, src.shape[1]), np.uint64)
        for s in sources:
            acc |= src[s:s + 1]
        out.append(ids[np.flatnonzero(unpack_rows(acc, n)[0])])
    return out


def assert_entries(rows, want, row_off, keys, proxy):
    lens = [len(w) for w in want]
    assert row_off.tolist() == np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64).tolist()
    assert len(keys) == len(proxy) == sum(lens)
    for r, (row, w) in enumerate(zip(rows, want)):
        lo, hi = int(row_off[r]), int(row_off[r + 1])
        k = keys[lo:hi]
        assert np.array_equal(k["sec_label"], w), f"row {r}: identities"
        assert np.all(k["dport"] == row[0]) and np.all(k["protocol"] == row[1]) and np.all(k["egress"] == row[2]), \
            f"row {r}: key template"
        assert np.all(proxy[lo:hi] == row[3]), f"row {r}: proxy port"


def check_expand(sc, rows, src, n, diag_cpu, threads=1):
    """expand() of `rows` over `src` against the numpy oracle; returns
    (row_off, keys, proxy)."""
    want = oracle(src, n, sc.ids, rows)
    row_off, keys, proxy = sc.expand(ExpandTable(rows), src, diag_cpu=diag_cpu, threads=threads)
    assert_entries(rows, want, row_off, keys, proxy)
    return row_off, keys, proxy


@functools.lru_cache(maxsize=None)
def boundary_case(n):
    """Sources 0-3 random and overlapping, 4 only the first bit, 5 only the
    last valid bit; rows: empty list, ALL, one source, three overlapping
    sources, first bit, last bit, two adjacent empty rows."""
    src = random_src(6, n, (0.5, 0.4, 0.5, 0.6, 0.0, 0.0), 40 + n)
    src[4, 0] = np.uint64(1)
    src[5, (n - 1) // 64] = np.uint64(1) << np.uint64((n - 1) % 64)
    src.setflags(write=False)
    sources = ([], [], [0], [1, 2, 3], [4], [5], [], [])
    rows = tuple(row_of(r, s, N.CG_EXP_ALL if r == 1 else 0) for r, s in enumerate(sources))
    return src, rows


def check_boundary(sc, n, diag_cpu):
    sc.set_identities(unlabelled(n))
    src, rows = boundary_case(n)
    row_off, keys, _ = check_expand(sc, rows, src, n, diag_cpu)
    lens = np.diff(row_off.astype(np.int64))
    assert lens[0] == 0 and lens[1] == n and lens[4] == 1 and lens[5] == 1
    assert row_off[6] == row_off[7] == row_off[8]  # adjacent empty rows share an offset
    assert keys[int(row_off[4])]["sec_label"] == 5000 and keys[int(row_off[5])]["sec_label"] == 5000 + n - 1
    three = keys[int(row_off[3]):int(row_off[4])]["sec_label"]
    assert len(np.unique(three)) == len(three), "an identity of overlapping sources is emitted twice"
    if n > 1:  # the three sources do overlap, and their union is not everything
        u = unpack_rows(src[1:4], n)
        assert np.any(u.sum(axis=0) > 1)


def check_no_rows(sc, diag_cpu):
    sc.set_identities(unlabelled(70))
    row_off, keys, proxy = sc.expand(ExpandTable([]), np.zeros((0, sc.words), np.uint64), diag_cpu=diag_cpu)
    assert row_off.tolist() == [0] and len(keys) == 0 and len(proxy) == 0
    # rows that select nothing: total = 0
    rows = [row_of(0, []), row_of(1, [0])]
    row_off, keys, _ = check_expand(sc, rows, np.zeros((1, sc.words), np.uint64), 70, diag_cpu)
    assert row_off.tolist() == [0, 0, 0] and len(keys) == 0


def sentinel_buffers(cap):
    keys = np.frombuffer(bytes([SENTINEL]) * (8 * cap), POLICY_KEY_DTYPE).copy()
    return keys, np.full(cap, SENTINEL * 0x0101, np.uint16)


def check_padding_ones(sc, n, diag_cpu):
    """Source padding bits all ones: exactly the n identities, nothing past
    them in the buffers."""
    sc.set_identities(unlabelled(n))
    src = np.full((2, sc.words), ~np.uint64(0), np.uint64)
    rows = [row_of(0, [0]), row_of(1, [0, 1])]
    keys, proxy = sentinel_buffers(2 * n + 64)
    row_off, total = sc.expand_into(ExpandTable(rows), src, keys, proxy, diag_cpu=diag_cpu)
    assert total == 2 * n and row_off.tolist() == [0, n, 2 * n]
    assert np.array_equal(keys[:n]["sec_label"], sc.ids) and np.array_equal(keys[n:2 * n]["sec_label"], sc.ids)
    s_keys, s_proxy = sentinel_buffers(64)
    assert keys[2 * n:].tobytes() == s_keys.tobytes() and np.array_equal(proxy[2 * n:], s_proxy)


@functools.lru_cache(maxsize=None)
def big_case():
    """300 rows over 4,099 identities at densities 0.01 / 0.5 / 0.99; every
    seventh row ORs its neighbour in."""
    src = random_src(BIG_ROWS, BIG_N, (0.01, 0.5, 0.99), 91)
    src.setflags(write=False)
    rows = tuple(row_of(r, [r, (r + 1) % BIG_ROWS] if r % 7 == 0 else [r]) for r in range(BIG_ROWS))
    return src, rows


def check_big(sc, diag_cpu):
    sc.set_identities(unlabelled(BIG_N))
    src, rows = big_case()
    return check_expand(sc, rows, src, BIG_N, diag_cpu, threads=4)


@functools.lru_cache(maxsize=None)
def wide_case():
    src = random_src(4, WIDE_N, (0.5, 0.01, 0.0, 0.0), 92)
    src[2, 0] = np.uint64(1)
    src[3, (WIDE_N - 1) // 64] = np.uint64(1) << np.uint64((WIDE_N - 1) % 64)
    src.setflags(write=False)
    rows = (row_of(0, [0]), row_of(1, [2]), row_of(2, [], N.CG_EXP_ALL), row_of(3, [3]), row_of(4, [0, 1]),
            row_of(5, []))
    return src, rows


def check_wide(sc, diag_cpu):
    sc.set_identities(unlabelled(WIDE_N))
    assert sc.words == SPAN + 2
    src, rows = wide_case()
    row_off, keys, _ = check_expand(sc, rows, src, WIDE_N, diag_cpu, threads=4)
    assert keys[int(row_off[3])]["sec_label"] == 5000 + WIDE_N - 1  # the last valid bit, in the second round


def check_cap(sc, diag_cpu):
    n = 130
    sc.set_identities(unlabelled(n))
    src, rows = boundary_case(n)
    tab = ExpandTable(rows)
    want_off, want_keys, want_proxy = sc.expand(tab, src, diag_cpu=diag_cpu)
    total = len(want_keys)
    assert total > 1
    keys, proxy = sentinel_buffers(total - 1)
    row_off, got = sc.expand_into(tab, src, keys, proxy, diag_cpu=diag_cpu)
    s_keys, s_proxy = sentinel_buffers(total - 1)
    assert got == total and np.array_equal(row_off, want_off)
    assert keys.tobytes() == s_keys.tobytes() and np.array_equal(proxy, s_proxy)
    keys, proxy = sentinel_buffers(total)
    row_off, got = sc.expand_into(tab, src, keys, proxy, diag_cpu=diag_cpu)
    assert got == total and np.array_equal(row_off, want_off)
    assert np.array_equal(keys, want_keys) and np.array_equal(proxy, want_proxy)
    assert_entries(rows, oracle(src, n, sc.ids, rows), row_off, keys, proxy)


def check_bad_source_index(sc, diag_cpu):
    sc.set_identities(unlabelled(70))
    src = np.zeros((2, sc.words), np.uint64)
    import pytest
    for bad in ([2], [0, 7]):
        with pytest.raises(N.CiliumGPUError) as ei:
            sc.expand(ExpandTable([row_of(0, [0]), row_of(1, bad)]), src, diag_cpu=diag_cpu)
        assert ei.value.code == N.CG_INVALID_ARGUMENT


# ------------------------------------------------------ against resolve.py --
MODES = ("default", "always", "never")
STATE_CASES = ("minikube", 11, 12)


def entries_to_dict(keys, proxy_be):
    """Raw entries in order → the dict resolve.py builds (host byte order);
    a repeated key takes its last value, as dict assignment does."""
    return {PolicyKey(int(k["sec_label"]), htons(int(k["dport"])), int(k["protocol"]), int(k["egress"])): htons(int(p))
            for k, p in zip(keys, proxy_be)}


@functools.lru_cache(maxsize=None)
def state_inputs(case):
    """(identity cache, repository) of a case: minikube, or the 132-identity
    cache of reach_case(seed) with a 40-rule repository with L7 rules."""
    if case == "minikube":
        return U.MK_CACHE, U.minikube_repo()
    cache = U.random_identities(130, 900 + case)  # as U.reach_case builds it, without its reach oracle
    cache[1] = {"reserved:host": ""}
    cache[2] = {"reserved:world": ""}
    return cache, U.random_repository(40, case, l7=True, cfg=R.PolicyConfig())


@functools.lru_cache(maxsize=None)
def state_oracle(case, mode, redirects):
    """resolve.endpoint_policy_map_state per endpoint (a few seconds for the
    seeded cases: computed once and shared by the CPU and the GPU test)."""
    cache, repo = state_inputs(case)
    mode0 = repo.cfg.enforcement
    repo.cfg.enforcement = mode
    try:
        return tuple(R.endpoint_policy_map_state(repo, cache[e], cache, U.REDIRECTS if redirects else None)
                     for e in cache)
    finally:
        repo.cfg.enforcement = mode0


def assert_oracle_is_mixed(case):
    """The seeded oracle (default mode, with redirects) is no all-or-nothing
    result: of its rows — the (port, protocol, direction) groups of each
    endpoint's state plus the L3 rows that came out empty — at least 10% hold
    some but not all identities; it has redirect entries; and some endpoint
    is unenforced in a direction."""
    cache, repo = state_inputs(case)
    n, rows, partial, redirects = len(cache), 0, 0, 0
    for state in state_oracle(case, "default", True):
        groups = {}
        for k, proxy in state.items():
            groups[(k.DestPort, k.Nexthdr, k.TrafficDirection)] = groups.get(
                (k.DestPort, k.Nexthdr, k.TrafficDirection), 0) + 1
            redirects += proxy != 0
        rows += len(groups) + sum((0, 0, d) not in groups for d in (0, 1))
        partial += sum(0 < c < n for c in groups.values())
    assert partial >= 0.10 * rows, f"{partial} of {rows} rows are partial"
    assert redirects >= 1
    assert any(not all(R.compute_policy_enforcement(repo, cache[e])) for e in cache)


def check_states(sc, case, mode, redirects, diag_cpu):
    cache, repo = state_inputs(case)
    want = state_oracle(case, mode, redirects)
    if case != "minikube" and mode == "default" and redirects:
        assert_oracle_is_mixed(case)
    sc.set_identities(cache)
    sc.set_repository(repo)
    mode0 = repo.cfg.enforcement
    repo.cfg.enforcement = mode
    try:
        got = sc.endpoint_policy_map_entries(list(cache), U.REDIRECTS if redirects else None, diag_cpu=diag_cpu)
    finally:
        repo.cfg.enforcement = mode0
    assert len(got) == len(want)
    for e, (keys, proxy), w in zip(cache, got, want):
        assert keys.dtype == POLICY_KEY_DTYPE and proxy.dtype == np.uint16 and len(keys) == len(proxy)
        assert entries_to_dict(keys, proxy) == w, (case, mode, redirects, e)


# ------------------------------------------------------------ PolicyMap.sync --
def raw_keys(tuples):
    """[(identity, dport host order, proto, egress)] → raw map keys."""
    a = np.zeros(len(tuples), POLICY_KEY_DTYPE)
    for i, (ident, port, proto, eg) in enumerate(tuples):
        a[i] = (ident, htons(port), proto, eg)
    return a


def dump_dict(pm):
    """{raw key tuple: proxy port as stored} of a map's dump."""
    return {(k.Identity, k.DestPort, k.Nexthdr, k.TrafficDirection): e.ProxyPort for k, e in pm.dump_to_slice()}
