"""Shared inputs and checks of test_selcache_tiles.py (host walkers,
diag_cpu=True) and test_selcache_tiles_gpu.py (kernels): the shapes at which
the selector-cache kernels and their launchers take a second trip — a second
LDS tile of rules, a second block column of words, a second reach launch, the
label scan past the staged labels, long value sets and requirement lists, a
second scan chunk and the grid strides of count and emit.  Every comparison
is exact.  Inputs and oracles are computed once per shape and shared.

Shapes that depend on the device take the CU count as `cus`; the CPU twin
passes CPU_CUS."""
import functools

import numpy as np

import selcache_expand_util as X
import selcache_util as U
from cilium_amd import _native as N
from cilium_amd import resolve as R
from cilium_amd.selcache import ExpandTable, unpack_rows

Sel = U.Sel
CPU_CUS = 256

# Constants of kernels_selcache.hip the shapes below are built around.
REACH_TILE = 4096     # kReachTile: rules per LDS tile of selcache_reach_kernel
REACH_THREADS = 256   # kReachThreads: words per block column
REACH_LAUNCH = 65535  # endpoints per launch of launch_selcache_reach
MATCH_THREADS = 1024  # kMatchThreads: identities per block column
MATCH_CHUNK = 256     # kMatchChunk: selectors per block at most
SC_FAST = 8           # kScFast: labels staged in registers per identity
SCAN_THREADS = 1024   # kScanThreads: rows per chunk of selcache_expand_scan_kernel


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


# ---------------------------------------- 1. reach over more than one tile --
TILE_N = 130
TILE_RULES = (REACH_TILE, REACH_TILE + 1, REACH_TILE + 70)
NAMED = (0, 63, 64, REACH_TILE - 1, REACH_TILE, REACH_TILE + 1)  # and the last rule
FILLED = 100           # endpoints 0-99 carry the filler rules
# Endpoints of the cross-tile cases (only at 4,166 rules); 115-129 are peers only.
EP_A, EP_B, EP_ING, EP_EG, EP_NONE = 110, 111, 112, 113, 114
TILE_SAMPLE = 175      # sampled cells; each costs one ingress and one egress call of resolve.py


def _id(n):
    return Sel({"k8s:id": f"i{n}"})


def _grp(g):
    return Sel({"k8s:grp": f"g{g % 3}"})


def _not_id(n):
    return Sel(None, [("k8s:id", "NotIn", (f"i{n}",))])


def _peer_in_group(g, k):
    """The k-th identity of 115-129 (peers only) in group g % 3."""
    return [n for n in range(115, TILE_N) if n % 3 == g % 3][k]


@functools.lru_cache(maxsize=None)
def tile_repository(n_rules):
    """(cache, repository, named) where the rule index decides the outcome.

    Identity n is {k8s:id=i<n>, k8s:grp=g<n % 3>}.  Rule r is a filler unless
    named below: its subject is endpoint e = r % 100 and it allows group
    g<e> on ingress and g<e + 1> on egress, so about a third of each of the
    rows 0-99 is set, by rules of every mask word of either tile.

    Named rule number j (rule index k of NAMED, or the last rule) has subject
    endpoint j and allows one identity of group g<j + 2> each way — a group
    no filler of endpoint j allows — so the cell is this rule's alone.

    At 4,166 rules, additionally (t0 = a rule of tile 0, t1 = of tile 1):
      EP_A:  t0 allows peers P and Q, t1 requires "not P": P denied across tiles;
      EP_B:  t1 allows peers P and Q, t0 requires "not P": the converse;
      EP_ING: selected by two t1 rules with ingress rules only (flags 1);
      EP_EG:  selected by two t1 rules with egress rules only (flags 2);
      EP_NONE: selected by no rule (zero rows, flags 0).

    named: {"alone": [(dir, endpoint, peer, rule index)],
            "cells": [(dir, endpoint, peer, allowed)], "flags": {endpoint: flags}}.
    """
    cache = {3000 + n: {"k8s:id": f"i{n}", "k8s:grp": f"g{n % 3}"} for n in range(TILE_N)}
    special, alone, cells, flags = {}, [], [], {}
    for j, k in enumerate(sorted({*(k for k in NAMED if k < n_rules), n_rules - 1})):
        pi, pe = _peer_in_group(j + 2, 0), _peer_in_group(j + 2, 1)
        special[k] = R.Rule(_id(j), [R.IngressRule([_id(pi)])], [R.EgressRule([_id(pe)])])
        alone += [(0, j, pi, k), (1, j, pe, k)]
        cells += [(0, j, pi, True), (1, j, pe, True), (0, j, pe, False), (1, j, pi, False)]
        flags[j] = 3
    if n_rules > REACH_TILE + 16:
        t0, t1 = 100, REACH_TILE + 4
        P, Q = 120, 121
        allow = lambda: ([R.IngressRule([_id(P), _id(Q)])], [R.EgressRule([_id(P), _id(Q)])])  # noqa: E731
        require = lambda: ([R.IngressRule([], [_not_id(P)])], [R.EgressRule([], [_not_id(P)])])  # noqa: E731
        special[t0] = R.Rule(_id(EP_A), *allow())
        special[t1] = R.Rule(_id(EP_A), *require())
        special[t1 + 1] = R.Rule(_id(EP_B), *allow())
        special[t0 + 1] = R.Rule(_id(EP_B), *require())
        for ep in (EP_A, EP_B):
            cells += [(d, ep, P, False) for d in (0, 1)] + [(d, ep, Q, True) for d in (0, 1)]
            flags[ep] = 3
        for k in (t1 + 2, t1 + 10):
            special[k] = R.Rule(_id(EP_ING), [R.IngressRule([_grp(k)])], [])
            special[k + 1] = R.Rule(_id(EP_EG), [], [R.EgressRule([_grp(k)])])
        peer = _peer_in_group(t1 + 2, 2)
        cells += [(0, EP_ING, peer, True), (1, EP_ING, peer, False), (1, EP_EG, peer, True), (0, EP_EG, peer, False),
                  (0, EP_NONE, 115, False), (1, EP_NONE, 116, False)]
        flags.update({EP_ING: 1, EP_EG: 2, EP_NONE: 0})
    rules = []
    for r in range(n_rules):
        e = r % FILLED
        rules.append(special.get(r) or R.Rule(_id(e), [R.IngressRule([_grp(e)])], [R.EgressRule([_grp(e + 1)])]))
    return cache, R.Repository(rules), {"alone": alone, "cells": cells, "flags": flags}


def _allows(repo, labels, d, e, p):
    return repo.allows_egress_label_access(labels[e], labels[p]) if d else \
        repo.allows_ingress_label_access(labels[p], labels[e])


@functools.lru_cache(maxsize=None)
def tile_oracle(n_rules):
    """resolve.py on the named cells and on TILE_SAMPLE seeded cells in both
    directions (about 400 calls at ~6 ms each over 4,166 rules; the whole
    130 x 130 matrix would take minutes).  Asserts what the construction
    promises before anything is compared with it.  Returns
    (dir[], endpoint[], peer[], allowed[]) over all checked cells and
    {endpoint: flags}."""
    cache, repo, named = tile_repository(n_rules)
    labels = list(cache.values())
    for d, e, p, k in named["alone"]:
        assert _allows(repo, labels, d, e, p), f"rule {k} does not allow its cell"
        without = R.Repository()
        without.rules = repo.rules[:k] + repo.rules[k + 1:]
        assert not _allows(without, labels, d, e, p), f"rule {k} is not alone in allowing its cell"
    for d, e, p, want in named["cells"]:
        assert _allows(repo, labels, d, e, p) == want, f"named cell {(d, e, p)}"
    for e, want in named["flags"].items():
        i_on, e_on = repo.get_rules_matching(labels[e])
        assert int(i_on) | (int(e_on) << 1) == want, f"flags of endpoint {e}"
    rng = np.random.default_rng(500 + n_rules)
    se, sp = rng.integers(0, TILE_N, TILE_SAMPLE), rng.integers(0, TILE_N, TILE_SAMPLE)
    sampled = [(d, int(e), int(p), _allows(repo, labels, d, int(e), int(p))) for e, p in zip(se, sp) for d in (0, 1)]
    U.assert_two_sided(np.array([c[3] for c in sampled]), f"sampled reach cells, {n_rules} rules")
    out = tuple(np.array(col) for col in zip(*(named["cells"] + sampled)))
    _freeze(*out)
    return out, dict(named["flags"])


def check_reach_tiles(sc, n_rules, diag_cpu):
    cache, repo, _ = tile_repository(n_rules)
    (d, e, p, want), flags = tile_oracle(n_rules)
    sc.set_identities(cache)
    sc.set_repository(repo)
    assert sc.info()["rules"] == n_rules
    got = sc.reach(list(cache), diag_cpu=diag_cpu)
    ref = got if diag_cpu else sc.reach(list(cache), diag_cpu=True)
    for g, r, what in zip(got, ref, ("ingress", "egress", "flags")):
        assert np.array_equal(g, r), f"{what}: the kernel and the host walker differ"
    both = np.stack([unpack_rows(got[0], TILE_N), unpack_rows(got[1], TILE_N)])
    cells = both[d, e, p]
    bad = np.flatnonzero(cells != want)
    assert bad.size == 0, f"(direction, endpoint, peer, allowed) {[(d[i], e[i], p[i], want[i]) for i in bad[:8]]}"
    assert {k: int(got[2][k]) for k in flags} == flags
    assert not np.any(got[0][:, -1] >> np.uint64(TILE_N % 64)) and not np.any(got[1][:, -1] >> np.uint64(TILE_N % 64))
    if EP_NONE in flags:
        assert not both[:, EP_NONE].any()


# ------------------------- 2. reach and match wider than one block column --
WIDE_IDS = REACH_THREADS * 64 + 65  # 16,449: 258 words; the second reach block has two live words,
#                                     the last with one valid bit
WIDE_EPS = (0, 255 * 64 + 17, 256 * 64 + 3, 9000, WIDE_IDS - 1)  # bit 0, words 255 and 256, the last bit
WIDE_COLS = (16383, 16384, 16447, 16448)


@functools.lru_cache(maxsize=None)
def wide_cache():
    return U.random_identities(WIDE_IDS, 61)


@functools.lru_cache(maxsize=None)
def wide_reach_case():
    """(repository, cell rows, cell columns, ingress[], egress[], flags[5])
    from resolve.py: 300 sampled cells and the WIDE_COLS of every endpoint."""
    cache = wide_cache()
    repo = U.random_repository(40, 65)
    ids, labels = list(cache), list(cache.values())
    rng = np.random.default_rng(62)
    a = np.concatenate([rng.integers(0, len(WIDE_EPS), 300), np.repeat(np.arange(len(WIDE_EPS)), len(WIDE_COLS))])
    b = np.concatenate([rng.integers(0, WIDE_IDS, 300), np.tile(WIDE_COLS, len(WIDE_EPS))])
    ing = np.array([repo.allows_ingress_label_access(labels[j], labels[WIDE_EPS[i]]) for i, j in zip(a, b)])
    eg = np.array([repo.allows_egress_label_access(labels[WIDE_EPS[i]], labels[j]) for i, j in zip(a, b)])
    fl = np.array([int(i_on) | (int(e_on) << 1) for i_on, e_on in
                   (repo.get_rules_matching(labels[e]) for e in WIDE_EPS)], np.uint8)
    _freeze(a, b, ing, eg, fl)
    return repo, [ids[e] for e in WIDE_EPS], a, b, ing, eg, fl


def check_reach_wide(sc, diag_cpu):
    repo, endpoints, a, b, ing_want, eg_want, fl_want = wide_reach_case()
    U.assert_two_sided(ing_want, "sampled ingress cells, N=16,449")
    U.assert_two_sided(eg_want, "sampled egress cells, N=16,449")
    assert len(set(fl_want.tolist())) > 1
    sc.set_identities(wide_cache())
    sc.set_repository(repo)
    assert sc.words == REACH_THREADS + 2
    got = sc.reach(endpoints, diag_cpu=diag_cpu)
    ref = got if diag_cpu else sc.reach(endpoints, diag_cpu=True)
    for g, r, what in zip(got, ref, ("ingress", "egress", "flags")):
        assert np.array_equal(g, r), f"{what}: the kernel and the host walker differ"
    ing, eg = unpack_rows(got[0], WIDE_IDS), unpack_rows(got[1], WIDE_IDS)
    assert np.array_equal(ing[a, b], ing_want)
    assert np.array_equal(eg[a, b], eg_want)
    assert np.array_equal(got[2], fl_want)
    pad = np.uint64(WIDE_IDS % 64)
    assert not np.any(got[0][:, -1] >> pad) and not np.any(got[1][:, -1] >> pad), "padding bits of word 257 are set"


def match_chunk(n, s, cus):
    """The selectors per block launch_selcache_match ends at."""
    gx = (n + MATCH_THREADS - 1) // MATCH_THREADS
    chunk = MATCH_CHUNK
    while chunk > 16 and gx * ((s + chunk - 1) // chunk) < 4 * max(cus, 1):
        chunk >>= 1
    while (s + chunk - 1) // chunk > 65535:
        chunk <<= 1
    return chunk


def wide_match_selectors(cus):
    """S for which the launcher stops halving its chunk at 32, not 16, with a
    last chunk of 5 selectors: N = 16,449 gives gx = 17 block columns, and
    the chunk stays at 32 once 17 * ceil(S / 32) >= 4 * CUs.  The smallest
    such S with S % 32 == 5 is (ceil(4 * CUs / 17) - 1) * 32 + 5: 1,925 at
    256 CUs (17 * 61 = 1,037 >= 1,024, while at a chunk of 64 there are
    17 * 31 = 527 blocks, so 64 is halved)."""
    gx = (WIDE_IDS + MATCH_THREADS - 1) // MATCH_THREADS
    s = ((4 * cus + gx - 1) // gx - 1) * 32 + 5
    assert match_chunk(WIDE_IDS, s, cus) == 32 and s % 32 == 5, "the launcher's chunk arithmetic has changed"
    return s


@functools.lru_cache(maxsize=None)
def wide_match_case(s):
    """(selectors, sampled rows, sampled columns, sel.matches on them)."""
    labels = list(wide_cache().values())
    sels = U.random_selectors(s, 63)
    rng = np.random.default_rng(64)
    ss, ii = rng.integers(0, s, 20000), rng.integers(0, WIDE_IDS, 20000)
    want = np.array([sels[a].matches(labels[b]) for a, b in zip(ss, ii)])
    _freeze(ss, ii, want)
    return sels, ss, ii, want


def check_match_wide(sc, cus, diag_cpu):
    s = wide_match_selectors(cus)
    sels, ss, ii, want = wide_match_case(s)
    U.assert_two_sided(want, "sampled match cells, N=16,449")
    sc.set_identities(wide_cache())
    bits = sc.match(sels, diag_cpu=diag_cpu, threads=8)
    assert bits.shape == (s, REACH_THREADS + 2)
    if not diag_cpu:
        assert np.array_equal(bits, sc.match(sels, diag_cpu=True, threads=8)), "the kernel and the host walker differ"
    assert not np.any(bits[:, -1] >> np.uint64(WIDE_IDS % 64))
    assert np.array_equal(unpack_rows(bits, WIDE_IDS)[ss, ii], want)


# --------------------------------------- 3. more endpoints than one launch --
MANY_N, MANY_E = 70, REACH_LAUNCH + 5
SPLIT_ROWS = (REACH_LAUNCH - 1, REACH_LAUNCH, REACH_LAUNCH + 1, MANY_E - 1)


@functools.lru_cache(maxsize=None)
def many_endpoints_case():
    cache = U.random_identities(MANY_N, 71)
    repo = U.random_repository(40, 72)
    want = U.oracle_reach(repo, cache, list(cache))
    eps = np.random.default_rng(73).permutation(np.arange(MANY_E) % MANY_N).astype(np.uint32)
    _freeze(eps, *want)
    return cache, repo, eps, want


def check_reach_many_endpoints(sc, diag_cpu):
    cache, repo, eps, (ing_want, eg_want, fl_want) = many_endpoints_case()
    U.assert_two_sided(ing_want, "ingress reach, N=70")
    U.assert_two_sided(eg_want, "egress reach, N=70")
    assert len(set(fl_want.tolist())) > 1
    # the rows on either side of the split belong to different identities with different rows
    assert len({ing_want[eps[a]].tobytes() + eg_want[eps[a]].tobytes() for a in SPLIT_ROWS}) > 1
    sc.set_identities(cache)
    sc.set_repository(repo)
    ing, eg, fl = sc.reach_indices(eps, diag_cpu=diag_cpu, threads=8)
    assert ing.shape == eg.shape == (MANY_E, 2) and fl.shape == (MANY_E,)
    ing, eg = unpack_rows(ing, MANY_N), unpack_rows(eg, MANY_N)
    for a in SPLIT_ROWS:
        assert np.array_equal(ing[a], ing_want[eps[a]]), f"ingress row {a}"
        assert np.array_equal(eg[a], eg_want[eps[a]]), f"egress row {a}"
        assert fl[a] == fl_want[eps[a]], f"flags of row {a}"
    assert np.array_equal(ing, ing_want[eps])
    assert np.array_equal(eg, eg_want[eps])
    assert np.array_equal(fl, fl_want[eps])


# --------------------------- 4. an empty identity table (host-visible part) --
def check_empty_table(sc, diag_cpu):
    """set_identities({}): W = 0 everywhere, and the handle serves a real
    table afterwards."""
    _, repo, _ = U.reach_case(11)
    sc.set_repository(repo)
    sc.set_identities({})
    assert sc.words == 0 and sc.info()["identities"] == 0
    sels = U.random_selectors(5, 1)
    assert sc.match(sels, diag_cpu=diag_cpu).shape == (5, 0)
    assert sc.match(None, diag_cpu=diag_cpu).shape == (sc.info()["selectors"], 0)
    assert sc.identities_of([R.WILDCARD], diag_cpu=diag_cpu) == [[]]
    rows = [X.row_of(0, []), X.row_of(1, [], N.CG_EXP_ALL), X.row_of(2, [])]
    row_off, keys, proxy = sc.expand(ExpandTable(rows), np.zeros((0, 0), np.uint64), diag_cpu=diag_cpu)
    assert row_off.tolist() == [0, 0, 0, 0] and len(keys) == 0 and len(proxy) == 0
    ing, eg, fl = sc.reach_indices(np.zeros(0, np.uint32), diag_cpu=diag_cpu)
    assert ing.shape == eg.shape == (0, 0) and fl.shape == (0,)


# ------- 5. match: long identities, long value sets, many requirements --
LONG_N = 130
LABEL_COUNTS = (0, 1, 7, 8, 9, 10, 16, 40)
HAND_AT = {"staged wins": 20, "first unstaged wins": 21, "last staged": 22, "eight, no hit": 90, "ninth hits": 91}


def _fill(j):
    return (f"k8s:fill{j}", "x")


def _hand(n, at, wave):
    """n labels: fillers, the wave label first, and `at` {index: (key, value)}."""
    items = [_fill(j) for j in range(n)]
    items[0] = ("k8s:wave", f"w{wave}")
    for i, kv in at.items():
        items[i] = kv
    assert len(dict(items)) == n
    return dict(items)


HAND = {
    "staged wins": _hand(12, {2: ("k8s:app", "a"), 11: ("container:app", "b")}, 0),
    "first unstaged wins": _hand(14, {8: ("k8s:app", "a"), 12: ("container:app", "c")}, 0),
    "last staged": _hand(12, {7: ("k8s:app", "b")}, 0),
    "eight, no hit": _hand(8, {}, 1),
    "ninth hits": _hand(9, {8: ("k8s:app", "c")}, 1),
}
_EXISTS = Sel(None, [("app", "Exists", ())])
_ABSENT = Sel(None, [("app", "DoesNotExist", ())])
# (hand-written identity, selector, matches): LabelArray.Get returns the first
# label in the identity's order that the key's source admits.
LONG_KAT = [
    ("staged wins", Sel({"any:app": "a"}), True),
    ("staged wins", Sel({"any:app": "b"}), False),
    ("staged wins", Sel({"container:app": "b"}), True),
    ("staged wins", Sel({"k8s:app": "a"}), True),
    ("first unstaged wins", Sel({"any:app": "a"}), True),
    ("first unstaged wins", Sel({"any:app": "c"}), False),
    ("first unstaged wins", Sel({"container:app": "c"}), True),
    ("first unstaged wins", Sel(None, [("app", "In", ("c",))]), False),
    ("last staged", Sel({"any:app": "b"}), True),
    ("last staged", Sel({"any:app": "a"}), False),
    ("last staged", _EXISTS, True),
    ("last staged", _ABSENT, False),
    ("eight, no hit", _EXISTS, False),
    ("eight, no hit", _ABSENT, True),
    ("eight, no hit", Sel(None, [("app", "NotIn", ("a",))]), True),
    ("ninth hits", Sel({"any:app": "c"}), True),
    ("ninth hits", _EXISTS, True),
    ("ninth hits", _ABSENT, False),
    ("ninth hits", Sel({"any:app": "a"}), False),
]


@functools.lru_cache(maxsize=None)
def long_cache():
    """130 identities whose label counts cycle through LABEL_COUNTS (offset so
    that the two identities of the ragged third wave have 8 and 9 labels):
    k8s:wave=w<wave>, deciding pairs of U.PAIRS and k8s:fill<j> fillers in a
    seeded random order, so deciding labels fall on either side of the staged
    ones; HAND replaces five of them."""
    rng = np.random.default_rng(51)
    cache = {}
    for i in range(LONG_N):
        c = LABEL_COUNTS[(i + 3) % len(LABEL_COUNTS)]
        items = [("k8s:wave", f"w{i // 64}")][:c]
        d = min(c - len(items), int(rng.integers(2, len(U.PAIRS) + 1)))
        items += [(U.PAIRS[p], U.VALUES[int(rng.integers(0, 3))]) for p in rng.permutation(len(U.PAIRS))[:d]]
        items += [_fill(j) for j in range(c - len(items))]
        cache[7000 + i] = dict(items[j] for j in rng.permutation(c))
    by_index = list(cache)
    for name, at in HAND_AT.items():
        cache[by_index[at]] = HAND[name]
    counts = [len(v) for v in cache.values()]
    for wave in (counts[:64], counts[64:128], counts[128:]):
        assert SC_FAST in wave and SC_FAST + 1 in wave
    for wave in (counts[:64], counts[64:128]):  # diverging tail lengths inside one wave
        assert len({c for c in wave if c > SC_FAST}) >= 4
    return cache


def _values(n, hit, where):
    """n values that no identity carries, with `hit` first, last or absent."""
    vals = [f"none{j}" for j in range(n)]
    if where == "first":
        vals[0] = hit
    elif where == "last":
        vals[-1] = hit
    return tuple(vals)


def _six(last):
    return Sel(None, [(k, "Exists", ()) for k in ("app", "tier", "env", "zone", "k8s:fill0")] + [last])


SIX_TRUE = _six(("k8s:fill1", "Exists", ()))
SIX_LAST_FAILS = _six(("k8s:fill1", "In", ("y",)))
FIVE = Sel(None, [(k, "Exists", ()) for k in ("app", "tier", "env", "zone", "k8s:fill0")])
# fails its first requirement for every identity of wave 0 (their wave label,
# where they have one, is w0) and holds for most of wave 1
WAVE0_FAILS_FIRST = Sel(None, [("k8s:wave", "In", ("w1", "w2")), ("app", "Exists", ())])
AFTER_EARLY_EXIT = (Sel(), Sel({"k8s:wave": "w0"}))


@functools.lru_cache(maxsize=None)
def long_match_case():
    """(cache, selectors, oracle bool[S][130], rows of LONG_KAT's selectors)."""
    cache = long_cache()
    sels = U.random_selectors(60, 52)
    sels += [SIX_TRUE, SIX_LAST_FAILS]
    for n in (33, 70):
        for op in ("In", "NotIn"):
            for where in ("first", "last", "absent"):
                sels.append(Sel(None, [("app", op, _values(n, "a", where))]))
    sels.append(Sel(None, [("app", "In", ("b", "b", "a", "b"))]))
    sels += [WAVE0_FAILS_FIRST, *AFTER_EARLY_EXIT]
    kat_rows = []
    for _, sel, _ in LONG_KAT:
        kat_rows.append(len(sels))
        sels.append(sel)
    want = np.array([[s.matches(lbls) for lbls in cache.values()] for s in sels], bool)
    _freeze(want)
    return cache, sels, want, kat_rows


def check_match_long(sc, diag_cpu):
    cache, sels, want, kat_rows = long_match_case()
    U.assert_two_sided(want, "match over long identities")
    labels = list(cache.values())
    # what the added selectors promise, on the oracle
    row = {s: want[sels.index(s)] for s in (SIX_TRUE, SIX_LAST_FAILS, WAVE0_FAILS_FIRST, *AFTER_EARLY_EXIT)}
    five = np.array([FIVE.matches(lbls) for lbls in labels])
    assert row[SIX_TRUE].any() and not row[SIX_TRUE].all()
    assert np.any(five & ~row[SIX_LAST_FAILS]) and not row[SIX_LAST_FAILS].any()
    assert not row[WAVE0_FAILS_FIRST][:64].any() and row[WAVE0_FAILS_FIRST][64:128].any()
    assert not any(Sel(None, [("k8s:wave", "In", ("w1", "w2"))]).matches(lbls) for lbls in labels[:64])
    assert sels[sels.index(WAVE0_FAILS_FIRST) + 1:][:2] == list(AFTER_EARLY_EXIT)
    assert row[AFTER_EARLY_EXIT[0]].all() and row[AFTER_EARLY_EXIT[1]][:64].sum() > 32
    for n in (33, 70):  # first / last hit, absent never does
        for op, hit in (("In", True), ("NotIn", False)):
            for where in ("first", "last", "absent"):
                r = want[sels.index(Sel(None, [("app", op, _values(n, "a", where))]))]
                a = np.array([R._label_get(lbls, "app") == "a" for lbls in labels])
                assert a.any() and np.array_equal(r[a], np.full(a.sum(), hit if where != "absent" else not hit))
    by_index = list(cache)
    for (name, sel, expect), r in zip(LONG_KAT, kat_rows):
        assert sel.matches(HAND[name]) == expect, f"oracle disagrees with the table: {name}, {sel}"
        assert bool(want[r, HAND_AT[name]]) == expect

    sc.set_identities(cache)
    bits = sc.match(sels, diag_cpu=diag_cpu)
    assert bits.shape == (len(sels), 3)
    got = unpack_rows(bits, LONG_N)
    for (name, sel, expect), r in zip(LONG_KAT, kat_rows):
        assert bool(got[r, HAND_AT[name]]) == expect, f"{name}: {sel}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"(selector, identity) {bad[:8].tolist()}: {sels[bad[0][0]]} on {labels[bad[0][1]]}"
    assert not np.any(bits[:, -1] >> np.uint64(LONG_N % 64))
    assert by_index[HAND_AT["ninth hits"]] in sc.identities_of([Sel({"any:app": "c"})], diag_cpu=diag_cpu)[0]


# --- 6. expansion: more rows than a scan chunk and than either grid --
EXP_N, EXP_SRC = 130, 64
EXP_DENSITIES = (0.0, 0.5, 0.99, 0.01)  # source rows 0, 4, 8, ... are all zero


def _next(r, ok):
    while not ok(r):
        r += 1
    return r


@functools.lru_cache(maxsize=None)
def many_rows_case(cus):
    """Case A: R = 8 * CUs + 5 rows over 130 identities — more than two scan
    chunks, than the emit grid (G = 4 * CUs) and than the count grid (8 * CUs).

    Every fourth row is empty, alternately by an empty source list and by an
    all-zero source row; the phase moves by one per G rows, so that some
    block's rows are non-empty, empty, non-empty in turn.  Around every
    boundary b (of a scan chunk or a grid) rows b-4..b-2 and b+1..b+3 are
    empty and rows b-1 and b are not: the running sum crosses the boundary
    between two non-empty rows, with a run of empty ones on either side.
    The last row is non-empty, and one row in each third is CG_EXP_ALL."""
    g = 4 * cus
    n_rows = 8 * cus + 5
    src = X.random_src(EXP_SRC, EXP_N, EXP_DENSITIES, 93)
    for s in range(EXP_SRC):  # a sparse source row is still not empty
        if s % 4:
            src[s, (2 * s) // 64] |= np.uint64(1) << np.uint64((2 * s) % 64)
    assert not src[0::4].any()
    bounds = sorted(b for b in {SCAN_THREADS, 2 * SCAN_THREADS, g, 2 * g} if 4 <= b < n_rows)
    full = {n_rows - 1} | {b - 1 for b in bounds} | set(bounds)
    runs = {r for b in bounds for r in (b - 4, b - 3, b - 2, b + 1, b + 2, b + 3) if r < n_rows} - full

    def empty(r):
        return r not in full and (r in runs or (r + 3 * (r // g)) % 4 == 3)
    every = {_next(n_rows * k // 6, lambda r: not empty(r)) for k in (1, 3, 5)}
    rows = []
    for r in range(n_rows):
        if r in every:
            rows.append(X.row_of(r, [], N.CG_EXP_ALL))
        elif empty(r):
            rows.append(X.row_of(r, [] if r % 8 < 4 else [4 * (r % 16)]))
        else:
            s = 1 + (r * 7) % (EXP_SRC - 1)
            s += s % 4 == 0
            rows.append(X.row_of(r, [s, 1 + r % 3] if r % 5 == 0 else [s]))
    _freeze(src)
    return src, tuple(rows), tuple(bounds)


def check_expand_many_rows(sc, cus, diag_cpu):
    src, rows, bounds = many_rows_case(cus)
    g, n_rows = 4 * cus, len(rows)
    sc.set_identities(X.unlabelled(EXP_N))
    want = X.oracle(src, EXP_N, sc.ids, rows)
    lens = np.array([len(w) for w in want])
    assert 0.10 * n_rows * EXP_N <= lens.sum() <= 0.90 * n_rows * EXP_N
    assert n_rows > SCAN_THREADS, "too few CUs for 8 * CUs + 5 rows to reach a second scan chunk"
    assert lens[-1] > 0 and sum(len(w) == EXP_N for w in want) >= 3
    for b in bounds:
        assert lens[b - 1] > 0 and lens[b] > 0 and not lens[b - 4:b - 1].any() and not lens[b + 1:b + 4].any()
    assert any(lens[b] > 0 and lens[b + g] == 0 and lens[b + 2 * g] > 0 for b in range(n_rows - 2 * g)), \
        "no emit block skips an empty row between two rows it writes"
    assert any(not r[5] and lens[i] == 0 for i, r in enumerate(rows)) and \
        any(r[5] and lens[i] == 0 for i, r in enumerate(rows))
    got = sc.expand(ExpandTable(rows), src, diag_cpu=diag_cpu, threads=4)
    X.assert_entries(rows, want, *got)
    if not diag_cpu:
        for a, b in zip(got, sc.expand(ExpandTable(rows), src, diag_cpu=True, threads=4)):
            assert np.array_equal(a, b), "the kernels and the host walker differ"


@functools.lru_cache(maxsize=None)
def wide_rows_case(cus):
    """Case B: R = 4 * CUs + 3 rows over X.WIDE_N identities (two emit rounds
    per row).  Even rows have density 0.01, odd rows are empty; the last
    three rows (the second rows of blocks 0, 1 and 2) are dense, dense and
    empty.  Block 0 so writes two two-round rows in turn, block 1 an empty
    and then a two-round row, block 2 a two-round row and then an empty one:
    `base` has to restart with every row."""
    g = 4 * cus
    src = X.random_src(8, X.WIDE_N, (0.01, 0.0), 94)
    src[0::2, X.SPAN] |= np.uint64(1 << 3)  # every dense row has entries in its second round too
    dense = lambda r: r % 2 == 0 if r < g else r - g < 2  # noqa: E731
    rows = tuple(X.row_of(r, [2 * (r % 4) + (0 if dense(r) else 1)]) for r in range(g + 3))
    _freeze(src)
    return src, rows


def check_expand_wide_rows(sc, cus, diag_cpu):
    src, rows = wide_rows_case(cus)
    g = 4 * cus
    sc.set_identities(X.unlabelled(X.WIDE_N))
    assert sc.words == X.SPAN + 2
    want = X.oracle(src, X.WIDE_N, sc.ids, rows)
    lens = np.array([len(w) for w in want])
    assert [bool(lens[r]) for r in (0, 1, 2, g, g + 1, g + 2)] == [True, False, True, True, True, False]
    second_round = sc.ids[64 * X.SPAN]
    assert all(w[-1] >= second_round > w[0] for w in want if len(w)), "a dense row lacks entries of either round"
    got = sc.expand(ExpandTable(rows), src, diag_cpu=diag_cpu, threads=4)
    X.assert_entries(rows, want, *got)
    if not diag_cpu:
        for a, b in zip(got, sc.expand(ExpandTable(rows), src, diag_cpu=True, threads=4)):
            assert np.array_equal(a, b), "the kernels and the host walker differ"


def fused_repeats(cus, n_endpoints):
    """The fewest repeats of the endpoint list whose two L3 rows per endpoint
    alone exceed the count kernel's grid of 8 * CUs rows (8 repeats of 132
    endpoints at 256 CUs: 2,112 rows and the L4 rows on top).  The
    per-endpoint Python work of endpoint_policy_map_entries is this case's
    cost, so no more than that."""
    return 8 * cus // (2 * n_endpoints) + 1


def check_fused_many_rows(sc, cus, diag_cpu):
    """Case C: endpoint_policy_map_entries over the 132 identities of
    X.state_inputs(11), repeated."""
    cache, repo = X.state_inputs(11)
    want = X.state_oracle(11, "default", True)
    n = len(cache)
    reps = fused_repeats(cus, n)
    assert 2 * n * reps > 8 * cus
    sc.set_identities(cache)
    sc.set_repository(repo)
    mode0 = repo.cfg.enforcement
    repo.cfg.enforcement = "default"
    try:
        got = sc.endpoint_policy_map_entries(list(cache) * reps, U.REDIRECTS, diag_cpu=diag_cpu, threads=4)
    finally:
        repo.cfg.enforcement = mode0
    assert len(got) == n * reps
    for i, (keys, proxy) in enumerate(got):
        k0, p0 = got[i % n]
        assert np.array_equal(keys, k0) and np.array_equal(proxy, p0), f"entry {i} differs from entry {i % n}"
    for e, (keys, proxy), w in zip(cache, got, want):
        assert X.entries_to_dict(keys, proxy) == w, e
