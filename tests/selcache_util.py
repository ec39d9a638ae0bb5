"""Shared inputs of test_selcache.py (host walkers) and test_selcache_gpu.py
(kernels): the hand-written operator KAT, seeded random identity caches,
selectors and repositories, and the resolve.py oracle over them (computed
once per shape and shared)."""
import functools

import numpy as np

from cilium_amd import resolve as R
from cilium_amd.policy import L7Rules, PortRuleHTTP
from cilium_amd.selcache import unpack_rows
from kat_util import load

KAT = load("repository_kat.json")
REACH = [c for c in KAT["cases"] if c.get("kind") == "reach"]
MK = next(c for c in KAT["cases"] if c["case"] == "MinikubeGettingStarted")

Sel = R.EndpointSelector.of

# ------------------------------------------------------------ operator KAT --
# Written from pkg/policy/api/selector.go:279-310 and pkg/labels/array.go:90-131:
# (name, labels in order, selector, matches).
K8S_THEN_CONTAINER = {"k8s:app": "a", "container:app": "b"}
CONTAINER_THEN_K8S = {"container:app": "b", "k8s:app": "a"}
OPERATOR_KAT = [
    ("matchLabels hit", {"k8s:app": "a"}, Sel({"k8s:app": "a"}), True),
    ("matchLabels miss value", {"k8s:app": "a"}, Sel({"k8s:app": "b"}), False),
    ("matchLabels miss key", {"k8s:app": "a"}, Sel({"k8s:tier": "a"}), False),
    ("matchLabels miss source", {"k8s:app": "a"}, Sel({"container:app": "a"}), False),
    ("matchLabels two, both hold", {"k8s:app": "a", "k8s:env": "p"}, Sel({"k8s:app": "a", "k8s:env": "p"}), True),
    ("matchLabels two, one fails", {"k8s:app": "a", "k8s:env": "p"}, Sel({"k8s:app": "a", "k8s:env": "q"}), False),
    ("In hit", {"k8s:app": "a"}, Sel(None, [("k8s:app", "In", ("x", "a"))]), True),
    ("In miss", {"k8s:app": "a"}, Sel(None, [("k8s:app", "In", ("x", "y"))]), False),
    ("In missing label", {"k8s:env": "a"}, Sel(None, [("k8s:app", "In", ("a",))]), False),
    ("NotIn hit (other value)", {"k8s:app": "a"}, Sel(None, [("k8s:app", "NotIn", ("x", "y"))]), True),
    ("NotIn hit (missing label)", {"k8s:env": "a"}, Sel(None, [("k8s:app", "NotIn", ("a",))]), True),
    ("NotIn miss", {"k8s:app": "a"}, Sel(None, [("k8s:app", "NotIn", ("x", "a"))]), False),
    ("Exists hit", {"k8s:app": "a"}, Sel(None, [("k8s:app", "Exists", ())]), True),
    ("Exists miss", {"k8s:env": "a"}, Sel(None, [("k8s:app", "Exists", ())]), False),
    ("DoesNotExist hit", {"k8s:env": "a"}, Sel(None, [("k8s:app", "DoesNotExist", ())]), True),
    ("DoesNotExist miss", {"k8s:app": "a"}, Sel(None, [("k8s:app", "DoesNotExist", ())]), False),
    ("selector source any", {"container:app": "a"}, Sel({"any:app": "a"}), True),
    ("selector without source is any", {"container:app": "a"}, Sel({"app": "a"}), True),
    ("label source any", {"any:app": "a"}, Sel({"k8s:app": "a"}), True),
    ("label without source is any", {"app": "a"}, Sel({"k8s:app": "a"}), True),
    ("first label wins: any:app=b misses", K8S_THEN_CONTAINER, Sel({"any:app": "b"}), False),
    ("first label wins: any:app=a hits", K8S_THEN_CONTAINER, Sel({"any:app": "a"}), True),
    ("reversed order: any:app=b hits", CONTAINER_THEN_K8S, Sel({"any:app": "b"}), True),
    ("a named source skips the other label", K8S_THEN_CONTAINER, Sel({"container:app": "b"}), True),
    ("empty value hits an empty label", {"k8s:app": ""}, Sel({"k8s:app": ""}), True),
    ("empty value misses a missing label", {"k8s:env": ""}, Sel({"k8s:app": ""}), False),
    ("empty value misses a non-empty label", {"k8s:app": "a"}, Sel({"k8s:app": ""}), False),
    ("In with the empty value, missing label", {"k8s:env": ""}, Sel(None, [("k8s:app", "In", ("",))]), False),
    ("the empty selector", {"k8s:app": "a"}, Sel(), True),
    ("the empty selector, no labels", {}, Sel(), True),
    ("reserved:all in matchLabels", {"k8s:app": "a"}, Sel({"reserved:all": ""}), True),
    ("reserved:all in matchLabels beside a failing pair", {"k8s:app": "a"},
     Sel({"reserved:all": "", "k8s:app": "zzz"}), True),
    ("reserved:all in matchLabels, no labels", {}, Sel({"reserved:all": ""}), True),
    ("reserved:all only in an expression is not special", {"k8s:app": "a"},
     Sel(None, [("reserved:all", "Exists", ())]), False),
    ("reserved:all only in an In expression is not special", {"k8s:app": "a"},
     Sel(None, [("reserved:all", "In", ("",))]), False),
    ("no labels: matchLabels", {}, Sel({"k8s:app": "a"}), False),
    ("no labels: NotIn", {}, Sel(None, [("k8s:app", "NotIn", ("a",))]), True),
    ("no labels: DoesNotExist", {}, Sel(None, [("k8s:app", "DoesNotExist", ())]), True),
    ("a value no identity carries", {"k8s:app": "a"}, Sel(None, [("k8s:app", "In", ("never-seen",))]), False),
    ("a key whose name is a value elsewhere", {"k8s:app": "tier"}, Sel({"k8s:tier": "app"}), False),
]


def check_operator_kat(sc, diag_cpu):
    """Every KAT row is its own identity; each selector is matched against
    its own row's identity (and the python oracle agrees with the table)."""
    cache = {100 + i: row[1] for i, row in enumerate(OPERATOR_KAT)}
    sc.set_identities(cache)
    bits = sc.match([row[2] for row in OPERATOR_KAT], diag_cpu=diag_cpu)
    got = unpack_rows(bits, len(cache))
    for i, (name, labels, sel, want) in enumerate(OPERATOR_KAT):
        assert sel.matches(labels) == want, f"oracle disagrees with the KAT: {name}"
        assert bool(got[i, i]) == want, name
    full = np.array([[s.matches(lbls) for lbls in cache.values()] for _, _, s, _ in OPERATOR_KAT])
    assert np.array_equal(got, full)


# ------------------------------------------------------- random match tables --
KEYS = ("app", "tier", "env", "zone")
SOURCES = ("k8s", "container", "any")
VALUES = ("a", "b", "c")
PAIRS = [f"{s}:{k}" for k in KEYS for s in SOURCES]
LONG_FILL = 10  # more than the labels the match kernel stages per identity


def random_identities(n, seed, first_id=1000):
    """n identities with 0-6 labels of 4 keys x 3 sources x 3 values, in random
    order; the middle one has LONG_FILL filler labels first, so every label
    that decides a selector lies past the kernel's staged labels."""
    rng = np.random.default_rng(seed)
    cache = {}
    for i in range(n):
        k = int(rng.integers(0, 7))
        lbls = {}
        if i == n // 2:
            lbls = {f"k8s:fill{j}": "x" for j in range(LONG_FILL)}
            k = max(k, 4)
        for p in rng.permutation(len(PAIRS))[:k]:
            lbls[PAIRS[p]] = VALUES[int(rng.integers(0, 3))]
        cache[first_id + i] = lbls
    return cache


def random_selector(rng):
    t = rng.random()
    if t < 0.03:
        return Sel()
    if t < 0.05:
        return Sel({"reserved:all": ""})
    ml, me = {}, []
    for _ in range(int(rng.integers(1, 3))):
        key = KEYS[int(rng.integers(0, 4))]
        s = int(rng.integers(0, 4))
        key = key if s == 3 else f"{SOURCES[s]}:{key}"
        vals = tuple(VALUES[int(v)] for v in rng.permutation(3)[:int(rng.integers(1, 3))])
        kind = rng.random()
        if kind < 0.35:
            ml[key] = vals[0]
        elif kind < 0.55:
            me.append((key, "In", vals))
        elif kind < 0.7:
            me.append((key, "NotIn", vals))
        elif kind < 0.85:
            me.append((key, "Exists", ()))
        else:
            me.append((key, "DoesNotExist", ()))
    return Sel(ml, me)


def random_selectors(s, seed):
    rng = np.random.default_rng(seed)
    return [random_selector(rng) for _ in range(s)]


@functools.lru_cache(maxsize=None)
def match_case(n, s=97, seed=7):
    """(identity cache, selectors, the oracle's bool matrix [s][n])."""
    cache = random_identities(n, seed + n)
    sels = random_selectors(s, seed * 31 + n)
    want = np.array([[sel.matches(lbls) for lbls in cache.values()] for sel in sels], bool).reshape(s, n)
    want.setflags(write=False)
    return cache, sels, want


def assert_two_sided(want, what):
    """The oracle's own matrix has at least 10% of each outcome, so neither
    all-zeros nor all-ones passes."""
    frac = float(np.mean(want))
    assert 0.10 <= frac <= 0.90, f"{what}: {frac:.3f} of the oracle's cells are set"


def check_match(sc, n, diag_cpu):
    cache, sels, want = match_case(n)
    assert_two_sided(want, f"match N={n}")
    sc.set_identities(cache)
    bits = sc.match(sels, diag_cpu=diag_cpu)
    assert bits.shape == (len(sels), (n + 63) // 64)
    assert np.array_equal(unpack_rows(bits, n), want)
    if n % 64:
        assert not np.any(bits[:, -1] >> np.uint64(n % 64)), "padding bits of the last word are set"
    ids = sc.identities_of(sels[:5], diag_cpu=diag_cpu)
    assert ids == [R.get_security_identities(cache, s) for s in sels[:5]]


# ------------------------------------------------------------------- reach --
def random_repository(n_rules, seed, l7=False, cfg=None):
    """Rules over the random label space: subjects that select ~1/5 of the
    identities, 1-2 direction rules each way with 1-2 peers, ToPorts on a
    third of them (with HTTP rules on port 80 when l7), requires on a few
    rules, entities on some."""
    rng = np.random.default_rng(seed)

    def subject():
        key = KEYS[int(rng.integers(0, 4))]
        if rng.random() < 0.5:
            return Sel({key: VALUES[int(rng.integers(0, 3))]})
        return Sel({f"k8s:{key}": VALUES[int(rng.integers(0, 3))]}, [(KEYS[int(rng.integers(0, 4))], "Exists", ())])

    def ports():
        if l7 and rng.random() < 0.5:
            return [R.PortRule([R.PortProtocol("80", "TCP")], L7Rules(HTTP=[PortRuleHTTP(Path="/", Method="GET")]))]
        return [R.PortRule([R.PortProtocol(str(int(rng.choice([80, 443]))), "TCP")])]

    def direction(cls, requires):
        out = []
        for _ in range(int(rng.integers(1, 3))):
            peers = [random_selector(rng) for _ in range(int(rng.integers(0, 3)))]
            req = [Sel(None, [(KEYS[int(rng.integers(0, 4))], "NotIn", (VALUES[int(rng.integers(0, 3))],))])] \
                if requires else []
            ent = [str(rng.choice(["world", "cluster", "host", "all"]))] if rng.random() < 0.1 else []
            out.append(cls(peers, req, ent, ports() if rng.random() < 0.33 else []))
        return out

    rules = []
    for _ in range(n_rules):
        requires = rng.random() < 0.1
        ing = direction(R.IngressRule, requires) if rng.random() < 0.8 else []
        eg = direction(R.EgressRule, requires and rng.random() < 0.5) if rng.random() < 0.6 else []
        rules.append(R.Rule(subject(), ing, eg))
    return R.Repository(rules, cfg)


def oracle_reach(repo, cache, endpoints):
    """(ing[E][N], eg[E][N], flags[E]) from resolve.py."""
    E, N = len(endpoints), len(cache)
    ing, eg, fl = np.zeros((E, N), bool), np.zeros((E, N), bool), np.zeros(E, np.uint8)
    for a, e in enumerate(endpoints):
        me = cache[e]
        i_on, e_on = repo.get_rules_matching(me)
        fl[a] = int(i_on) | (int(e_on) << 1)
        for b, peer in enumerate(cache.values()):
            ing[a, b] = repo.allows_ingress_label_access(peer, me)
            eg[a, b] = repo.allows_egress_label_access(me, peer)
    return ing, eg, fl


@functools.lru_cache(maxsize=None)
def reach_case(seed, n=130, n_rules=40):
    cache = random_identities(n, 900 + seed)
    cache[1] = {"reserved:host": ""}
    cache[2] = {"reserved:world": ""}
    repo = random_repository(n_rules, seed)
    want = oracle_reach(repo, cache, list(cache))
    for a in want:
        a.setflags(write=False)
    return cache, repo, want


def check_reach(sc, cache, repo, endpoints, want, diag_cpu):
    sc.set_identities(cache)
    sc.set_repository(repo)
    ing, eg, fl = sc.reach(endpoints, diag_cpu=diag_cpu)
    n = len(cache)
    assert np.array_equal(unpack_rows(ing, n), want[0])
    assert np.array_equal(unpack_rows(eg, n), want[1])
    assert np.array_equal(fl, want[2])
    if n % 64 and len(endpoints):
        assert not np.any(ing[:, -1] >> np.uint64(n % 64)) and not np.any(eg[:, -1] >> np.uint64(n % 64))


def check_reach_random(sc, seed, diag_cpu):
    cache, repo, want = reach_case(seed)
    assert_two_sided(want[0], f"ingress reach seed={seed}")
    assert_two_sided(want[1], f"egress reach seed={seed}")
    assert len(set(want[2].tolist())) > 1
    check_reach(sc, cache, repo, list(cache), want, diag_cpu)


def golden_reach_inputs(case):
    """A golden reach case as (cache, endpoint ids, [(endpoint row, peer column, allowed)])."""
    sets = []
    for frm, to, _ in case["asserts"]:
        for lbls in (frm, to):
            if lbls not in sets:
                sets.append(lbls)
    cache = {500 + i: lbls for i, lbls in enumerate(sets)}
    ident = lambda lbls: 500 + sets.index(lbls)  # noqa: E731
    ingress = case["dir"] == "ingress"
    subjects = []
    for frm, to, _ in case["asserts"]:
        s = ident(to if ingress else frm)
        if s not in subjects:
            subjects.append(s)
    checks = [(subjects.index(ident(to if ingress else frm)), sets.index(frm if ingress else to), allowed)
              for frm, to, allowed in case["asserts"]]
    return cache, subjects, checks


def check_golden_reach(sc, case, diag_cpu):
    cache, subjects, checks = golden_reach_inputs(case)
    sc.set_identities(cache)
    sc.set_repository(R.Repository([R.Rule.from_json(r) for r in case["rules"]]))
    ing, eg, _ = sc.reach(subjects, diag_cpu=diag_cpu)
    rows = unpack_rows(ing if case["dir"] == "ingress" else eg, len(cache))
    for row, col, allowed in checks:
        assert bool(rows[row, col]) == allowed, (case["case"], row, col)


def rule_can_reach_repo():
    """rule_test.go:38-115 (TestRuleCanReach), second rule: allowed, denied by
    FromRequires, undecided."""
    rule = {"endpointSelector": {"matchLabels": {"bar": ""}},
            "ingress": [{"fromEndpoints": [{"matchLabels": {"foo": ""}}],
                         "fromRequires": [{"matchLabels": {"baz": ""}}]}]}
    cache = {10: {"bar": ""}, 11: {"foo": ""}, 12: {"baz": ""}, 13: {"foo": "", "baz": ""}}
    return R.Repository([R.Rule.from_json(rule)]), cache


def check_rule_can_reach(sc, diag_cpu):
    repo, cache = rule_can_reach_repo()
    decisions = [repo.can_reach_ingress(cache[p], cache[10]) for p in (11, 12, 13)]
    assert decisions == ["denied", "undecided", "allowed"]
    sc.set_identities(cache)
    sc.set_repository(repo)
    ing, eg, fl = sc.reach([10], diag_cpu=diag_cpu)
    assert unpack_rows(ing, 4)[0].tolist() == [False, False, False, True]  # only "allowed" sets the bit
    assert not eg.any() and fl.tolist() == [1]


def check_empty_repository(sc, diag_cpu):
    cache = random_identities(70, 3)
    sc.set_identities(cache)
    sc.set_repository(R.Repository())
    ing, eg, fl = sc.reach(list(cache), diag_cpu=diag_cpu)
    assert ing.shape == (70, 2) and not ing.any() and not eg.any() and not fl.any()


# --------------------------------------------------------- policy map states --
MK_CACHE = {300: {"id": "app1"}, 301: {"id": "app2"}, 302: {"id": "app3"}, 1: {"reserved:host": ""},
            2: {"reserved:world": ""}, 5: {"reserved:init": "", "id": "app1"}}
REDIRECTS = {(True, "TCP", 80): 15001, (False, "TCP", 80): 15002}


def check_map_states(sc, repo, cache, diag_cpu):
    """endpoint_policy_map_states == endpoint_policy_map_state per endpoint,
    for every enforcement mode, with and without redirect ports."""
    sc.set_identities(cache)
    sc.set_repository(repo)
    mode0 = repo.cfg.enforcement
    try:
        for mode in ("default", "always", "never"):
            repo.cfg.enforcement = mode
            for redirects in (None, REDIRECTS):
                got = sc.endpoint_policy_map_states(list(cache), redirects, diag_cpu=diag_cpu)
                for e, g in zip(cache, got):
                    assert g == R.endpoint_policy_map_state(repo, cache[e], cache, redirects), (mode, redirects, e)
    finally:
        repo.cfg.enforcement = mode0


def minikube_repo():
    return R.Repository([R.Rule.from_json(r) for r in MK["rules"]], R.PolicyConfig())
