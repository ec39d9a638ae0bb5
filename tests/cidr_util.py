"""Shared inputs of test_cidr.py (host) and test_cidr_gpu.py (kernels): the
reference-pinned fixture, the prefix and selector pools of the differential
test — the same prefix identities natively (set_cidr_identities) and as
explicit label identities carrying cidr_labels() — seeded shapes, a mixed
label / CIDR repository, and the end-to-end policy with its brute-force
oracle.  Everything is compared for equality; nothing has a tolerance."""
import functools
import ipaddress

import numpy as np

import selcache_util as U
from cilium_amd import cidr as CIDR
from cilium_amd import resolve as R
from cilium_amd.selcache import ExpandTable, unpack_rows
from kat_util import load

KAT = load("cidr_kat.json")
Sel = R.EndpointSelector.of

# ------------------------------------------------------------------- pools --
V4_LENGTHS = (0, 1, 8, 24, 31, 32)
V6_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)  # every u32 boundary of the compare
V4_BASE = "10.11.12.13"
V6_BASE = "a0b:c0d:8000:1:ffff:fffe:8001:203"  # begins with the bytes of 10.11.12.13
V6_OTHER = "a0b:c0d:8000:1:ffff:fffe:8001:202"  # differs in the last bit only


def pool_prefixes():
    """Prefix identities of the differential test: both families at every
    listed length (so a /0 of each), a v4 and a v6 prefix sharing leading
    bytes, neighbours that differ in one bit at a word boundary, and
    IPv4-mapped IPv6 prefixes on both sides of /96."""
    out = [f"{V4_BASE}/{n}" for n in V4_LENGTHS] + [f"{V6_BASE}/{n}" for n in V6_LENGTHS]
    out += ["10.11.12.12/32", "10.11.12.14/31", "11.0.0.0/8", "138.0.0.0/1", f"{V6_OTHER}/128",
            "a0b:c0d:8000:1:ffff:ffff::/96", "a0b:c0d:8000:0::/64", "a0b:c0d:0:1::/64", "a0b:c0c::/32", "8a0b::/1",
            "::ffff:10.11.12.13/128", "::ffff:10.11.12.0/120", "::ffff:0.0.0.0/96", "::ffff:0:0/95", "::fffe:0:0/96",
            "::10.11.12.13/128", "::/128", "::1/128", "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff/128",
            "255.255.255.255/32", "0.0.0.0/32"]
    return {2000 + i: p for i, p in enumerate(out)}


def _cidr_key(prefix):
    return CIDR.ip_string_to_label(prefix)


def pool_selectors():
    """The selector pool of the differential test."""
    sels = [Sel({_cidr_key(f"{V4_BASE}/{n}"): ""}) for n in V4_LENGTHS]
    sels += [Sel({_cidr_key(f"{V6_BASE}/{n}"): ""}) for n in V6_LENGTHS]
    sels += [Sel({_cidr_key(f"{V6_OTHER}/{n}"): ""}) for n in (127, 128)]
    sels += [Sel({k: ""}) for k in (
        "cidr:0.0.0.0/0", "cidr:0--0/0", "any:0.0.0.0/0", "0--0/0", "any:10.0.0.0/8", "10.11.12.0/24",
        "k8s:10.0.0.0/8", "reserved:10.0.0.0/8", "cidr:world", "k8s:world",
        "reserved:world", "any:world", "world", "reserved:host", "reserved:all",
        # IPv4-mapped IPv6 text
        "cidr:10.11.12.13/128", "cidr:10.11.12.0/120", "cidr:0.0.0.0/96", "cidr:0--ffff-0-0/96", "cidr:0--fffe-0-0/95",
        "cidr:0--a0b-c0d/128", "cidr:10.11.12.13/64", "cidr:0--ffff-a0b-c0d/128",
        # non-canonical keys: each names no label GetCIDRLabels prints
        "cidr:010.0.0.0/8", "cidr:10.0.0.0/08", "cidr:10.11.12.13/8", "cidr:10.0.0.1/8", "cidr:10.0.0.0/33",
        "cidr:10.0.0.0/", "cidr:10.0.0.0", "cidr:10.0.0/8", "cidr:10.0.0.0.0/8", "cidr:256.0.0.0/8",
        "cidr:A0B--0/16", "cidr:a0b--0/16", "cidr:0a0b--0/16", "cidr:a0b-0-0-0-0-0-0-0/16", "cidr:a0b--/16",
        "cidr:--/0", "cidr:0--0/129", "cidr:a0b:c0d--0/32", "cidr:a0b-c0d--0/32", "cidr:a0b-c0d-8000-1--0/64",
        "cidr:a0b-c0d-8000-1-0-0-0-0/64", "cidr:/8", "cidr:", "cidr:-/0", "cidr:0--0--0/0")]
    sels += [Sel({"cidr:10.0.0.0/8": "x"}), Sel({"reserved:world": "x"})]
    for key in ("cidr:10.0.0.0/8", "cidr:0--0/0", "reserved:world", "k8s:app", "app", "any:tier"):
        sels += [Sel(None, [(key, "Exists", ())]), Sel(None, [(key, "DoesNotExist", ())]),
                 Sel(None, [(key, "NotIn", ("",))]), Sel(None, [(key, "In", ("", "x"))]),
                 Sel(None, [(key, "In", ("x", "y"))]), Sel(None, [(key, "NotIn", ("x",))])]
    # a cidr: label combined with requirements on other keys (FromRequires folded in by with_requirements)
    sels += [Sel({"cidr:10.0.0.0/8": "", "k8s:app": "a"}), Sel({"cidr:10.0.0.0/8": "", "reserved:world": ""}),
             R.with_requirements(Sel({"cidr:10.0.0.0/8": ""}), (("k8s:app", "DoesNotExist", ()),)),
             R.with_requirements(Sel({"cidr:10.0.0.0/8": ""}), (("cidr:10.11.12.13/32", "DoesNotExist", ()),)),
             R.with_requirements(Sel({"cidr:0--0/0": ""}), (("cidr:a0b-c0d-8000-1--0/64", "NotIn", ("",)),)),
             R.with_requirements(Sel({"reserved:world": ""}), (("any:0.0.0.0/0", "Exists", ()),)),
             Sel({"cidr:10.0.0.0/8": "", "cidr:10.11.12.0/24": ""}), Sel({"cidr:10.0.0.0/8": "", "cidr:11.0.0.0/8": ""}),
             Sel(), Sel({"reserved:all": "", "cidr:nonsense": "zzz"})]
    return sels


def explicit_cache(labels, prefixes):
    """The parent's formulation: the label identities, then every prefix
    identity as a label identity carrying cidr_labels(prefix)."""
    out = dict(labels)
    for ident, p in prefixes.items():
        assert ident not in out
        out[ident] = CIDR.cidr_labels(p)
    return out


def oracle_match(sels, cache):
    return np.array([[s.matches(lbls) for lbls in cache.values()] for s in sels], bool).reshape(len(sels), len(cache))


# ------------------------------------------------------------ seeded shapes --
_LEN4 = (32, 32, 32, 32, 24, 24, 16, 8, 31, 1, 0)
_LEN6 = (128, 128, 64, 64, 96, 97, 112, 33, 32, 1, 0)


def random_prefixes(c, seed, first_id=70000):
    """c distinct-numbered prefix identities, mostly /32 and /128, addresses
    from a few clustered networks so that shorter prefixes contain many."""
    rng = np.random.default_rng(seed)
    out = {}
    for i in range(c):
        if rng.random() < 0.65:
            a = bytes([int(rng.choice([10, 10, 10, 11, 192])), int(rng.integers(0, 4)), int(rng.integers(0, 256)),
                       int(rng.integers(0, 256))])
            n = int(rng.choice(_LEN4))
            out[first_id + i] = CIDR.Net(CIDR._mask(a, CIDR.cidr_mask(n, 32)), n).text()
        else:
            a = bytes([0x20, 0x01, 0x0d, 0xb8, 0, int(rng.integers(0, 3))]) + bytes(4) + \
                (b"\xff\xff" if rng.random() < 0.2 else bytes([0, int(rng.integers(0, 2))])) + \
                bytes(int(x) for x in rng.integers(0, 256, 4))
            if rng.random() < 0.1:
                a = CIDR._V4_IN_V6 + a[12:]
            n = int(rng.choice(_LEN6))
            out[first_id + i] = CIDR.Net(CIDR._mask(a, CIDR.cidr_mask(n, 128)), n).text()
    return out


def cidr_selectors(prefixes, s, seed):
    """s selectors over the prefixes' own labels: an ancestor of a random
    prefix identity, sometimes negated or joined with another requirement."""
    rng = np.random.default_rng(seed)
    plist = list(prefixes.values())
    sels = []
    for _ in range(s):
        lbls = list(CIDR.cidr_labels(plist[int(rng.integers(0, len(plist)))])) if plist else ["reserved:world"]
        key = lbls[int(rng.integers(0, len(lbls)))]
        t = rng.random()
        if t < 0.6:
            sels.append(Sel({key: ""}))
        elif t < 0.7:
            sels.append(Sel(None, [(key, "DoesNotExist", ())]))
        elif t < 0.8:
            sels.append(Sel({key: ""}, [(lbls[int(rng.integers(0, len(lbls)))], "Exists", ())]))
        elif t < 0.9:
            sels.append(Sel(None, [(key, "NotIn", ("", "x"))]))
        else:
            sels.append(Sel({key: ""}, [("k8s:app", "DoesNotExist", ())]))
    return sels


@functools.lru_cache(maxsize=None)
def shape_case(n, c, s=48):
    """(label cache, prefix identities, selectors, the explicit cache, the
    resolve.py oracle's bool matrix [s][n + c])."""
    labels = U.random_identities(n, 40 + n) if n else {}
    prefixes = random_prefixes(c, 1000 + 7 * n + c)
    sels = U.random_selectors(s // 3, 5 + n + c) + cidr_selectors(prefixes, s - s // 3 - 6, 77 + n + c) + \
        [Sel(), Sel({"reserved:world": ""}), Sel({"cidr:0.0.0.0/0": ""}), Sel({"cidr:0--0/0": ""}),
         Sel(None, [("cidr:10.0.0.0/8", "DoesNotExist", ())]), Sel({"cidr:10.0.0.0/8": ""})]
    assert len(sels) == s
    full = explicit_cache(labels, prefixes)
    want = oracle_match(sels, full)
    want.setflags(write=False)
    return labels, prefixes, sels, full, want


def load_pair(native, explicit, labels, prefixes):
    native.set_identities(labels)
    native.set_cidr_identities(prefixes)
    explicit.set_cidr_identities({})
    explicit.set_identities(explicit_cache(labels, prefixes))


def check_sections(native, n, c):
    assert native.info()["identities"] == n + c and native.info()["words"] == (n + c + 63) // 64
    assert native.words == (n + c + 63) // 64 and len(native.ids) == n + c


def check_bits(got, want_bits, want_rows, n, c, what):
    """got[S][W] against the explicit-label words and the oracle's rows, the
    word the label section ends in bit by bit, and the padding bits."""
    total = n + c
    assert got.shape == want_bits.shape == (len(want_rows), (total + 63) // 64), what
    if total and n % 64 and c:
        w = n // 64
        for b in range(min(64, total - 64 * w)):
            col = (got[:, w] >> np.uint64(b)) & np.uint64(1)
            assert np.array_equal(col.astype(bool), want_rows[:, 64 * w + b]), f"{what}: boundary word, bit {b}"
    assert np.array_equal(unpack_rows(got, total), want_rows), what
    assert np.array_equal(got, want_bits), what
    if total % 64:
        assert not np.any(got[:, -1] >> np.uint64(total % 64)), f"{what}: padding bits of the last word are set"


def check_shape(native, explicit, n, c, s, diag_cpu):
    """match through `native` (kernel or host walker) = the host walker = the
    explicit-label cache through the same path = resolve.py."""
    labels, prefixes, sels, full, want = shape_case(n, c, s)
    load_pair(native, explicit, labels, prefixes)
    check_sections(native, n, c)
    walker = native.match(sels, diag_cpu=True)
    exp = explicit.match(sels, diag_cpu=diag_cpu)
    check_bits(walker, exp, want, n, c, f"host walker N={n} C={c}")
    if not diag_cpu:
        check_bits(native.match(sels), exp, want, n, c, f"kernel N={n} C={c}")
        assert np.array_equal(exp, explicit.match(sels, diag_cpu=True))


# ----------------------------------------------------- reach, expand, state --
LABEL_CACHE = {300: {"k8s:app": "a", "k8s:tier": "web"}, 301: {"k8s:app": "b"}, 302: {"k8s:app": "a", "k8s:env": "p"},
               303: {"container:app": "c"}, 304: {"k8s:app": "b", "k8s:tier": "db"},
               1: {"reserved:host": ""}, 2: {"reserved:world": ""}}
ENDPOINTS = [300, 301, 302, 303, 304]


def mixed_repository(cfg=None):
    """Label rules and CIDR rules, L3-only and with toPorts, FromRequires on
    a cidr: key, entities beside them."""
    tcp80 = [R.PortRule([R.PortProtocol("80", "TCP")])]
    udp53 = [R.PortRule([R.PortProtocol("53", "UDP")])]
    rules = [
        R.Rule(Sel({"k8s:app": "a"}),
               [R.IngressRule(FromCIDR=["10.0.0.0/8", "2001:db8::/32"]),
                R.IngressRule(FromEndpoints=[Sel({"k8s:app": "b"})], ToPorts=tcp80)],
               [R.EgressRule(ToCIDRSet=[R.CIDRRule("10.0.0.0/8", ["10.96.0.0/12", "10.1.0.0/16"])], ToPorts=tcp80),
                R.EgressRule(ToCIDR=["192.0.2.55/32"]),
                R.EgressRule(ToEndpoints=[Sel({"k8s:tier": "db"})])]),
        R.Rule(Sel({"k8s:app": "b"}),
               [R.IngressRule(FromCIDRSet=[R.CIDRRule("0.0.0.0/0", ["10.0.0.0/8"])]),
                R.IngressRule(FromEndpoints=[Sel()], FromRequires=[Sel(None, [("cidr:11.0.0.0/8", "DoesNotExist", ())])])],
               [R.EgressRule(ToCIDR=["::/0"], ToPorts=udp53), R.EgressRule(ToEntities=["world"], ToPorts=tcp80)]),
        R.Rule(Sel({"app": "c"}), [], [R.EgressRule(ToCIDR=["0.0.0.0/0"]), R.EgressRule(ToCIDR=["2001:db8:0:1::/64"],
                                                                                      ToPorts=tcp80)]),
        R.Rule(Sel({"k8s:tier": "db"}), [R.IngressRule(FromEntities=["host"]), R.IngressRule(FromCIDR=["10.2.3.4"])], []),
    ]
    return R.Repository(rules, cfg or R.PolicyConfig())


STATE_PREFIXES = ["10.0.0.0/8", "10.5.0.0/16", "10.96.0.0/12", "10.97.1.1/32", "10.1.2.0/24", "10.2.3.4/32", "11.1.0.0/16",
                  "192.0.2.55/32", "192.0.2.0/24", "2001:db8::/32", "2001:db8:0:1::5/128", "2001:db9::/32", "::/0",
                  "0.0.0.0/0", "128.0.0.0/1", "10.128.0.0/9"]


def state_prefixes():
    return {900 + i: p for i, p in enumerate(STATE_PREFIXES)}


def expand_rows(s):
    """One expansion row per selector plus an all-identities row."""
    from cilium_amd import _native as N
    return ExpandTable([(0x5000, 6, r & 1, 0, 0, [r]) for r in range(s)] + [(0, 0, 0, 0, N.CG_EXP_ALL, [])])


def check_reach_expand_equal(native, explicit, diag_cpu):
    """reach over the mixed repository and an expansion of the match matrix:
    the native prefix section against the explicit-label cache, as arrays,
    and reach against resolve.py."""
    prefixes = state_prefixes()
    load_pair(native, explicit, LABEL_CACHE, prefixes)
    repo = mixed_repository()
    full = explicit_cache(LABEL_CACHE, prefixes)
    for sc in (native, explicit):
        sc.set_repository(repo)
    a, b = native.reach(ENDPOINTS, diag_cpu=diag_cpu), explicit.reach(ENDPOINTS, diag_cpu=diag_cpu)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    want = U.oracle_reach(repo, full, ENDPOINTS)
    assert want[0].any() and want[1].any() and not want[0].all() and not want[1].all()
    assert np.array_equal(unpack_rows(a[0], len(full)), want[0])
    assert np.array_equal(unpack_rows(a[1], len(full)), want[1])
    assert np.array_equal(a[2], want[2])
    sels = pool_selectors()[:40]
    src = native.match(sels, diag_cpu=diag_cpu)
    table = expand_rows(len(sels))
    ra, rb = native.expand(table, src, diag_cpu=diag_cpu), explicit.expand(table, src, diag_cpu=diag_cpu)
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)
    assert set(prefixes) <= set(ra[1]["sec_label"].tolist())  # sec_label of a prefix bit is its identity number
    return repo, full


def check_states(sc, repo, full, diag_cpu, entries_to_dict):
    """endpoint_policy_map_entries over both sections = resolve.endpoint_policy_map_state
    over the combined identity cache, for the enforcement modes that resolve."""
    mode0 = repo.cfg.enforcement
    try:
        for mode in ("default", "always"):
            repo.cfg.enforcement = mode
            got = sc.endpoint_policy_map_entries(ENDPOINTS, U.REDIRECTS, diag_cpu=diag_cpu)
            for e, (keys, proxy) in zip(ENDPOINTS, got):
                want = R.endpoint_policy_map_state(repo, full[e], full, U.REDIRECTS)
                assert entries_to_dict(keys, proxy) == want, (mode, e)
                if e == 300:  # the toCIDRSet + toPorts rule gave L4 entries for prefix identities
                    assert any(k.Identity >= 900 and k.DestPort == 80 for k in want)
    finally:
        repo.cfg.enforcement = mode0


# -------------------------------------------------------------- end to end --
E2E_POLICY = [{"endpointSelector": {"matchLabels": {"id.app1": ""}},
               "egress": [{"toCIDRSet": [{"cidr": "10.0.0.0/8", "except": ["10.96.0.0/12"]}],
                           "toPorts": [{"ports": [{"port": "80", "protocol": "TCP"}]}]},
                          {"toCIDR": ["192.0.2.55/32"]},
                          {"toCIDR": ["2001:db8:cafe::/48"]}]}]
E2E_APP1 = 300
E2E_LABELS = {E2E_APP1: {"container:id.app1": ""}, 301: {"container:id.app2": ""},
              1: {"reserved:host": ""}, 2: {"reserved:world": ""}}


def _edges(net):
    n = ipaddress.ip_network(net)
    lo, hi = int(n.network_address), int(n.broadcast_address)
    top = (1 << n.max_prefixlen) - 1
    return [x for x in (lo - 1, lo, hi, hi + 1) if 0 <= x <= top]


def e2e_probes(repo):
    """(family, address int, dport, proto) probes: both edges (inside and
    just outside) of every resultant prefix and of the exception, addresses
    inside the remainder and inside the exception, one outside everything;
    port 80/TCP, a wrong port, and UDP."""
    v4, v6 = set(), set()
    for n in CIDR.get_cidr_prefixes(repo.rules):
        (v4 if n.family == 4 else v6).update(_edges(str(n)))
    v4.update(_edges("10.96.0.0/12"))
    v4.update(int(ipaddress.ip_address(a)) for a in ("10.1.2.3", "10.200.0.9", "10.100.0.1", "10.111.255.254",
                                                     "8.8.8.8", "192.0.2.54", "192.0.2.56"))
    v6.update(int(ipaddress.ip_address(a)) for a in ("2001:db8:cafe:1::1", "2001:db8:caff::1", "2001:db8::1", "::1"))
    ports = ((80, 6), (81, 6), (80, 17))
    return [(4, a, p, pr) for a in sorted(v4) for p, pr in ports] + [(6, a, p, pr) for a in sorted(v6) for p, pr in ports]


def e2e_oracle(policy, family, addr, dport, proto):
    """The rule text evaluated by brute force: some egress rule holds a CIDR
    (or a CIDR set member minus its exceptions) that contains the address,
    and has no toPorts or lists the port."""
    ip = ipaddress.ip_address(addr) if family == 6 else ipaddress.IPv4Address(addr)
    for rule in policy:
        for eg in rule.get("egress", []):
            hit = any(ip in ipaddress.ip_network(c, strict=False) for c in eg.get("toCIDR", [])
                      if ipaddress.ip_network(c, strict=False).version == family)
            for cs in eg.get("toCIDRSet", []):
                net = ipaddress.ip_network(cs["cidr"])
                if net.version == family and ip in net and not any(ip in ipaddress.ip_network(x)
                                                                   for x in cs.get("except", [])):
                    hit = True
            if not hit:
                continue
            tp = eg.get("toPorts")
            if not tp:
                return True
            for pr in tp:
                for pp in pr["ports"]:
                    want = {"TCP": (6,), "UDP": (17,), "ANY": (6, 17)}[pp.get("protocol", "ANY").upper()]
                    if int(pp["port"]) == dport and proto in want:
                        return True
    return False


def run_e2e(cl, on_gpu):
    """Policy JSON → allocator → ipcache + selector cache → policy map →
    verdicts on addresses, every probe against the brute-force oracle.  On
    the GPU: sync_policy_maps and the fused ipcache + L4 kernels; on a host
    handle the same tables through the host walkers."""
    from cilium_amd.classifier import L4_TUPLE_DTYPE
    from cilium_amd.policy import htons
    repo = R.Repository([R.Rule.from_json(r) for r in E2E_POLICY],
                        R.PolicyConfig(always_allow_localhost=False, enforcement="always"))
    ic, sc, pm = cl.ipcache(), cl.selector_cache(), cl.policy_map()
    try:
        alloc = CIDR.CIDRIdentityAllocator(base=1000, ipcache=ic)
        nets = CIDR.get_cidr_prefixes(repo.rules)
        ids = alloc.allocate(nets)
        assert len(set(ids)) == len(ids) == len(nets) >= 6 and min(ids) >= 1000
        for n, i in zip(nets, ids):
            assert ic.lookup(str(n)) == (i, 0)
        sc.set_identities(E2E_LABELS)
        sc.set_cidr_identities(alloc.identities())
        sc.set_repository(repo)
        if on_gpu:
            sc.sync_policy_maps([E2E_APP1], [pm])
        else:
            (keys, proxy), = sc.endpoint_policy_map_entries([E2E_APP1], diag_cpu=True)
            pm.sync(keys, proxy)
        probes = e2e_probes(repo)
        want = np.array([e2e_oracle(E2E_POLICY, *p) for p in probes])
        assert 0.2 < want.mean() < 0.8, want.mean()
        got = np.zeros(len(probes), bool)
        for fam in (4, 6):
            idx = [i for i, p in enumerate(probes) if p[0] == fam]
            t = np.zeros(len(idx), L4_TUPLE_DTYPE)
            for k, i in enumerate(idx):
                t[k] = (0, htons(probes[i][2]), probes[i][3], 0, 100)
            if fam == 4:
                remote = np.array([int.from_bytes(probes[i][1].to_bytes(4, "big"), "little") for i in idx], np.uint32)
                none = np.zeros((0, 16), np.uint8)
            else:
                remote = np.array([list(probes[i][1].to_bytes(16, "big")) for i in idx], np.uint8).reshape(-1, 16)
                none = np.zeros(0, np.uint32)
            if on_gpu:
                v = pm.verdicts_via_ipcache(ic, remote, t)
            else:
                r4, r6 = ic.eval_host_diag(remote, none) if fam == 4 else ic.eval_host_diag(none, remote)
                t["identity"] = (r4 if fam == 4 else r6)[:, 0]
                v = pm.eval_host_diag(t)
            got[idx] = v >= 0
        bad = [probes[i] for i in np.flatnonzero(got != want)]
        assert not bad, bad
        # released prefixes leave the ipcache; the datapath then sees world
        alloc.release(nets)
        assert alloc.identities() == {} and all(ic.lookup(str(n)) is None for n in nets)
    finally:
        sc.destroy()
        pm.destroy()
        ic.destroy()


def run_egress_world(cl, sc, on_gpu):
    """test/runtime/Policies.go:1152-1162: app1's egress under a 0.0.0.0/0
    toCIDR rule and enforcement always, as test_egress_world_e2e.py checks
    the toEntities variants: the destination through the ipcache, app1's
    egress map, and for a pod destination that pod's ingress map."""
    from cilium_amd import _native as N
    from cilium_amd.classifier import L4_TUPLE_DTYPE
    from cilium_amd.policy import htons
    c = KAT["egress_to_world_cidr"]
    ids = {n: 300 + i for i, n in enumerate(c["pods"])}
    cache = {ids[n]: {f"container:id.{n}": ""} for n in c["pods"]}
    cache.update({1: {"reserved:host": ""}, 2: {"reserved:world": ""}})
    repo = R.Repository([R.Rule.from_json(r) for r in c["policy"]],
                        R.PolicyConfig(always_allow_localhost=False, enforcement=c["enforcement"]))
    ic = cl.ipcache()
    maps = {n: cl.policy_map() for n in c["pods"]}
    try:
        ic.update([f"{c['addrs'][n]}/32" for n in c["pods"]], [[ids[n], 0] for n in c["pods"]])
        alloc = CIDR.CIDRIdentityAllocator(base=1000, ipcache=ic)
        assert alloc.allocate(CIDR.get_cidr_prefixes(repo.rules)) == [2] and alloc.identities() == {}
        sc.set_identities(cache)
        sc.set_cidr_identities(alloc.identities())
        sc.set_repository(repo)
        pods = list(c["pods"])
        if on_gpu:
            sc.sync_policy_maps([ids[n] for n in pods], [maps[n] for n in pods])
        else:
            for n, (k, p) in zip(pods, sc.endpoint_policy_map_entries([ids[n] for n in pods], diag_cpu=True)):
                maps[n].sync(k, p)
        bad = []
        for dst, proto, dport, want in c["asserts"]:
            a = np.array([int.from_bytes(ipaddress.ip_address(c["addrs"][dst]).packed, "little")], np.uint32)
            eg = np.zeros(1, L4_TUPLE_DTYPE)
            eg[0] = (0, htons(dport), proto, 0, 100)
            if on_gpu:
                ok = int(maps["app1"].verdicts_via_ipcache(ic, a, eg)[0]) >= 0
            else:
                eg["identity"] = ic.eval_host_diag(a, np.zeros((0, 16), np.uint8))[0][:, 0]
                ok = int(maps["app1"].eval_host_diag(eg)[0]) >= 0
            if ok and dst in ids:
                ing = np.zeros(1, L4_TUPLE_DTYPE)
                ing[0] = (ids["app1"], htons(dport), proto, N.CG_L4_F_INGRESS, 100)
                v = maps[dst].verdicts(ing, mode=N.CG_L4_INGRESS) if on_gpu else maps[dst].eval_host_diag(ing)
                ok = int(v[0]) >= 0
            if ok != want:
                bad.append(dst)
        assert not bad, bad
    finally:
        for m in maps.values():
            m.destroy()
        ic.destroy()
