"""CIDR policy on the CPU.

Reference-pinned (tests/golden/cidr_kat.json): GetCIDRLabels, MatchesAll,
GetAsEndpointSelectors, RemoveCIDRs, getPrefixesFromCIDR / GetCIDRPrefixes,
CIDRRule.sanitize and the CIDR checks of the direction rules.

The selector cache's prefix section (cg_selcache_set_cidr_identities) under
the library's host walkers: against resolve.py fed cidr_labels() dicts, and
— the feature's defining test — against the same prefix identities handed
to a second cache as explicit label identities: match, reach and expansion
are array-equal.  The same checks run through the kernels in
test_cidr_gpu.py."""
import numpy as np
import pytest

import cidr_util as CU
import selcache_util as U
from cilium_amd import _native as N
from cilium_amd import cidr as CIDR
from cilium_amd import resolve as R
from cilium_amd.selcache import unpack_rows
from selcache_expand_util import entries_to_dict

KAT = CU.KAT
Sel = R.EndpointSelector.of


@pytest.fixture()
def sc(host):
    s = host.selector_cache()
    yield s
    s.destroy()


@pytest.fixture()
def sc2(host):
    s = host.selector_cache()
    yield s
    s.destroy()


# ------------------------------------------------------- reference-pinned --
@pytest.mark.parametrize("case", KAT["cidr_labels"]["cases"], ids=lambda c: c["prefix"])
def test_get_cidr_labels(case):
    lbls = CIDR.cidr_labels(case["prefix"])
    assert all(k in lbls for k in case["has"]) and not any(k in lbls for k in case["lacks"])
    assert len(lbls) == case["count"] and set(lbls.values()) == {""}
    assert list(lbls)[-1] == "reserved:world"
    order = [k for k in lbls if k in case["has"]]
    assert order == case["has"]  # /0 first, the prefix itself last before reserved:world


def test_cidr_matches_all():
    for c, want in KAT["matches_all"]["cases"]:
        assert (c in CIDR.CIDR_MATCH_ALL) == want


@pytest.mark.parametrize("case", KAT["as_endpoint_selectors"]["cases"], ids=lambda c: ",".join(c["cidrs"]))
def test_get_as_endpoint_selectors(case):
    got = R.cidr_selectors(case["cidrs"])
    assert got == [Sel({k: ""}) for k in case["selectors"]]
    assert any(s.matches({"reserved:world": ""}) for s in got)
    rule = R.EgressRule(ToEndpoints=[Sel({"a": "b"})], ToEntities=["host"], ToCIDR=case["cidrs"])
    assert rule.destination_selectors() == [Sel({"a": "b"}), Sel({"reserved:host": ""})] + got


@pytest.mark.parametrize("case", KAT["remove_cidrs"]["cases"], ids=lambda c: f"{c['allow'][0]}-{len(c['remove'])}")
def test_remove_cidrs(case):
    allow = [CIDR.parse_cidr_go(c)[1] for c in case["allow"]]
    remove = [CIDR.parse_cidr_go(c)[1] for c in case["remove"]]
    if case["expect"] is None:
        with pytest.raises(ValueError):
            CIDR.remove_cidrs(allow, remove)
    else:
        assert [str(n) for n in CIDR.remove_cidrs(allow, remove)] == case["expect"]


def test_get_prefixes_from_cidr():
    for given, want in KAT["prefixes_from_cidr"]["cases"].items():
        rule = R.Rule(Sel({"bar": ""}), [], [R.EgressRule(ToCIDR=[given])])
        assert [str(n) for n in CIDR.get_cidr_prefixes([rule])] == [want]


@pytest.mark.parametrize("case", KAT["get_cidr_prefixes"]["cases"], ids=lambda c: c["expect"][0])
def test_get_cidr_prefixes(case):
    rules = [R.Rule.from_json(r) for r in case["rules"]]
    for r in rules:
        r.sanitize()
    assert [str(n) for n in CIDR.get_cidr_prefixes(rules)] == case["expect"]
    assert CIDR.get_cidr_prefixes([]) == []


def test_cidr_rule_sanitize():
    for c, want in KAT["cidr_rule_sanitize"]["cases"]:
        if want is None:
            with pytest.raises(ValueError):
                CIDR.cidr_rule_sanitize(CIDR.CIDRRule(c))
        else:
            assert CIDR.cidr_rule_sanitize(CIDR.CIDRRule(c)) == want
            assert CIDR.cidr_sanitize(c) == want


def test_cidr_sanitize_forms():
    """rule_validation.go:360-425."""
    with pytest.raises(ValueError, match="IP must be specified"):
        CIDR.cidr_sanitize("")
    assert CIDR.cidr_sanitize("192.0.2.3") == 0 and CIDR.cidr_sanitize("fdff::ff") == 0  # a bare IP: the zero value
    with pytest.raises(ValueError, match="Unable to parse CIDR"):
        CIDR.cidr_sanitize("192.0.2.300")
    with pytest.raises(ValueError, match="Unable to parse CIDRRule"):
        CIDR.cidr_rule_sanitize(CIDR.CIDRRule("192.0.2.3"))  # only <IP>/<prefix>
    assert CIDR.cidr_mask_size(bytes([254, 0, 0, 255])) == (0, 0)  # what "non-contiguous mask" refuses
    assert CIDR.cidr_mask_size(bytes([255, 240, 0, 0])) == (12, 32)
    ok = CIDR.CIDRRule("10.0.0.0/8", ["10.96.0.0/12", "10.0.0.0/8"])
    assert CIDR.cidr_rule_sanitize(ok) == 8
    with pytest.raises(ValueError, match="does not contain exclude CIDR prefix 11.0.0.0/8"):
        CIDR.cidr_rule_sanitize(CIDR.CIDRRule("10.0.0.0/8", ["11.0.0.0/8"]))
    with pytest.raises(ValueError, match="does not contain"):
        CIDR.cidr_rule_sanitize(CIDR.CIDRRule("10.0.0.0/8", ["a00::/8"]))  # another family
    with pytest.raises(ValueError):
        CIDR.cidr_rule_sanitize(CIDR.CIDRRule("10.0.0.0/8", ["10.0.0.1"]))


def _rule(**direction):
    key = "ingress" if any(k.startswith("from") for k in direction) else "egress"
    return R.Rule.from_json({"endpointSelector": {}, key: [direction]})


PORTS = [{"ports": [{"port": "80", "protocol": "TCP"}]}]
SANITIZE = [  # rule_validation.go:70-110, :147-190 and the prefix-length cap
    (_rule(fromCIDR=["10.0.0.0/8"]), None),
    (_rule(fromCIDRSet=[{"cidr": "10.0.0.0/8", "except": ["10.1.0.0/16"]}]), None),
    (_rule(toCIDR=["10.0.0.0/8", "10.1.2.3"], toPorts=PORTS), None),
    (_rule(toCIDRSet=[{"cidr": "f00d::/64"}], toPorts=PORTS), None),
    (_rule(fromCIDR=["10.0.0.0/8"], toPorts=PORTS), "Combining FromCIDR and ToPorts is not supported yet"),
    (_rule(fromCIDRSet=[{"cidr": "10.0.0.0/8"}], toPorts=PORTS), "Combining FromCIDRSet and ToPorts is not supported yet"),
    (_rule(fromCIDR=["10.0.0.0/8"], fromEndpoints=[{}]), "Combining FromCIDR and FromEndpoints is not supported yet"),
    (_rule(fromCIDR=["10.0.0.0/8"], fromEntities=["world"]), "Combining FromCIDR and FromEntities is not supported yet"),
    (_rule(fromCIDR=["10.0.0.0/8"], fromCIDRSet=[{"cidr": "11.0.0.0/8"}]),
     "Combining FromCIDR and FromCIDRSet is not supported yet"),
    (_rule(toCIDR=["10.0.0.0/8"], toEndpoints=[{}]), "Combining ToCIDR and ToEndpoints is not supported yet"),
    (_rule(toCIDRSet=[{"cidr": "10.0.0.0/8"}], toEntities=["world"]),
     "Combining ToCIDRSet and ToEntities is not supported yet"),
    (_rule(toCIDR=["10.0.0.0/8"], toServices=[{"k8sService": {"serviceName": "x"}}]),
     "Combining ToCIDR and ToServices is not supported yet"),
    (_rule(toCIDR=[""]), "IP must be specified"),
    (_rule(toCIDR=["10.0.0.0/33"]), "Unable to parse CIDR: invalid CIDR address: 10.0.0.0/33"),
    (_rule(toCIDRSet=[{"cidr": "10.0.0.0/8", "except": ["12.0.0.0/8"]}]),
     "allow CIDR prefix 10.0.0.0/8 does not contain exclude CIDR prefix 12.0.0.0/8"),
    (_rule(toCIDR=[f"a::/{n}" for n in range(1, 41)]), None),
    (_rule(toCIDR=[f"a::/{n}" for n in range(1, 41)] + ["10.0.0.0/8"]), None),  # /8 is among the 40 lengths
    (_rule(toCIDR=[f"a::/{n}" for n in range(1, 42)]), "too many egress CIDR prefix lengths 41/40"),
    (_rule(fromCIDR=[f"a::/{n}" for n in range(0, 41)]), "too many ingress CIDR prefix lengths 41/40"),
]


@pytest.mark.parametrize("n", range(len(SANITIZE)))
def test_direction_rule_sanitize(n):
    rule, err = SANITIZE[n]
    if err is None:
        rule.sanitize()
        return
    with pytest.raises(ValueError) as ei:
        rule.sanitize()
    assert str(ei.value) == err


def test_ip_string_and_label_forms():
    """net.IP.String and maskedIPToLabelString, including what Python's
    ipaddress prints differently."""
    S = CIDR.ip_string_to_label
    assert S("::ffff:1.2.3.4/128") == "cidr:1.2.3.4/128"       # To4 accepts the masked address: dotted
    assert S("::ffff:1.2.3.4/96") == "cidr:0.0.0.0/96"
    assert S("::ffff:1.2.3.4/95") == "cidr:0--fffe-0-0/95"
    assert S("::1.2.3.4/128") == "cidr:0--102-304/128"         # IPv4-compatible, not mapped: hex
    assert S("::/0") == "cidr:0--0/0" and S("::1") == "cidr:0--1/128" and S("1::/16") == "cidr:1--0/16"
    assert S("2001:DB8:0:0:1:0:0:1/128") == "cidr:2001-db8--1-0-0-1/128"   # the first of two equal runs
    assert S("2001:db8:0:1:0:0:0:1/128") == "cidr:2001-db8-0-1--1/128"     # the longest run
    assert S("1:0:2:0:3:0:4:0/128") == "cidr:1-0-2-0-3-0-4-0/128"         # a single zero group is not shortened
    assert S("010.1.2.3/8") == "cidr:10.0.0.0/8" and S("10.1.2.3") == "cidr:10.1.2.3/32"
    assert S("10.0.0.0/33") is None and S("nonsense") is None and S("1.2.3/8") is None
    labels = CIDR.cidr_labels("::ffff:10.11.12.13/128")
    assert list(labels)[:2] == ["cidr:0--0/0", "cidr:0--0/1"] and "cidr:0--ffff-0-0/96" not in labels
    assert "cidr:0.0.0.0/96" in labels and "cidr:10.11.12.13/128" in labels and "cidr:0--ff00-0-0/88" in labels
    assert CIDR.Net(CIDR.parse_ip("::ffff:1.2.3.0"), 120).text() == "::ffff:1.2.3.0/120"


def test_rule_fields_and_selectors():
    """from_json keeps the four CIDR members apart (and toServices out of
    them); the selectors come in the reference's order; IsLabelBased."""
    r = R.Rule.from_json({"endpointSelector": {}, "egress": [
        {"toCIDR": ["10.0.0.0/8"]}, {"toCIDRSet": [{"cidr": "10.0.0.0/8", "except": ["10.128.0.0/9"]}]},
        {"toServices": [{"k8sService": {"serviceName": "x"}}]}, {"toEndpoints": [{}]}],
        "ingress": [{"fromCIDR": ["::/0", "0.0.0.0/0"]}, {"fromCIDRSet": [{"cidr": "0.0.0.0/0"}]}]})
    r.sanitize()
    e = r.Egress
    assert e[0].ToCIDR == ["10.0.0.0/8"] and not e[0].ToCIDRSet and not e[0].ToServices
    assert e[1].ToCIDRSet == [CIDR.CIDRRule("10.0.0.0/8", ["10.128.0.0/9"])] and not e[1].ToCIDR
    assert e[2].ToServices and not e[2].ToCIDR
    assert [x.is_label_based() for x in e] == [False, False, False, True]
    assert e[0].destination_selectors() == [Sel({"cidr:10.0.0.0/8": ""})]
    assert e[1].destination_selectors() == [Sel({"cidr:10.0.0.0/9": ""})]
    assert e[2].destination_selectors() == []
    i = r.Ingress
    assert i[0].source_selectors() == [Sel({"reserved:world": ""}), Sel({"cidr:0--0/0": ""}), Sel({"cidr:0.0.0.0/0": ""})]
    assert i[1].source_selectors() == [Sel({"reserved:world": ""}), Sel({"cidr:0.0.0.0/0": ""})]
    assert [x.is_label_based() for x in i] == [False, False]
    assert R.IngressRule([Sel()], [], ["host"], [], ["10.0.0.0/8"]).FromCIDR == ["10.0.0.0/8"]  # positional, as before


def test_cidr_l4_and_l3_resolution():
    """mergeL4Egress sees a CIDR + toPorts rule's selectors (rule.go:312-316,
    :442-478) and canReachEgress a CIDR-only L3 rule."""
    repo = CU.mixed_repository()
    me = CU.LABEL_CACHE[300]
    l4 = repo.resolve_l4_egress_policy(me)
    f = l4["80/TCP"]
    want = [Sel({CIDR.ip_string_to_label(c): ""}) for c in CIDR.compute_resultant_cidr_set(
        [CIDR.CIDRRule("10.0.0.0/8", ["10.96.0.0/12", "10.1.0.0/16"])])]
    assert f.Endpoints == want and len(want) == 9  # 3 left of 10.0.0.0/8 minus the /12, then 6 for the /16 out of 10.0.0.0/10
    assert repo.allows_egress_label_access(me, CIDR.cidr_labels("192.0.2.55/32"))
    assert not repo.allows_egress_label_access(me, CIDR.cidr_labels("192.0.2.54/32"))
    assert not repo.allows_egress_label_access(me, CIDR.cidr_labels("10.5.0.0/16"))  # L4 only
    assert repo.allows_ingress_label_access(CIDR.cidr_labels("10.5.0.0/16"), me)


# ---------------------------------------------------------------- allocator --
def test_allocator(host):
    ic = host.ipcache()
    a = CIDR.CIDRIdentityAllocator(base=256, ipcache=ic)
    ids = a.allocate(["10.0.0.0/8", "10.1.2.3/24", "10.0.0.0/8", "::/0", "0.0.0.0/0", "f00d::1"])
    assert ids == [256, 257, 256, 2, 2, 258]  # one identity per distinct prefix; a /0 is reserved:world
    assert a.identities() == {256: "10.0.0.0/8", 257: "10.1.2.0/24", 258: "f00d::1/128"}
    assert ic.lookup("10.0.0.0/8") == (256, 0) and ic.lookup("10.1.2.0/24") == (257, 0)
    assert ic.lookup("f00d::1/128") == (258, 0) and ic.lookup("0.0.0.0/0") == (2, 0) and ic.lookup("::/0") == (2, 0)
    r4, _ = ic.eval_host_diag(np.array([int.from_bytes(bytes([10, 1, 2, 9]), "little")], np.uint32),
                              np.zeros((0, 16), np.uint8))
    assert int(r4[0, 0]) == 257  # the datapath's longest-prefix lookup returns the same identity
    a.release(["10.0.0.0/8", "0.0.0.0/0"])
    assert a.lookup("10.0.0.0/8") == 256 and ic.lookup("10.0.0.0/8") == (256, 0)  # one reference left
    a.release(["10.0.0.0/8"])
    assert a.lookup("10.0.0.0/8") is None and ic.lookup("10.0.0.0/8") is None
    assert a.allocate(["11.0.0.0/8"]) == [256]  # a freed number is reused
    small = CIDR.CIDRIdentityAllocator(base=300, max_id=301)
    with pytest.raises(RuntimeError):
        small.allocate(["1.0.0.0/8", "2.0.0.0/8", "3.0.0.0/8"])
    assert small.identities() == {}  # all or nothing
    with pytest.raises(ValueError):
        small.allocate(["1.0.0.0/8", "bogus"])
    assert small.identities() == {}
    with pytest.raises(ValueError):
        CIDR.CIDRIdentityAllocator(base=255)
    ic.destroy()


# ------------------------------------------------ host walkers vs resolve.py --
def test_pool_against_resolve(sc):
    """cg_diag_selcache_match_host with a prefix section against resolve.py
    fed cidr_labels() dicts."""
    prefixes, sels = CU.pool_prefixes(), CU.pool_selectors()
    full = CU.explicit_cache(CU.LABEL_CACHE, prefixes)
    sc.set_identities(CU.LABEL_CACHE)
    sc.set_cidr_identities(prefixes)
    got = unpack_rows(sc.match(sels, diag_cpu=True, threads=3), len(full))
    want = CU.oracle_match(sels, full)
    bad = [(s.label_selector_string(), list(full)[i]) for s_i, s in enumerate(sels)
           for i in np.flatnonzero(got[s_i] != want[s_i])]
    assert not bad, bad[:10]
    sub = want[:, len(CU.LABEL_CACHE):]
    assert sub.any(axis=1).sum() >= 40 and (~sub).any(axis=1).sum() >= 40
    assert sc.identities_of(sels[:8], diag_cpu=True) == [R.get_security_identities(full, s) for s in sels[:8]]
    assert dict(sc.identity_cache) == full and list(sc.identity_cache) == list(full)


def test_reach_and_states_against_resolve(sc, sc2):
    repo, full = CU.check_reach_expand_equal(sc, sc2, diag_cpu=True)
    CU.check_states(sc, repo, full, True, entries_to_dict)
    got = sc.endpoint_policy_map_states(CU.ENDPOINTS, U.REDIRECTS, diag_cpu=True)
    assert got == [R.endpoint_policy_map_state(repo, full[e], full, U.REDIRECTS) for e in CU.ENDPOINTS]


# ------------------------------------------------------------- differential --
def test_differential_pool(sc, sc2):
    """The defining test: native prefix identities = the same identities as
    explicit labels, for match, reach and expansion, under the host walker."""
    prefixes, sels = CU.pool_prefixes(), CU.pool_selectors()
    CU.load_pair(sc, sc2, CU.LABEL_CACHE, prefixes)
    n, c = len(CU.LABEL_CACHE), len(prefixes)
    CU.check_sections(sc, n, c)
    a, b = sc.match(sels, diag_cpu=True), sc2.match(sels, diag_cpu=True)
    CU.check_bits(a, b, CU.oracle_match(sels, CU.explicit_cache(CU.LABEL_CACHE, prefixes)), n, c, "pool")
    repo = CU.mixed_repository()
    for s in (sc, sc2):
        s.set_repository(repo)
    for x, y in zip(sc.reach(CU.ENDPOINTS, diag_cpu=True), sc2.reach(CU.ENDPOINTS, diag_cpu=True)):
        assert np.array_equal(x, y)
    table = CU.expand_rows(len(sels))
    for x, y in zip(sc.expand(table, a, diag_cpu=True), sc2.expand(table, a, diag_cpu=True)):
        assert np.array_equal(x, y)
    ents = [s.endpoint_policy_map_entries(CU.ENDPOINTS, diag_cpu=True) for s in (sc, sc2)]
    for (k1, p1), (k2, p2) in zip(*ents):
        assert np.array_equal(k1, k2) and np.array_equal(p1, p2)


@pytest.mark.parametrize("c", [0, 1, 63, 64, 65])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_differential_shapes(sc, sc2, n, c):
    CU.check_shape(sc, sc2, n, c, 48, diag_cpu=True)


def test_differential_big_shape(sc, sc2):
    CU.check_shape(sc, sc2, 100, 1100, 257, diag_cpu=True)


# ---------------------------------------------------------------------- ABI --
def _recs(*items):
    from cilium_amd.classifier import CIDR_DTYPE
    a = np.zeros(len(items), CIDR_DTYPE)
    for i, (fam, plen, addr) in enumerate(items):
        a[i] = (fam, plen, (0, 0), tuple(addr) + (0,) * (16 - len(addr)))
    return a


def _set_raw(sc, ids, recs):
    ids = np.asarray(ids, np.uint32)
    return N.lib.cg_selcache_set_cidr_identities(sc.cl.h, sc.id, N.ptr(ids), N.ptr(recs), len(ids))


def test_abi_invalid_records_keep_tables(sc):
    sels = [Sel({"cidr:10.0.0.0/8": ""}), Sel({"reserved:world": ""}), Sel({"k8s:app": "a"})]
    sc.set_identities(CU.LABEL_CACHE)
    sc.set_cidr_identities({900: "10.1.0.0/16", 901: "11.0.0.0/8"})
    sc.set_repository(CU.mixed_repository())
    before, info = sc.match(sels, diag_cpu=True), sc.info()
    for bad in (_recs((5, 8, (10,))), _recs((4, 8, (10,)), (0, 0, ())), _recs((4, 33, (10,))), _recs((6, 129, (10,))),
                _recs((4, 8, (10,)), (6, 255, ()))):
        assert _set_raw(sc, list(range(700, 700 + len(bad))), bad) == N.CG_INVALID_ARGUMENT
        assert sc.info() == info and np.array_equal(sc.match(sels, diag_cpu=True), before)
    assert N.lib.cg_selcache_set_cidr_identities(sc.cl.h, sc.id, None, None, 2) == N.CG_INVALID_ARGUMENT
    assert N.lib.cg_selcache_set_cidr_identities(sc.cl.h, sc.id + 999, None, None, 0) == N.CG_NOT_FOUND
    assert sc.info() == info


def test_abi_masks_host_bits(sc, sc2):
    """Address bits below the prefix are masked, as the ipcache's NewKey does;
    a v4 record's addr[4..15] is ignored."""
    sels = [Sel({k: ""}) for k in ("cidr:10.0.0.0/8", "cidr:10.255.0.0/16", "cidr:a0b--0/16", "cidr:a0b-c0d--0/32",
                                   "cidr:0.0.0.0/0", "cidr:10.255.255.255/32")]
    dirty = _recs((4, 8, (10, 255, 255, 255, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9)), (6, 16, (0x0a, 0x0b, 0x0c, 0x0d) * 4),
                  (4, 0, (255, 255, 255, 255)), (4, 32, (10, 255, 255, 255)))
    sc.set_cidr_identities({1: "1.0.0.0/8", 2: "2.0.0.0/8", 3: "3.0.0.0/8", 4: "4.0.0.0/8"})  # the wrapper's sizes
    assert _set_raw(sc, [1, 2, 3, 4], dirty) == 0
    sc2.set_cidr_identities({1: "10.0.0.0/8", 2: "a0b::/16", 3: "0.0.0.0/0", 4: "10.255.255.255/32"})
    a, b = sc.match(sels, diag_cpu=True), sc2.match(sels, diag_cpu=True)
    assert np.array_equal(a, b)
    assert unpack_rows(a, 4).tolist() == [[True, False, False, True], [False, False, False, True],
                                          [False, True, False, False], [False, False, False, False],
                                          [True, False, False, True], [False, False, False, True]]


def test_section_replacement(sc):
    """Either section is replaced alone and the other stays; an empty prefix
    section restores the label-only results."""
    labels, prefixes, sels, full, want = CU.shape_case(65, 63)
    sc.set_identities(labels)
    sc.set_repository(CU.mixed_repository())
    label_only = sc.match(sels, diag_cpu=True)
    assert label_only.shape == (len(sels), 2) and sc.info()["identities"] == 65
    sc.set_cidr_identities(prefixes)
    both = sc.match(sels, diag_cpu=True)
    assert sc.info()["identities"] == 128 and np.array_equal(unpack_rows(both, 128), want)
    assert np.array_equal(unpack_rows(both, 65), unpack_rows(label_only, 65))
    # the label section alone: the prefix section keeps its records and moves to the new boundary
    sc.set_identities(dict(list(labels.items())[:10]))
    assert sc.info()["identities"] == 73 and list(sc.ids[10:]) == list(prefixes)
    moved = unpack_rows(sc.match(sels, diag_cpu=True), 73)
    assert np.array_equal(moved[:, :10], want[:, :10]) and np.array_equal(moved[:, 10:], want[:, 65:])
    assert np.array_equal(unpack_rows(sc.match(None, diag_cpu=True), 73),
                          CU.oracle_match(sc.compile_repository(sc.repo)[0], sc.identity_cache))  # republished
    # the prefix section alone
    sc.set_identities(labels)
    few = dict(list(prefixes.items())[:3])
    sc.set_cidr_identities(few)
    assert np.array_equal(unpack_rows(sc.match(sels, diag_cpu=True), 68), np.hstack([want[:, :65], want[:, 65:68]]))
    sc.set_cidr_identities({})
    assert sc.info()["identities"] == 65 and np.array_equal(sc.match(sels, diag_cpu=True), label_only)
    assert sc.identity_cache is labels


def test_prefix_identity_is_no_endpoint(sc):
    sc.set_identities(CU.LABEL_CACHE)
    sc.set_cidr_identities({900: "10.0.0.0/8"})
    sc.set_repository(CU.mixed_repository())
    with pytest.raises(ValueError, match="prefix identity"):
        sc.reach([900], diag_cpu=True)
    with pytest.raises(ValueError, match="prefix identity"):
        sc.endpoint_policy_map_entries([300, 900], diag_cpu=True)
    with pytest.raises(N.CiliumGPUError):  # the library bounds endpoint indices by both sections
        sc.reach_indices(np.array([len(CU.LABEL_CACHE) + 1], np.uint32), diag_cpu=True)
    assert sc.reach_indices(np.array([len(CU.LABEL_CACHE)], np.uint32), diag_cpu=True)[2].tolist() == [0]


# --------------------------------------------------------------- end to end --
def test_e2e_host_tables(host):
    CU.run_e2e(host, on_gpu=False)


def _fromcidr_case(suite):
    c = KAT["from_cidr_and_labels"]
    ids = {n: 400 + i for i, n in enumerate(c["pods"])}
    labels = {ids[n]: lbl for n, lbl in c["pods"].items()}
    labels.update({1: {"reserved:host": ""}, 2: {"reserved:world": ""}})
    alloc = CIDR.CIDRIdentityAllocator(base=1000)
    repo = R.Repository([R.Rule.from_json(r) for r in suite["policy"]], R.PolicyConfig(always_allow_localhost=False))
    nets = CIDR.get_cidr_prefixes(repo.rules)
    assert [str(n) for n in nets] == suite["prefixes"]
    pids = dict(zip(suite["prefixes"], alloc.allocate(nets)))
    who = lambda name: ids.get(name, pids.get(name, 2))  # noqa: E731
    return repo, labels, alloc.identities(), ids["httpd1"], [(who(name), want) for name, want in suite["asserts"]]


@pytest.mark.parametrize("suite", KAT["from_cidr_and_labels"]["suites"], ids=lambda s: s["name"])
def test_from_cidr_and_labels_host(host, sc, suite):
    """Policies.go:840-920 through the map entries and policy_can_access_ingress
    with the identities given: CIDR rules do not admit another endpoint's
    identity."""
    from cilium_amd.classifier import L4_TUPLE_DTYPE
    repo, labels, prefixes, httpd1, asserts = _fromcidr_case(suite)
    sc.set_identities(labels)
    sc.set_cidr_identities(prefixes)
    sc.set_repository(repo)
    (keys, proxy), = sc.endpoint_policy_map_entries([httpd1], diag_cpu=True)
    assert entries_to_dict(keys, proxy) == R.endpoint_policy_map_state(repo, labels[httpd1], sc.identity_cache)
    pm = host.policy_map()
    pm.sync(keys, proxy)
    t = np.zeros(len(asserts), L4_TUPLE_DTYPE)
    for i, (ident, _) in enumerate(asserts):
        t[i] = (ident, 0, 1, N.CG_L4_F_INGRESS, 100)
    got = pm.eval_host_diag(t) >= 0
    pm.destroy()
    assert got.tolist() == [w for _, w in asserts]


def test_egress_to_world_cidr_host(host, sc):
    """The 0.0.0.0/0 toCIDR variant of "Tests Egress To World"
    (Policies.go:1152-1162): the /0 allocates reserved:world, and the
    reserved:world selector GetAsEndpointSelectors adds admits it."""
    CU.run_egress_world(host, sc, on_gpu=False)
