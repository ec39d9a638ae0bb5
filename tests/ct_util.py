"""What test_l4_frames_ct.py (host evaluator, map API) and
test_l4_frames_ct_gpu.py (kernel) share: a Python restatement of the conntrack
half of the ingress policy program, and builders that derive conntrack
entries from frames.

The restatement follows the reference function by function: ct_lookup4 /
ct_lookup6 (lib/conntrack.h:467-590, :310-437) with __ct_lookup (:221-285) as a
dict membership test, ipv{4,6}_ct_tuple_reverse (:439-456, :287-307),
get_ct_map4/6 (bpf_lxc.c:101-107), the tail of ipv4_policy / ipv6_policy
(bpf_lxc.c:948-976, :814-842) with redirect_to_proxy (:109-112), ct_create4/6
(conntrack.h:691-772, :616-667) and ct_delete4/6.  The walk in front of the
lookup and policy_can_access_ingress are frames_util's.  It shares nothing
with csrc/ct_walk.h.

A conntrack table here is a dict {(scope, kind, tuple bytes): value dict}; the
tuple bytes are struct ipv4_ct_tuple / ipv6_ct_tuple as the datapath stores
them (lib/common.h:338-367)."""
import functools
import ipaddress
import json
import os
import struct

import numpy as np

import frames_util as F
from cilium_amd import _native as N
from cilium_amd.classifier import CT_ENTRY_DTYPE, CT_KEY_DTYPE, CT_RECORD_DTYPE

TUPLE_F_OUT, TUPLE_F_IN, TUPLE_F_RELATED, TUPLE_F_SERVICE = 0, 1, 2, 4
CT_NEW, CT_ESTABLISHED, CT_REPLY, CT_RELATED = 0, 1, 2, 3
KIND_TCP, KIND_ANY = 0, 1
OP_NONE, OP_CREATE, OP_DELETE = 0, 1, 2
DROP_CT_CREATE_FAILED = -155
STATE_NAMES = {0: "none", 1: "new", 2: "established", 3: "reply", 4: "related"}


# ------------------------------------------------------------- tuples ----
def tuple_bytes(t: dict) -> bytes:
    """struct ipv{4,6}_ct_tuple, packed: daddr, saddr, dport, sport, nexthdr, flags."""
    return t["daddr"] + t["saddr"] + struct.pack("<HHBB", t["dport"], t["sport"], t["nexthdr"], t["flags"])


def tuple_reverse(t: dict) -> dict:
    r = dict(t, daddr=t["saddr"], saddr=t["daddr"], sport=t["dport"], dport=t["sport"])
    if r["flags"] & TUPLE_F_IN:
        r["flags"] &= ~TUPLE_F_IN
    else:
        r["flags"] |= TUPLE_F_IN
    return r


def get_ct_map(t: dict) -> int:
    return KIND_TCP if t["nexthdr"] == 6 else KIND_ANY


def load_tuple(skb: bytes, family: int, l4_off: int, nexthdr: int):
    """The tuple as ipv4_policy / ipv6_policy and the head of ct_lookup4/6 fill
    it for CT_INGRESS, before any lookup: → tuple dict, or a negative code."""
    if family == 4:
        t = dict(daddr=bytes(skb[30:34]), saddr=bytes(skb[26:30]))
    else:
        t = dict(daddr=bytes(skb[38:54]), saddr=bytes(skb[22:38]))  # the copy taken at bpf_lxc.c:764-766
    t.update(nexthdr=nexthdr, flags=TUPLE_F_OUT, dport=0, sport=0)
    if family == 4 and nexthdr == 1:
        ty = F.skb_load_bytes(skb, l4_off, 1)
        if ty is None:
            return F.DROP_CT_INVALID_HDR
        if ty[0] in (3, 11, 12):  # ICMP_DEST_UNREACH, ICMP_TIME_EXCEEDED, ICMP_PARAMETERPROB
            t["flags"] |= TUPLE_F_RELATED
        elif ty[0] == 0:  # ICMP_ECHOREPLY
            t["dport"] = 8  # ICMP_ECHO, a constant into a __be16
        elif ty[0] == 8:
            t["sport"] = ty[0]
    elif family == 6 and nexthdr == 58:
        ty = F.skb_load_bytes(skb, l4_off, 1)
        if ty is None:
            return F.DROP_CT_INVALID_HDR
        if ty[0] in (1, 2, 3, 4):  # ICMPV6_DEST_UNREACH, _PKT_TOOBIG, _TIME_EXCEED, _PARAMPROB
            t["flags"] |= TUPLE_F_RELATED
        elif ty[0] == 129:  # ICMPV6_ECHO_REPLY
            t["dport"] = 128
        elif ty[0] == 128:
            t["sport"] = ty[0]
    elif nexthdr == 6:
        if F.skb_load_bytes(skb, l4_off + 12, 2) is None:
            return F.DROP_CT_INVALID_HDR
        ports = F.skb_load_bytes(skb, l4_off, 4)
        if ports is None:
            return F.DROP_CT_INVALID_HDR
        t["dport"], t["sport"] = struct.unpack("<HH", ports)
    elif nexthdr == 17:
        ports = F.skb_load_bytes(skb, l4_off, 4)
        if ports is None:
            return F.DROP_CT_INVALID_HDR
        t["dport"], t["sport"] = struct.unpack("<HH", ports)
    else:
        return F.DROP_CT_UNKNOWN_PROTO
    return t


def ct_lookup(ctmap: dict, scope: int, kind: int, t: dict):
    """The two lookups of ct_lookup4/6 → (CT_*, the tuple as the function leaves it, the matched value or None)."""
    v = ctmap.get((scope, kind, tuple_bytes(t)))
    if v is not None:
        return (CT_RELATED if t["flags"] & TUPLE_F_RELATED else CT_REPLY), t, v
    t = tuple_reverse(t)
    v = ctmap.get((scope, kind, tuple_bytes(t)))
    return (CT_ESTABLISHED if v is not None else CT_NEW), t, v


def redirect_to_proxy(verdict, state):
    return verdict > 0 and state in (CT_NEW, CT_ESTABLISHED)


# ------------------------------------------------------------ records ----
def key_record(scope, kind, family, t):
    k = np.zeros(1, CT_KEY_DTYPE)[0]
    n = 4 if family == 4 else 16
    k["daddr"][:n] = np.frombuffer(t["daddr"], np.uint8)
    k["saddr"][:n] = np.frombuffer(t["saddr"], np.uint8)
    k["dport"], k["sport"], k["nexthdr"], k["flags"] = t["dport"], t["sport"], t["nexthdr"], t["flags"]
    k["scope"], k["family"], k["kind"] = scope, family, kind
    return k


def keys_array(items):
    """[(scope, kind, family, tuple)] → CT_KEY_DTYPE array."""
    out = np.zeros(len(items), CT_KEY_DTYPE)
    for i, it in enumerate(items):
        out[i] = key_record(*it)
    return out


def evaluate(frames, slot_tables, ctmap, *, global_map=False, **kw):
    """frames_util.evaluate, then for every frame whose walk reached the policy
    the lookup and the tail of ipv{4,6}_policy.  → (verdicts, FRAME_INFO
    records, CT_RECORD records, policy hits).  The policy call and its hits
    are those of the evaluation without conntrack, as cilium_gpu.h states."""
    out, info, l4o, hits = F.evaluate(frames, slot_tables, **kw)
    rec = np.zeros(len(frames), CT_RECORD_DTYPE)
    for i, skb in enumerate(frames):
        if not info[i]["t"]["flags"] & N.CG_L4_F_INGRESS:
            continue  # returned before ct_lookup's lookups: state none
        family = int(info[i]["family"])
        t = load_tuple(skb, family, int(l4o[i]), int(info[i]["t"]["proto"]))
        assert isinstance(t, dict), "the walk completed, so the tuple loads"
        scope = 0 if global_map else int(info[i]["lxc_id"])
        kind = get_ct_map(t)
        state, t, val = ct_lookup(ctmap, scope, kind, t)
        verdict = int(out[i])
        op = OP_NONE
        if state not in (CT_REPLY, CT_RELATED) and verdict < 0:
            if state == CT_ESTABLISHED:
                op = OP_DELETE
            res = F.DROP_POLICY
        else:
            if state == CT_NEW:
                op = OP_CREATE
            res = verdict if redirect_to_proxy(verdict, state) else 0
        out[i] = res
        r = rec[i]
        r["state"], r["op"] = 1 + state, op
        if val is not None:
            r["rev_nat_index"], r["loopback"] = val.get("rev_nat_index", 0), val.get("loopback", 0)
        r["key"] = key_record(scope, kind, family, t)
    return out, info, rec, hits


# ------------------------------------------------------------- apply ----
def record_tuple(r):
    n = 4 if r["key"]["family"] == 4 else 16
    k = r["key"]
    return dict(daddr=bytes(k["daddr"][:n]), saddr=bytes(k["saddr"][:n]), dport=int(k["dport"]), sport=int(k["sport"]),
                nexthdr=int(k["nexthdr"]), flags=int(k["flags"]))


def apply(ctmap: dict, records, pkt_len, src_labels, max_entries):
    """ct_create4/6 with a zero ct_state and ct_delete4/6 per record, in order,
    on a map of max_entries keys: → results (0 / DROP_CT_CREATE_FAILED).  A
    frame whose new keys do not both fit writes neither (cilium_gpu.h)."""
    res = np.zeros(len(records), np.int32)
    for i, r in enumerate(records):
        if r["op"] == OP_NONE:
            continue
        t = record_tuple(r)
        scope, kind, family = int(r["key"]["scope"]), int(r["key"]["kind"]), int(r["key"]["family"])
        k = (scope, kind, tuple_bytes(t))
        if r["op"] == OP_DELETE:
            ctmap.pop(k, None)
            continue
        icmp = dict(t, nexthdr=1 if family == 4 else 58, sport=0, dport=0, flags=t["flags"] | TUPLE_F_RELATED)
        kr = (scope, kind, tuple_bytes(icmp))
        fresh = len({k, kr} - set(ctmap))
        if len(ctmap) + fresh > max_entries:
            res[i] = DROP_CT_CREATE_FAILED
            continue
        entry = dict(rx_packets=1, rx_bytes=int(pkt_len[i]), src_sec_id=int(src_labels[i]), flags=0, family=family)
        ctmap[k] = dict(entry)
        ctmap[kr] = dict(entry, flags=N.CG_CT_E_SEEN_NON_SYN)
    return res


# ------------------------------------------------------------ builders ----
def frame_tuple(skb: bytes):
    """(family, tuple as loaded) of a frame whose walk completes, else None."""
    if len(skb) < F.ETH_HLEN:
        return None
    et = int.from_bytes(skb[12:14], "big")
    if et not in (0x0800, 0x86DD):
        return None
    w = F.walk(skb, et)
    if w["code"]:
        return None
    family = 4 if et == 0x0800 else 6
    t = load_tuple(skb, family, w["l4_off"], w["proto"])
    return (family, t) if isinstance(t, dict) else None


def entry_for(skb: bytes, want: str, scope: int, kind=None):
    """The (scope, kind, family, tuple) that makes the frame read `want`:
    "reply" — the tuple as loaded (an ICMP error then reads related) —
    or "established", the reversed tuple.  kind: the frame's own map unless given."""
    family, t = frame_tuple(skb)
    if want == "established":
        t = tuple_reverse(t)
    return scope, get_ct_map(t) if kind is None else kind, family, t


def ctmap_of(items, values=None):
    """The oracle's dict for [(scope, kind, family, tuple)]."""
    values = values or [{}] * len(items)
    return {(s, k, tuple_bytes(t)): dict(v, family=f) for (s, k, f, t), v in zip(items, values)}


def values_array(values):
    v = np.zeros(len(values), CT_ENTRY_DTYPE)
    for i, d in enumerate(values):
        v["rev_nat_index"][i] = d.get("rev_nat_index", 0)
        v["flags"][i] = N.CG_CT_E_LB_LOOPBACK if d.get("loopback") else 0
    return v


def derive_table(frames, scopes, seed, shares=(0.25, 0.25, 0.05)):
    """Entries derived from the frames: of those whose walk completes, about
    shares[0] get their reply key, shares[1] their established key, shares[2]
    both (the reply wins); every fifth entry carries a rev_nat_index, every
    ninth the loopback bit.  scopes[i]: the scope frame i is looked up in (None:
    no endpoint).  → (items, values)."""
    rng = np.random.default_rng(seed)
    items, values, seen = [], [], set()
    for i, skb in enumerate(frames):
        ft = frame_tuple(skb)
        r = rng.random()
        if ft is None or scopes[i] is None:
            continue
        wants = (["reply"] if r < shares[0] else ["established"] if r < shares[0] + shares[1]
                 else ["reply", "established"] if r < sum(shares) else [])
        for w in wants:
            it = entry_for(skb, w, int(scopes[i]))
            k = (it[0], it[1], tuple_bytes(it[3]))
            if k in seen:
                continue
            seen.add(k)
            items.append(it)
            values.append(dict(rev_nat_index=(len(items) * 7) & 0xFFFF if len(items) % 5 == 0 else 0,
                               loopback=1 if len(items) % 9 == 0 else 0))
    return items, values


def build_map(cl, items, values=None, **kw):
    ct = cl.conntrack_map(**kw)
    if items:
        ct.update(keys_array(items), values_array(values) if values else None)
    return ct


# ---------------------------------------- the shared frames' tables ----
@functools.lru_cache(maxsize=None)
def shared_table(ci: int, global_map: bool = False):
    """(items, values) derived from frames_util.shared_frames() for resolver
    combination F.COMBOS[ci]: each frame's scope is the endpoint that combination gives it."""
    raw, off, pkt_len, labels, lxc = F.shared_frames()
    frames = F.split(raw, off)
    _, b = F.resolver_args(F.COMBOS[ci], None, None, lxc, labels)
    _, info, _, _ = F.evaluate(frames, F.slot_tables(), pkt_len=pkt_len, **b)
    scopes = [(0 if global_map else int(r["lxc_id"])) if r["t"]["flags"] & N.CG_L4_F_INGRESS else None for r in info]
    return derive_table(frames, scopes, seed=100 + ci)


@functools.lru_cache(maxsize=None)
def shared_expected(ci: int, ignore_drop: bool, global_map: bool = False):
    """The oracle's (verdicts, FRAME_INFO, CT_RECORD, hits) for the shared frames over shared_table(ci)."""
    raw, off, pkt_len, labels, lxc = F.shared_frames()
    items, values = shared_table(ci, global_map)
    _, b = F.resolver_args(F.COMBOS[ci], None, None, lxc, labels)
    return evaluate(F.split(raw, off), F.slot_tables(), ctmap_of(items, values), global_map=global_map,
                    pkt_len=pkt_len, ignore_drop=ignore_drop, **b)


# ---------------------------------------------------- the golden cases ----
def load_golden():
    with open(os.path.join(os.path.dirname(__file__), "golden", "ct_frames.json")) as f:
        return json.load(f)


def golden_item(e: dict):
    d, s = ipaddress.ip_address(e["daddr"]).packed, ipaddress.ip_address(e["saddr"]).packed
    t = dict(daddr=d, saddr=s, dport=e["dport"], sport=e["sport"], nexthdr=e["nexthdr"], flags=e["flags"])
    return e["scope"], e["kind"], 4 if len(d) == 4 else 6, t


def golden_world(cl):
    """(array, policy map, conntrack map, raw, off, resolver keywords, cases) of ct_frames.json."""
    g = load_golden()
    pm, arr = cl.policy_map(), cl.policy_array()
    for p in g["policy"]:
        pm.allow(g["label"], p["dport"], p["proto"], 0, p["proxy_port"])
    arr.set(g["slot"], pm)
    items = [golden_item(e) for c in g["frames"] for e in c["entries"]]
    ct = build_map(cl, items)
    raw, off = F.join([bytes.fromhex(c["hex"]) for c in g["frames"]])
    n = len(g["frames"])
    kw = dict(lxc_ids=np.full(n, g["slot"]), src_labels=np.full(n, g["label"]))
    return arr, pm, ct, raw, off, kw, g["frames"]


def check_golden(cases, v, rec):
    for i, c in enumerate(cases):
        got = dict(verdict=int(v[i]), state=STATE_NAMES[int(rec["state"][i])],
                   op={0: "none", 1: "create", 2: "delete"}[int(rec["op"][i])])
        assert got == {f: c[f] for f in got}, c["name"]
        if "key" in c:
            assert rec["key"][i] == key_record(*golden_item(c["key"])), c["name"]


def assert_records_equal(got, exp, what=""):
    """Field by field, so that a failure names the field and the frame."""
    for f in ("state", "op", "loopback", "rev_nat_index"):
        bad = np.flatnonzero(got[f] != exp[f])
        assert not len(bad), f"{what}: {f} differs at {bad[:5]}: got {got[f][bad[:5]]}, expected {exp[f][bad[:5]]}"
    bad = np.flatnonzero(got["key"] != exp["key"])
    assert not len(bad), f"{what}: key differs at {bad[:5]}: got {got['key'][bad[:5]]}, expected {exp['key'][bad[:5]]}"
    assert got.tobytes() == exp.tobytes(), f"{what}: padding bytes differ"


# ---------------------------------------------------------- near misses ----
def _near_misses(item):
    """Keys that differ from `item` in exactly one respect."""
    scope, kind, family, t = item
    a = bytearray(t["daddr"])
    a[-1] ^= 1
    b = bytearray(t["saddr"])
    b[0] ^= 0x80
    return {
        "scope": (scope ^ 1, kind, family, t),
        "kind": (scope, kind ^ 1, family, t),
        "flags in": (scope, kind, family, dict(t, flags=t["flags"] ^ TUPLE_F_IN)),
        "flags related": (scope, kind, family, dict(t, flags=t["flags"] ^ TUPLE_F_RELATED)),
        "flags service": (scope, kind, family, dict(t, flags=t["flags"] ^ TUPLE_F_SERVICE)),
        "nexthdr": (scope, kind, family, dict(t, nexthdr=t["nexthdr"] ^ 23)),
        "swapped ports": (scope, kind, family, dict(t, dport=t["sport"], sport=t["dport"])),
        "daddr bit": (scope, kind, family, dict(t, daddr=bytes(a))),
        "saddr bit": (scope, kind, family, dict(t, saddr=bytes(b))),
    }


def near_miss_check(cl, run):
    """For an IPv4 and an IPv6 TCP frame and both directions: the exact key
    hits, each near miss alone reads NEW, all of them together still read NEW."""
    g = load_golden()
    frames = [bytes.fromhex(c["hex"]) for c in g["frames"] if c["name"] in
              ("IPv4 established and allowed with a proxy port gives the port",
               "IPv6 established and allowed with a proxy port gives the port")]
    assert len(frames) == 2
    pm, arr = cl.policy_map(), cl.policy_array()
    arr.set(g["slot"], pm)
    raw, off = F.join(frames)
    kw = dict(lxc_ids=[g["slot"]] * 2, src_labels=[g["label"]] * 2)
    for want, state in (("reply", N.CG_CT_STATE_REPLY), ("established", N.CG_CT_STATE_ESTABLISHED)):
        exact = [entry_for(f, want, g["slot"]) for f in frames]
        misses = [_near_misses(it) for it in exact]
        assert all(t["dport"] != t["sport"] for _, _, _, t in exact)
        tables = [("exact", exact, state)] + [(name, [m[name] for m in misses], N.CG_CT_STATE_NEW) for name in misses[0]]
        tables.append(("all near misses", [it for m in misses for it in m.values()], N.CG_CT_STATE_NEW))
        for name, items, exp in tables:
            ct = build_map(cl, items)
            _, _, rec = run(arr, raw, off, ct, kw)
            assert rec["state"].tolist() == [exp, exp], (want, name)
            ct.destroy()
    arr.destroy()
    pm.destroy()


# -------------------------------------------------------- probe chains ----
def loadable_keys(family, n, seed):
    """n distinct random keys that a TCP / UDP frame loads as they are:
    TUPLE_F_OUT, nexthdr 6 in the TCP map and 17 in the ANY map, scopes 0..3."""
    rng = np.random.default_rng(seed)
    size = 4 if family == 4 else 16
    k = np.zeros(n, CT_KEY_DTYPE)
    k["daddr"][:, :size] = rng.integers(0, 256, (n, size))
    k["saddr"][:, :size] = rng.integers(0, 256, (n, size))
    k["dport"], k["sport"] = rng.integers(0, 65536, n), rng.integers(0, 65536, n)
    k["scope"], k["kind"], k["family"] = rng.integers(0, 4, n), rng.integers(0, 2, n), family
    k["nexthdr"] = np.where(k["kind"] == KIND_TCP, 6, 17)
    _, first = np.unique(k, return_index=True)
    return k[np.sort(first)]


def frame_for_key(k) -> bytes:
    """The frame whose tuple, as loaded, is k."""
    ports = struct.pack("<HH", int(k["dport"]), int(k["sport"]))
    if k["family"] == 4:
        ip = struct.pack(">BBHHHBBH", 0x45, 0, 40, 0, 0, 64, int(k["nexthdr"]), 0) + bytes(k["saddr"][:4]) + \
            bytes(k["daddr"][:4])
        return bytes(12) + b"\x08\x00" + ip + ports + bytes(16)
    ip = struct.pack(">IHBB", 0x60000000, 20, int(k["nexthdr"]), 64) + bytes(k["saddr"]) + bytes(k["daddr"])
    return bytes(12) + b"\x86\xdd" + ip + ports + bytes(16)


def table_buckets(family, n):
    """The builder's sizing (csrc/ct_map.h): at most 3 of 7 slots a bucket on
    average for IPv4, 1 of 3 for IPv6, a power of two."""
    b = 1
    while b * (3 if family == 4 else 1) < n:
        b <<= 1
    return b


def chain_table(family, n_fill=3000):
    """n_fill keys, then more than three buckets' worth of keys whose hash (the
    table's own, cg_diag_ct_hash) lands in the table's last bucket: their
    chain wraps the table's end and sets the recorded probe bound.
    → (keys, index of the first chain key, buckets)."""
    from cilium_amd.classifier import ConntrackMap
    slots = 7 if family == 4 else 3
    n_chain = 3 * slots + 2
    keys = loadable_keys(family, n_fill + 200_000, 40 + family)
    fill, cand = keys[:n_fill], keys[n_fill:]
    buckets = table_buckets(family, n_fill + n_chain)
    cand = cand[(ConntrackMap.key_hashes(cand) & np.uint32(buckets - 1)) == buckets - 1][:n_chain]
    assert len(cand) == n_chain
    return np.concatenate([fill, cand]), n_fill, buckets


def probe_chain_check(cl, run):
    """Every key of a table with chains at the probe bound is found by the
    walk (a frame per key reads REPLY), and every deleted key misses afterwards."""
    pm, arr = cl.policy_map(), cl.policy_array()
    arr.set_many([0, 1, 2, 3], [pm] * 4)
    for family in (4, 6):
        keys, first, buckets = chain_table(family)
        raw, off = F.join([frame_for_key(k) for k in keys])
        kw = dict(lxc_ids=keys["scope"], src_labels=np.zeros(len(keys), np.uint32))
        ct = cl.conntrack_map()
        ct.update(keys)
        b, probes = ct.table_info()[family]
        assert b == buckets and probes >= 3  # past three full buckets, through bucket 0
        _, _, rec = run(arr, raw, off, ct, kw)
        assert rec["key"]["flags"].tolist() == [0] * len(keys) and np.array_equal(rec["key"], keys)
        bad = np.flatnonzero(rec["state"] != N.CG_CT_STATE_REPLY)
        assert not len(bad), (family, bad[:5])
        gone = np.zeros(len(keys), bool)
        gone[first::2] = True
        gone[:first:10] = True
        ct.delete(keys[gone])
        _, _, rec = run(arr, raw, off, ct, kw)
        assert (rec["state"][gone] == N.CG_CT_STATE_NEW).all(), family
        assert (rec["state"][~gone] == N.CG_CT_STATE_REPLY).all(), family
        ct.destroy()
    arr.destroy()
    pm.destroy()
