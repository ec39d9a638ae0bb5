"""What test_l4_egress.py (host evaluator, headers, apply) and
test_l4_egress_gpu.py (kernel) share: a Python restatement of the endpoint's
from-container program up to its verdict, frame builders, and the egress world.

The restatement follows the reference function by function: handle_ingress
(bpf_lxc.c:708-742), handle_ipv4_from_lxc (:432-570), handle_ipv6 (:389-416)
with icmp6_handle (lib/icmp6.h:390-412), ipv6_l3_from_lxc (:114-266), the
source checks of lib/lxc.h:31-88, lb{4,6}_extract_key → extract_l4_port
(lib/lb.h:192-216) with l4_load_port (lib/l4.h:62-65), the head of ct_lookup4/6
with dir = CT_EGRESS (lib/conntrack.h:496-556, :339-400), policy_can_egress
(lib/policy.h:150-177) and ct_create4/6 as CT_EGRESS (conntrack.h:691-772,
:616-667).  The program is the one built with CONNTRACK, LB_L3, LB_L4 over an
empty services map.  ipv6_hdrlen, the tuple loader, the two lookups and the map
builders are frames_util's / ct_util's; direction and header handling are
here.  It shares nothing with csrc/egress_walk.h."""
import functools
import ipaddress
import json
import os
import struct

import numpy as np

import ct_util as T
import frames_util as F
import l4_array_util as U
from cilium_amd import _native as N
from cilium_amd import synth
from cilium_amd.classifier import CT_RECORD_DTYPE, FRAME_INFO_DTYPE, PolicyArray
from cilium_amd.policy import htons

DROP_INVALID_SMAC, DROP_INVALID_DMAC, DROP_INVALID_SIP, DROP_UNKNOWN_L4 = -130, -131, -132, -142
ANSWERED, NO_HEADER, EFAULT = -3, -4, -14
ETH_P_IP, ETH_P_IPV6, ETH_P_ARP = 0x0800, 0x86DD, 0x0806
ALL_CODES = [-140, -4, -134, -3, -139, -130, -131, -132, -156, -157, -14, -135, -137, -133, 0]


def is_err(ret):
    return ret < 0


# --------------------------------------------------------- the program ----
def extract_l4_port(skb, nexthdr, l4_off):
    """lib/lb.h:192-216: 0, skb_load_bytes's own error, or DROP_UNKNOWN_L4."""
    if nexthdr in (6, 17):
        if F.skb_load_bytes(skb, l4_off + 2, 2) is None:  # l4_load_port passes the error on
            return EFAULT
        return 0
    if nexthdr in (58, 1):
        return 0
    return DROP_UNKNOWN_L4


def src_checks(skb, hdr, sip_ok):
    """is_valid_lxc_src_mac / is_valid_gw_dst_mac / is_valid_lxc_src_ip{,v4}, in
    the if / else-if order of bpf_lxc.c:456-461, :132-137."""
    if not hdr["flags"] & N.CG_EPH_F_NO_SMAC and bytes(skb[6:12]) != hdr["lxc_mac"]:
        return DROP_INVALID_SMAC
    if not hdr["flags"] & N.CG_EPH_F_NO_DMAC and bytes(skb[0:6]) != hdr["node_mac"]:
        return DROP_INVALID_DMAC
    if not hdr["flags"] & N.CG_EPH_F_NO_SIP and not sip_ok:
        return DROP_INVALID_SIP
    return 0


def from_container(skb: bytes, hdr: dict) -> dict:
    """The program up to ct_lookup's lookups.  code 0: `tuple` is the tuple as
    the head of ct_lookup4/6 loaded it (flags TUPLE_F_IN [| RELATED])."""
    r = dict(code=0, family=0, proto=0, l4_off=0, tuple=None, daddr=None)
    proto = int.from_bytes(skb[12:14], "big")  # skb->protocol
    if proto == ETH_P_ARP:
        return dict(r, code=ANSWERED)  # tail_handle_arp: arp_respond, no policy
    if proto not in (ETH_P_IP, ETH_P_IPV6):
        return dict(r, code=F.DROP_UNKNOWN_L3)
    if proto == ETH_P_IP:
        r["family"] = 4
        if len(skb) < F.ETH_HLEN + 20:  # revalidate_data
            return dict(r, code=F.DROP_INVALID)
        ip4 = skb[F.ETH_HLEN:F.ETH_HLEN + 20]
        nexthdr = r["proto"] = ip4[9]
        sip_ok = bool(hdr["flags"] & N.CG_EPH_F_IPV4) and bytes(ip4[12:16]) == hdr["ipv4"]  # no LXC_IPV4: never valid
        ret = src_checks(skb, hdr, sip_ok)
        if ret:
            return dict(r, code=ret)
        r["daddr"] = bytes(ip4[16:20])
        l4_off = r["l4_off"] = F.ETH_HLEN + (ip4[0] & 0xF) * 4  # ipv4_hdrlen
    else:
        r["family"] = 6
        if len(skb) < F.ETH_HLEN + 40:
            return dict(r, code=F.DROP_INVALID)
        ip6 = skb[F.ETH_HLEN:F.ETH_HLEN + 40]
        r["proto"] = ip6[6]
        if ip6[6] == 58:  # ip6->nexthdr == IPPROTO_ICMPV6: the fixed header's field
            if F.ETH_HLEN + 40 + 8 > len(skb):
                return dict(r, code=F.DROP_INVALID)
            type_ = skb[F.ETH_HLEN + 40]  # icmp6_load_type
            if type_ == 135:
                return dict(r, code=ANSWERED)  # icmp6_handle_ns
            if type_ == 128 and bytes(ip6[24:40]) == hdr["router_ip6"]:
                return dict(r, code=ANSWERED)  # icmp6_send_echo_reply
        ret = src_checks(skb, hdr, bytes(ip6[8:24]) == hdr["ipv6"])
        if ret:
            return dict(r, code=ret)
        r["daddr"] = bytes(ip6[24:40])
        hdrlen, nexthdr = F.ipv6_hdrlen(skb, F.ETH_HLEN, ip6[6])
        if hdrlen < 0:
            return dict(r, code=hdrlen)
        r["proto"] = nexthdr
        l4_off = r["l4_off"] = F.ETH_HLEN + hdrlen
    ret = extract_l4_port(skb, nexthdr, l4_off)
    if is_err(ret) and ret != DROP_UNKNOWN_L4:
        return dict(r, code=ret)
    # no service: orig_dip = daddr.  ct_lookup4/6 with dir = CT_EGRESS
    t = T.load_tuple(skb, r["family"], l4_off, nexthdr)
    if not isinstance(t, dict):
        return dict(r, code=t)
    t["flags"] |= T.TUPLE_F_IN  # dir == CT_EGRESS
    r["tuple"] = t
    return r


def policy_can_egress(table, identity, dport, proto, ignore_drop):
    """lib/policy.h:150-177 over __policy_can_access with dir = CT_EGRESS and
    is_fragment = false → (verdict, the key hit or None)."""
    hit = None
    for key in ((identity, dport, proto, 1), (identity, 0, 0, 1), (0, dport, proto, 1)):
        if key in table:
            hit = key
            break
    if hit is None:
        return (0 if ignore_drop else F.DROP_POLICY), None
    return (0 if hit[1] == 0 and hit[2] == 0 else table[hit]), hit


def evaluate(frames, slot_tables, headers, *, lxc_ids, dst_labels=None, ipcache=None, pkt_len=None, ignore_drop=False,
             ctmap=None, global_map=False):
    """frames: list of bytes; slot_tables: {lxc: (map index, table dict)};
    headers: {lxc: header dict}; ctmap: the oracle's dict or None (no map:
    every packet CT_NEW, no records).  → (verdicts, FRAME_INFO records, CT
    records, l4 offsets, {(map index, key): [packets, bytes]})."""
    n = len(frames)
    out, info = np.zeros(n, np.int32), np.zeros(n, FRAME_INFO_DTYPE)
    rec, l4o, hits = np.zeros(n, CT_RECORD_DTYPE), np.zeros(n, np.uint32), {}
    for i, skb in enumerate(frames):
        lxc = int(lxc_ids[i])
        fi = info[i]
        fi["lxc_id"] = lxc
        if lxc not in slot_tables:
            out[i] = F.DROP_MISSED_TAIL_CALL
            continue
        if lxc not in headers:
            out[i] = NO_HEADER
            continue
        length = int(pkt_len[i]) if pkt_len is not None else len(skb)
        fi["t"]["len"] = length
        if len(skb) < F.ETH_HLEN:
            out[i] = F.DROP_INVALID
            continue
        hdr = headers[lxc]
        w = from_container(skb, hdr)
        fi["family"], fi["t"]["proto"], l4o[i] = w["family"], w["proto"], w["l4_off"]
        if w["code"]:
            out[i] = w["code"]
            continue
        t = w["tuple"]
        scope, kind = (0 if global_map else lxc), T.get_ct_map(t)
        if ctmap is not None:
            state, t, val = T.ct_lookup(ctmap, scope, kind, t)
        else:
            state, t, val = T.CT_NEW, T.tuple_reverse(t), None
        ident = ipcache(w["daddr"]) if ipcache is not None else int(dst_labels[i])
        fi["t"]["identity"], fi["t"]["flags"] = ident, N.CG_L4_F_WALKED
        # the engine evaluates the policy on the reversed tuple's dport whatever the state (cilium_gpu.h)
        dport = t["dport"] if state in (T.CT_NEW, T.CT_ESTABLISHED) else t["sport"]
        fi["t"]["dport"] = dport
        mi, table = slot_tables[lxc]
        verdict, hit = policy_can_egress(table, ident, dport, t["nexthdr"], ignore_drop)
        if hit is not None:
            c = hits.setdefault((mi, hit), [0, 0])
            c[0] += 1
            c[1] += length
        op = T.OP_NONE
        if state not in (T.CT_REPLY, T.CT_RELATED) and verdict < 0:
            if state == T.CT_ESTABLISHED:
                op = T.OP_DELETE
            res = verdict
        else:
            if state == T.CT_NEW:
                op = T.OP_CREATE
            res = verdict if T.redirect_to_proxy(verdict, state) else 0
        out[i] = res
        if ctmap is not None:
            r = rec[i]
            r["state"], r["op"], r["pad0"], r["pad2"][0] = 1 + state, op, 1, hdr["seclabel"]
            if val is not None:
                r["rev_nat_index"], r["loopback"] = val.get("rev_nat_index", 0), val.get("loopback", 0)
            r["key"] = T.key_record(scope, kind, w["family"], t)
    return out, info, rec, l4o, hits


def apply(ctmap: dict, records, pkt_len, src_labels, max_entries):
    """ct_util.apply with the direction of each record: dir 1 is ct_create* as
    CT_EGRESS (tx counters, src_sec_id from the record)."""
    res = np.zeros(len(records), np.int32)
    for i, r in enumerate(records):
        if r["pad0"] != 1:
            res[i] = T.apply(ctmap, records[i:i + 1], pkt_len[i:i + 1], src_labels[i:i + 1], max_entries)[0]
            continue
        if r["op"] == T.OP_NONE:
            continue
        t = T.record_tuple(r)
        scope, kind, family = int(r["key"]["scope"]), int(r["key"]["kind"]), int(r["key"]["family"])
        k = (scope, kind, T.tuple_bytes(t))
        if r["op"] == T.OP_DELETE:
            ctmap.pop(k, None)
            continue
        icmp = dict(t, nexthdr=1 if family == 4 else 58, sport=0, dport=0, flags=t["flags"] | T.TUPLE_F_RELATED)
        kr = (scope, kind, T.tuple_bytes(icmp))
        if len(ctmap) + len({k, kr} - set(ctmap)) > max_entries:
            res[i] = T.DROP_CT_CREATE_FAILED
            continue
        entry = dict(tx_packets=1, tx_bytes=int(pkt_len[i]), src_sec_id=int(r["pad2"][0]), flags=0, family=family)
        ctmap[k] = dict(entry)
        ctmap[kr] = dict(entry, flags=N.CG_CT_E_SEEN_NON_SYN)
    return res


def dump_of(ctmap: dict):
    """The oracle's dict in cg_ct_map_dump's order and fields:
    [(scope, kind, family, tuple bytes, {field: value})]."""
    out = []
    for (scope, kind, tb), v in ctmap.items():
        vals = {f: int(v.get(f, 0)) for f in ("rx_packets", "rx_bytes", "tx_packets", "tx_bytes", "src_sec_id", "flags")}
        out.append((scope, kind, v["family"], tb, vals))
    return sorted(out, key=lambda x: x[:4])


def dump_got(ct):
    keys, vals = ct.dump()
    out = []
    for k, v in zip(keys, vals):
        n = 4 if k["family"] == 4 else 16
        tb = bytes(k["daddr"][:n]) + bytes(k["saddr"][:n]) + struct.pack("<HHBB", int(k["dport"]), int(k["sport"]),
                                                                         int(k["nexthdr"]), int(k["flags"]))
        out.append((int(k["scope"]), int(k["kind"]), int(k["family"]), tb,
                    {f: int(v[f]) for f in ("rx_packets", "rx_bytes", "tx_packets", "tx_bytes", "src_sec_id", "flags")}))
    return sorted(out, key=lambda x: x[:4])


# -------------------------------------------------------- frame builders ----
def mac(s):
    return bytes(int(x, 16) for x in s.split(":"))


def eth(hdr, ethertype, payload, smac=None, dmac=None):
    return (dmac or hdr["node_mac"]) + (smac or hdr["lxc_mac"]) + struct.pack(">H", ethertype) + payload


def ip4(hdr, dst, proto, l4, *, src=None, ihl=5, frag=0, **kw):
    ip = struct.pack(">BBHHHBBH", 0x40 | ihl, 0, 4 * ihl + len(l4), 0, frag, 64, proto, 0) + \
        (hdr["ipv4"] if src is None else ipaddress.ip_address(src).packed) + ipaddress.ip_address(dst).packed
    return eth(hdr, ETH_P_IP, ip + bytes(4 * (ihl - 5)) + l4, **kw)


def ip6(hdr, dst, nexthdr, payload, *, src=None, **kw):
    ip = struct.pack(">IHBB", 0x60000000, len(payload), nexthdr, 64) + \
        (hdr["ipv6"] if src is None else ipaddress.ip_address(src).packed) + ipaddress.ip_address(dst).packed
    return eth(hdr, ETH_P_IPV6, ip + payload, **kw)


def tcp(sport, dport, flags=0x02):
    return struct.pack(">HHIIBBHHH", sport, dport, 1, 0, 0x50, flags, 1000, 0, 0)


def udp(sport, dport, n=8):
    return struct.pack(">HHHH", sport, dport, 8 + n, 0) + bytes(n)


def icmp(type_, code=0, body=b""):
    return struct.pack(">BBHI", type_, code, 0, 0) + body


def reply_of(frame: bytes, mac_src=bytes(6), mac_dst=bytes(6)) -> bytes:
    """The frame a peer sends back: addresses and TCP / UDP ports swapped."""
    f = bytearray(frame)
    f[0:6], f[6:12] = mac_dst, mac_src
    if f[12:14] == b"\x08\x00":
        l4 = 14 + (f[14] & 0xF) * 4
        f[26:30], f[30:34] = frame[30:34], frame[26:30]
    else:
        l4 = 54
        f[22:38], f[38:54] = frame[38:54], frame[22:38]
    f[l4:l4 + 2], f[l4 + 2:l4 + 4] = frame[l4 + 2:l4 + 4], frame[l4:l4 + 2]
    return bytes(f)


def icmp_error_for(frame: bytes, hdr: dict, outward: bool) -> bytes:
    """An ICMP dest-unreach about the IPv4 flow of `frame` (sent by the
    endpoint): outward=True is the endpoint's own error going out to the flow's
    destination, else the error coming in from the destination."""
    src, dst = frame[26:30], frame[30:34]
    body = icmp(3, 1, frame[14:14 + 28])
    a, b = (src, dst) if outward else (dst, src)
    ip = struct.pack(">BBHHHBBH", 0x45, 0, 20 + len(body), 0, 0, 64, 1, 0) + a + b
    if outward:
        return eth(hdr, ETH_P_IP, ip + body)
    return bytes(12) + b"\x08\x00" + ip + body


# ------------------------------------------------------------ the world ----
NODE_MAC, ROUTER_IP6 = mac("02:00:00:00:00:01"), "fd00::1"
EMPTY_SLOT = U.EMPTY_SLOT  # has a header, no map: the missed tail call comes first
NO_HEADER_SLOT = 9         # has a map, no header
# slot -> index into U.build_maps()
SLOT_MAP = {0: 3, 1: 2, 7: 3, 300: 3, 65535: 2, NO_HEADER_SLOT: 1, 11: 0}
HEADER_SPECS = {
    0: dict(mac="0a:00:00:00:00:10", ipv4="10.0.0.10", ipv6="fd00::10", seclabel=1000),
    1: dict(mac="0a:00:00:00:00:11", ipv4=None, ipv6="fd00::11", seclabel=1001),  # no IPv4
    7: dict(mac="0a:00:00:00:00:12", ipv4="10.0.0.12", ipv6="fd00::12", seclabel=1002, verify_smac=False),
    300: dict(mac="0a:00:00:00:00:13", ipv4="10.0.0.13", ipv6="fd00::13", seclabel=0x01020304, verify_dmac=False),
    65535: dict(mac="0a:00:00:00:00:14", ipv4="10.0.0.14", ipv6="fd00::14", seclabel=1004, verify_sip=False),
    11: dict(mac="0a:00:00:00:00:15", ipv4="10.0.0.15", ipv6="fd00::15", seclabel=1005),
    EMPTY_SLOT: dict(mac="0a:00:00:00:00:16", ipv4="10.0.0.16", ipv6="fd00::16", seclabel=1006),
}


def header_record(spec):
    return PolicyArray.header(node_mac=NODE_MAC, router_ip6=ROUTER_IP6, **spec)


def header_dict(rec) -> dict:
    """An ENDPOINT_HEADER_DTYPE record as from_container() takes it."""
    return dict(lxc_mac=bytes(rec["lxc_mac"]), node_mac=bytes(rec["node_mac"]), ipv4=bytes(rec["ipv4"]),
                ipv6=bytes(rec["ipv6"]), router_ip6=bytes(rec["router_ip6"]), seclabel=int(rec["seclabel"]),
                flags=int(rec["flags"]))


@functools.lru_cache(maxsize=None)
def headers():
    return {slot: header_dict(header_record(spec)[0]) for slot, spec in HEADER_SPECS.items()}


@functools.lru_cache(maxsize=None)
def slot_tables():
    dicts = []
    for keys, ports, _ in U.tables():
        dicts.append({(int(k["sec_label"]), int(k["dport"]), int(k["protocol"]), int(k["egress"])): int(p)
                      for k, p in zip(keys, ports)})
    return {slot: (mi, dicts[mi]) for slot, mi in SLOT_MAP.items()}


def build_array(cl, maps):
    arr = cl.policy_array()
    arr.set_many(list(SLOT_MAP), [maps[i] for i in SLOT_MAP.values()])
    slots = list(HEADER_SPECS)
    arr.set_headers(slots, np.concatenate([header_record(HEADER_SPECS[s]) for s in slots]))
    return arr


DST4 = F.SRC4 + ["10.1.2.3"]
DST6 = F.SRC6 + [ROUTER_IP6, ROUTER_IP6]


@functools.lru_cache(maxsize=None)
def shared_frames():
    """(raw, off, pkt_len, dst_labels, lxc_ids) of U.N_TUPLES seeded egress
    frames from the world's endpoints to addresses the ipcache of frames_util
    knows (and some it does not), ports from the tables."""
    ports = np.concatenate([k["dport"][(k["dport"] != 0) & (k["egress"] == 1)] for k, _, _ in U.tables()])
    pool = [0, 1, 7, 300, 65535, 11, 0, 300]
    recs = np.concatenate([header_record(HEADER_SPECS[s]) for s in pool])
    raw, off, wire, lxc = synth.l4_egress_frames(U.N_TUPLES, pool, recs, F._packed(DST4), F._packed(DST6), ports,
                                                 seed=53, min_len=60, max_len=150, mix=(0.5, 0.28, 0.22),
                                                 ext_share=0.3, port_hit=0.8)
    rng = np.random.default_rng(29)
    lxc = lxc.copy()
    r = rng.random(U.N_TUPLES)
    lxc[r < 0.02] = EMPTY_SLOT
    lxc[(r >= 0.02) & (r < 0.04)] = NO_HEADER_SLOT
    ids = np.concatenate([np.arange(1, 6), 256 + np.arange(U.SMALL_IDS), [777, 900_001]]).astype(np.uint32)
    labels = ids[rng.integers(0, len(ids), U.N_TUPLES)]
    pkt_len = wire + rng.integers(0, 3, U.N_TUPLES).astype(np.uint32) * 70_000  # skb->len past 16 bits
    return raw, off, pkt_len, labels, lxc


# resolver combinations: dst_labels or the ipcache
COMBOS = [dict(lab=True), dict(lab=False)]
COMBO_IDS = ["labels", "ipcache"]


def resolver_args(combo, ipc, labels, sl=slice(None)):
    """(keywords for PolicyArray.frame_egress_*, for evaluate())."""
    if combo["lab"]:
        return dict(dst_labels=labels[sl]), dict(dst_labels=labels[sl])
    return dict(ipcache=ipc), dict(ipcache=F.ipcache_fn)


@functools.lru_cache(maxsize=None)
def shared_table(global_map: bool = False):
    """(items, values) of the shared conntrack table, derived from the shared
    frames: every ICMP error frame that reaches the lookup gets the key it
    reads as related; of the others a quarter their reply key, a quarter their
    established key, 5% both."""
    raw, off, pkt_len, labels, lxc = shared_frames()
    rng = np.random.default_rng(77)
    items, values, seen = [], [], set()
    hd, st = headers(), slot_tables()
    for i, skb in enumerate(F.split(raw, off)):
        r = rng.random()
        s = int(lxc[i])
        if s not in st or s not in hd or len(skb) < F.ETH_HLEN:
            continue
        w = from_container(skb, hd[s])
        if w["code"]:
            continue
        t = w["tuple"]
        if t["flags"] & T.TUPLE_F_RELATED:
            wants = ["reply"]
        else:
            wants = ["reply"] if r < 0.25 else ["established"] if r < 0.5 else ["reply", "established"] if r < 0.55 else []
        for want in wants:
            tt = t if want == "reply" else T.tuple_reverse(t)
            it = (0 if global_map else s, T.get_ct_map(tt), w["family"], tt)
            k = (it[0], it[1], T.tuple_bytes(tt))
            if k in seen:
                continue
            seen.add(k)
            items.append(it)
            values.append(dict(rev_nat_index=(len(items) * 7) & 0xFFFF if len(items) % 5 == 0 else 0,
                               loopback=1 if len(items) % 9 == 0 else 0))
    return items, values


@functools.lru_cache(maxsize=None)
def shared_expected(ci: int, ignore_drop: bool, with_ct: bool = True, global_map: bool = False):
    """The oracle's (verdicts, FRAME_INFO, CT_RECORD, l4 offsets, hits) for the shared frames."""
    raw, off, pkt_len, labels, lxc = shared_frames()
    _, b = resolver_args(COMBOS[ci], None, labels)
    ctmap = T.ctmap_of(*shared_table(global_map)) if with_ct else None
    return evaluate(F.split(raw, off), slot_tables(), headers(), lxc_ids=lxc, pkt_len=pkt_len, ignore_drop=ignore_drop,
                    ctmap=ctmap, global_map=global_map, **b)


def extracted_tuples(info):
    """The cg_l4_tuple records the oracle's info describes (for the twin array
    driven through cg_l4_array_verdicts_* with CG_L4_EGRESS) and the mask of
    frames that reached the policy."""
    done = (info["t"]["flags"] & N.CG_L4_F_WALKED) != 0
    t = info["t"][done].copy()
    t["flags"] = 0
    return t, done


# ------------------------------------------------------ the golden cases ----
def load_kat():
    with open(os.path.join(os.path.dirname(__file__), "golden", "l4_egress_kat.json")) as f:
        return json.load(f)


def kat_header_spec(h: dict) -> dict:
    spec = {k: h[k] for k in ("mac", "node_mac", "ipv4", "ipv6", "router_ip6", "seclabel")}
    spec.update({k: h[k] for k in ("verify_smac", "verify_dmac", "verify_sip") if k in h})
    return spec


def kat_world(cl):
    """(array, maps, conntrack map, raw, off, lxc ids, dst labels, cases) of
    l4_egress_kat.json: one slot per header, every slot on the one map."""
    g = load_kat()
    pm, arr = cl.policy_map(), cl.policy_array()
    for p in g["policy"]:
        pm.allow(p["identity"], p["dport"], p["proto"], p["egress"], p["proxy_port"])
    for name, h in g["headers"].items():
        if h.get("map", True):
            arr.set(h["slot"], pm)
        if h.get("header", True):
            arr.set_header(h["slot"], **kat_header_spec(h))
    items = [T.golden_item(e) for c in g["frames"] for e in c.get("entries", [])]
    ct = T.build_map(cl, items)
    raw, off = F.join([bytes.fromhex(c["hex"]) for c in g["frames"]])
    lxc = np.array([g["headers"][c["header"]]["slot"] for c in g["frames"]], np.uint16)
    labels = np.array([c.get("dst_label", g["dst_label"]) for c in g["frames"]], np.uint32)
    return arr, pm, ct, raw, off, lxc, labels, g


def kat_oracle_world(g):
    """(slot_tables, headers, ctmap) of the KAT for evaluate()."""
    table = {(p["identity"], htons(p["dport"]), p["proto"], p["egress"]): htons(p["proxy_port"]) for p in g["policy"]}
    st = {h["slot"]: (0, table) for h in g["headers"].values() if h.get("map", True)}
    hd = {h["slot"]: header_dict(PolicyArray.header(**kat_header_spec(h))[0])
          for h in g["headers"].values() if h.get("header", True)}
    items = [T.golden_item(e) for c in g["frames"] for e in c.get("entries", [])]
    return st, hd, T.ctmap_of(items)


def check_kat(g, v, rec, ignore_drop=False):
    for i, c in enumerate(g["frames"]):
        got = dict(verdict=int(v[i]), state=T.STATE_NAMES[int(rec["state"][i])],
                   op={0: "none", 1: "create", 2: "delete"}[int(rec["op"][i])])
        if ignore_drop:  # the file states the verdict of that build; the ops are those of an allowed packet
            assert c["verdict"] != F.DROP_POLICY or "verdict_ignore_drop" in c, c["name"]
            assert (got["verdict"], got["state"]) == (c.get("verdict_ignore_drop", c["verdict"]), c["state"]), c["name"]
            continue
        assert got == dict(verdict=c["verdict"], state=c["state"], op=c["op"]), c["name"]
        if "key" in c and not ignore_drop:
            assert rec["key"][i] == T.key_record(*T.golden_item(c["key"])), c["name"]
            assert int(rec["pad0"][i]) == 1 and int(rec["pad2"][i][0]) == g["headers"][c["header"]]["seclabel"], c["name"]


# ------------------------------------------- a one-endpoint world ----
def egress_world(cl, ports=((2000, 80, 6, 1, 0),)):
    pm, arr = cl.policy_map(), cl.policy_array()
    for ident, port, proto, egress, proxy in ports:
        pm.allow(ident, port, proto, egress, proxy)
    arr.set(5, pm)
    arr.set_header(5, mac="0a:00:00:00:00:05", node_mac=NODE_MAC, ipv4="10.0.0.5", ipv6="fd00::5",
                   router_ip6=ROUTER_IP6, seclabel=4242)
    return pm, arr, header_dict(arr.get_header(5))



# ---------------------------------------------------------- round trips ----
def check_round_trips(cl, egress, ingress):
    """egress(arr, raw, off, **kw) / ingress(arr, raw, off, **kw) → (verdicts,
    info, records).  No hand-written keys: every entry comes from apply."""
    pm, arr, hd = egress_world(cl, ports=((2000, 53, 17, 1, 0), (2000, 5353, 17, 0, 0)))
    ct = cl.conntrack_map()
    peer_mac = mac("0a:00:00:00:99:99")

    def eg(frame, label=2000):
        raw, off = F.join([frame])
        v, _, rec = egress(arr, raw, off, lxc_ids=[5], dst_labels=[label], conntrack=ct)
        return int(v[0]), rec

    def ing(frame, label=2000):
        raw, off = F.join([frame])
        v, _, rec = ingress(arr, raw, off, lxc_ids=[5], src_labels=[label], conntrack=ct)
        return int(v[0]), rec

    # UDP flows: their related keys live in the ANY map, where an ICMP error looks (a TCP flow's do not)
    # 1. egress request -> apply -> the reply coming in reads REPLY and passes the ingress policy that denies it
    syn = ip4(hd, "10.1.0.1", 17, udp(40000, 53))
    back = reply_of(syn, peer_mac, hd["lxc_mac"])
    v, rec = ing(back)
    assert v == F.DROP_POLICY and rec["state"][0] == N.CG_CT_STATE_NEW  # before: new and denied
    v, rec = eg(syn)
    assert v == 0 and rec["op"][0] == T.OP_CREATE and rec["key"]["flags"][0] == N.CG_TUPLE_F_OUT
    assert ct.apply(rec, [60]).tolist() == [0]
    v, rec = ing(back)
    assert v == 0 and rec["state"][0] == N.CG_CT_STATE_REPLY and rec["op"][0] == T.OP_NONE
    assert eg(syn)[1]["state"][0] == N.CG_CT_STATE_ESTABLISHED
    # 2. an ICMP error for the egress flow reads RELATED, in both directions
    v, rec = ing(icmp_error_for(syn, hd, outward=False))
    assert v == 0 and rec["state"][0] == N.CG_CT_STATE_RELATED
    # 3. ingress request -> apply -> the endpoint's answer going out reads REPLY though egress policy denies it
    req = bytes(6) + peer_mac + syn[12:26] + bytes([10, 1, 0, 9]) + hd["ipv4"] + udp(50000, 5353)
    ans = reply_of(req, hd["lxc_mac"], hd["node_mac"])
    v, rec = eg(ans)
    assert v == F.DROP_POLICY and rec["state"][0] == N.CG_CT_STATE_NEW
    v, rec = ing(req)
    assert v == 0 and rec["op"][0] == T.OP_CREATE and rec["key"]["flags"][0] == N.CG_TUPLE_F_IN
    assert ct.apply(rec, [60], [2000]).tolist() == [0]
    v, rec = eg(ans)
    assert v == 0 and rec["state"][0] == N.CG_CT_STATE_REPLY and rec["pad0"][0] == 1
    # the endpoint's own ICMP error about that flow, going out
    v, rec = eg(icmp_error_for(ans, hd, outward=True))
    assert v == 0 and rec["state"][0] == N.CG_CT_STATE_RELATED
    # the two flows' entries: tx counted on the egress-created pair, rx on the ingress-created one
    _, vals = ct.dump()
    assert sorted(zip(vals["tx_packets"].tolist(), vals["rx_packets"].tolist())) == [(0, 1), (0, 1), (1, 0), (1, 0)]
    for x in (ct, arr, pm):
        x.destroy()
