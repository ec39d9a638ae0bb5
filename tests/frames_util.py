"""What test_l4_frames.py (host evaluator) and test_l4_frames_gpu.py (kernel)
share: a Python restatement of the ingress policy program's header walk, the
two evaluation orders of cg_l4_frames_verdicts_*, and the world they run in
(l4_array_util's maps and slots, an ipcache, an endpoint map).

The restatement follows the reference's own control flow, function by
function (bpf_lxc.c ipv4_policy :890-950 / ipv6_policy :744-816, lib/ipv6.h
ipv6_hdrlen :61-98, lib/ipv4.h :45-61, lib/conntrack.h ct_lookup4 :467-584 /
ct_lookup6 :310-437 and the tuple reversal :439-456, lib/policy.h :46-146,
lib/eps.h :26-46), over skb_load_bytes on a bytes object.  It shares nothing
with csrc/frame_walk.h."""
import functools
import ipaddress
import json
import os

import numpy as np

import l4_array_util as U
from cilium_amd import _native as N
from cilium_amd import synth
from cilium_amd.classifier import ENDPOINT_KEY_DTYPE, FRAME_INFO_DTYPE
from cilium_amd.policy import htons

DROP_POLICY, DROP_INVALID, DROP_CT_INVALID_HDR, DROP_CT_UNKNOWN_PROTO = -133, -134, -135, -137
DROP_UNKNOWN_L3, DROP_MISSED_TAIL_CALL, DROP_INVALID_EXTHDR, DROP_FRAG_NOSUPPORT = -139, -140, -156, -157
NOT_LOCAL, TO_HOST = -1, -2
ETH_HLEN = 14
IPV6_MAX_HEADERS = 4
NEXTHDR_HOP, NEXTHDR_ROUTING, NEXTHDR_FRAGMENT, NEXTHDR_AUTH, NEXTHDR_NONE, NEXTHDR_DEST = 0, 43, 44, 51, 59, 60
WORLD_ID = 2


# ------------------------------------------------------------ the walk ----
def skb_load_bytes(skb: bytes, off: int, n: int):
    """None on failure (off + n past skb->len), else the bytes."""
    return skb[off:off + n] if off + n <= len(skb) else None


def ipv6_hdrlen(skb, l3_off, nexthdr):
    """lib/ipv6.h:61-98 → (len or a negative code, nexthdr)."""
    length = 40
    nh = nexthdr
    for _ in range(IPV6_MAX_HEADERS):
        if nh == NEXTHDR_NONE:
            return DROP_INVALID_EXTHDR, nexthdr
        if nh == NEXTHDR_FRAGMENT:
            return DROP_FRAG_NOSUPPORT, nexthdr
        if nh in (NEXTHDR_HOP, NEXTHDR_ROUTING, NEXTHDR_AUTH, NEXTHDR_DEST):
            opthdr = skb_load_bytes(skb, l3_off + length, 2)
            if opthdr is None:
                return DROP_INVALID, nexthdr
            nh = opthdr[0]
            if nh == NEXTHDR_AUTH:  # tested on the value just assigned
                length += (opthdr[1] + 2) << 2  # ipv6_authlen
            else:
                length += (opthdr[1] + 1) << 3  # ipv6_optlen
            continue
        return length, nh
    return DROP_INVALID_EXTHDR, nexthdr


def ct_lookup(skb, tuple_, l4_off, icmp_proto, echo_request, echo_reply):
    """The head of ct_lookup4 / ct_lookup6 with an empty table and dir =
    CT_INGRESS: fills sport / dport, then the CT_NEW path reverses the tuple.
    Returns 0 or a negative code."""
    nexthdr = tuple_["nexthdr"]
    if nexthdr == icmp_proto:
        type_ = skb_load_bytes(skb, l4_off, 1)
        if type_ is None:
            return DROP_CT_INVALID_HDR
        tuple_["sport"] = tuple_["dport"] = 0
        if type_[0] == echo_reply:
            tuple_["dport"] = echo_request  # a constant assigned to a __be16: no htons
        elif type_[0] == echo_request:
            tuple_["sport"] = type_[0]
    elif nexthdr == 6:
        if skb_load_bytes(skb, l4_off + 12, 2) is None:
            return DROP_CT_INVALID_HDR
        ports = skb_load_bytes(skb, l4_off, 4)
        if ports is None:
            return DROP_CT_INVALID_HDR
        # 4 bytes into &tuple->dport: dport, then sport behind it (common.h struct ipv4_ct_tuple)
        tuple_["dport"], tuple_["sport"] = int.from_bytes(ports[:2], "little"), int.from_bytes(ports[2:], "little")
    elif nexthdr == 17:
        ports = skb_load_bytes(skb, l4_off, 4)
        if ports is None:
            return DROP_CT_INVALID_HDR
        tuple_["dport"], tuple_["sport"] = int.from_bytes(ports[:2], "little"), int.from_bytes(ports[2:], "little")
    else:
        return DROP_CT_UNKNOWN_PROTO
    # __ct_lookup misses (CT_NEW), the tuple is reversed and misses again
    tuple_["sport"], tuple_["dport"] = tuple_["dport"], tuple_["sport"]
    return 0


def walk(skb: bytes, ethertype: int) -> dict:
    """ipv4_policy / ipv6_policy up to the policy call.  code 0: the call's
    arguments are dport / proto / fragment."""
    r = dict(code=0, dport=0, proto=0, fragment=False, l4_off=0, saddr=None)
    tuple_ = dict(nexthdr=0, sport=0, dport=0)
    if ethertype == 0x0800:
        if len(skb) < ETH_HLEN + 20:  # revalidate_data
            return dict(r, code=DROP_INVALID)
        ip4 = skb[ETH_HLEN:ETH_HLEN + 20]
        tuple_["nexthdr"] = r["proto"] = ip4[9]
        r["saddr"] = bytes(ip4[12:16])
        r["l4_off"] = l4_off = ETH_HLEN + (ip4[0] & 0xF) * 4  # ipv4_hdrlen
        # ipv4_is_fragment: frag_off & htons(0xBFFF), the two bytes as they lie
        r["fragment"] = bool(ip4[6] & 0xBF or ip4[7] & 0xFF)
        ret = ct_lookup(skb, tuple_, l4_off, 1, 8, 0)
    else:
        if len(skb) < ETH_HLEN + 40:
            return dict(r, code=DROP_INVALID)
        ip6 = skb[ETH_HLEN:ETH_HLEN + 40]
        tuple_["nexthdr"] = r["proto"] = ip6[6]
        r["saddr"] = bytes(ip6[8:24])
        hdrlen, tuple_["nexthdr"] = ipv6_hdrlen(skb, ETH_HLEN, tuple_["nexthdr"])
        if hdrlen < 0:
            return dict(r, code=hdrlen)
        r["proto"] = tuple_["nexthdr"]
        r["l4_off"] = l4_off = ETH_HLEN + hdrlen
        ret = ct_lookup(skb, tuple_, l4_off, 58, 128, 129)
    if ret < 0:
        return dict(r, code=ret)
    r["dport"] = tuple_["dport"]
    return r


def policy_can_access_ingress(table: dict, src_label, dport, proto, is_fragment, ignore_drop):
    """lib/policy.h:46-146 over {(identity, dport, proto, egress): proxy_port_be}:
    → (verdict, the key that was hit or None)."""
    hit, ret = None, None
    if not is_fragment and (src_label, dport, proto, 0) in table:
        hit = (src_label, dport, proto, 0)
        ret = table[hit]
    elif (src_label, 0, 0, 0) in table:
        hit, ret = (src_label, 0, 0, 0), 0  # TC_ACT_OK
    elif not is_fragment and (0, dport, proto, 0) in table:
        hit = (0, dport, proto, 0)
        ret = table[hit]
    else:
        ret = DROP_FRAG_NOSUPPORT if is_fragment else DROP_POLICY
    if ret < 0:
        ret = 0 if ignore_drop else DROP_POLICY
    return ret, hit


def evaluate(frames, slot_tables, *, lxc_ids=None, endpoints=None, src_labels=None, ipcache=None, pkt_len=None,
             ignore_drop=False):
    """Both evaluation orders.  frames: list of bytes; slot_tables: {lxc_id:
    (map index, table dict)}; endpoints: {address bytes: (lxc_id, flags)};
    ipcache: address bytes → identity.  → (verdicts, FRAME_INFO records,
    l4 offsets, {(map index, key): [packets, bytes]})."""
    n = len(frames)
    out = np.zeros(n, np.int32)
    info = np.zeros(n, FRAME_INFO_DTYPE)
    l4o = np.zeros(n, np.uint32)
    hits = {}
    for i, skb in enumerate(frames):
        length = int(pkt_len[i]) if pkt_len is not None else len(skb)
        rec = info[i]

        def ethertype():
            return int.from_bytes(skb[12:14], "big")

        if endpoints is not None:
            # from-netdev: the endpoint lookup by daddr in front of the tail call
            rec["t"]["len"] = length
            if len(skb) < ETH_HLEN or ethertype() not in (0x0800, 0x86DD):
                out[i] = NOT_LOCAL
                continue
            et = ethertype()
            rec["family"] = 4 if et == 0x0800 else 6
            if len(skb) < ETH_HLEN + (20 if et == 0x0800 else 40):
                out[i] = DROP_INVALID
                continue
            daddr = skb[30:34] if et == 0x0800 else skb[38:54]
            ep = endpoints.get(bytes(daddr))  # lookup_ip{4,6}_endpoint
            if ep is None:
                out[i] = NOT_LOCAL
                continue
            lxc = rec["lxc_id"] = ep[0]
            if ep[1] & N.CG_ENDPOINT_F_HOST:
                out[i] = TO_HOST
                continue
        else:
            lxc = rec["lxc_id"] = int(lxc_ids[i])
        if lxc not in slot_tables:  # tail_call falls through
            out[i] = DROP_MISSED_TAIL_CALL
            continue
        if endpoints is None:
            rec["t"]["len"] = length
            if len(skb) < ETH_HLEN:
                out[i] = DROP_INVALID
                continue
            et = ethertype()
            if et not in (0x0800, 0x86DD):  # handle_policy's switch on skb->protocol
                out[i] = DROP_UNKNOWN_L3
                continue
            rec["family"] = 4 if et == 0x0800 else 6
        w = walk(skb, et)
        rec["t"]["proto"] = w["proto"]
        l4o[i] = w["l4_off"]
        if w["code"]:
            out[i] = w["code"]
            continue
        rec["t"]["dport"] = w["dport"]
        rec["t"]["flags"] = N.CG_L4_F_INGRESS | (N.CG_L4_F_FRAGMENT if w["fragment"] else 0)
        label = ipcache(w["saddr"]) if ipcache is not None else int(src_labels[i])
        rec["t"]["identity"] = label
        mi, table = slot_tables[lxc]
        out[i], hit = policy_can_access_ingress(table, label, w["dport"], w["proto"], w["fragment"], ignore_drop)
        if hit is not None:
            c = hits.setdefault((mi, hit), [0, 0])
            c[0] += 1
            c[1] += length
    return out, info, l4o, hits


# ----------------------------------------------------------- the world ----
def split(raw, off):
    raw = np.asarray(raw, np.uint8)
    return [raw[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(off) - 1)]


def join(frames):
    off = np.zeros(len(frames) + 1, np.uint64)
    np.cumsum([len(f) for f in frames], out=off[1:])
    return np.frombuffer(b"".join(frames), np.uint8).copy(), off


@functools.lru_cache(maxsize=None)
def slot_tables():
    """{lxc_id: (index into build_maps(), {(id, dport, proto, egress): proxy_port_be})}."""
    dicts = []
    for keys, ports, _ in U.tables():
        dicts.append({(int(k["sec_label"]), int(k["dport"]), int(k["protocol"]), int(k["egress"])): int(p)
                      for k, p in zip(keys, ports)})
    return {slot: (mi, dicts[mi]) for slot, mi in U.SLOT_MAP.items()}


# endpoint addresses: every slot of l4_array_util (the empty one included), and the host
EP4 = {f"10.0.0.{10 + i}": (s, 0) for i, s in enumerate(U.SLOTS)}
EP4["10.0.0.1"] = (0, N.CG_ENDPOINT_F_HOST)
EP6 = {f"fd00::{10 + i:x}": (s, 0) for i, s in enumerate(U.SLOTS)}
EP6["fd00::1"] = (0, N.CG_ENDPOINT_F_HOST)
NOT_LOCAL4, NOT_LOCAL6 = ["10.0.9.9", "192.0.2.1"], ["fd00::9:9", "2001:db8::1"]

# ipcache: identities the tables know (256.., 1..5, 777) behind prefixes of several lengths
IPCACHE = [("10.1.0.0/16", 256), ("10.1.2.0/24", 257), ("10.1.2.3/32", 777), ("10.1.2.4/32", 258),
           ("10.2.0.0/15", 4), ("172.16.5.0/28", 300), ("172.16.5.7/32", 0), ("0.0.0.0/0", 5),
           ("fd01::/16", 256), ("fd01:0:0:1::/64", 259), ("fd01::1:0:0:0:7/128", 777), ("fd01:0:0:2::/64", 0),
           ("fd02::/64", 1)]
SRC4 = ["10.1.9.9", "10.1.2.9", "10.1.2.3", "10.1.2.4", "10.3.3.3", "172.16.5.3", "172.16.5.7", "8.8.8.8"]
SRC6 = ["fd01::5", "fd01:0:0:1::5", "fd01:0:0:1::7", "fd01:0:0:2::1", "fd02::9", "2001:db8::7", "fd01::1:0:0:0:7"]


def _packed(addrs):
    return np.array([list(ipaddress.ip_address(a).packed) for a in addrs], np.uint8)


def build_endpoints(cl):
    ep = cl.endpoint_map()
    for table in (EP4, EP6):
        addrs = list(table)
        ep.write_endpoints(addrs, [table[a][0] for a in addrs], np.array([table[a][1] for a in addrs], np.uint32))
    return ep


def endpoints_dict():
    return {ipaddress.ip_address(a).packed: v for t in (EP4, EP6) for a, v in t.items()}


def build_ipcache(cl):
    ipc = cl.ipcache()
    ipc.update([c for c, _ in IPCACHE], [[i, 0] for _, i in IPCACHE])
    return ipc


def ipcache_fn(addr: bytes) -> int:
    """lookup_ip{4,6}_remote_endpoint as its callers resolve it: the longest
    covering prefix's sec_label, WORLD_ID on a miss or a zero label."""
    a = ipaddress.ip_address(addr)
    best = None
    for cidr, ident in IPCACHE:
        net = ipaddress.ip_network(cidr)
        if net.version == a.version and a in net and (best is None or net.prefixlen > best[0]):
            best = (net.prefixlen, ident)
    return best[1] if best and best[1] else WORLD_ID


@functools.lru_cache(maxsize=None)
def shared_frames():
    """(raw, off, pkt_len, src_labels, lxc_ids) of U.N_TUPLES seeded frames to
    the world's endpoints and a few foreign addresses, ports drawn from the
    tables, lengths varied so that the starts cover every residue mod 16."""
    ports = np.concatenate([k["dport"][k["dport"] != 0] for k, _, _ in U.tables()])
    raw, off, wire = synth.l4_frames(U.N_TUPLES, _packed(list(EP4) + NOT_LOCAL4), _packed(list(EP6) + NOT_LOCAL6),
                                     _packed(SRC4), _packed(SRC6), ports, seed=31, min_len=60, max_len=150,
                                     mix=(0.6, 0.25, 0.15), ext_share=0.3)
    rng = np.random.default_rng(17)
    ids = np.concatenate([np.arange(1, 6), 256 + np.arange(U.SMALL_IDS), [777, 900_001]]).astype(np.uint32)
    labels = ids[rng.integers(0, len(ids), U.N_TUPLES)]
    lxc = np.array(U.SLOTS, np.uint16)[rng.integers(0, len(U.SLOTS), U.N_TUPLES)]
    pkt_len = wire + rng.integers(0, 3, U.N_TUPLES).astype(np.uint32) * 70_000  # skb->len past 16 bits
    return raw, off, pkt_len, labels, lxc


COMBOS = [dict(lxc=True, lab=True), dict(lxc=True, lab=False), dict(lxc=False, lab=True), dict(lxc=False, lab=False)]


def resolver_args(combo, ep, ipc, lxc, labels, sl=slice(None)):
    """(keyword arguments for PolicyArray.frame_verdicts, for evaluate())."""
    a, b = {}, {}
    if combo["lxc"]:
        a["lxc_ids"] = b["lxc_ids"] = lxc[sl]
    else:
        a["endpoints"], b["endpoints"] = ep, endpoints_dict()
    if combo["lab"]:
        a["src_labels"] = b["src_labels"] = labels[sl]
    else:
        a["ipcache"], b["ipcache"] = ipc, ipcache_fn
    return a, b


def load_kat():
    with open(os.path.join(os.path.dirname(__file__), "golden", "l4_frames_kat.json")) as f:
        return json.load(f)


# the KAT's world: one map in slot 5, every frame from identity 1000
KAT_SLOT, KAT_LABEL = 5, 1000
KAT_KEYS = [(1000, 80, 6), (1000, 53, 17), (1000, None, 1), (1000, None, 58)]  # None: the raw echo-request dport


def kat_table():
    """The KAT map as policy_can_access_ingress() takes it."""
    return {(i, htons(p) if p is not None else (8 if pr == 1 else 128), pr, 0): 0 for i, p, pr in KAT_KEYS}


def build_kat_map(cl):
    pm = cl.policy_map()
    for ident, port, proto in KAT_KEYS:
        # allow() takes host order and stores htons(): the echo keys are stored as the raw 8 / 128
        pm.allow(ident, port if port is not None else htons(8 if proto == 1 else 128), proto, 0, 0)
    return pm
