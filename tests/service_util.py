"""What test_l4_service.py (host evaluator, service map, apply) and
test_l4_service_gpu.py (kernel) share: a Python restatement of the service
steps of the from-container program, on top of egress_util / ct_util, the
service world and the shared service batch.

The restatement follows the reference function by function:
lb{4,6}_extract_key (lib/lb.h:590-602, :334-349), lb{4,6}_lookup_service
(:604-635, :351-380), lb{4,6}_local (:700-775, :426-483) with ct_lookup4/6 as
CT_SERVICE (lib/conntrack.h:467-590, :310-437), lb*_select_slave (:158-190,
:124-156), lb*_lookup_slave (:637-651, :382-396), the tuple's part of
lb{4,6}_xlate (:653-697, :398-424), lb{4,6}_rev_nat with flags 0 (:485-576,
:254-317), handle_ipv4_from_lxc / ipv6_l3_from_lxc around them
(bpf_lxc.c:468-570, :148-266), and ct_create4/6 / ct_update{4,6}_slave
(conntrack.h:600-772) for apply.  The key is a dict that the functions mutate
as the C mutates *key.  It shares nothing with csrc/lb_walk.h.

A services map here is {(family, address bytes, dport, slave): dict(target,
port, count, rev_nat, weight)}, a reverse-NAT map {(family, index): (address
bytes, port)}; ports as the datapath stores them."""
import functools
import ipaddress
import json
import os
import struct

import numpy as np

import ct_util as T
import egress_util as E
import frames_util as F
import l4_array_util as U
from cilium_amd import _native as N
from cilium_amd.classifier import CT_RECORD_DTYPE, FRAME_INFO_DTYPE, LB_XLATE_DTYPE, ConntrackMap
from cilium_amd.policy import htons

DROP_NO_SERVICE = -158
CT_SERVICE = 2
OP_UPDATE_SLAVE = 3
NONE, MISS, TRANSLATED, NO_SERVICE = 0, 1, 2, 3
F_L3, F_PORT, F_LOOPBACK, F_REVNAT = 1, 2, 4, 8


# ------------------------------------------------------------ lib/lb.h ----
def kb(family, key):
    return family, key["address"], key["dport"], key["slave"]


def lb_lookup_service(svcmap, family, key):
    """lb{4,6}_lookup_service: LB_L4 then LB_L3; key["dport"] is zeroed as the C zeroes it."""
    if key["dport"]:
        svc = svcmap.get(kb(family, key))
        if svc is not None and svc["count"] != 0:
            return svc
        key["dport"] = 0
    svc = svcmap.get(kb(family, key))
    if svc is not None and svc["count"] != 0:
        return svc
    return None


def lb_lookup_slave(svcmap, family, key, slave):
    key["slave"] = slave
    return svcmap.get(kb(family, key))


def lb_select_slave(hash_, count):
    return hash_ % count + 1  # the weighted branch is #if 0


def service_key_hash(scope, kind, family, t):
    """What a NULL hash stands for: the engine's hash of the CT_SERVICE key."""
    return int(ConntrackMap.key_hashes(T.key_record(scope, kind, family, t).reshape(1))[0])


def lb_local(world, ctmap, scope, skb, family, l4_off, key, tuple_, svc, state, saddr, hash_):
    """lb4_local / lb6_local.  tuple_: dict(daddr, saddr, nexthdr), mutated.
    → (ret, the CT_SERVICE step's (ct state, op, slave, key tuple) or None)."""
    t = T.load_tuple(skb, family, l4_off, tuple_["nexthdr"])  # the head of ct_lookup*
    if not isinstance(t, dict):
        return DROP_NO_SERVICE, None
    t["flags"] |= T.TUPLE_F_SERVICE  # dir == CT_SERVICE: TUPLE_F_SERVICE where the others put OUT / IN
    kind = T.get_ct_map(t)
    entry = ctmap.get((scope, kind, T.tuple_bytes(t)))
    op = T.OP_NONE
    if entry is not None:
        ret = T.CT_RELATED if t["flags"] & T.TUPLE_F_RELATED else T.CT_REPLY
        state["rev_nat_index"], state["loopback"] = entry.get("rev_nat_index", 0), entry.get("loopback", 0)
        state["slave"] = entry.get("slave", 0)
    else:
        ret = T.CT_NEW  # no reversal for CT_SERVICE
        if hash_ is None:
            hash_ = service_key_hash(scope, kind, family, t)
        state["slave"] = lb_select_slave(hash_, svc["count"])
        op = T.OP_CREATE  # ct_create*(CT_SERVICE): carried out by apply
    if hash_ is None:
        hash_ = service_key_hash(scope, kind, family, t)
    rec = [ret, op, state["slave"], kind, t]
    svc = lb_lookup_slave(world["services"], family, key, state["slave"])
    if svc is None:
        svc = lb_lookup_service(world["services"], family, key)
        if svc is None:
            return DROP_NO_SERVICE, rec
        state["slave"] = lb_select_slave(hash_, svc["count"])
        if op == T.OP_NONE:
            rec[1] = OP_UPDATE_SLAVE  # ct_update*_slave
        rec[2] = state["slave"]
    state["rev_nat_index"] = svc["rev_nat"]
    new_saddr = None
    if family == 4:
        state["addr"] = svc["target"]
        if saddr == svc["target"]:
            new_saddr = world["loopback"]
            state["loopback"] = 1
            state["addr"] = new_saddr
            state["svc_addr"] = saddr
        if not state["loopback"]:
            tuple_["daddr"] = svc["target"]
    else:
        tuple_["daddr"] = svc["target"]
    # lb*_xlate: the packet
    state["pkt_daddr"] = svc["target"]
    if new_saddr is not None and new_saddr != bytes(4):
        state["pkt_saddr"] = new_saddr
    if svc["port"] and key["dport"] != svc["port"] and tuple_["nexthdr"] in (6, 17):
        state["pkt_dport"] = svc["port"]  # l4_modify_port
        state["port_rewritten"] = True
    return 0, rec


def new_state():
    return dict(rev_nat_index=0, loopback=0, slave=0, addr=bytes(4), svc_addr=bytes(4))


def evaluate(frames, slot_tables, headers, world, *, lxc_ids, ipcache, ctmap, hash=None, pkt_len=None,
             ignore_drop=False, global_map=False):
    """egress_util.evaluate with the service steps in their place.  world:
    dict(services, revnat, loopback).  → (verdicts, FRAME_INFO, CT_EGRESS
    records, CT_SERVICE records, LB_XLATE records, l4 offsets, hits)."""
    n = len(frames)
    out, info = np.zeros(n, np.int32), np.zeros(n, FRAME_INFO_DTYPE)
    rec, srec = np.zeros(n, CT_RECORD_DTYPE), np.zeros(n, CT_RECORD_DTYPE)
    xl, l4o, hits = np.zeros(n, LB_XLATE_DTYPE), np.zeros(n, np.uint32), {}
    for i, skb in enumerate(frames):
        lxc = int(lxc_ids[i])
        fi = info[i]
        fi["lxc_id"] = lxc
        if lxc not in slot_tables:
            out[i] = F.DROP_MISSED_TAIL_CALL
            continue
        if lxc not in headers:
            out[i] = E.NO_HEADER
            continue
        length = int(pkt_len[i]) if pkt_len is not None else len(skb)
        fi["t"]["len"] = length
        if len(skb) < F.ETH_HLEN:
            out[i] = F.DROP_INVALID
            continue
        hdr = headers[lxc]
        w = E.from_container(skb, hdr)
        fi["family"], fi["t"]["proto"], l4o[i] = w["family"], w["proto"], w["l4_off"]
        head_failed = w["code"] in (F.DROP_CT_INVALID_HDR, F.DROP_CT_UNKNOWN_PROTO)  # from_container got past step 7
        if w["code"] and not head_failed:
            out[i] = w["code"]
            continue
        family, nexthdr, l4_off = w["family"], w["proto"], w["l4_off"]
        n_a = 4 if family == 4 else 16
        src = bytes(skb[26:30]) if family == 4 else bytes(skb[22:38])
        tuple_ = dict(daddr=w["daddr"], saddr=src, nexthdr=nexthdr)
        scope = 0 if global_map else lxc
        st_new = new_state()
        st_new.update(pkt_daddr=tuple_["daddr"], pkt_saddr=src, pkt_dport=None)
        x = xl[i]
        # lb*_extract_key; DROP_UNKNOWN_L4 goes to skip_service_lookup
        if E.extract_l4_port(skb, nexthdr, l4_off) == 0:
            key = dict(address=tuple_["daddr"], dport=0, slave=0)
            if nexthdr in (6, 17):
                key["dport"] = struct.unpack("<H", F.skb_load_bytes(skb, l4_off + 2, 2))[0]
            st_new["pkt_dport"] = key["dport"]
            svc = lb_lookup_service(world["services"], family, key)
            x["status"] = MISS
            if svc is not None:
                if key["dport"] == 0:
                    x["flags"] |= F_L3
                ret, sr = lb_local(world, ctmap, scope, skb, family, l4_off, key, tuple_, svc, st_new, src,
                                   None if hash is None else int(hash[i]))
                if sr is not None:
                    r = srec[i]
                    r["state"], r["op"], r["pad0"], r["pad1"] = 1 + sr[0], sr[1], CT_SERVICE, sr[2]
                    r["key"] = T.key_record(scope, sr[3], family, sr[4])
                    x["slave"] = sr[2]
                if ret < 0:
                    x["status"] = NO_SERVICE
                    out[i] = ret
                    continue
                x["status"] = TRANSLATED
                if st_new["loopback"]:
                    x["flags"] |= F_LOOPBACK
                if st_new.get("port_rewritten"):
                    x["flags"] |= F_PORT
        if head_failed:
            out[i] = w["code"]
            continue
        # ct_lookup* as CT_EGRESS on tuple.daddr after lb*_local, the ports re-read from the rewritten packet
        t = T.load_tuple(skb, family, l4_off, nexthdr)
        t["flags"] |= T.TUPLE_F_IN
        t["daddr"] = tuple_["daddr"]
        if nexthdr in (6, 17) and x["status"] == TRANSLATED:
            t["sport"] = st_new["pkt_dport"]  # the bytes at l4_off + 2 land in tuple.sport
        kind = T.get_ct_map(t)
        state, t, val = T.ct_lookup(ctmap, scope, kind, t)
        ident = ipcache(tuple_["daddr"])  # orig_dip
        fi["t"]["identity"], fi["t"]["flags"] = ident, N.CG_L4_F_WALKED
        dport = t["dport"] if state in (T.CT_NEW, T.CT_ESTABLISHED) else t["sport"]
        fi["t"]["dport"] = dport
        mi, table = slot_tables[lxc]
        verdict, hit = E.policy_can_egress(table, ident, dport, t["nexthdr"], ignore_drop)
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
        r = rec[i]
        r["state"], r["op"], r["pad0"], r["pad2"][0] = 1 + state, op, 1, hdr["seclabel"]
        if val is not None:
            r["rev_nat_index"], r["loopback"] = val.get("rev_nat_index", 0), val.get("loopback", 0)
        r["key"] = T.key_record(scope, kind, family, t)
        translated = x["status"] == TRANSLATED
        if op == T.OP_CREATE and translated:  # ct_create*(CT_EGRESS, &ct_state_new)
            r["rev_nat_index"], r["loopback"], r["pad1"] = st_new["rev_nat_index"], st_new["loopback"], st_new["slave"]
            r["pad2"][1] = int.from_bytes(st_new["addr"], "little")
            r["pad3"] = int.from_bytes(st_new["svc_addr"], "little")
        l4 = nexthdr in (6, 17)
        pkt_sport = struct.unpack("<H", skb[l4_off:l4_off + 2])[0] if l4 else 0
        pkt_d, pkt_s = st_new["pkt_daddr"], st_new["pkt_saddr"]
        rn = int(r["rev_nat_index"])
        reported = False
        if state in (T.CT_REPLY, T.CT_RELATED) and rn:  # lb{4,6}_rev_nat(…, flags 0)
            nat = world["revnat"].get((family, rn))
            if nat is not None:
                reported = True
                if nat[1] and l4:  # reverse_map_l4_port
                    pkt_sport = nat[1]
                if family == 4 and r["loopback"]:
                    pkt_d = pkt_s  # the old source is the new destination
                pkt_s = nat[0]
                x["flags"] |= F_REVNAT
        if translated or reported:
            x["rev_nat_index"] = st_new["rev_nat_index"] if translated else rn
            if reported:
                x["rev_nat_index"] = rn
            x["dport"] = st_new["pkt_dport"] if l4 else 0
            x["sport"], x["family"] = pkt_sport, family
            x["daddr"][:n_a] = np.frombuffer(pkt_d, np.uint8)
            x["saddr"][:n_a] = np.frombuffer(pkt_s, np.uint8)
    return out, info, rec, srec, xl, l4o, hits


# ------------------------------------------------------------- apply ----
def apply(ctmap: dict, records, pkt_len, src_labels, max_entries):
    """cg_ct_map_apply with the fields the service route fills: ct_create4/6
    with the record's ct_state for any dir, ct_update{4,6}_slave."""
    res = np.zeros(len(records), np.int32)
    for i, r in enumerate(records):
        if r["op"] == T.OP_NONE:
            continue
        t = T.record_tuple(r)
        scope, kind, family = int(r["key"]["scope"]), int(r["key"]["kind"]), int(r["key"]["family"])
        k = (scope, kind, T.tuple_bytes(t))
        if r["op"] == T.OP_DELETE:
            ctmap.pop(k, None)
            continue
        if r["op"] == OP_UPDATE_SLAVE:
            if k in ctmap:
                ctmap[k]["slave"] = int(r["pad1"])
            continue
        dir_ = int(r["pad0"])
        keys = [k]
        addr = int(r["pad2"][1]).to_bytes(4, "little")
        if family == 4 and dir_ == 1 and addr != bytes(4):  # conntrack.h:725-753
            t2 = dict(t, daddr=addr)
            if r["loopback"]:
                t2.update(flags=T.TUPLE_F_IN, saddr=int(r["pad3"]).to_bytes(4, "little"))
            keys.append((scope, kind, T.tuple_bytes(t2)))
        icmp = dict(t, nexthdr=1 if family == 4 else 58, sport=0, dport=0, flags=t["flags"] | T.TUPLE_F_RELATED)
        kr = (scope, kind, T.tuple_bytes(icmp))
        if len(ctmap) + len(set(keys + [kr]) - set(ctmap)) > max_entries:
            res[i] = T.DROP_CT_CREATE_FAILED
            continue
        if dir_ == 0:
            entry = dict(rx_packets=1, rx_bytes=int(pkt_len[i]), src_sec_id=int(src_labels[i]))
        else:
            entry = dict(tx_packets=1, tx_bytes=int(pkt_len[i]), src_sec_id=int(r["pad2"][0]) if dir_ == 1 else 0)
        entry.update(flags=N.CG_CT_E_LB_LOOPBACK if r["loopback"] else 0, family=family,
                     rev_nat_index=int(r["rev_nat_index"]), loopback=int(r["loopback"]), slave=int(r["pad1"]))
        for kk in keys:
            ctmap[kk] = dict(entry)
        ctmap[kr] = dict(entry, flags=entry["flags"] | N.CG_CT_E_SEEN_NON_SYN)
    return res


DUMP_FIELDS = ("rx_packets", "rx_bytes", "tx_packets", "tx_bytes", "src_sec_id", "flags", "rev_nat_index", "slave")


def dump_of(ctmap: dict):
    """The oracle's dict in cg_ct_map_dump's order and fields (an entry the
    table started with says `loopback`, one that apply wrote has `flags`)."""
    out = []
    for (s, k, tb), v in ctmap.items():
        vals = {f: int(v.get(f, 0)) for f in DUMP_FIELDS}
        if "flags" not in v and v.get("loopback"):
            vals["flags"] = N.CG_CT_E_LB_LOOPBACK
        out.append((s, k, v["family"], tb, vals))
    return sorted(out, key=lambda x: x[:4])


def dump_got(ct):
    keys, vals = ct.dump()
    out = []
    for k, v in zip(keys, vals):
        n = 4 if k["family"] == 4 else 16
        tb = bytes(k["daddr"][:n]) + bytes(k["saddr"][:n]) + struct.pack("<HHBB", int(k["dport"]), int(k["sport"]),
                                                                         int(k["nexthdr"]), int(k["flags"]))
        out.append((int(k["scope"]), int(k["kind"]), int(k["family"]), tb, {f: int(v[f]) for f in DUMP_FIELDS}))
    return sorted(out, key=lambda x: x[:4])


# ------------------------------------------------------------ the world ----
LOOPBACK = "10.0.0.250"


def pk(a):
    return ipaddress.ip_address(a).packed


def fam(a):
    return 4 if len(a) == 4 else 6


def world_of(services, revnat, loopback=LOOPBACK):
    """services: [(addr, dport host order, slave, target or None, port host order, count, rev_nat, weight)];
    revnat: [(index, addr, port host order)]."""
    sv = {}
    for a, dport, slave, target, port, count, rn, weight in services:
        ap = pk(a)
        sv[(fam(ap), ap, htons(dport), slave)] = dict(target=pk(target) if target else bytes(len(ap)), port=htons(port),
                                                      count=count, rev_nat=rn, weight=weight)
    return dict(services=sv, revnat={(fam(pk(a)), i): (pk(a), htons(p)) for i, a, p in revnat}, loopback=pk(loopback))


def build_service_map(cl, world):
    svc = cl.service_map(ipv4_loopback=str(ipaddress.ip_address(world["loopback"])))
    ks = [svc.key(a, d, s) for (_, a, d, s) in world["services"]]
    vs = [svc.value(v["target"], v["port"], v["count"], v["rev_nat"], v["weight"]) for v in world["services"].values()]
    if ks:
        svc.update(ks, vs)
    for (f, i), (a, p) in world["revnat"].items():
        svc.update_revnat([i], [a], [p])
    return svc


def values_array(values):
    """ct_util.values_array plus the slave."""
    v = T.values_array(values)
    for i, d in enumerate(values):
        v["slave"][i] = d.get("slave", 0)
    return v


def build_ct(cl, items, values, **kw):
    ct = cl.conntrack_map(**kw)
    if items:
        ct.update(T.keys_array(items), values_array(values))
    return ct


# The VIPs are destinations of egress_util.shared_frames(); what stands behind
# each is chosen so that the shared batch reaches every path of the steps.
VIP4 = [F.SRC4[0], F.SRC4[1], F.SRC4[2], F.SRC4[3]]
VIP6 = [F.SRC6[0], F.SRC6[1]]


def _ports_to(frames, vip):
    """The TCP / UDP destination ports (host order) of the IPv4 frames sent to vip."""
    ports = set()
    for skb in frames:
        if len(skb) >= 38 and skb[12:14] == b"\x08\x00" and bytes(skb[30:34]) == pk(vip) and skb[23] in (6, 17):
            l4 = 14 + (skb[14] & 0xF) * 4
            if len(skb) >= l4 + 4:
                ports.add(int.from_bytes(skb[l4 + 2:l4 + 4], "big"))
    return sorted(ports)


@functools.lru_cache(maxsize=None)
def shared_world():
    """The services over the shared egress batch's destinations:
    VIP4[0]  an L3 service, three backends, one of them the sender 10.0.0.10 (the loopback case), port kept;
    VIP4[1]  on every second port an L4 master with count 0 (passed over), on every fourth an L4 service of
             its own, and behind them an L3 service whose backends rewrite the port;
    VIP4[2]  an L3 service of count 2 whose slave 2 is missing: the 7d fallback fails;
    VIP4[3]  L4 services of count 2 whose slave 2 is missing while a raw {VIP, 0, 2} with a count exists: the
             7d fallback re-selects; no L3 master, so ICMP to it misses;
    VIP6[0]  an L3 service, two backends, port rewritten.  Every other destination misses."""
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    frames = F.split(raw, off)
    p1, p3 = _ports_to(frames, VIP4[1]), _ports_to(frames, VIP4[3])
    sv = [
        (VIP4[0], 0, 0, None, 0, 3, 0, 0),
        (VIP4[0], 0, 1, "10.3.3.3", 0, 0, 11, 0),
        (VIP4[0], 0, 2, "10.0.0.10", 0, 0, 11, 0),
        (VIP4[0], 0, 3, "172.16.5.3", 0, 0, 11, 0),
        (VIP4[1], 0, 0, None, 0, 2, 0, 0),
        (VIP4[1], 0, 1, "10.3.3.3", 8080, 0, 12, 0),
        (VIP4[1], 0, 2, "8.8.8.8", 9090, 0, 12, 5),
        (VIP4[2], 0, 0, None, 0, 2, 0, 0),
        (VIP4[2], 0, 1, "172.16.5.7", 0, 0, 13, 0),
        (VIP4[3], 0, 2, "172.16.5.7", 53, 1, 14, 0),
        (VIP6[0], 0, 0, None, 0, 2, 0, 0),
        (VIP6[0], 0, 1, "fd01:0:0:1::7", 8443, 0, 21, 0),
        (VIP6[0], 0, 2, "fd02::9", 8443, 0, 21, 0),
    ]
    sv += [(VIP4[1], p, 0, None, 0, 0, 0, 0) for p in p1[::2]]
    for p in p1[1::4]:
        sv += [(VIP4[1], p, 0, None, 0, 1, 0, 0), (VIP4[1], p, 1, "172.16.5.3", p, 0, 15, 0)]
    for p in p3:
        sv += [(VIP4[3], p, 0, None, 0, 2, 0, 0), (VIP4[3], p, 1, "10.3.3.3", 0, 0, 14, 0)]
    rn = [(11, VIP4[0], 0), (12, VIP4[1], 80), (13, VIP4[2], 0), (21, VIP6[0], 443), (35, "10.9.9.9", 4000),
          (36, "fd00::abcd", 0)]
    return world_of(sv, rn)


@functools.lru_cache(maxsize=None)
def shared_hash():
    return np.random.default_rng(404).integers(0, 1 << 32, U.N_TUPLES, dtype=np.uint64).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def shared_table(global_map: bool = False):
    """(items, values) of the conntrack table under the shared service batch:
    egress_util.shared_table() (with rev_nat indices that have reverse-NAT
    entries, some that have none), plus CT_SERVICE entries derived from the
    frames that hit a service: a third of them get their service key with a
    slave, so that they read REPLY (ICMP errors: RELATED)."""
    items, values = E.shared_table(global_map)
    items, values = list(items), [dict(v) for v in values]
    rn_pool = [11, 12, 35, 36, 21, 99]
    for j, v in enumerate(values):
        if v["rev_nat_index"]:
            v["rev_nat_index"] = rn_pool[j % len(rn_pool)]
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    world, rng = shared_world(), np.random.default_rng(91)
    hd, st, seen = E.headers(), E.slot_tables(), set()
    for i, skb in enumerate(F.split(raw, off)):
        s = int(lxc[i])
        if s not in st or s not in hd or len(skb) < F.ETH_HLEN:
            continue
        w = E.from_container(skb, hd[s])
        if w["code"] or not any(k[0] == w["family"] and k[1] == w["daddr"] for k in world["services"]):
            continue
        r = rng.random()
        t = dict(w["tuple"], flags=(w["tuple"]["flags"] & T.TUPLE_F_RELATED) | T.TUPLE_F_SERVICE)
        if not (t["flags"] & T.TUPLE_F_RELATED or r < 0.34):
            continue
        it = (0 if global_map else s, T.get_ct_map(t), w["family"], t)
        k = (it[0], it[1], T.tuple_bytes(t))
        if k in seen:
            continue
        seen.add(k)
        items.append(it)
        values.append(dict(rev_nat_index=0, loopback=0, slave=1 + len(items) % 3))
    return items, values


def ctmap_of(items, values):
    return T.ctmap_of(items, values)


@functools.lru_cache(maxsize=None)
def shared_expected(with_hash: bool, ignore_drop: bool = False, global_map: bool = False, empty: bool = False):
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    world = world_of([], []) if empty else shared_world()
    items, values = E.shared_table(global_map) if empty else shared_table(global_map)
    return evaluate(F.split(raw, off), E.slot_tables(), E.headers(), world, lxc_ids=lxc, ipcache=F.ipcache_fn,
                    ctmap=ctmap_of(items, values), hash=shared_hash() if with_hash else None, pkt_len=pkt_len,
                    ignore_drop=ignore_drop, global_map=global_map)


WINDOWS = [(3, 1), (5, 63), (7, 64), (11, 65), (13, 1000)]


def assert_same(got, exp, sl=slice(None), what=""):
    """(verdicts, info, records, svc_records, xlate) byte for byte."""
    names = ("verdicts", "info", "records", "svc_records", "xlate")
    for name, g, e in zip(names, got, exp):
        e = e[sl]
        if g.tobytes() != e.tobytes():
            bad = [i for i in range(len(g)) if g[i:i + 1].tobytes() != e[i:i + 1].tobytes()]
            raise AssertionError(f"{what}{name} differ at {bad[:5]} of {len(bad)}: got {g[bad[0]]} want {e[bad[0]]}")


# ------------------------------------------------------ the golden cases ----
def load_kat():
    with open(os.path.join(os.path.dirname(__file__), "golden", "l4_service_kat.json")) as f:
        return json.load(f)


def kat_world(g):
    return world_of([tuple(s) for s in g["services"]], [tuple(r) for r in g["revnat"]], g["loopback"])


STATUS_NAMES = {NONE: "none", MISS: "miss", TRANSLATED: "translated", NO_SERVICE: "no-service"}
FLAG_NAMES = {F_L3: "l3", F_PORT: "port", F_LOOPBACK: "loopback", F_REVNAT: "revnat"}
OP_NAMES = {0: "none", 1: "create", 2: "delete", 3: "update_slave"}


def kat_ct_items(g):
    items, values = [], []
    for c in g["frames"]:
        for e in c["entries"]:
            it = T.golden_item(dict(e, dport=htons(e["dport"]), sport=htons(e["sport"])))
            items.append(it)
            values.append(dict(rev_nat_index=e.get("rev_nat_index", 0), slave=e.get("slave", 0)))
    return items, values


def kat_setup(cl):
    """(array, policy map, ipcache, conntrack map, service map, raw, off, lxc ids, hashes, cases) of l4_service_kat.json."""
    g = load_kat()
    h = g["header"]
    pm, arr, ipc = cl.policy_map(), cl.policy_array(), cl.ipcache()
    for p in g["policy"]:
        pm.allow(p["identity"], p["dport"], p["proto"], 1, p["proxy_port"])
    arr.set(h["slot"], pm)
    arr.set_header(h["slot"], **{k: h[k] for k in h if k != "slot"})
    for cidr, ident in g["ipcache"]:
        ipc.upsert(cidr, ident)
    ct = build_ct(cl, *kat_ct_items(g))
    svc = build_service_map(cl, kat_world(g))
    raw, off = F.join([bytes.fromhex(c["hex"]) for c in g["frames"]])
    lxc = np.full(len(g["frames"]), h["slot"], np.uint16)
    hashes = np.array([c["hash"] for c in g["frames"]], np.uint32)
    return arr, pm, ipc, ct, svc, raw, off, lxc, hashes, g


def kat_oracle(g):
    """The oracle's outputs for the KAT's frames."""
    h = g["header"]
    table = {(p["identity"], htons(p["dport"]), p["proto"], 1): htons(p["proxy_port"]) for p in g["policy"]}
    from cilium_amd.classifier import PolicyArray
    hd = {h["slot"]: E.header_dict(PolicyArray.header(**{k: h[k] for k in h if k != "slot"})[0])}
    nets = [(ipaddress.ip_network(c), i) for c, i in g["ipcache"]]

    def ipcache(addr):
        a = ipaddress.ip_address(addr)
        best = max((n for n in nets if a.version == n[0].version and a in n[0]), key=lambda n: n[0].prefixlen,
                   default=None)
        return best[1] if best else N.CG_WORLD_ID
    frames = [bytes.fromhex(c["hex"]) for c in g["frames"]]
    return evaluate(frames, {h["slot"]: (0, table)}, hd, kat_world(g), lxc_ids=[h["slot"]] * len(frames),
                    ipcache=ipcache, ctmap=ctmap_of(*kat_ct_items(g)),
                    hash=np.array([c["hash"] for c in g["frames"]], np.uint32))


def _addr(a, family):
    return str(ipaddress.ip_address(bytes(a[:4 if family == 4 else 16])))


def check_kat_case(c, v, info, rec, srec, x):
    """One frame's outputs against the fixture's hand-written expectation."""
    e, name = c["expect"], c["name"]
    assert int(v) == e["verdict"], name
    ex = e["xlate"]
    flags = sorted(FLAG_NAMES[b] for b in FLAG_NAMES if int(x["flags"]) & b)
    assert (STATUS_NAMES[int(x["status"])], flags, int(x["slave"])) == (ex["status"], sorted(ex["flags"]),
                                                                       ex["slave"]), name
    fam = int(x["family"])
    if ex["daddr"] is None:
        assert x.tobytes()[4:] == bytes(44), name
    else:
        assert (_addr(x["daddr"], fam), _addr(x["saddr"], fam), int(x["dport"]), int(x["sport"]),
                int(x["rev_nat_index"])) == (ex["daddr"], ex["saddr"], htons(ex["dport"]), htons(ex["sport"]),
                                             ex["rev_nat_index"]), name
    if "identity" in e:
        assert int(info["t"]["identity"]) == e["identity"], name
    for r, want, dir_ in ((rec, e["rec"], 1), (srec, e["srec"], CT_SERVICE)):
        assert (T.STATE_NAMES[int(r["state"])], OP_NAMES[int(r["op"])]) == (want["state"], want["op"]), name
        if want["state"] == "none":
            assert r.tobytes() == bytes(64), name
            continue
        assert int(r["pad0"]) == dir_, name
        if "daddr" not in want:
            continue
        k, kf = r["key"], int(r["key"]["family"])
        conv = (lambda p: p) if want.get("raw_ports") else htons
        assert (_addr(k["daddr"], kf), _addr(k["saddr"], kf), int(k["dport"]), int(k["sport"]), int(k["flags"])) == \
            (want["daddr"], want["saddr"], conv(want["dport"]), conv(want["sport"]), want["flags"]), name
        assert int(r["pad1"]) == want["slave"], name
        if dir_ == 1:
            assert (int(r["rev_nat_index"]), int(r["loopback"]), _addr(r["pad2"][1:2].view(np.uint8), 4),
                    _addr(r["pad3"].reshape(1).view(np.uint8), 4)) == \
                (want["rev_nat_index"], want["loopback"], want["addr"], want["svc_addr"]), name


def check_kat(g, v, info, rec, srec, xl):
    for i, c in enumerate(g["frames"]):
        check_kat_case(c, v[i], info[i], rec[i], srec[i], xl[i])


# ---------------------------------------------------------- round trips ----
def check_round_trips(cl, egress, ingress):
    """egress(arr, raw, off, **kw) → (verdicts, info, records, svc_records,
    xlate); ingress(arr, raw, off, **kw) → (verdicts, info, records).  No
    hand-made keys: the maps are written by update_service and apply."""
    pm, arr, hd = E.egress_world(cl, ports=((2000, 8080, 6, 1, 0),))
    ct, ipc, svc = cl.conntrack_map(), cl.ipcache(), cl.service_map(ipv4_loopback=LOOPBACK)
    ipc.upsert("10.2.0.0/16", 2000)
    backends = [("10.2.0.1", 8080), ("10.2.0.2", 8080)]
    svc.update_service(("10.96.0.1", 80), backends, True, 5)
    syn = E.ip4(hd, "10.96.0.1", 6, E.tcp(40000, 80))
    raw, off = F.join([syn])

    def eg():
        return egress(arr, raw, off, lxc_ids=[5], ipcache=ipc, conntrack=ct, services=svc)

    # 1. an egress frame to the VIP, then apply: the service records first
    v, _, rec, srec, x = eg()
    assert v[0] == 0 and x["status"][0] == TRANSLATED and x["flags"][0] == F_PORT and x["rev_nat_index"][0] == 5
    assert (srec["state"][0], srec["op"][0], rec["state"][0], rec["op"][0]) == (1, T.OP_CREATE, 1, T.OP_CREATE)
    slave, target = int(x["slave"][0]), _addr(x["daddr"][0], 4)
    assert target == backends[slave - 1][0] and srec["pad1"][0] == slave
    assert ct.apply(srec, [74]).tolist() == [0] and ct.apply(rec, [74]).tolist() == [0]
    # 2. the same frame reads REPLY with the same slave on the service key, ESTABLISHED on the translated key
    v, _, rec, srec, x = eg()
    assert v[0] == 0 and (srec["state"][0], srec["op"][0], srec["pad1"][0]) == (N.CG_CT_STATE_REPLY, 0, slave)
    assert (rec["state"][0], rec["op"][0]) == (N.CG_CT_STATE_ESTABLISHED, 0) and _addr(x["daddr"][0], 4) == target
    assert _addr(rec["key"]["saddr"][0], 4) == target and rec["rev_nat_index"][0] == 5
    # 3. the backend's reply on the ingress route reads CT_REPLY with the service's rev_nat_index
    back = bytes(6) + bytes(6) + syn[12:26] + pk(target) + hd["ipv4"] + E.tcp(8080, 40000, 0x12)
    braw, boff = F.join([back])
    v, _, irec = ingress(arr, braw, boff, lxc_ids=[5], src_labels=[2000], conntrack=ct)
    assert v[0] == 0 and irec["state"][0] == N.CG_CT_STATE_REPLY and irec["rev_nat_index"][0] == 5
    # 4. update_service removes that backend: the slot cache fills its slave slot with the other backend, so the
    #    flow's slave number still finds an entry in lb*_lookup_slave (any entry counts) and moves to that backend
    other = backends[2 - slave]
    svc.update_service(("10.96.0.1", 80), [other], True, 5)
    keys, vals = svc.dump()
    assert vals["count"][0] == 2 and [_addr(t, 4) for t in vals["target"][1:]] == [other[0]] * 2
    v, _, rec, srec, x = eg()
    assert (srec["state"][0], srec["pad1"][0], x["slave"][0]) == (N.CG_CT_STATE_REPLY, slave, slave)
    assert _addr(x["daddr"][0], 4) == other[0] and (rec["state"][0], rec["op"][0]) == (N.CG_CT_STATE_NEW, T.OP_CREATE)
    # and once the slot itself is gone (a raw delete), lb*_lookup_service with the slave number finds nothing
    svc.delete(svc.key("10.96.0.1", htons(80), slave))
    v, _, rec, srec, x = eg()
    assert v[0] == DROP_NO_SERVICE and x["status"][0] == NO_SERVICE and not rec["state"][0]
    for o in (svc, ct, ipc, arr, pm):
        o.destroy()
