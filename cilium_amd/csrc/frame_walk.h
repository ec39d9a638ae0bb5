// frame_walk.h — the endpoint's ingress policy program, handle_policy
// (bpf/bpf_lxc.c:1030-1058), from the Ethernet header to the arguments of
// policy_can_access_ingress and on through l4_walk.h, for one frame: the
// frames kernel (kernels_l4_frames.hip) runs it per lane and
// cg_diag_l4_frames_eval_host per frame over host_view().
//
// The program restated is the one built with CONNTRACK over an empty
// conntrack table: every packet is CT_NEW, so the tuple that reaches the
// policy is the reversed one (lib/conntrack.h:579-584, :422-426); tc_index and
// cb[CB_POLICY] are 0.  skb_load_bytes(off, n) fails when off + n passes the
// frame's length, and revalidate_data uses the same bound.  ct_walk.h puts the
// lookup against a conntrack map behind frame_verdict for the callers who
// pass one.
//
// ld(off): the four bytes at frame offset off, the first in bits 0..7.  The
// walk asks only for offsets it has checked against the length; bytes of the
// word past the frame's end are never used.
#pragma once

#include "dev_types.h"
#include "l4_walk.h"

namespace cg {

constexpr uint32_t kEthHlen = 14, kEthIp4 = 0x0800, kEthIp6 = 0x86DD;

// ipv4_policy's / ipv6_policy's locals at the call of policy_can_access_ingress
// (or where the walk returned): fields not reached stay 0.
struct FrameTuple {
  uint32_t l4_off;
  uint32_t proto;  // tuple.nexthdr
  uint32_t dport;  // tuple.dport after the reversal, as cg_l4_tuple holds it
  uint32_t frag;   // is_fragment
};

template <class Ld>
CG_HDI uint32_t frame_ethertype(Ld ld) {  // needs 14 bytes
  const uint32_t w = ld(12);
  return ((w & 0xFF) << 8) | ((w >> 8) & 0xFF);
}
template <class Ld>
CG_HDI uint32_t frame_be32(Ld ld, uint32_t off) {
  return __builtin_bswap32(ld(off));
}
template <class Ld>
CG_HDI uint64_t frame_be64(Ld ld, uint32_t off) {
  return (uint64_t)frame_be32(ld, off) << 32 | frame_be32(ld, off + 4);
}

// The head of ct_lookup4 / ct_lookup6 (lib/conntrack.h:496-556, :339-400) and
// the reversal: ICMP reads its type byte — echo request puts the type into
// sport (a plain assignment, no htons), so the reversed dport is the raw u16
// 8 / 128; echo reply sets dport, which the reversal moves to sport; every
// other type leaves both 0.  TCP loads its flags (2 bytes at +12) and then
// the ports, UDP the ports: the 4 bytes at l4_off land in {dport, sport}, so
// the reversed dport is the packet's destination port as stored.
template <class Ld>
CG_HDI int32_t frame_l4(Ld ld, uint32_t len, uint32_t icmp, uint32_t echo, FrameTuple* t) {
  const uint64_t o = t->l4_off;
  if (t->proto == icmp) {
    if (o + 1 > len) return CG_DROP_CT_INVALID_HDR;
    t->dport = (ld((uint32_t)o) & 0xFF) == echo ? echo : 0u;
    return 0;
  }
  if (t->proto == 6) {
    if (o + 14 > len) return CG_DROP_CT_INVALID_HDR;  // the flags at +12; the ports lie before them
  } else if (t->proto == 17) {
    if (o + 4 > len) return CG_DROP_CT_INVALID_HDR;
  } else {
    return CG_DROP_CT_UNKNOWN_PROTO;
  }
  t->dport = ld((uint32_t)o) >> 16;
  return 0;
}

// ipv4_policy up to ct_lookup4 (bpf_lxc.c:904-923): ihl as found (0..4 are not
// rejected, the version nibble is not looked at, lib/ipv4.h:45-48);
// is_fragment = frag_off & htons(0xBFFF) (lib/ipv4.h:50-61).
template <class Ld>
CG_HDI int32_t frame_walk4(Ld ld, uint32_t len, FrameTuple* t) {
  if (len < kEthHlen + 20) return CG_DROP_INVALID;
  const uint32_t f = ld(kEthHlen + 6);  // frag_off (2), ttl, protocol
  t->proto = f >> 24;
  t->frag = (f & 0xFFBFu) != 0;
  t->l4_off = kEthHlen + (ld(kEthHlen) & 0xF) * 4;
  return frame_l4(ld, len, 1, 8, t);
}

// ipv6_policy up to ct_lookup6 (bpf_lxc.c:758-798) with ipv6_hdrlen
// (lib/ipv6.h:61-98): at most IPV6_MAX_HEADERS = 4 rounds, so three extension
// headers pass and a fourth gives DROP_INVALID_EXTHDR whatever follows; the
// length added is the AUTH form when the header's *next* header is AUTH, as
// the reference tests nh after assigning it.  tuple.nexthdr stays
// ip6->nexthdr when ipv6_hdrlen fails.
template <class Ld>
CG_HDI int32_t frame_walk6(Ld ld, uint32_t len, FrameTuple* t) {
  if (len < kEthHlen + 40) return CG_DROP_INVALID;
  uint32_t nh = ld(kEthHlen + 6) & 0xFF;
  t->proto = nh;
  uint32_t hdrlen = 40;
  bool done = false;
  for (int i = 0; i < 4 && !done; ++i) {
    if (nh == 59) return CG_DROP_INVALID_EXTHDR;
    if (nh == 44) return CG_DROP_FRAG_NOSUPPORT;
    if (nh == 0 || nh == 43 || nh == 51 || nh == 60) {
      if ((uint64_t)kEthHlen + hdrlen + 2 > len) return CG_DROP_INVALID;
      const uint32_t w = ld(kEthHlen + hdrlen);
      nh = w & 0xFF;
      const uint32_t hl = (w >> 8) & 0xFF;
      hdrlen += nh == 51 ? (hl + 2) << 2 : (hl + 1) << 3;
    } else {
      done = true;
    }
  }
  if (!done) return CG_DROP_INVALID_EXTHDR;
  t->proto = nh;
  t->l4_off = kEthHlen + hdrlen;
  return frame_l4(ld, len, 58, 128, t);
}

// Frame i of a blob whose window is [lo, hi) = [off[0], off[n]): a range that
// runs backwards is empty, one that leaves the window is cut to it.
CG_HDI uint32_t frame_range(uint64_t a, uint64_t b, uint64_t lo, uint64_t hi, uint64_t* start) {
  if (a < lo) a = lo;
  if (b > hi) b = hi;
  *start = a;
  if (b <= a) return 0;
  return b - a > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)(b - a);
}

// A member map's record (the field order of L4Dev, as l4_array_kernel reads it).
CG_HDI L4Dev frame_map_rec(const L4ArrDev& A, uint32_t idx) {
  const uint4 a = load16(A.recs + idx), b = load16(reinterpret_cast<const char*>(A.recs + idx) + 16);
  L4Dev t;
  t.slots = reinterpret_cast<const L4Slot*>(((uint64_t)a.y << 32) | a.x);
  t.fp = reinterpret_cast<const uint32_t*>(((uint64_t)a.w << 32) | a.z);
  t.bucket_mask = b.x;
  t.max_entries = b.y;
  t.counters = reinterpret_cast<unsigned long long*>(((uint64_t)b.w << 32) | b.z);
  return t;
}

// lookup_ip6_remote_endpoint resolved to the identity, as l4_array_kernel's
// family 6 resolves it.
CG_HDI uint32_t frame_ipc6(const IpcacheDev& ipc, uint64_t hi, uint64_t lo) {
  const uint32_t tb = (uint32_t)(hi >> (64 - ipc.v6_bits));
  uint32_t k;
  if (!ipc_v6_bucket(ipc.code6[tb >> 5], tb, &k)) return (uint32_t)kIpcMiss;
  const uint4 en = load16(ipc.ent6 + 4 * (size_t)k);
  const uint64_t* rec = ipc.runs6 + 4 * (size_t)en.y;
  return ipc_v6_identity(ipc, hi, lo, en, load16(rec), (uint32_t)rec[2]);
}

// One frame through the program.  kEp: the endpoint comes from the endpoint
// map by destination address (the lookup of bpf_netdev.c:414-420 in front of
// the tail call), else lxc names it.  kIpc: cb[CB_SRC_LABEL] is the ipcache
// resolution of the source address, else `label`.  The two evaluation orders
// are the ones cilium_gpu.h states for cg_l4_frames_verdicts_*.  *o gets what
// the frame's stages found, *l4_off the L4 offset once known;
// count(map, entry id) runs on a policy hit.
template <bool kEp, bool kIpc, class Ld, class Count>
CG_HDI int32_t frame_verdict(const L4ArrDev& A, const EpMapDev& E, const IpcacheDev& ipc, Ld ld, uint32_t len,
                             uint32_t lxc, uint32_t label, uint32_t pkt_len, uint32_t mode, cg_l4_frame_info* o,
                             uint32_t* l4_off, Count count) {
  *o = cg_l4_frame_info{};
  *l4_off = 0;
  uint32_t et = 0;
  if (kEp) {
    o->t.len = pkt_len;
    if (len < kEthHlen) return CG_FRAME_NOT_LOCAL;
    et = frame_ethertype(ld);
    if (et != kEthIp4 && et != kEthIp6) return CG_FRAME_NOT_LOCAL;
    o->family = et == kEthIp4 ? 4 : 6;
    uint64_t ent = 0;
    int found;
    if (et == kEthIp4) {
      if (len < kEthHlen + 20) return CG_DROP_INVALID;
      const uint32_t d = frame_be32(ld, kEthHlen + 16);
      found = ex4_find(E.ex4, E.ex4_mask, E.ex4_probes, d, ipc_ex4_hash(d) & E.ex4_mask, &ent);
    } else {
      if (len < kEthHlen + 40) return CG_DROP_INVALID;
      const uint64_t hi = frame_be64(ld, kEthHlen + 24), lo = frame_be64(ld, kEthHlen + 32);
      found = ex6_find(E.ex6, E.ex6_mask, E.ex6_probes, hi, lo, ipc_ex6_hash(hi, lo) & E.ex6_mask, &ent);
    }
    if (!found) return CG_FRAME_NOT_LOCAL;
    lxc = (uint32_t)ent & 0xFFFF;
    o->lxc_id = (uint16_t)lxc;
    if ((uint32_t)(ent >> 32) & CG_ENDPOINT_F_HOST) return CG_FRAME_TO_HOST;
  } else {
    o->lxc_id = (uint16_t)lxc;
  }
  const uint32_t sw = A.slot[lxc];
  if (sw == 0) return CG_DROP_MISSED_TAIL_CALL;  // the tail call missed: no program ran
  if (!kEp) {
    o->t.len = pkt_len;
    if (len < kEthHlen) return CG_DROP_INVALID;
    et = frame_ethertype(ld);
    if (et != kEthIp4 && et != kEthIp6) return CG_DROP_UNKNOWN_L3;
    o->family = et == kEthIp4 ? 4 : 6;
  }
  const L4Dev t = frame_map_rec(A, sw - 1);
  FrameTuple ft{};
  const int32_t err = et == kEthIp4 ? frame_walk4(ld, len, &ft) : frame_walk6(ld, len, &ft);
  o->t.proto = (uint8_t)ft.proto;
  *l4_off = ft.l4_off;
  if (err) return err;
  const uint32_t flags = CG_L4_F_INGRESS | (ft.frag ? CG_L4_F_FRAGMENT : 0u);
  o->t.dport = (uint16_t)ft.dport;
  o->t.flags = (uint8_t)flags;
  uint32_t id = label;
  if (kIpc) {
    if (et == kEthIp4) id = (uint32_t)ipc_v4_value(ipc, frame_be32(ld, kEthHlen + 12));
    else id = frame_ipc6(ipc, frame_be64(ld, kEthHlen + 8), frame_be64(ld, kEthHlen + 16));
  }
  o->t.identity = id;
  const uint32_t w1 = l4_mode_word(ft.dport | ft.proto << 16 | flags << 24, mode);
  uint32_t val = 0;
  const int which = l4_resolve(t, [&](uint32_t b) { return t.fp[b]; }, id, w1, (w1 >> 24) & CG_L4_F_FRAGMENT, &val);
  if (which) count(t, val & 0xFFFF);
  return l4_wrap(l4_verdict(which, val, w1 >> 24), mode);
}

}  // namespace cg
