// ct_walk.h — the conntrack lookup of the endpoint's ingress policy program:
// ct_lookup4 / ct_lookup6 (bpf/lib/conntrack.h:467-590, :310-437) over one
// snapshot of the cilium_ct{4,6}_* / cilium_ct_any{4,6}_* maps, and the tail of
// ipv4_policy / ipv6_policy that acts on its result (bpf_lxc.c:948-974,
// :814-840).  The frames kernel (kernels_l4_frames.hip, l4_frames_kernel<P> for
// the programs P with conntrack) runs it per lane and the
// cg_diag_l4_frames_*_eval_host evaluators per frame over host_view(); the walk
// up to the policy verdict is frame_walk.h's.  The from-container program
// (egress_walk.h) ends in the same tail, ct_tail, as CT_EGRESS.
//
// __ct_lookup (conntrack.h:221-285) decides its return value by the key's
// presence alone: lifetime, the closing bits and the accounting counters are
// updated on a hit but never tested, so over a snapshot the state of a frame
// is a function of which keys are there.
//
// The device table (one per family), built for HBM: 128-byte buckets, open
// addressing over buckets with linear probing, filled from slot 0 up.
//   v4  7 keys of 16 B {daddr, saddr, dport, sport, nexthdr, flags, scope}:
//       struct ipv4_ct_tuple as the datapath stores it (lib/common.h:359-367)
//       and the 16-bit scope behind it; words 28..31 hold the 7 u16
//       rev_nat_index values (for a TUPLE_F_SERVICE key, whose rev_nat_index
//       is always 0, the entry's slave), the slot count (byte 126) and the
//       lb_loopback bits (byte 127).
//   v6  3 keys of 40 B {daddr[16], saddr[16], dport, sport, nexthdr, flags,
//       scope}: struct ipv6_ct_tuple (:338-346) and the scope; words 30..31
//       hold 3 u16 rev_nat_index values, the count and the loopback bits.
// The map kind (TCP / ANY, get_ct_map4/6 bpf_lxc.c:101-107) is bit 7 of the
// key's flags byte, which the datapath's TUPLE_F_* (0..7) never set.  A key
// sits in the first bucket of its probe sequence that had room, so a search
// ends at the first bucket that is not full; `probes` (the longest distance
// the build made) bounds it.  The builder sizes the table so that a bucket
// holds at most half its slots on average: a hit and a miss normally read one
// line.
#pragma once

#include "dev_types.h"
#include "frame_walk.h"

namespace cg {

constexpr uint32_t kCtKindBit = 0x80;  // in the key's flags byte: the ANY map
constexpr int kCt4Words = 4, kCt4Slots = 7, kCt6Words = 10, kCt6Slots = 3;
constexpr uint32_t kCtLineWords = 32;

struct CtMapDev {
  const uint32_t* t4;  // (mask4 + 1) lines of 32 words
  const uint32_t* t6;
  uint32_t mask4, mask6, probes4, probes6;
  uint32_t global;  // every frame looks up scope 0
};

template <int W>
struct CtKey {
  uint32_t w[W];
};
struct CtLine {
  uint32_t w[kCtLineWords];
};

template <int W>
CG_HDI uint32_t ct_hash(const CtKey<W>& k) {
  uint32_t h = 0x9E3779B1u * W;
#pragma unroll
  for (int i = 0; i < W; ++i) {
    h = (h + k.w[i]) * 0x85EBCA77u;
    h ^= h >> 15;
  }
  return l4_fin(h);
}

// The words of tuple_reverse (conntrack.h:439-456, :287-307): addresses and
// ports swapped, TUPLE_F_IN flipped.  The last two words are {dport | sport
// << 16, nexthdr | flags << 8 | scope << 16} in both families.
template <int W>
CG_HDI CtKey<W> ct_reverse(const CtKey<W>& k) {
  constexpr int A = (W - 2) / 2;  // words per address
  CtKey<W> r;
#pragma unroll
  for (int i = 0; i < A; ++i) {
    r.w[i] = k.w[A + i];
    r.w[A + i] = k.w[i];
  }
  r.w[W - 2] = k.w[W - 2] << 16 | k.w[W - 2] >> 16;
  r.w[W - 1] = k.w[W - 1] ^ (1u << 8);
  return r;
}

// One bucket, as eight 16-byte loads of one 128-byte line.
CG_HDI CtLine ct_line(const uint32_t* tab, uint32_t bucket) {
  CtLine L;
  const uint32_t* p = tab + (size_t)bucket * kCtLineWords;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const uint4 v = load16(p + 4 * q);
    L.w[4 * q] = v.x;
    L.w[4 * q + 1] = v.y;
    L.w[4 * q + 2] = v.z;
    L.w[4 * q + 3] = v.w;
  }
  return L;
}

// 1: the key is in the line (*val = rev_nat_index | lb_loopback << 16);
// 0: it is not and the line has room, which ends the search; -1: not here and
// the line is full.
template <int W, int S>
CG_HDI int ct_line_match(const CtLine& L, const CtKey<W>& k, uint32_t* val) {
  const uint32_t cnt = (L.w[31] >> 16) & 0xFF, lb = L.w[31] >> 24;
  int hit = -1;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    bool eq = (uint32_t)j < cnt;
#pragma unroll
    for (int i = 0; i < W; ++i) eq = eq && L.w[W * j + i] == k.w[i];
    if (eq) hit = j;
  }
  if (hit < 0) return cnt < (uint32_t)S ? 0 : -1;
  uint32_t rn = 0;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    constexpr int base = W * S;
    const uint32_t v = (L.w[base + j / 2] >> (16 * (j & 1))) & 0xFFFF;
    if (hit == j) rn = v;
  }
  *val = rn | ((lb >> hit) & 1u) << 16;
  return 1;
}

// The search from bucket h on, `first` being that bucket's line already
// loaded (the two lookups of a frame load their first lines together).
template <int W, int S>
CG_HDI int ct_find(const uint32_t* tab, uint32_t mask, uint32_t probes, const CtKey<W>& k, uint32_t h,
                   const CtLine& first, uint32_t* val) {
  int r = ct_line_match<W, S>(first, k, val);
  for (uint32_t p = 1; r < 0 && p <= probes; ++p) r = ct_line_match<W, S>(ct_line(tab, (h + p) & mask), k, val);
  return r > 0;
}

// ct_lookup4 / ct_lookup6 after the tuple is loaded: the tuple as loaded (the
// reverse direction) first, then the reversed one; *k is left as the
// reference leaves the tuple (reversed unless the first lookup hit).  → the
// state, 1 + CT_* (CG_CT_STATE_*).
template <int W, int S>
CG_HDI uint32_t ct_lookup(const uint32_t* tab, uint32_t mask, uint32_t probes, CtKey<W>* k, uint32_t* val) {
  const CtKey<W> fwd = ct_reverse(*k);
  const uint32_t h1 = ct_hash(*k) & mask, h2 = ct_hash(fwd) & mask;
  // both first lines are in flight before the first is tested
  const CtLine l1 = ct_line(tab, h1), l2 = ct_line(tab, h2);
  if (ct_find<W, S>(tab, mask, probes, *k, h1, l1, val))
    return (k->w[W - 1] >> 8) & 2u ? CG_CT_STATE_RELATED : CG_CT_STATE_REPLY;
  *k = fwd;
  return ct_find<W, S>(tab, mask, probes, fwd, h2, l2, val) ? CG_CT_STATE_ESTABLISHED : CG_CT_STATE_NEW;
}

// The tuple's ports, flags and related bit as the head of ct_lookup4/6 sets
// them, for a frame whose walk (frame_l4) has passed: dport | sport << 16 as
// the key's word holds them, *flags = TUPLE_F_OUT [| TUPLE_F_RELATED].
//   ICMP    dest-unreach 3, time-exceeded 11, parameter-problem 12: related;
//           echo reply 0: dport = 8; echo request 8: sport = the type.
//   ICMPv6  dest-unreach 1, packet-too-big 2, time-exceeded 3, parameter-
//           problem 4: related; echo reply 129: dport = 128; echo request
//           128: sport = the type.  (Constants assigned to a __be16: no htons.)
//   TCP/UDP the four bytes at l4_off land in {dport, sport}.
template <class Ld>
CG_HDI uint32_t ct_ports(Ld ld, uint32_t family, uint32_t proto, uint32_t l4_off, uint32_t* flags) {
  *flags = 0;  // TUPLE_F_OUT for CT_INGRESS
  const uint32_t w = ld(l4_off);
  if (proto == 6 || proto == 17) return w;
  const uint32_t type = w & 0xFF;
  if (family == 4) {
    if (type == 3 || type == 11 || type == 12) *flags = 2;
    return type == 0 ? 8u : type == 8 ? 8u << 16 : 0u;
  }
  if (type >= 1 && type <= 4) *flags = 2;
  return type == 129 ? 128u : type == 128 ? 128u << 16 : 0u;
}

// A record's 64 bytes as 16 words (cg_ct_record, cilium_gpu.h): the caller
// stores them as four 16-byte pieces.
struct CtRecWords {
  uint32_t w[16];
};

// The tail of the program behind the policy's verdict v, for a frame whose walk
// reached the policy: the two lookups and what the program does with the state
// (bpf_lxc.c:954-976, :820-840), in both directions:
//   REPLY / RELATED            0, never a proxy port;
//   policy denies, ESTABLISHED CG_DROP_POLICY, op DELETE of the matched key;
//   policy denies, NEW         CG_DROP_POLICY;
//   NEW and allowed            the policy's verdict, op CREATE;
//   ESTABLISHED and allowed    the policy's verdict.
// dir: 0 (CT_INGRESS) or CG_TUPLE_F_IN (CT_EGRESS, conntrack.h:504-506,
// :347-349); the flag's value 1 is also the record's dir byte.  The record is
// built in a local and assigned once, so that in the kernels it stays in
// registers whatever the caller does with *rec around the call (the six
// instantiations with conntrack sit 1 to 3 VGPRs under their limit of 128).
template <class Ld>
CG_HDI int32_t ct_tail(const CtMapDev& C, Ld ld, uint32_t family, uint32_t proto, uint32_t l4_off, uint32_t lxc,
                       uint32_t dir, int32_t v, CtRecWords* rec) {
  CtRecWords r;
#pragma unroll
  for (int i = 0; i < 16; ++i) r.w[i] = 0;
  const uint32_t scope = C.global ? 0u : lxc;
  const uint32_t kind = proto == 6 ? CG_CT_MAP_TCP : CG_CT_MAP_ANY;
  uint32_t tf;
  const uint32_t ports = ct_ports(ld, family, proto, l4_off, &tf);
  tf |= dir;
  const uint32_t last = proto | (tf | (kind == CG_CT_MAP_ANY ? kCtKindBit : 0u)) << 8 | scope << 16;
  uint32_t state, val = 0;
  if (family == 4) {
    CtKey<kCt4Words> k;
    k.w[0] = ld(kEthHlen + 16);  // daddr, saddr: the header's bytes as they lie
    k.w[1] = ld(kEthHlen + 12);
    k.w[2] = ports;
    k.w[3] = last;
    state = ct_lookup<kCt4Words, kCt4Slots>(C.t4, C.mask4, C.probes4, &k, &val);
    r.w[4] = k.w[0];
    r.w[8] = k.w[1];
    r.w[12] = k.w[2];
    r.w[13] = k.w[3];
  } else {
    CtKey<kCt6Words> k;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      k.w[i] = ld(kEthHlen + 24 + 4 * i);
      k.w[4 + i] = ld(kEthHlen + 8 + 4 * i);
    }
    k.w[8] = ports;
    k.w[9] = last;
    state = ct_lookup<kCt6Words, kCt6Slots>(C.t6, C.mask6, C.probes6, &k, &val);
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[4 + i] = k.w[i];
    r.w[12] = k.w[8];
    r.w[13] = k.w[9];
  }
  // the record's tuple carries the datapath's flags; the kind has its own byte
  r.w[13] = r.w[13] & 0xFFFFu & ~(kCtKindBit << 8);
  r.w[14] = scope | family << 16 | kind << 24;
  const bool reply = state == CG_CT_STATE_REPLY || state == CG_CT_STATE_RELATED;
  uint32_t op = CG_CT_OP_NONE;
  int32_t out = v;
  if (reply) out = 0;
  else if (v < 0) op = state == CG_CT_STATE_ESTABLISHED ? CG_CT_OP_DELETE : CG_CT_OP_NONE;
  else if (state == CG_CT_STATE_NEW) op = CG_CT_OP_CREATE;
  r.w[0] = state | op << 8 | (val >> 16) << 16 | dir << 24;
  r.w[1] = val & 0xFFFF;
  *rec = r;
  return out;
}

// ct_tail over a tuple the caller holds instead of the frame's own: ports and
// tf as ct_ports gives them, aw(src, i) word i of the source / destination
// address.  The from-container program with services (egress_walk.h) passes
// the translated tuple.  It restates ct_tail's body rather than sharing it:
// the kernels built on ct_tail keep their code, and their register counts,
// as they are.
template <class Aw>
CG_HDI int32_t ct_tail_tuple(const CtMapDev& C, Aw aw, uint32_t ports, uint32_t tf, uint32_t family, uint32_t proto,
                             uint32_t lxc, uint32_t dir, int32_t v, CtRecWords* rec) {
  CtRecWords r;
#pragma unroll
  for (int i = 0; i < 16; ++i) r.w[i] = 0;
  const uint32_t scope = C.global ? 0u : lxc;
  const uint32_t kind = proto == 6 ? CG_CT_MAP_TCP : CG_CT_MAP_ANY;
  tf |= dir;
  const uint32_t last = proto | (tf | (kind == CG_CT_MAP_ANY ? kCtKindBit : 0u)) << 8 | scope << 16;
  uint32_t state, val = 0;
  if (family == 4) {
    CtKey<kCt4Words> k;
    k.w[0] = aw(false, 0);  // daddr, saddr: the header's bytes as they lie
    k.w[1] = aw(true, 0);
    k.w[2] = ports;
    k.w[3] = last;
    state = ct_lookup<kCt4Words, kCt4Slots>(C.t4, C.mask4, C.probes4, &k, &val);
    r.w[4] = k.w[0];
    r.w[8] = k.w[1];
    r.w[12] = k.w[2];
    r.w[13] = k.w[3];
  } else {
    CtKey<kCt6Words> k;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      k.w[i] = aw(false, i);
      k.w[4 + i] = aw(true, i);
    }
    k.w[8] = ports;
    k.w[9] = last;
    state = ct_lookup<kCt6Words, kCt6Slots>(C.t6, C.mask6, C.probes6, &k, &val);
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[4 + i] = k.w[i];
    r.w[12] = k.w[8];
    r.w[13] = k.w[9];
  }
  // the record's tuple carries the datapath's flags; the kind has its own byte
  r.w[13] = r.w[13] & 0xFFFFu & ~(kCtKindBit << 8);
  r.w[14] = scope | family << 16 | kind << 24;
  const bool reply = state == CG_CT_STATE_REPLY || state == CG_CT_STATE_RELATED;
  uint32_t op = CG_CT_OP_NONE;
  int32_t out = v;
  if (reply) out = 0;
  else if (v < 0) op = state == CG_CT_STATE_ESTABLISHED ? CG_CT_OP_DELETE : CG_CT_OP_NONE;
  else if (state == CG_CT_STATE_NEW) op = CG_CT_OP_CREATE;
  r.w[0] = state | op << 8 | (val >> 16) << 16 | dir << 24;
  r.w[1] = val & 0xFFFF;
  *rec = r;
  return out;
}

// One frame through the ingress program with conntrack.  frame_verdict runs as
// it does without (the policy's verdict under `mode`, its counters, *o and
// *l4_off); a frame whose walk did not reach the policy returns that code with
// an all-zero record, every other goes through ct_tail as CT_INGRESS.
template <bool kEp, bool kIpc, class Ld, class Count>
CG_HDI int32_t frame_ct_verdict(const L4ArrDev& A, const EpMapDev& E, const IpcacheDev& ipc, const CtMapDev& C, Ld ld,
                                uint32_t len, uint32_t lxc, uint32_t label, uint32_t pkt_len, uint32_t mode,
                                cg_l4_frame_info* o, uint32_t* l4_off, CtRecWords* rec, Count count) {
  const int32_t v = frame_verdict<kEp, kIpc>(A, E, ipc, ld, len, lxc, label, pkt_len, mode, o, l4_off, count);
  if (!(o->t.flags & CG_L4_F_INGRESS)) {  // the walk returned before ct_lookup's lookups
#pragma unroll
    for (int i = 0; i < 16; ++i) rec->w[i] = 0;
    return v;
  }
  return ct_tail(C, ld, o->family, o->t.proto, *l4_off, o->lxc_id, 0u, v, rec);
}

}  // namespace cg
