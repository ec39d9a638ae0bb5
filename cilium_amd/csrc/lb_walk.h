// lb_walk.h — service load-balancing in front of the from-container program's
// conntrack and policy: lb{4,6}_lookup_service (bpf/lib/lb.h:604-635, :351-380),
// lb{4,6}_local (:700-775, :426-483) with its ct_lookup* as CT_SERVICE
// (lib/conntrack.h:467-590, :310-437), lb*_lookup_slave (:637-651, :382-396),
// lb{4,6}_xlate as far as the tuple goes (:653-697, :398-424), and what
// lb{4,6}_rev_nat would write on an egress reply (:485-576, :254-317), over one
// snapshot of cilium_lb{4,6}_services / cilium_lb{4,6}_reverse_nat.  The frames
// kernel (kernels_l4_frames.hip, l4_frames_kernel<EgressSvcProg>) runs it per
// lane and cg_diag_l4_frames_egress_svc_eval_host per frame over host_view().
// The frame is never written: the translation lives in the tuple the steps
// behind it take.  Checksums and store errors are not modelled.
//
// The device tables, built for HBM (one per family, open addressing with linear
// probing, at most half full, an unused slot ends a search):
//   v4  32-byte slots: {address, dport | slave << 16, used, port | count << 16}
//       {target, rev_nat_index | weight << 16, 0, 0}.  The first 16 bytes decide
//       a master lookup (the key and count); a slave lookup reads both halves.
//   v6  64-byte slots: {address[4]} {dport | slave << 16, used, port | count <<
//       16, rev_nat_index | weight << 16} {target[4]} {0}: a master lookup reads
//       32 bytes, a slave lookup 48.
// Reverse NAT is a dense array indexed by the u16: v4 8 bytes {address, port |
// present << 16}, v6 32 bytes {address[4], port | present << 16, 0, 0, 0}, as
// long as the highest index in use.
//
// Per frame the L4 master key {daddr, dport, 0} and the L3 master key {daddr,
// 0, 0} are both known before either is needed: both first slots are requested
// before the first is tested.  A frame that hits a master then reads one bucket
// line of the conntrack table (the CT_SERVICE key) and one slave slot.
//
// A backend deleted under a flow (lb.h:737-744): when the slave slot the flow's
// entry names is gone, the reference calls lb*_lookup_service again with the key
// as lookup_slave left it, slave number included.  With key.dport != 0 that
// asks for {daddr, dport, slave} — the key that just missed — then for {daddr,
// 0, slave} with count != 0; with key.dport == 0 it asks for the key that just
// missed.  The control plane writes count 0 into every slave slot, so over maps
// it wrote the fallback finds nothing and the frame leaves with DROP_NO_SERVICE;
// only a raw entry {daddr, 0, slave} with a count makes it re-select.  Both are
// restated as written (the repeat of the lookup that just missed is not made: it
// reads the same snapshot).
#pragma once

#include "ct_walk.h"
#include "dev_types.h"
#include "frame_walk.h"

namespace cg {

struct LbMapDev {
  const uint32_t* s4;  // (mask4 + 1) slots of 8 words
  const uint32_t* s6;  // (mask6 + 1) slots of 16 words
  uint32_t mask4, mask6, probes4, probes6;
  const uint32_t* rn4;  // nrn4 entries of 2 words
  const uint32_t* rn6;  // nrn6 entries of 8 words
  uint32_t nrn4, nrn6;
  uint32_t loopback;  // IPV4_LOOPBACK (node_config.h), network order
};

// What the from-container program with services takes beside the policy array:
// the headers, the service maps, and the per-frame arrays only it has.
struct EpHdrSvcDev {
  EpHdrDev H;
  LbMapDev L;
  const uint32_t* hash;  // get_hash_recalc per frame, or NULL: ct_hash of the CT_SERVICE key
  uint4* svc_recs;       // 4 per frame, may be NULL
  uint4* xlate;          // 3 per frame, may be NULL
};

// A: words per address.  ds: dport | slave << 16.
template <int A>
struct LbKey {
  uint32_t a[A];
  uint32_t ds;
};
// The part of a slot a master lookup needs: pc = port | count << 16,
// rw = rev_nat_index | weight << 16 (v4: filled by lb_rest).
template <int A>
struct LbHead {
  LbKey<A> k;
  uint32_t used, pc, rw;
};
constexpr int lb_slot_words(int A) { return A == 1 ? 8 : 16; }

template <int A>
CG_HDI uint32_t lb_hash(const LbKey<A>& k) {
  uint32_t h = 0x9E3779B1u * (A + 1);
#pragma unroll
  for (int i = 0; i < A; ++i) {
    h = (h + k.a[i]) * 0x85EBCA77u;
    h ^= h >> 15;
  }
  h = (h + k.ds) * 0x85EBCA77u;
  h ^= h >> 15;
  return l4_fin(h);
}

template <int A>
CG_HDI LbHead<A> lb_head(const uint32_t* tab, uint32_t slot) {
  const uint32_t* p = tab + (size_t)slot * lb_slot_words(A);
  LbHead<A> h;
  if constexpr (A == 1) {
    const uint4 q = load16(p);
    h.k.a[0] = q.x;
    h.k.ds = q.y;
    h.used = q.z;
    h.pc = q.w;
    h.rw = 0;
  } else {
    const uint4 q0 = load16(p), q1 = load16(p + 4);
    h.k.a[0] = q0.x;
    h.k.a[1] = q0.y;
    h.k.a[2] = q0.z;
    h.k.a[3] = q0.w;
    h.k.ds = q1.x;
    h.used = q1.y;
    h.pc = q1.z;
    h.rw = q1.w;
  }
  return h;
}

// The target of a slot, and rev_nat_index | weight << 16.
template <int A>
CG_HDI void lb_rest(const uint32_t* tab, uint32_t slot, const LbHead<A>& h, uint32_t* target, uint32_t* rw) {
  const uint32_t* p = tab + (size_t)slot * lb_slot_words(A);
  if constexpr (A == 1) {
    const uint4 q = load16(p + 4);
    target[0] = q.x;
    *rw = q.y;
  } else {
    const uint4 q = load16(p + 8);
    target[0] = q.x;
    target[1] = q.y;
    target[2] = q.z;
    target[3] = q.w;
    *rw = h.rw;
  }
}

// The search from slot h on, `first` being that slot's head already loaded.
// → the slot, or -1.
template <int A>
CG_HDI int32_t lb_find(const uint32_t* tab, uint32_t mask, uint32_t probes, const LbKey<A>& k, uint32_t h,
                       const LbHead<A>& first, LbHead<A>* out) {
  LbHead<A> hd = first;
  for (uint32_t p = 0;; ++p) {
    if (!hd.used) return -1;
    bool eq = hd.k.ds == k.ds;
#pragma unroll
    for (int i = 0; i < A; ++i) eq = eq && hd.k.a[i] == k.a[i];
    if (eq) {
      *out = hd;
      return (int32_t)((h + p) & mask);
    }
    if (p >= probes) return -1;
    hd = lb_head<A>(tab, (h + p + 1) & mask);
  }
}

// A translation record's 48 bytes as 12 words (cg_lb_xlate, cilium_gpu.h).
struct LbXlateWords {
  uint32_t w[12];
};

// What the service steps leave for the steps behind them.
template <int A>
struct LbState {
  int32_t code;  // 0, or CG_DROP_NO_SERVICE
  uint32_t status, flags, slave, rev_nat;
  uint32_t daddr[A];                    // tuple.daddr after lb*_local
  uint32_t pkt_daddr[A], pkt_saddr[A];  // the packet's addresses after lb*_xlate
  uint32_t dport;                       // the packet's destination port after lb*_xlate, as stored
  uint32_t addr, svc_addr;              // ct_state.addr / .svc_addr (v4)
};

// Steps 7b-7e for one frame whose protocol passed extract_l4_port.  da / sa: the
// header's addresses as they lie; ports: the head of ct_lookup*'s {dport |
// sport << 16} and tf its flags besides the direction; key_dport:
// lb*_extract_key's key.dport; ct_err: the head of ct_lookup* fails for this
// frame.  code 0 is a miss (the program runs on as without services) or a
// translation, as status says.  *srec: the CT_SERVICE step's record, written
// once the lookup ran.  The state is built in locals and returned whole, so
// that in the kernel it stays in registers.
template <int A, int W, int S>
CG_HDI LbState<A> lb_local(const LbMapDev& L, const uint32_t* tab, uint32_t mask, uint32_t probes, const uint32_t* ct,
                           uint32_t ct_mask, uint32_t ct_probes, const uint32_t* da, const uint32_t* sa,
                           uint32_t ports, uint32_t tf, uint32_t key_dport, uint32_t proto, uint32_t family,
                           uint32_t scope, bool ct_err, const uint32_t* hash, CtRecWords* srec) {
  LbState<A> s;
  s.code = 0;
  s.status = CG_LB_MISS;
  s.flags = s.slave = s.rev_nat = s.addr = s.svc_addr = 0;
  s.dport = key_dport;
#pragma unroll
  for (int i = 0; i < A; ++i) {
    s.daddr[i] = s.pkt_daddr[i] = da[i];
    s.pkt_saddr[i] = sa[i];
  }
  // 7b. lb*_lookup_service: both masters' first slots are in flight before either is tested
  uint32_t dport = key_dport;
  LbKey<A> k4, k3;
#pragma unroll
  for (int i = 0; i < A; ++i) k4.a[i] = k3.a[i] = da[i];
  k4.ds = dport;
  k3.ds = 0;
  const uint32_t h4 = lb_hash(k4) & mask, h3 = lb_hash(k3) & mask;
  const LbHead<A> f4 = lb_head<A>(tab, h4), f3 = lb_head<A>(tab, h3);
  LbHead<A> m;
  int32_t slot = -1;
  if (dport) {
    slot = lb_find<A>(tab, mask, probes, k4, h4, f4, &m);
    if (slot >= 0 && (m.pc >> 16) == 0) slot = -1;
    if (slot < 0) dport = 0;  // key->dport = 0, and it stays
  }
  if (slot < 0) {
    slot = lb_find<A>(tab, mask, probes, k3, h3, f3, &m);
    if (slot >= 0 && (m.pc >> 16) == 0) slot = -1;
  }
  if (slot < 0) return s;
  s.flags = dport ? 0u : CG_LB_F_L3;
  // 7c. lb*_local: ct_lookup* as CT_SERVICE, one lookup of the tuple as loaded
  s.status = CG_LB_NO_SERVICE;
  s.code = CG_DROP_NO_SERVICE;
  if (ct_err) return s;
  const uint32_t kind = proto == 6 ? CG_CT_MAP_TCP : CG_CT_MAP_ANY;
  tf |= CG_TUPLE_F_SERVICE;
  CtKey<W> ck;
#pragma unroll
  for (int i = 0; i < A; ++i) {
    ck.w[i] = da[i];
    ck.w[A + i] = sa[i];
  }
  ck.w[W - 2] = ports;
  ck.w[W - 1] = proto | (tf | (kind == CG_CT_MAP_ANY ? kCtKindBit : 0u)) << 8 | scope << 16;
  const uint32_t full = ct_hash(ck), hb = full & ct_mask;
  uint32_t val = 0;
  const bool hit = ct_find<W, S>(ct, ct_mask, ct_probes, ck, hb, ct_line(ct, hb), &val);
  const uint32_t state = !hit ? CG_CT_STATE_NEW : tf & CG_TUPLE_F_RELATED ? CG_CT_STATE_RELATED : CG_CT_STATE_REPLY;
  const uint32_t hv = hash ? *hash : full;
  uint32_t op = hit ? CG_CT_OP_NONE : CG_CT_OP_CREATE;
  // a service key's 16-bit value on the device is its slave; lb*_select_slave's _rr_seq branch is compiled out
  uint32_t slave = hit ? val & 0xFFFF : hv % (m.pc >> 16) + 1;
  // 7d. lb*_lookup_slave, and lb*_lookup_service again with the key as it now stands
  LbKey<A> ks = k3;
  ks.ds = dport | slave << 16;
  uint32_t hs = lb_hash(ks) & mask;
  slot = lb_find<A>(tab, mask, probes, ks, hs, lb_head<A>(tab, hs), &m);
  if (slot < 0 && dport) {  // {daddr, dport, slave} just missed; key->dport = 0
    dport = 0;
    ks.ds = slave << 16;
    hs = lb_hash(ks) & mask;
    slot = lb_find<A>(tab, mask, probes, ks, hs, lb_head<A>(tab, hs), &m);
    if (slot >= 0 && (m.pc >> 16) == 0) slot = -1;
    if (slot >= 0) {
      slave = hv % (m.pc >> 16) + 1;
      if (hit) op = CG_CT_OP_UPDATE_SLAVE;  // a CREATE carries the slave it ends with
    }
  }
  s.slave = slave;
  // the record: the key as ct_create* / ct_update*_slave take it, flags TUPLE_F_SERVICE [| RELATED]
  srec->w[0] = state | op << 8 | 2u << 24;  // dir CT_SERVICE
  srec->w[1] = slave << 16;
#pragma unroll
  for (int i = 0; i < A; ++i) {
    srec->w[4 + i] = da[i];
    srec->w[8 + i] = sa[i];
  }
  srec->w[12] = ports;
  srec->w[13] = proto | tf << 8;
  srec->w[14] = scope | family << 16 | kind << 24;
  if (slot < 0) return s;
  // 7e. the translation
  uint32_t target[A], rw;
  lb_rest<A>(tab, (uint32_t)slot, m, target, &rw);
  s.code = 0;
  s.status = CG_LB_TRANSLATED;
  s.rev_nat = rw & 0xFFFF;
  bool loop = false;
  if constexpr (A == 1) {  // lb4_local: state->addr, and the loopback case (lb.h:751-770)
    loop = sa[0] == target[0];
    s.addr = loop ? L.loopback : target[0];
    s.svc_addr = loop ? sa[0] : 0u;
    s.pkt_saddr[0] = loop && L.loopback ? L.loopback : sa[0];  // lb4_xlate stores a non-zero new_saddr only
  }
#pragma unroll
  for (int i = 0; i < A; ++i) {
    s.pkt_daddr[i] = target[i];
    s.daddr[i] = loop ? da[i] : target[i];
  }
  const uint32_t port = m.pc & 0xFFFF;
  const bool rewrite = (proto == 6 || proto == 17) && port && dport != port;
  s.dport = rewrite ? port : key_dport;
  s.flags |= (loop ? CG_LB_F_LOOPBACK : 0u) | (rewrite ? CG_LB_F_PORT : 0u);
  return s;
}

// What lb{4,6}_rev_nat(…, flags 0) would write for a REPLY / RELATED frame whose
// entry carries rev_nat_index: → false when the index has no entry.
template <int A>
CG_HDI bool lb_rev_nat(const LbMapDev& L, uint32_t index, uint32_t* addr, uint32_t* port) {
  if constexpr (A == 1) {
    if (index >= L.nrn4) return false;
    const uint32_t a = L.rn4[2 * (size_t)index], p = L.rn4[2 * (size_t)index + 1];
    addr[0] = a;
    *port = p & 0xFFFF;
    return (p >> 16) != 0;
  } else {
    if (index >= L.nrn6) return false;
    const uint4 a = load16(L.rn6 + 8 * (size_t)index);
    const uint32_t p = L.rn6[8 * (size_t)index + 4];
    addr[0] = a.x;
    addr[1] = a.y;
    addr[2] = a.z;
    addr[3] = a.w;
    *port = p & 0xFFFF;
    return (p >> 16) != 0;
  }
}

}  // namespace cg
