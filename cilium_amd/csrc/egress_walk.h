// egress_walk.h — the endpoint's from-container program up to its verdict:
// handle_ingress (bpf/bpf_lxc.c:708-742), handle_ipv4_from_lxc (:432-570),
// handle_ipv6 + ipv6_l3_from_lxc (:389-416, :114-266), for one frame.  The
// frames kernel (kernels_l4_frames.hip, l4_frames_kernel<EgressProg>) runs it
// per lane and cg_diag_l4_frames_egress_eval_host per frame over host_view().
//
// The program restated is the one built with CONNTRACK, LB_L3 and LB_L4.
// egress_verdict runs it over an empty services map: lb{4,6}_extract_key runs
// (its load can fail), the service lookup finds nothing,
// ct_state_new.rev_nat_index stays 0.  egress_svc_verdict runs it over a service
// map, with the steps of lb_walk.h between extract_key and conntrack.  The order
// of the checks is the one cilium_gpu.h states for
// cg_l4_frames_egress_verdicts_*.  The header walk behind the source checks
// (ipv4_hdrlen / ipv6_hdrlen, the head of ct_lookup4/6) is frame_walk.h's, the
// lookups and what follows them are ct_walk.h's ct_tail: the head of
// ct_lookup* fills ports the same way for both directions, only the tuple's
// flags start as TUPLE_F_IN.
#pragma once

#include "ct_walk.h"
#include "dev_types.h"
#include "frame_walk.h"
#include "lb_walk.h"

namespace cg {

constexpr uint32_t kEthArp = 0x0806;

// A header's 64 bytes (cg_endpoint_header) as four 16-byte loads:
//   a = {lxc_mac[0..3], lxc_mac[4..5] | node_mac[0..1] << 16, node_mac[2..5], ipv4}
//   b = ipv6, c = router_ip6, d = {seclabel, flags, 0, 0}.
struct EpHdrWords {
  uint4 a, b, c, d;
};
CG_HDI EpHdrWords egress_header(const EpHdrDev& H, uint32_t idx) {
  const char* p = reinterpret_cast<const char*>(H.recs) + (size_t)idx * 64;
  return {load16(p), load16(p + 16), load16(p + 32), load16(p + 48)};
}

// is_valid_lxc_src_mac, is_valid_gw_dst_mac (lib/lxc.h:31-43, :76-88) and the
// source address test the caller hands in, in the reference's if / else-if
// order.  The MACs are compared as the three words that hold them.
template <class Ld>
CG_HDI int32_t egress_src_checks(Ld ld, const EpHdrWords& h, bool sip_ok) {
  const uint32_t flags = h.d.y;
  const uint32_t w0 = ld(0), w1 = ld(4), w2 = ld(8);
  const bool smac = (w1 >> 16) == (h.a.x & 0xFFFF) && w2 == (h.a.x >> 16 | (h.a.y & 0xFFFF) << 16);
  const bool dmac = w0 == (h.a.y >> 16 | h.a.z << 16) && (w1 & 0xFFFF) == h.a.z >> 16;
  if (!(flags & CG_EPH_F_NO_SMAC) && !smac) return CG_DROP_INVALID_SMAC;
  if (!(flags & CG_EPH_F_NO_DMAC) && !dmac) return CG_DROP_INVALID_DMAC;
  if (!(flags & CG_EPH_F_NO_SIP) && !sip_ok) return CG_DROP_INVALID_SIP;
  return 0;
}

// The program from its entry to lb{4,6}_extract_key (steps 1-7 of cilium_gpu.h)
// for egress_svc_verdict; it restates the head of egress_verdict below rather
// than sharing it, so that the kernels built on egress_verdict keep their code,
// and their register counts, as they are.  → 0 with *h, *ft, *sw (the slot's word), *family and *err (the head of
// ct_lookup*'s code for this frame, 0 / CT_INVALID_HDR / CT_UNKNOWN_PROTO) set,
// or the code the frame leaves with.  *o and *l4_off as in frame_verdict.
template <class Ld>
CG_HDI int32_t egress_head(const L4ArrDev& A, const EpHdrDev& H, Ld ld, uint32_t len, uint32_t lxc, uint32_t pkt_len,
                           cg_l4_frame_info* o, uint32_t* l4_off, uint32_t* sw_out, EpHdrWords* h_out,
                           FrameTuple* ft_out, uint32_t* family_out, int32_t* err_out) {
  *o = cg_l4_frame_info{};
  *l4_off = 0;
  o->lxc_id = (uint16_t)lxc;
  const uint32_t sw = A.slot[lxc];
  if (sw == 0) return CG_DROP_MISSED_TAIL_CALL;  // no program in the slot: nothing ran
  const uint32_t hw = H.idx[lxc];
  if (hw == 0) return CG_FRAME_NO_HEADER;
  o->t.len = pkt_len;
  if (len < kEthHlen) return CG_DROP_INVALID;
  const uint32_t et = frame_ethertype(ld);
  if (et == kEthArp) return CG_FRAME_ANSWERED;  // tail_handle_arp replies itself
  if (et != kEthIp4 && et != kEthIp6) return CG_DROP_UNKNOWN_L3;
  const uint32_t family = et == kEthIp4 ? 4 : 6;
  o->family = (uint8_t)family;
  const EpHdrWords h = egress_header(H, hw - 1);
  FrameTuple ft{};
  int32_t err;
  if (family == 4) {
    if (len < kEthHlen + 20) return CG_DROP_INVALID;
    o->t.proto = (uint8_t)(ld(kEthHlen + 6) >> 24);
    const bool sip = (h.d.y & CG_EPH_F_IPV4) && ld(kEthHlen + 12) == h.a.w;
    if (const int32_t e = egress_src_checks(ld, h, sip)) return e;
    err = frame_walk4(ld, len, &ft);
  } else {
    if (len < kEthHlen + 40) return CG_DROP_INVALID;
    const uint32_t nh = ld(kEthHlen + 6) & 0xFF;
    o->t.proto = (uint8_t)nh;
    const uint32_t d0 = ld(kEthHlen + 24), d1 = ld(kEthHlen + 28), d2 = ld(kEthHlen + 32), d3 = ld(kEthHlen + 36);
    if (nh == 58) {  // icmp6_handle, before the source checks (bpf_lxc.c:403-411)
      if (len < kEthHlen + 40 + 8) return CG_DROP_INVALID;
      const uint32_t type = ld(kEthHlen + 40) & 0xFF;
      if (type == 135) return CG_FRAME_ANSWERED;
      if (type == 128 && d0 == h.c.x && d1 == h.c.y && d2 == h.c.z && d3 == h.c.w) return CG_FRAME_ANSWERED;
    }
    const bool sip = ld(kEthHlen + 8) == h.b.x && ld(kEthHlen + 12) == h.b.y && ld(kEthHlen + 16) == h.b.z &&
                     ld(kEthHlen + 20) == h.b.w;
    if (const int32_t e = egress_src_checks(ld, h, sip)) return e;
    err = frame_walk6(ld, len, &ft);
  }
  o->t.proto = (uint8_t)ft.proto;
  *l4_off = ft.l4_off;
  // extract_l4_port (lib/lb.h:192-216) comes before the head of ct_lookup*: a
  // TCP / UDP frame without the 2 bytes at l4_off + 2 leaves with the load's
  // own error; frame_l4 reports such a frame as CT_INVALID_HDR.
  if (err == CG_DROP_CT_INVALID_HDR && (ft.proto == 6 || ft.proto == 17) && (uint64_t)ft.l4_off + 4 > len)
    return CG_FRAME_EFAULT;
  if (err != 0 && err != CG_DROP_CT_INVALID_HDR && err != CG_DROP_CT_UNKNOWN_PROTO) return err;  // ipv6_hdrlen's
  *sw_out = sw;
  *h_out = h;
  *ft_out = ft;
  *family_out = family;
  *err_out = err;
  return 0;
}

// policy_can_egress on the slot's map: the mode word clears the direction and
// the fragment bit.
template <class Count>
CG_HDI int32_t egress_policy(const L4ArrDev& A, uint32_t sw, uint32_t id, uint32_t dport, uint32_t proto,
                             uint32_t mode, Count count) {
  const L4Dev t = frame_map_rec(A, sw - 1);
  const uint32_t w1 = l4_mode_word(dport | proto << 16, mode);
  uint32_t val = 0;
  const int which = l4_resolve(t, [&](uint32_t b) { return t.fp[b]; }, id, w1, false, &val);
  if (which) count(t, val & 0xFFFF);
  return l4_wrap(l4_verdict(which, val, w1 >> 24), mode);
}

// One frame through the program.  kIpc: the destination identity is the
// ipcache resolution of the header's daddr, else `label`.  kCt: the two lookups
// of ct_lookup* against C and a record in *rec; else every packet is CT_NEW and
// rec is not touched.  *o, *l4_off and count as in frame_verdict.
template <bool kIpc, bool kCt, class Ld, class Count>
CG_HDI int32_t egress_verdict(const L4ArrDev& A, const EpHdrDev& H, const IpcacheDev& ipc, const CtMapDev& C, Ld ld,
                              uint32_t len, uint32_t lxc, uint32_t label, uint32_t pkt_len, uint32_t mode,
                              cg_l4_frame_info* o, uint32_t* l4_off, CtRecWords* rec, Count count) {
  *o = cg_l4_frame_info{};
  *l4_off = 0;
  if (kCt) {
#pragma unroll
    for (int i = 0; i < 16; ++i) rec->w[i] = 0;
  }
  o->lxc_id = (uint16_t)lxc;
  const uint32_t sw = A.slot[lxc];
  if (sw == 0) return CG_DROP_MISSED_TAIL_CALL;  // no program in the slot: nothing ran
  const uint32_t hw = H.idx[lxc];
  if (hw == 0) return CG_FRAME_NO_HEADER;
  o->t.len = pkt_len;
  if (len < kEthHlen) return CG_DROP_INVALID;
  const uint32_t et = frame_ethertype(ld);
  if (et == kEthArp) return CG_FRAME_ANSWERED;  // tail_handle_arp replies itself
  if (et != kEthIp4 && et != kEthIp6) return CG_DROP_UNKNOWN_L3;
  const uint32_t family = et == kEthIp4 ? 4 : 6;
  o->family = (uint8_t)family;
  const EpHdrWords h = egress_header(H, hw - 1);
  FrameTuple ft{};
  int32_t err;
  if (family == 4) {
    if (len < kEthHlen + 20) return CG_DROP_INVALID;
    o->t.proto = (uint8_t)(ld(kEthHlen + 6) >> 24);
    const bool sip = (h.d.y & CG_EPH_F_IPV4) && ld(kEthHlen + 12) == h.a.w;
    if (const int32_t e = egress_src_checks(ld, h, sip)) return e;
    err = frame_walk4(ld, len, &ft);
  } else {
    if (len < kEthHlen + 40) return CG_DROP_INVALID;
    const uint32_t nh = ld(kEthHlen + 6) & 0xFF;
    o->t.proto = (uint8_t)nh;
    const uint32_t d0 = ld(kEthHlen + 24), d1 = ld(kEthHlen + 28), d2 = ld(kEthHlen + 32), d3 = ld(kEthHlen + 36);
    if (nh == 58) {  // icmp6_handle, before the source checks (bpf_lxc.c:403-411)
      if (len < kEthHlen + 40 + 8) return CG_DROP_INVALID;
      const uint32_t type = ld(kEthHlen + 40) & 0xFF;
      if (type == 135) return CG_FRAME_ANSWERED;
      if (type == 128 && d0 == h.c.x && d1 == h.c.y && d2 == h.c.z && d3 == h.c.w) return CG_FRAME_ANSWERED;
    }
    const bool sip = ld(kEthHlen + 8) == h.b.x && ld(kEthHlen + 12) == h.b.y && ld(kEthHlen + 16) == h.b.z &&
                     ld(kEthHlen + 20) == h.b.w;
    if (const int32_t e = egress_src_checks(ld, h, sip)) return e;
    err = frame_walk6(ld, len, &ft);
  }
  o->t.proto = (uint8_t)ft.proto;
  *l4_off = ft.l4_off;
  // extract_l4_port (lib/lb.h:192-216) comes before the head of ct_lookup*: a
  // TCP / UDP frame without the 2 bytes at l4_off + 2 leaves with the load's
  // own error; frame_l4 reports such a frame as CT_INVALID_HDR.
  if (err == CG_DROP_CT_INVALID_HDR && (ft.proto == 6 || ft.proto == 17) && (uint64_t)ft.l4_off + 4 > len)
    return CG_FRAME_EFAULT;
  if (err) return err;
  o->t.dport = (uint16_t)ft.dport;
  o->t.flags = (uint8_t)CG_L4_F_WALKED;
  uint32_t id = label;
  if (kIpc) {
    if (family == 4) id = (uint32_t)ipc_v4_value(ipc, frame_be32(ld, kEthHlen + 16));
    else id = frame_ipc6(ipc, frame_be64(ld, kEthHlen + 24), frame_be64(ld, kEthHlen + 32));
  }
  o->t.identity = id;
  // policy_can_egress: the mode word clears the direction and the fragment bit
  const L4Dev t = frame_map_rec(A, sw - 1);
  const uint32_t w1 = l4_mode_word(ft.dport | ft.proto << 16, mode);
  uint32_t val = 0;
  const int which = l4_resolve(t, [&](uint32_t b) { return t.fp[b]; }, id, w1, false, &val);
  if (which) count(t, val & 0xFFFF);
  const int32_t v = l4_wrap(l4_verdict(which, val, w1 >> 24), mode);
  if (!kCt) return v;

  const int32_t out = ct_tail(C, ld, family, ft.proto, ft.l4_off, lxc, CG_TUPLE_F_IN, v, rec);
  rec->w[2] = h.d.x;  // src_sec_id = SECLABEL
  return out;
}

// The same program over a services map (lb_walk.h): steps 7a-7e between
// lb*_extract_key and the conntrack lookup, steps 8-12 on the translated tuple,
// and the reverse-NAT report of an egress reply.  Always with the ipcache and
// the conntrack map: lb*_local is conntrack, and the backend's identity exists
// only after the translation.  hash: the frame's get_hash_recalc, or NULL.
// put_srec(record): takes the CT_SERVICE step's record; *x: the translation record.
template <class Ld, class Count, class PutSrec>
CG_HDI int32_t egress_svc_verdict(const L4ArrDev& A, const EpHdrDev& H, const LbMapDev& L, const IpcacheDev& ipc,
                                  const CtMapDev& C, Ld ld, uint32_t len, uint32_t lxc, uint32_t pkt_len,
                                  uint32_t mode, const uint32_t* hash, cg_l4_frame_info* o, uint32_t* l4_off,
                                  CtRecWords* rec, PutSrec put_srec, LbXlateWords* x, Count count) {
  // the CT_SERVICE step's record leaves through put_srec, once on every path and before the conntrack tail:
  // its 16 words are not live while the tail holds its two bucket lines
  CtRecWords sr;
  CtRecWords* const srec = &sr;
#pragma unroll
  for (int i = 0; i < 16; ++i) rec->w[i] = srec->w[i] = 0;
#pragma unroll
  for (int i = 0; i < 12; ++i) x->w[i] = 0;
  uint32_t sw, family;
  EpHdrWords h;
  FrameTuple ft;
  int32_t err;
  if (const int32_t e = egress_head(A, H, ld, len, lxc, pkt_len, o, l4_off, &sw, &h, &ft, &family, &err)) {
    put_srec(sr);
    return e;
  }
  // 7a. a protocol extract_l4_port passes (its DROP_UNKNOWN_L4 skips the service steps); key.dport is the two
  // bytes at l4_off + 2, 0 for ICMP / ICMPv6.  The head of ct_lookup* runs inside lb*_local first: its ports and
  // flags are those of the CT_EGRESS lookup behind it.
  const uint32_t proto = ft.proto;
  const bool l4 = proto == 6 || proto == 17;
  const bool svc = l4 || proto == 1 || proto == 58;
  uint32_t tf = 0, ports = 0;
  if (!err) ports = ct_ports(ld, family, proto, ft.l4_off, &tf);
  const uint32_t key_dport = l4 ? ld(ft.l4_off) >> 16 : 0u;
  const uint32_t scope = C.global ? 0u : lxc;
  uint32_t da[4] = {0, 0, 0, 0}, sa[4] = {0, 0, 0, 0};  // tuple.daddr after 7e, tuple.saddr
  uint32_t pd[4] = {0, 0, 0, 0}, ps[4] = {0, 0, 0, 0};  // the packet's addresses after the translation
  uint32_t status = CG_LB_NONE, flags = 0, slave = 0, rev_nat = 0, dport = key_dport, addr = 0, svc_addr = 0;
  int32_t e = 0;
  if (family == 4) {
    da[0] = pd[0] = ld(kEthHlen + 16);
    sa[0] = ps[0] = ld(kEthHlen + 12);
    if (svc) {
      const LbState<1> s = lb_local<1, kCt4Words, kCt4Slots>(L, L.s4, L.mask4, L.probes4, C.t4, C.mask4, C.probes4, da,
                                                             sa, ports, tf, key_dport, proto, family, scope, err != 0,
                                                             hash, srec);
      e = s.code, status = s.status, flags = s.flags, slave = s.slave, rev_nat = s.rev_nat, dport = s.dport;
      addr = s.addr, svc_addr = s.svc_addr;
      da[0] = s.daddr[0], pd[0] = s.pkt_daddr[0], ps[0] = s.pkt_saddr[0];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      da[i] = pd[i] = ld(kEthHlen + 24 + 4 * i);
      sa[i] = ps[i] = ld(kEthHlen + 8 + 4 * i);
    }
    if (svc) {
      const LbState<4> s = lb_local<4, kCt6Words, kCt6Slots>(L, L.s6, L.mask6, L.probes6, C.t6, C.mask6, C.probes6, da,
                                                             sa, ports, tf, key_dport, proto, family, scope, err != 0,
                                                             hash, srec);
      e = s.code, status = s.status, flags = s.flags, slave = s.slave, rev_nat = s.rev_nat, dport = s.dport;
#pragma unroll
      for (int i = 0; i < 4; ++i) da[i] = s.daddr[i], pd[i] = s.pkt_daddr[i], ps[i] = s.pkt_saddr[i];
    }
  }
  put_srec(sr);
  const bool xl = status == CG_LB_TRANSLATED;
  x->w[0] = status | flags << 8 | slave << 16;
  if (e) return e;  // DROP_NO_SERVICE
  if (err) return err;  // step 8: the head of ct_lookup* as CT_EGRESS
  // 8-12 on the translated tuple: the reference re-reads the ports from the rewritten packet
  if (flags & CG_LB_F_PORT) ports = (ports & 0xFFFFu) | dport << 16;
  const uint32_t pol_dport = l4 ? dport : ft.dport;
  o->t.dport = (uint16_t)pol_dport;
  o->t.flags = (uint8_t)CG_L4_F_WALKED;
  uint32_t id;  // orig_dip = tuple.daddr after lb*_local (bpf_lxc.c:493, :180)
  if (family == 4) id = (uint32_t)ipc_v4_value(ipc, __builtin_bswap32(da[0]));
  else
    id = frame_ipc6(ipc, (uint64_t)__builtin_bswap32(da[0]) << 32 | __builtin_bswap32(da[1]),
                    (uint64_t)__builtin_bswap32(da[2]) << 32 | __builtin_bswap32(da[3]));
  o->t.identity = id;
  const int32_t v = egress_policy(A, sw, id, pol_dport, proto, mode, count);
  const int32_t out = ct_tail_tuple(
      C, [&](bool src, int i) { return src ? sa[i] : da[i]; }, ports, tf, family, proto, lxc, CG_TUPLE_F_IN, v, rec);
  rec->w[2] = h.d.x;  // src_sec_id = SECLABEL
  const uint32_t state = rec->w[0] & 0xFF;
  if (xl && ((rec->w[0] >> 8) & 0xFF) == CG_CT_OP_CREATE) {  // ct_create* with ct_state_new as lb*_local left it
    rec->w[0] |= (flags & CG_LB_F_LOOPBACK ? 1u : 0u) << 16;
    rec->w[1] = rev_nat | slave << 16;
    rec->w[3] = addr;
    rec->w[15] = svc_addr;
  }
  uint32_t sport = l4 ? ports & 0xFFFFu : 0u;
  const uint32_t rn = rec->w[1] & 0xFFFF;
  if ((state == CG_CT_STATE_REPLY || state == CG_CT_STATE_RELATED) && rn) {  // lb{4,6}_rev_nat(…, flags 0)
    uint32_t na[4] = {0, 0, 0, 0}, np = 0;
    const bool have = family == 4 ? lb_rev_nat<1>(L, rn, na, &np) : lb_rev_nat<4>(L, rn, na, &np);
    if (have) {
      flags |= CG_LB_F_REVNAT;
      if (l4 && np) sport = np;
      if (family == 4 && ((rec->w[0] >> 16) & 0xFF)) pd[0] = ps[0];  // loopback: the old source is the destination
#pragma unroll
      for (int i = 0; i < 4; ++i) ps[i] = na[i];
      rev_nat = rn;
    }
  }
  if (xl || (flags & CG_LB_F_REVNAT)) {
    x->w[0] = status | flags << 8 | slave << 16;
    x->w[1] = rev_nat | (l4 ? dport : 0u) << 16;
    x->w[2] = sport | family << 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) x->w[4 + i] = pd[i], x->w[8 + i] = ps[i];
  }
  return out;
}

}  // namespace cg
