// egress_walk.h — the endpoint's from-container program up to its verdict:
// handle_ingress (bpf/bpf_lxc.c:708-742), handle_ipv4_from_lxc (:432-570),
// handle_ipv6 + ipv6_l3_from_lxc (:389-416, :114-266), for one frame.  The
// frames kernel (kernels_l4_frames.hip, l4_frames_kernel<EgressProg>) runs it
// per lane and cg_diag_l4_frames_egress_eval_host per frame over host_view().
//
// The program restated is the one built with CONNTRACK, LB_L3 and LB_L4 over an
// empty services map: lb{4,6}_extract_key runs (its load can fail), the
// service lookup finds nothing, ct_state_new.rev_nat_index stays 0.  The order
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

}  // namespace cg
