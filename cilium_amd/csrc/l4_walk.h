// l4_walk.h — __policy_can_access (bpf/lib/policy.h:46-110) for one tuple over
// the cuckoo table of dev_types.h, as the L4 kernels (kernels.hip) run it per
// lane and cg_diag_l4_eval_host per tuple over host_view().  No counters here.
#pragma once

#include "dev_types.h"

namespace cg {

// Verdict for one tuple given which lookup hit (1: L4, 2: L3, 3: wildcard
// identity L4, 0: none) and the slot value {entry id, proxy_port_be << 16}.
CG_HDI int32_t l4_verdict(int which, uint32_t val, uint32_t flags) {
  if (which == 1 || which == 3) return (int32_t)(val >> 16);  // return policy->proxy_port
  if (which == 2) return 0;  // TC_ACT_OK: the L3 entry's proxy_port is ignored
  if (flags & CG_L4_F_CB_POLICY) return 0;
  return (flags & CG_L4_F_FRAGMENT) ? CG_DROP_FRAG_NOSUPPORT : CG_DROP_POLICY;
}

// The verdict wrappers (bpf/lib/policy.h:126-163).  mode & 3:
// CG_L4_CAN_ACCESS = __policy_can_access with the tuple's own direction and
// fragment flags; CG_L4_INGRESS = policy_can_access_ingress (dir CT_INGRESS,
// the tuple's is_fragment); CG_L4_EGRESS = policy_can_egress (dir CT_EGRESS,
// is_fragment false).  Both wrappers return DROP_POLICY for any negative
// result, or TC_ACT_OK when built with IGNORE_DROP (mode & CG_L4_IGNORE_DROP).
CG_HDI uint32_t l4_mode_word(uint32_t w1, uint32_t mode) {
  const uint32_t m = mode & 3u;
  if (m == CG_L4_INGRESS) return w1 | (CG_L4_F_INGRESS << 24);
  if (m == CG_L4_EGRESS) return w1 & ~((CG_L4_F_INGRESS | CG_L4_F_FRAGMENT) << 24);
  return w1;
}
CG_HDI int32_t l4_wrap(int32_t v, uint32_t mode) {
  if ((mode & 3u) != CG_L4_CAN_ACCESS && v < 0) return (mode & CG_L4_IGNORE_DROP) ? 0 : CG_DROP_POLICY;
  return v;
}

// The three policy_key lookups of __policy_can_access (bpf/lib/policy.h:61-109)
// in priority order: j=0 {id, dport, proto, dir} (skipped for fragments),
// j=1 {id, 0, 0, dir}, j=2 {0, dport, proto, dir} (skipped for fragments).
// The keys share their hash products: h_j = fin(lo_j*M1 + hi_j*M2) with
// lo in {id, id, 0} and hi in {pp, eg, pp}.
//
// Candidates come from the fingerprint words: a zero-byte test on word^fp
// (it can flag a byte next to a true match as well, which only costs a slot
// read); bit p = slot*8 + j*2 + c for key j, bucket choice c.  A policy key
// sits in one slot, so the lowest j whose slot key matches is the verdict;
// candidates are walked in bit order and a j=0 match ends the walk.
struct L4Cand {
  uint64_t cand;   // candidate bits (slot*8 + j*2 + c)
  uint32_t bk[6];  // bucket of (key j, choice c) at index j*2+c
  uint32_t w0, pp, eg;
};

// fpw(b): bucket b's fingerprint word (from LDS or from global memory)
template <typename FpWord>
CG_HDI L4Cand l4_candidates(const L4Dev& t, FpWord fpw, uint32_t w0, uint32_t w1, bool frag) {
  L4Cand r;
  const uint32_t flags = w1 >> 24;
  // key.egress = !dir with dir = CT_INGRESS(1) / CT_EGRESS(0)
  r.eg = (flags & CG_L4_F_INGRESS) ? 0u : (1u << 24);
  r.pp = (w1 & 0xFFFFFF) | r.eg;  // dport | proto << 16 | egress << 24
  r.w0 = w0;
  const uint32_t P = w0 * kL4MulLo, Q = r.pp * kL4MulHi, E = r.eg * kL4MulHi;
  const uint32_t h[3] = {l4_fin(P + Q), l4_fin(P + E), l4_fin(Q)};
  r.cand = 0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    uint32_t fp;
    l4_place_h(h[j], t.bucket_mask, &r.bk[2 * j], &r.bk[2 * j + 1], &fp);
    if (j != 1 && frag) continue;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const uint32_t x = fpw(r.bk[2 * j + c]) ^ (fp * 0x01010101u);
      const uint32_t z = (x - 0x01010101u) & ~x & 0x80808080u;  // bit 8s+7: byte s zero
      r.cand |= (uint64_t)(z >> 7) << (j * 2 + c);
    }
  }
  return r;
}

// The slot a candidate bit names (selects, not indexing: a dynamically
// indexed array would live in scratch).
CG_HDI uint4 l4_slot(const L4Dev& t, const L4Cand& r, int bit) {
  const uint32_t jc = bit & 7;
  // masks, not a select chain: the compiler turns that into a scratch array
  const uint32_t b = (r.bk[0] & (0u - (jc == 0))) | (r.bk[1] & (0u - (jc == 1))) | (r.bk[2] & (0u - (jc == 2))) |
                     (r.bk[3] & (0u - (jc == 3))) | (r.bk[4] & (0u - (jc == 4))) | (r.bk[5] & (0u - (jc >= 5)));
  return load16(t.slots + (size_t)b * 4 + (bit >> 3));
}

CG_HDI bool l4_key_is(const L4Cand& r, int j, const uint4& v) {
  const uint32_t klo = j == 2 ? 0u : r.w0;
  const uint32_t khi = j == 1 ? r.eg : r.pp;
  return v.x == klo && v.y == khi;
}

// The first candidate's slot arrives loaded (v0, issued together with the
// other tuples' first loads); later ones load here (false fingerprint matches
// and tuples that need more than one key are the minority).
CG_HDI int l4_walk(const L4Dev& t, const L4Cand& r, const uint4& v0, uint32_t* val) {
  uint64_t cand = r.cand;
  if (!cand) return 0;
  int best = 0;
  {
    const int bit = __builtin_ctzll(cand);
    cand &= cand - 1;
    const int j = (bit & 7) >> 1;
    if (l4_key_is(r, j, v0)) {
      *val = v0.z;
      best = j + 1;
      if (j == 0) return best;
    }
  }
  while (cand) {
    const int bit = __builtin_ctzll(cand);
    cand &= cand - 1;
    const int j = (bit & 7) >> 1;
    if (best && j + 1 >= best) continue;
    const uint4 v = l4_slot(t, r, bit);
    if (l4_key_is(r, j, v)) {
      *val = v.z;
      best = j + 1;
      if (j == 0) break;
    }
  }
  return best;
}

// Candidates, the first one's slot, the walk.
template <typename FpWord>
CG_HDI int l4_resolve(const L4Dev& t, FpWord fpw, uint32_t w0, uint32_t w1, bool frag, uint32_t* val) {
  const L4Cand r = l4_candidates(t, fpw, w0, w1, frag);
  const uint4 v0 = r.cand ? l4_slot(t, r, __builtin_ctzll(r.cand)) : make_uint4(0, 0, 0, 0);
  return l4_walk(t, r, v0, val);
}

}  // namespace cg
