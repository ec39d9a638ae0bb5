// lpm_walk.h — check_v4 / check_v6 (bpf/bpf_xdp.c:97-156) for one packet over
// the prefilter tables of dev_types.h.  lpm_kernel (kernels.hip) issues its
// loads phase by phase for several packets of a lane; these are the steps
// between the loads, taking what a phase loaded, so
// cg_diag_prefilter_eval_host loads the same words through host_view() and
// calls them in the same order.  No counters here.
#pragma once

#include "dev_types.h"

namespace cg {

CG_HDI uint64_t u64_of(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }

// Endpoint probes continue past the first slot (the first one is issued by
// the caller together with the other packets' loads).
CG_HDI bool ep4_probe_more(const LpmDev& t, uint32_t a, uint32_t h) {
  for (uint32_t probe = 1; probe <= t.ep4_mask; ++probe) {
    h = (h + 1) & t.ep4_mask;
    const uint32_t k = t.ep4_keys[h];
    if (k == a) return true;
    if (k == 0) return false;
  }
  return false;
}

CG_HDI bool ep6_probe_more(const LpmDev& t, uint64_t hi, uint64_t lo, uint32_t h) {
  for (uint32_t probe = 1; probe <= t.ep6_mask; ++probe) {
    h = (h + 1) & t.ep6_mask;
    const uint4 k = load16(t.ep6_keys + 2 * (size_t)h);
    if (u64_of(k.x, k.y) == hi && u64_of(k.z, k.w) == lo) return true;
    if ((k.x | k.y | k.z | k.w) == 0) return false;
  }
  return false;
}

// Is a (as stored) a local endpoint: ek = ep4_keys[h], h = ep_hash32(a) & ep4_mask.
CG_HDI bool ep4_has(const LpmDev& t, uint32_t a, uint32_t ek, uint32_t h) {
  if (a == 0) return t.ep4_zero;
  if (ek == a) return true;
  if (ek == 0) return false;
  return ep4_probe_more(t, a, h);
}

// The same for (hi, lo): e = its slot at h = ep_hash128(hi, lo) & ep6_mask.
CG_HDI bool ep6_has(const LpmDev& t, uint64_t hi, uint64_t lo, uint4 e, uint32_t h) {
  if ((hi | lo) == 0) return t.ep6_zero;
  if (u64_of(e.x, e.y) == hi && u64_of(e.z, e.w) == lo) return true;
  if ((e.x | e.y | e.z | e.w) == 0) return false;
  return ep6_probe_more(t, hi, lo, h);
}

// A mixed /16: its /24 code, then for a partial /24 the leaf by rank.
CG_HDI bool v4_mixed(const LpmDev& t, uint32_t s, uint32_t tw) {
  const uint32_t q = s >> 16;
  const uint32_t m = t.top_rank[q >> 4] + __builtin_popcount(lpm_partials(tw) & ((1u << (2 * (q & 15))) - 1));
  const uint32_t k = (s >> 8) & 255;
  const uint32_t* chunk = t.mid + (size_t)m * 16;
  const uint4 cw = load16(chunk + 4 * (k >> 6));
  const uint32_t wi = (k >> 4) & 3;
  const uint32_t w = wi == 0 ? cw.x : wi == 1 ? cw.y : wi == 2 ? cw.z : cw.w;
  const uint32_t c = (w >> (2 * (k & 15))) & 3;
  if (c != kLpmPartial) return c == 1;
  uint32_t rank = t.leaf_base[m];
  for (uint32_t j = 0; j < (k >> 6); ++j) {
    const uint4 x = load16(chunk + 4 * j);
    rank += __builtin_popcount(lpm_partials(x.x)) + __builtin_popcount(lpm_partials(x.y)) +
            __builtin_popcount(lpm_partials(x.z)) + __builtin_popcount(lpm_partials(x.w));
  }
  rank += (wi > 0 ? __builtin_popcount(lpm_partials(cw.x)) : 0) + (wi > 1 ? __builtin_popcount(lpm_partials(cw.y)) : 0) +
          (wi > 2 ? __builtin_popcount(lpm_partials(cw.z)) : 0);
  rank += __builtin_popcount(lpm_partials(w) & ((1u << (2 * (k & 15))) - 1));
  return (t.leaves[(size_t)rank * 4 + ((s & 0xFF) >> 6)] >> (s & 63)) & 1;
}

// Is source s (host order) covered: tw = top[s >> 20] (0 with the v4 filter off).
CG_HDI bool v4_covered(const LpmDev& t, uint32_t s, uint32_t tw) {
  const uint32_t c = (tw >> (2 * ((s >> 16) & 15))) & 3;
  bool drop = c == 1;
  if (c == kLpmPartial) drop = v4_mixed(t, s, tw);
  return drop;
}

// A mixed bucket's candidate intervals [L, R] from its v6_mix entry; empty for
// a bucket that is not mixed.  The caller loads records R and R - 1 ahead.
struct V6Window {
  int64_t L, R;
};
CG_HDI V6Window v6_window(uint32_t mx, bool mixed) {
  V6Window w;
  const uint32_t span = mx & 15;
  w.R = mixed ? (int64_t)(mx >> 4) : -1;
  w.L = span == 15 ? 0 : w.R - span;
  return w;
}

// Binary search over intervals [L, R] for the last lo <= addr (more than two
// candidates in a mixed bucket: rare with ~2 buckets per interval).
CG_HDI int64_t v6_search(const LpmDev& t, uint64_t hi, uint64_t lo, int64_t L, int64_t R) {
  int64_t ans = -1;
  while (L <= R) {
    const int64_t m = (L + R) >> 1;
    const uint4 x = load16(t.v6_iv + 4 * m);
    if (le128(u64_of(x.x, x.y), u64_of(x.z, x.w), hi, lo)) {
      ans = m;
      L = m + 1;
    } else {
      R = m - 1;
    }
  }
  return ans;
}

// Is (hi, lo) covered in its mixed bucket's window: the last interval starting
// at or below it is record R (c1lo, c1hi: its start and end), else R - 1 (c0),
// else searched for below them; it covers the address iff it ends at or above it.
CG_HDI bool v6_covered(const LpmDev& t, uint64_t hi, uint64_t lo, const V6Window& w, uint4 c1lo, uint4 c1hi,
                       uint4 c0lo, uint4 c0hi) {
  uint64_t eh = 0, el = 0;
  bool found = false;
  if (le128(u64_of(c1lo.x, c1lo.y), u64_of(c1lo.z, c1lo.w), hi, lo)) {
    eh = u64_of(c1hi.x, c1hi.y);
    el = u64_of(c1hi.z, c1hi.w);
    found = true;
  } else if (w.R - 1 >= w.L) {
    if (le128(u64_of(c0lo.x, c0lo.y), u64_of(c0lo.z, c0lo.w), hi, lo)) {
      eh = u64_of(c0hi.x, c0hi.y);
      el = u64_of(c0hi.z, c0hi.w);
      found = true;
    } else if (w.R - 2 >= w.L) {
      const int64_t ans = v6_search(t, hi, lo, w.L, w.R - 2);
      if (ans >= 0) {
        const uint4 x = load16(t.v6_iv + 4 * ans + 2);
        eh = u64_of(x.x, x.y);
        el = u64_of(x.z, x.w);
        found = true;
      }
    }
  }
  return found && le128(hi, lo, eh, el);
}

}  // namespace cg
