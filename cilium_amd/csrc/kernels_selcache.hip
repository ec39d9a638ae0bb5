// kernels_selcache.hip — label selectors over the identity cache as bitsets
// (selcache.h; EndpointSelector.Matches, pkg/policy/api/selector.go:279-310;
// LabelArray.Get, pkg/labels/array.go:90-131; canReachIngress / canReachEgress,
// pkg/policy/rule.go:352-440; GetRulesMatching, repository.go:624-643).
//
// selcache_match_kernel: one lane per identity, so a wave covers 64
// consecutive identities and its __ballot is one output word.  Each lane
// stages its first kScFast labels in registers once and then walks a chunk
// of selectors: the requirement stream (selector headers, requirements,
// value ids) is wave-uniform and read through scalar loads, the label scan
// is per lane and branch-free (the staged labels are tested last to first, so
// the first hit in the identity's order is the one that stays).  An identity
// with more labels continues the scan in its global records.  Integer work
// on registers; memory traffic is the label records once per block and chunk
// and one 8-byte word per (selector, wave).
//
// selcache_cidr_match_kernel: the same for the prefix section (ScCidr), whose
// identities stand for GetCIDRLabels' label set without storing it.  One lane
// per prefix identity with its 24-byte record in registers; per requirement
// the classification record (ScReqCidr: address, mask words, length, family,
// kind) comes through scalar loads and the test is sc_cidr_found — a masked
// XOR over four words and two compares, no branch — followed by the label
// kernel's sc_req_holds.  No LDS, no atomics, no scratch.  The word in which
// the label section ends belongs to this kernel alone: its grid starts at
// word N / 64 and the label lanes of that one wave go through sc_matches, the
// host walker's label path, so the word is written once and whole, and the
// label kernel (which stops before it) and this one never store to the same
// address.
//
// selcache_reach_kernel: one block per (endpoint, 256 words).  The rules are
// taken in tiles: the block first ballots, per 64 rules, whether the rule's
// subject row has the endpoint's bit (the rule is "selected"), leaving one
// mask word per 64 rules in LDS; then every thread walks the set bits — the
// same in all lanes — and ORs the selected rules' allow rows and complemented
// require rows at its word.  Both directions in one pass.  Bound by reading
// rows of M, each read coalesced over the block's words.
//
// Expansion (convertL4FilterToPolicyMapKeys, pkg/endpoint/policy.go:111-130;
// computeDesiredL4PolicyMapEntries, :144-193; computeDesiredL3PolicyMapEntries,
// :298-371) turns bitset rows into policy-map entries in three launches.  A
// row's set D[r] (sc_exp_word) is never stored: count and emit both recompute
// it from the source rows, which for the common one-source row costs the same
// read a stored D would, and spares an R x W workspace and its write.
//   selcache_expand_count_kernel: one block per row, lanes stride the row's
//     words (coalesced), popcount, block reduce: row_off[r] = |D[r]|.
//   selcache_expand_scan_kernel: one block, exclusive 64-bit scan of the row
//     counts in place with a carried running sum; no block waits on another.
//   selcache_expand_emit_kernel: one block per row, a round covers kExpSpan
//     words, one per lane.  A wave scan of the popcounts gives each word's
//     base; then per non-zero word (read wave-uniformly) lane l tests bit l,
//     ranks itself with mbcnt and writes its key and proxy port at base +
//     rank: ascending bit order, whole lines, no atomics.  Wider rows take
//     further rounds with the base carried.
#include <hip/hip_runtime.h>

#include "dev_types.h"
#include "kernels.h"

namespace cg {

namespace {

constexpr int kScFast = 8;             // labels staged in registers per identity
constexpr int kMatchThreads = 1024;    // 16 waves: the block's words of one row fill a 128-byte line
constexpr uint32_t kMatchChunk = 256;  // selectors per block at most
constexpr int kReachThreads = 256;
constexpr uint32_t kReachTile = 4096;  // rules per LDS tile (64 mask words)
static_assert(kReachTile % kReachThreads == 0 && kReachThreads % 64 == 0, "whole waves ballot the tile");

__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

__global__ __launch_bounds__(kMatchThreads) void selcache_match_kernel(ScIdentDev I, ScSelDev T, uint32_t chunk,
                                                                       unsigned long long* __restrict__ bits) {
  const uint32_t i = blockIdx.x * kMatchThreads + threadIdx.x;
  const uint32_t w = uni(i >> 6);  // this wave's word: 64 consecutive identities
  // whole waves past the section (nothing below synchronises the block); with a
  // prefix section the word the labels end in is selcache_cidr_match_kernel's
  if (w >= (I.nc ? I.n >> 6 : I.words)) return;
  const bool valid = i < I.n;
  uint32_t lo = 0, nl = 0;
  if (valid) {
    lo = I.lab_off[i];
    nl = I.lab_off[i + 1] - lo;
  }
  uint32_t lk[kScFast], ls[kScFast], lv[kScFast];
#pragma unroll
  for (int j = 0; j < kScFast; ++j) {
    lk[j] = kScNoKey;  // an absent slot equals no selector key
    ls[j] = 0;
    lv[j] = 0;
    if ((uint32_t)j < nl) {
      const uint4 x = *reinterpret_cast<const uint4*>(I.labels + lo + j);
      lk[j] = x.x;
      ls[j] = x.y;
      lv[j] = x.z;
    }
  }
  const uint32_t s0 = blockIdx.y * chunk;
  const uint32_t s1 = s0 + chunk < T.n ? s0 + chunk : T.n;
  for (uint32_t s = s0; s < s1; ++s) {
    const uint32_t su = uni(s);
    const ScSel h = T.sels[su];
    bool m = valid;
    if (!(h.nreq & kScAlways)) {
      const uint32_t nreq = uni(h.nreq), rbeg = uni(h.rbeg);
      for (uint32_t r = 0; r < nreq; ++r) {
        const uint4 qx = *reinterpret_cast<const uint4*>(T.reqs + uni(rbeg + r));
        const uint32_t key = uni(qx.x), src = uni(qx.y), op_nv = uni(qx.z), vbeg = uni(qx.w);
        bool found = false;
        uint32_t got = 0;
#pragma unroll
        for (int j = kScFast - 1; j >= 0; --j) {  // last to first: the earliest hit is kept
          const bool hit = sc_label_hit(lk[j], ls[j], key, src);
          found = found || hit;
          got = hit ? lv[j] : got;
        }
        if (nl > (uint32_t)kScFast && !found) {  // a long identity: its remaining records, in order
          for (uint32_t j = kScFast; j < nl; ++j) {
            const uint4 x = *reinterpret_cast<const uint4*>(I.labels + lo + j);
            if (sc_label_hit(x.x, x.y, key, src)) {
              found = true;
              got = x.z;
              break;
            }
          }
        }
        const uint32_t nv = op_nv >> 8;
        bool in = false;
        for (uint32_t v = 0; v < nv; ++v) in = in || T.vals[uni(vbeg + v)] == got;
        in = in && found;
        m = m && sc_req_holds(op_nv & 0xFFu, found, in);
        if (__ballot(m) == 0ull) break;  // no identity of the wave can still match
      }
    }
    const unsigned long long word = __ballot(m);  // lanes past the table vote 0: zero padding bits
    if ((threadIdx.x & 63u) == 0) bits[(size_t)su * I.words + w] = word;
  }
}

__global__ __launch_bounds__(kMatchThreads) void selcache_cidr_match_kernel(ScIdentDev I, ScSelDev T, uint32_t chunk,
                                                                            unsigned long long* __restrict__ bits) {
  const uint32_t w0 = I.n >> 6;  // the first word with prefix bits
  const unsigned long long i = ((unsigned long long)w0 << 6) + (unsigned long long)blockIdx.x * kMatchThreads + threadIdx.x;  // bit index
  if ((i >> 6) >= I.words) return;  // whole waves past the table
  const uint32_t w = uni((uint32_t)(i >> 6));
  const bool is_label = i < I.n;  // only in the wave of word w0, when the label section ends inside it
  const bool mixed = w == w0 && (I.n & 63u);
  const bool valid = !is_label && i - I.n < I.nc;
  uint32_t p0 = 0, p1 = 0, p2 = 0, p3 = 0, plen = 0, pfam = 0;
  if (valid) {
    const uint2* rec = reinterpret_cast<const uint2*>(I.cidrs + (i - I.n));
    const uint2 x = rec[0], y = rec[1], z = rec[2];
    p0 = x.x, p1 = x.y, p2 = y.x, p3 = y.y, plen = z.x, pfam = z.y;
  }
  const uint32_t s0 = blockIdx.y * chunk;
  const uint32_t s1 = s0 + chunk < T.n ? s0 + chunk : T.n;
  for (uint32_t s = s0; s < s1; ++s) {
    const uint32_t su = uni(s);
    const ScSel h = T.sels[su];
    bool m = valid;
    if (!(h.nreq & kScAlways)) {
      const uint32_t nreq = uni(h.nreq), rbeg = uni(h.rbeg);
      for (uint32_t r = 0; r < nreq; ++r) {
        const uint32_t ri = uni(rbeg + r);
        const uint32_t op = uni(T.reqs[ri].op_nv) & 0xFFu;
        const uint4* cq = reinterpret_cast<const uint4*>(T.creqs + ri);
        const uint4 qa = cq[0], qm = cq[1], qk = cq[2];
        ScReqCidr q;
        q.a[0] = uni(qa.x), q.a[1] = uni(qa.y), q.a[2] = uni(qa.z), q.a[3] = uni(qa.w);
        q.mask[0] = uni(qm.x), q.mask[1] = uni(qm.y), q.mask[2] = uni(qm.z), q.mask[3] = uni(qm.w);
        q.len = uni(qk.x), q.family = uni(qk.y), q.kind = uni(qk.z), q.has_empty = uni(qk.w);
        const bool found = sc_cidr_found(p0, p1, p2, p3, plen, pfam, q);
        m = m && sc_req_holds(op, found, found && q.has_empty);
        if (__ballot(m) == 0ull) break;  // no prefix identity of the wave can still match
      }
    }
    if (mixed && is_label) m = sc_matches(I, T, su, (uint32_t)i);
    const unsigned long long word = __ballot(m);  // lanes past the table vote 0: zero padding bits
    if ((threadIdx.x & 63u) == 0) bits[(size_t)su * I.words + w] = word;
  }
}

__global__ __launch_bounds__(kReachThreads) void selcache_reach_kernel(ScRuleDev R, uint32_t n_ids, uint32_t W,
                                                                       const uint32_t* __restrict__ eps,
                                                                       unsigned long long* __restrict__ ing,
                                                                       unsigned long long* __restrict__ eg,
                                                                       uint8_t* __restrict__ flags) {
  __shared__ unsigned long long selmask[kReachTile / 64];
  const uint32_t ei = blockIdx.y;
  const uint32_t e = uni(eps[ei]);
  const bool eok = e < n_ids;  // an index outside the table selects no rule
  const uint32_t w = blockIdx.x * kReachThreads + threadIdx.x;
  const bool live = w < W;
  unsigned long long allow0 = 0, allow1 = 0, deny0 = 0, deny1 = 0;
  uint32_t fl = 0;
  for (uint32_t t0 = 0; t0 < R.n; t0 += kReachTile) {
    // which rules of the tile select the endpoint: one mask word per 64 rules
    for (uint32_t k = threadIdx.x; k < kReachTile; k += kReachThreads) {
      const uint32_t r = t0 + k;
      bool sel = false;
      if (eok && r < R.n) sel = (R.M[(size_t)R.subject[r] * W + (e >> 6)] >> (e & 63u)) & 1ull;
      const unsigned long long b = __ballot(sel);
      if ((threadIdx.x & 63u) == 0) selmask[k >> 6] = b;
    }
    __syncthreads();
    const uint32_t left = R.n - t0;
    const uint32_t nw = ((left < kReachTile ? left : kReachTile) + 63u) >> 6;
    for (uint32_t q = 0; q < nw; ++q) {
      const unsigned long long mq = selmask[q];
      unsigned long long mask = (unsigned long long)uni((uint32_t)mq) | ((unsigned long long)uni((uint32_t)(mq >> 32)) << 32);
      while (mask) {
        const uint32_t r = t0 + q * 64u + (uint32_t)__builtin_ctzll(mask);
        mask &= mask - 1;
        fl |= R.flags[r];
        if (live) {
          for (uint32_t x = R.req_off[0][r]; x < R.req_off[0][r + 1]; ++x) deny0 |= ~R.M[(size_t)R.req_idx[0][x] * W + w];
          for (uint32_t x = R.allow_off[0][r]; x < R.allow_off[0][r + 1]; ++x) allow0 |= R.M[(size_t)R.allow_idx[0][x] * W + w];
          for (uint32_t x = R.req_off[1][r]; x < R.req_off[1][r + 1]; ++x) deny1 |= ~R.M[(size_t)R.req_idx[1][x] * W + w];
          for (uint32_t x = R.allow_off[1][r]; x < R.allow_off[1][r + 1]; ++x) allow1 |= R.M[(size_t)R.allow_idx[1][x] * W + w];
        }
      }
    }
    __syncthreads();  // the next tile overwrites the masks
  }
  if (live) {
    const unsigned long long valid = (w == W - 1 && (n_ids & 63u)) ? (1ull << (n_ids & 63u)) - 1ull : ~0ull;
    ing[(size_t)ei * W + w] = allow0 & ~deny0 & valid;
    eg[(size_t)ei * W + w] = allow1 & ~deny1 & valid;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) flags[ei] = (uint8_t)fl;
}

constexpr int kCountThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int kExpThreads = 1024;            // 16 waves
constexpr uint32_t kExpSpan = kExpThreads;   // words per emit round: one per lane
static_assert(kCountThreads % 64 == 0 && kScanThreads % 64 == 0 && kExpThreads % 64 == 0, "whole waves");

__global__ __launch_bounds__(kCountThreads) void selcache_expand_count_kernel(ScExpDev X,
                                                                              unsigned long long* __restrict__ row_off) {
  __shared__ uint32_t part[kCountThreads / 64];
  for (uint32_t r = blockIdx.x; r < X.n_rows; r += gridDim.x) {
    const ScExpRow row = X.rows[r];
    uint32_t c = 0;  // at most n_ids < 2^32
    for (uint32_t w = threadIdx.x; w < X.words; w += kCountThreads) c += (uint32_t)__popcll(sc_exp_word(X, row, w));
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long t = 0;
      for (int k = 0; k < kCountThreads / 64; ++k) t += part[k];
      row_off[r] = t;
    }
    __syncthreads();  // the next row overwrites the partial sums
  }
}

// In place: row_off[i] holds row i's count on entry and the sum of the counts
// before it on exit; row_off[n] (and *total) the sum of all.  Every element
// is read and rewritten by the same thread.
__global__ __launch_bounds__(kScanThreads) void selcache_expand_scan_kernel(unsigned long long* __restrict__ row_off,
                                                                            uint32_t n,
                                                                            unsigned long long* __restrict__ total) {
  __shared__ unsigned long long wave_sum[kScanThreads / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long carry = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += kScanThreads) {
    const uint32_t i = i0 + threadIdx.x;
    const unsigned long long v = i < n ? row_off[i] : 0ull;
    unsigned long long incl = v;
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long t = __shfl_up(incl, d);
      if (lane >= (uint32_t)d) incl += t;
    }
    if (lane == 63u) wave_sum[wave] = incl;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (uint32_t k = 0; k < kScanThreads / 64; ++k) {
      const unsigned long long s = wave_sum[k];
      before += k < wave ? s : 0ull;
      all += s;
    }
    __syncthreads();  // the next chunk overwrites the wave sums
    if (i < n) row_off[i] = carry + before + incl - v;
    carry += all;
  }
  if (threadIdx.x == 0) {
    row_off[n] = carry;
    if (total) *total = carry;
  }
}

__device__ __forceinline__ unsigned long long lane64(unsigned long long v, uint32_t j) {  // j wave-uniform
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)j);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)j);
  return (unsigned long long)lo | ((unsigned long long)hi << 32);
}

__global__ __launch_bounds__(kExpThreads) void selcache_expand_emit_kernel(ScExpDev X,
                                                                           const unsigned long long* __restrict__ row_off,
                                                                           unsigned long long cap, uint2* __restrict__ keys,
                                                                           uint16_t* __restrict__ proxy) {
  __shared__ uint32_t wave_sum[kExpThreads / 64];
  if (row_off[X.n_rows] > cap) return;  // the same value in every block: the buffers stay untouched
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t r = blockIdx.x; r < X.n_rows; r += gridDim.x) {
    unsigned long long base = row_off[r];
    const unsigned long long end = row_off[r + 1];
    if (end == base) continue;  // an empty row, for the whole block
    const ScExpRow row = X.rows[r];
    for (uint32_t w0 = 0; w0 < X.words; w0 += kExpSpan) {
      const uint32_t w = w0 + threadIdx.x;
      const unsigned long long word = w < X.words ? sc_exp_word(X, row, w) : 0ull;
      const uint32_t cnt = (uint32_t)__popcll(word);
      uint32_t incl = cnt;
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d);
        if (lane >= (uint32_t)d) incl += t;
      }
      if (lane == 63u) wave_sum[wave] = incl;
      __syncthreads();
      uint32_t before = 0, all = 0;
      for (uint32_t k = 0; k < kExpThreads / 64; ++k) {
        const uint32_t s = wave_sum[k];
        before += k < wave ? s : 0u;
        all += s;
      }
      __syncthreads();  // the next round overwrites the wave sums
      const unsigned long long mine = base + before + (incl - cnt);  // where this lane's word starts
      unsigned long long nz = __ballot(word != 0ull);
      while (nz) {
        const uint32_t j = (uint32_t)__builtin_ctzll(nz);
        nz &= nz - 1;
        const unsigned long long wj = lane64(word, j);
        const unsigned long long bj = lane64(mine, j);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(wj >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)wj, 0u));
        const unsigned long long at = bj + rank;
        // sc_exp_word cleared the padding bits, so the identity index is < n_ids;
        // `at < end` holds when count and emit saw the same source matrix
        if (((wj >> lane) & 1ull) && at < end) {
          const uint32_t ident = (w0 + (wave << 6) + j) * 64u + lane;
          keys[at] = make_uint2(X.ids[ident], row.tmpl);
          proxy[at] = row.proxy_be;
        }
      }
      base += all;
    }
  }
}

}  // namespace

uint32_t selcache_expand_span() { return kExpSpan; }

int launch_selcache_expand(const ScExpDev& X, unsigned long long* row_off, void* keys, uint16_t* proxy,
                           unsigned long long cap, unsigned long long* total, void* stream, int cus) {
  const hipStream_t st = (hipStream_t)stream;
  const uint32_t per_cu = (uint32_t)(cus > 0 ? cus : 1);
  int err;
  if (X.n_rows) {
    const uint32_t g = X.n_rows < 8u * per_cu ? X.n_rows : 8u * per_cu;
    hipLaunchKernelGGL(selcache_expand_count_kernel, dim3(g), dim3(kCountThreads), 0, st, X, row_off);
    if ((err = (int)hipGetLastError())) return err;
  }
  hipLaunchKernelGGL(selcache_expand_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, row_off, X.n_rows, total);
  if ((err = (int)hipGetLastError())) return err;
  if (X.n_rows && X.words && cap) {
    const uint32_t g = X.n_rows < 4u * per_cu ? X.n_rows : 4u * per_cu;
    hipLaunchKernelGGL(selcache_expand_emit_kernel, dim3(g), dim3(kExpThreads), 0, st, X, row_off, cap, (uint2*)keys,
                       proxy);
    if ((err = (int)hipGetLastError())) return err;
  }
  return 0;
}

int launch_selcache_match(const ScIdentDev& I, const ScSelDev& T, unsigned long long* bits, void* stream, int cus) {
  if (T.n == 0) return 0;
  // selectors per block: as many as keeps every CU busy with a few blocks,
  // and few enough blocks for the grid's y extent
  auto chunk_of = [&](uint32_t gx) {
    uint32_t chunk = kMatchChunk;
    const uint64_t want = 4ull * (uint64_t)(cus > 0 ? cus : 1);
    while (chunk > 16 && (uint64_t)gx * ((T.n + chunk - 1) / chunk) < want) chunk >>= 1;
    while ((T.n + chunk - 1) / chunk > 65535u) chunk <<= 1;
    return chunk;
  };
  // the label section's whole words (all of its words without a prefix section)
  const uint32_t lwords = I.nc ? I.n >> 6 : I.words;
  if (lwords) {
    const uint32_t gx = (uint32_t)(((uint64_t)lwords * 64 + kMatchThreads - 1) / kMatchThreads);
    const uint32_t chunk = chunk_of(gx);
    const dim3 g(gx, (T.n + chunk - 1) / chunk), b(kMatchThreads);
    hipLaunchKernelGGL(selcache_match_kernel, g, b, 0, (hipStream_t)stream, I, T, chunk, bits);
    const int err = (int)hipGetLastError();
    if (err) return err;
  }
  if (I.nc) {  // from the word the label section ends in to the last
    const uint64_t lanes = (uint64_t)(I.words - (I.n >> 6)) * 64;
    const uint32_t gx = (uint32_t)((lanes + kMatchThreads - 1) / kMatchThreads);
    const uint32_t chunk = chunk_of(gx);
    const dim3 g(gx, (T.n + chunk - 1) / chunk), b(kMatchThreads);
    hipLaunchKernelGGL(selcache_cidr_match_kernel, g, b, 0, (hipStream_t)stream, I, T, chunk, bits);
    return (int)hipGetLastError();
  }
  return 0;
}

int launch_selcache_reach(const ScRuleDev& R, uint32_t n_ids, uint32_t words, const uint32_t* eps, size_t n,
                          unsigned long long* ing, unsigned long long* eg, uint8_t* flags, void* stream) {
  if (n == 0) return 0;
  const uint32_t gx = words ? (words + kReachThreads - 1) / kReachThreads : 1;  // no identities: flags only
  for (size_t off = 0; off < n; off += 65535) {
    const size_t cnt = n - off < 65535 ? n - off : 65535;
    const dim3 g(gx, (unsigned)cnt), b(kReachThreads);
    hipLaunchKernelGGL(selcache_reach_kernel, g, b, 0, (hipStream_t)stream, R, n_ids, words, eps + off,
                       ing + off * words, eg + off * words, flags + off);
    const int err = (int)hipGetLastError();
    if (err) return err;
  }
  return 0;
}

}  // namespace cg
