// http_walk.h — the per-lane pieces of NetworkPolicyMap::Allowed
// (envoy/cilium_network_policy.h:223-237) that the verdict kernel
// (kernels_http.hip), the raw path's overflow walker and the persistent ring
// (kernels_http_raw.hip) run: a comb-table DFA step (comb.h), the accept
// label of a state, the remote identity's PNPR mask row and the first rule
// two masks share.  What the ring runs over its staged block is a template
// on the type of the pointer to the program's block: const uint32_t* (global
// memory, or LDS through a generic pointer) or const lds_u32* (LDS by
// address space: ds_read, not flat loads).  All of it is host+device:
// http_eval_host (http_pack.cc) is one lane of http_kernel_global built from
// these functions, so the CPU suite runs the kernels' own walk.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_types.h"

namespace cg {

// LDS by address space: through a generic pointer an LDS access compiles to
// a flat load (waiting on vmcnt like an HBM load).
#define CG_LDS __attribute__((address_space(3)))
typedef CG_LDS uint8_t lds_u8;
typedef CG_LDS uint32_t lds_u32;
typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));  // (HIP's uint4 class takes no address space)
typedef CG_LDS v4u32 lds_v4;
CG_HDI uint4 to_uint4(v4u32 v) { return make_uint4(v.x, v.y, v.z, v.w); }

namespace walk {

// The typed reads of a block: the cell a byte offset into it, and 16 bytes.
CG_HDI const uint32_t* cell_at(const uint32_t* p, uint32_t byte_off) {
  return reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(p) + byte_off);
}
CG_HDI const lds_u32* cell_at(const lds_u32* p, uint32_t byte_off) {
  return (const lds_u32*)((const lds_u8*)p + byte_off);
}
CG_HDI uint4 quad_at(const uint32_t* p) { return *reinterpret_cast<const uint4*>(p); }
CG_HDI uint4 quad_at(const lds_u32* p) { return to_uint4(*(const lds_v4*)p); }

// nx = e.lo == st ? e.hi : max(st, dead), the select of a comb transition.
// The walk is VALU-issue bound (PMC: ~60% of SIMD cycles issue VALU; each
// wave64 instruction holds the SIMD for 4 cycles), so the select uses SDWA
// word selects: compare the check half and pick the next half in two
// instructions.  It goes through VCC, which serializes several chains per
// lane — one chain per lane measured fastest.
CG_HDI uint32_t comb_select(uint32_t e, uint32_t dead, uint32_t st) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t dflt = max(st, dead);
  uint32_t nx;
  asm("v_cmp_eq_u32_sdwa vcc, %1, %2 src0_sel:WORD_0 src1_sel:DWORD\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_sdwa %0, %3, %1, vcc dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1"
      : "=v"(nx)
      : "v"(e), "v"(st), "v"(dflt)
      : "vcc");
  return nx;
#else
  return (e & 0xFFFF) == st ? e >> 16 : (st > dead ? st : dead);
#endif
}

// One comb transition (comb.h), branch-free: every lane reads the table and
// selects; the miss target max(S, dead) is one VALU.
template <class P>
CG_HDI uint32_t comb_step(P __restrict__ cells, uint32_t dead, uint32_t st, uint32_t b) {
  return comb_select(*cell_at(cells, (st << 2) + (b << 2)), dead, st);
}

// The class-mode step (comb.h): states are byte offsets and the string
// holds class codes 4*c, so the cell address is st + code — one SDWA add
// with the byte select, no shift.  The block sits at LDS address 0 in the
// fast path, so the add is the whole address.
template <class P>
CG_HDI uint32_t comb_step_cls(P __restrict__ cells, uint32_t dead, uint32_t st, uint32_t code) {
  return comb_select(*cell_at(cells, st + code), dead, st);
}

template <bool kCls, class P>
CG_HDI uint32_t step(P __restrict__ cells, uint32_t dead, uint32_t st, uint32_t x) {
  return kCls ? comb_step_cls(cells, dead, st, x) : comb_step(cells, dead, st, x);
}

// Accept label of state st (its header cell).
template <bool kCls, class P>
CG_HDI uint32_t state_label(P __restrict__ cells, uint32_t st) {
  return (kCls ? cell_at(cells, st)[-1] : cells[st - 1]) >> 16;
}
// The same with the header cell's offset worked out in 32 bits before it
// meets the pointer, as the ring's walk reads it (the two compile to
// different address arithmetic on a 64-bit pointer).
template <bool kCls, class P>
CG_HDI uint32_t state_label32(P __restrict__ cells, uint32_t st) {
  return *cell_at(cells, kCls ? st - 4 : 4 * (st - 1)) >> 16;
}

// Block offset of the PNPR mask of remote identity `remote` from the
// program's remote table (open addressing, {identity, mask offset} slots).
template <class P>
CG_HDI uint32_t remote_row_hashed(P __restrict__ blk, const HttpProg& pg, uint32_t remote) {
  // both candidate buckets read together (dev_types.h rtab_b1/rtab_b2)
  const uint32_t h = rtab_hash(remote);
  const P b1 = blk + pg.rtab_off + kRtabBucketCells * rtab_b1h(h, pg.rtab_nb);
  const P b2 = blk + pg.rtab_off + kRtabBucketCells * rtab_b2h(h, pg.rtab_nb);
  const uint4 k1 = quad_at(b1), k2 = quad_at(b2);
  const uint4 r1 = quad_at(b1 + 4), r2 = quad_at(b2 + 4);
  // an empty slot holds an identity outside the table with the default row
  uint32_t row = pg.default_remote;
  row = k1.x == remote ? r1.x : row;
  row = k1.y == remote ? r1.y : row;
  row = k1.z == remote ? r1.z : row;
  row = k1.w == remote ? r1.w : row;
  row = k2.x == remote ? r2.x : row;
  row = k2.y == remote ? r2.y : row;
  row = k2.z == remote ? r2.z : row;
  row = k2.w == remote ? r2.w : row;
  return row;
}

// The same for any program: from its direct array when it has one, else from
// the remote table.  (The ring reads the direct array through its own typed
// pointer, kernels_http_raw.hip ring_remote_row.)
CG_HDI uint32_t remote_row(const uint32_t* __restrict__ blk, const HttpProg& pg, uint32_t remote) {
  if (pg.flags & kProgRemoteDirect) {  // uniform: the direct array (dev_types.h)
    const uint32_t d = remote - pg.rdir_base;
    const bool in = d < pg.rdir_len;
    const uint32_t v = reinterpret_cast<const uint16_t*>(blk + pg.rdir_off)[in ? d : 0];
    return in ? v : pg.default_remote;
  }
  return remote_row_hashed(blk, pg, remote);
}

// u64 word w of the block mask at block offset a (u32 units, 8-byte aligned).
CG_HDI unsigned long long blk_word(const uint32_t* __restrict__ blk, uint32_t a, uint32_t w) {
  return *reinterpret_cast<const unsigned long long*>(blk + a + 2 * w);
}

// The first rule (lowest bit) the rule masks at block offsets a and row
// share, or kNoHit: the first rule that allows the request, in Envoy's
// evaluation order (http.cc build_prog).
constexpr uint32_t kNoHit = 0xFFFFFFFFu;
template <int W>
CG_HDI uint32_t first_meet_w(const uint32_t* __restrict__ blk, uint32_t a, uint32_t row) {
  // every word read up front, no per-lane exits: the lowest word with a
  // shared bit wins
  unsigned long long x[W];
#pragma unroll
  for (int w = 0; w < W; ++w) x[w] = blk_word(blk, a, w) & blk_word(blk, row, w);
  unsigned long long sel = 0;
  uint32_t base = 0;
#pragma unroll
  for (int w = W - 1; w >= 0; --w) {
    const bool nz = x[w] != 0;
    sel = nz ? x[w] : sel;
    base = nz ? 64u * w : base;
  }
  return sel ? base + (uint32_t)__builtin_ctzll(sel) : kNoHit;
}

// The same by a plain loop over the words, each read as two cells, leaving
// at the first word with a shared bit: any W and any pointer type (the
// ring's; first_meet's default branch reads whole words).
template <class P>
CG_HDI uint32_t first_meet_loop(P __restrict__ blk, uint32_t a, uint32_t row, uint32_t W) {
  for (uint32_t w = 0; w < W; ++w) {
    const unsigned long long x = ((unsigned long long)*(blk + a + 2 * w + 1) << 32 | *(blk + a + 2 * w)) &
                                 ((unsigned long long)*(blk + row + 2 * w + 1) << 32 | *(blk + row + 2 * w));
    if (x) return w * 64 + (uint32_t)__builtin_ctzll(x);
  }
  return kNoHit;
}

CG_HDI uint32_t first_meet(const uint32_t* __restrict__ blk, uint32_t a, uint32_t row, uint32_t W) {
  switch (W) {  // uniform
    case 1: return first_meet_w<1>(blk, a, row);
    case 2: return first_meet_w<2>(blk, a, row);
    case 3: return first_meet_w<3>(blk, a, row);
    case 4: return first_meet_w<4>(blk, a, row);
    default:
      for (uint32_t w = 0; w < W; ++w) {
        const unsigned long long x = blk_word(blk, a, w) & blk_word(blk, row, w);
        if (x) return w * 64 + (uint32_t)__builtin_ctzll(x);
      }
      return kNoHit;
  }
}

// ---- one slot of a packed batch (dev_types.h HttpBatchHeader), as
// http_chunks and http_tiles (kernels_http.hip) take it ----

// A chunk the kernels walk: its tiles lie inside the batch's tile table, at
// most kChunkTiles of them.  Any other chunk is skipped, its slots untouched.
CG_HDI bool chunk_ok(const HttpChunk& ch, uint32_t ntiles) {
  return !(ch.first_tile + ch.ntiles > ntiles || ch.ntiles > kChunkTiles);
}

// A real program that is not allow-all is walked, from the workgroup's LDS
// copy when its rebased block fits there (http_kernel), else from global
// memory (http_kernel_global).  (http_chunks keeps these two lines written
// out: as calls they changed its code)
CG_HDI bool prog_walked(bool real, const HttpProg& pg) { return real && !(pg.flags & kProgAllowAll); }
CG_HDI bool prog_in_lds(const HttpDev& T, const HttpProg& pg, bool walkp) {
  return walkp && (pg.flags & kProgRebased) && pg.cell_count <= T.lds_cells;
}
// An unwalked program's verdict for a counted slot: no policy for the port →
// allow; unknown policy → deny; a scope without HTTP rules → allow
// (cilium_network_policy.h:129-138,187-191).
CG_HDI bool trivial_allows(uint32_t prog, bool real) { return prog == kProgAllow || real; }

// The second word of a slot's meta (overflow arena offset / 16 | flags << 24):
// whether the slot holds a request to decide, and whether its string is in
// the overflow arena.
CG_HDI bool slot_counted(uint32_t m1) { return !((m1 >> 24) & (CG_HTTP_F_PAD | CG_HTTP_F_MALFORMED)); }
CG_HDI bool slot_overflow(uint32_t m1) { return ((m1 >> 24) & CG_HTTP_F_OVERFLOW) != 0; }

// Byte k of a 16-byte string unit.
CG_HDI uint32_t get_byte(const uint4& w, int k) {
  const uint32_t word = (k < 4) ? w.x : (k < 8) ? w.y : (k < 12) ? w.z : w.w;
  return (word >> ((k & 3) * 8)) & 0xFFu;
}

// Records longer than a slot live in the overflow arena: byte loop.
template <bool kCls>
CG_HDI uint32_t walk_arena(const uint32_t* __restrict__ cells, uint32_t dead, uint32_t st,
                           const uint8_t* __restrict__ arena, uint32_t aoff, uint32_t len) {
  for (uint32_t p = 0; p < len && st != dead; ++p) st = step<kCls>(cells, dead, st, arena[aoff + p]);
  return st;
}

// The overflow string of a lane whose meta word is m (arena entry: u32 length,
// bytes).  An entry reaching past the batch's arena (arena_bytes, from its
// header) ends in the dead state: only the always mask can still allow it.
template <bool kCls>
CG_HDI uint32_t walk_overflow(const uint32_t* __restrict__ cells, uint32_t dead, uint32_t st,
                              const uint8_t* __restrict__ arena, uint64_t arena_bytes, uint2 m, bool ov) {
  if (!ov) return st;
  const uint64_t aoff = (uint64_t)(m.y & 0xFFFFFFu) * 16u;
  if (aoff + 4 > arena_bytes) return dead;
  const uint32_t len = *reinterpret_cast<const uint32_t*>(arena + aoff);
  if (aoff + 4 + len > arena_bytes) return dead;
  return walk_arena<kCls>(cells, dead, st, arena, (uint32_t)aoff + 4, len);
}

}  // namespace walk
}  // namespace cg
