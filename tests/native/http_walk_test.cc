// http_walk_test.cc — http_walk.h on the CPU (built by tests/test_http_walk.py
// with hipcc, host side only).  The header is host+device and the host
// evaluator is built from it, so what holds here holds for the code the
// kernels compile: the comb step against the definition in comb.h's header
// comment, both label reads, first_meet for W = 1..6 against first_meet_loop
// and a bit-by-bit reference, remote_row over the direct array and both
// buckets of the remote table, and walk_overflow's bounds rule.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "http_walk.h"

using namespace cg;
using namespace cg::walk;

static int bad = 0;
#define CHECK(c, ...)                      \
  do {                                     \
    if (!(c) && bad++ < 10) {              \
      fprintf(stderr, "line %d: ", __LINE__); \
      fprintf(stderr, __VA_ARGS__);        \
      fputc('\n', stderr);                 \
    }                                      \
  } while (0)

// comb.h: next(S, b) = cell[S+b].lo == S ? cell[S+b].hi : max(S, D); in
// class mode states are byte offsets 4*S and x the code 4*c.
static uint32_t ref_next(const std::vector<uint32_t>& cells, uint32_t dead, uint32_t s, uint32_t x, bool scaled) {
  const uint32_t e = scaled ? cells[(s + x) / 4] : cells[s + x];
  if ((e & 0xFFFF) == s) return e >> 16;
  return s > dead ? s : dead;
}

static void test_steps(std::mt19937& rng) {
  for (int iter = 0; iter < 4000; ++iter) {
    const bool cls = iter & 1;
    const uint32_t unit = cls ? 4 : 1;  // a state's value per cell index
    std::vector<uint32_t> cells(2048);
    for (auto& c : cells) c = (uint32_t)rng();
    const uint32_t D = 256 + rng() % 512;
    // the exception hit, a dead-default row (S < D), a self-default row (S > D), D itself
    const int kind = (iter >> 1) & 3;
    const uint32_t S = kind == 1 ? 1 + rng() % (D - 1) : kind == 2 ? D + 1 + rng() % 700 : kind == 3 ? D : 1 + rng() % 1700;
    const uint32_t b = cls ? rng() % 64 : rng() % 256;
    const uint32_t st = S * unit, dead = D * unit, x = b * unit;
    uint32_t& cell = cells[S + b];
    if (kind == 0) cell = st | (uint32_t)(rng() & 0xFFFF) << 16;
    else if ((cell & 0xFFFF) == st) cell ^= 1;
    const uint32_t want = ref_next(cells, dead, st, x, cls);
    if (kind == 0) CHECK(want == cell >> 16, "hit");
    if (kind == 1) CHECK(want == dead, "dead default");
    if (kind == 2) CHECK(want == st, "self default");
    if (kind == 3) CHECK(want == dead, "D");
    const uint32_t got = cls ? comb_step_cls(cells.data(), dead, st, x) : comb_step(cells.data(), dead, st, x);
    CHECK(got == want, "step cls=%d kind=%d: %u, want %u", (int)cls, kind, got, want);
    CHECK((cls ? step<true>(cells.data(), dead, st, x) : step<false>(cells.data(), dead, st, x)) == want, "step<>");
    // the label of S: its header cell S - 1, high half
    const uint32_t lab = cells[S - 1] >> 16;
    const uint32_t l1 = cls ? state_label<true>(cells.data(), st) : state_label<false>(cells.data(), st);
    const uint32_t l2 = cls ? state_label32<true>(cells.data(), st) : state_label32<false>(cells.data(), st);
    CHECK(l1 == lab && l2 == lab, "label cls=%d: %u %u, want %u", (int)cls, l1, l2, lab);
  }
}

static uint32_t ref_meet(const std::vector<uint32_t>& blk, uint32_t a, uint32_t row, uint32_t W) {
  for (uint32_t bit = 0; bit < 64 * W; ++bit)
    if ((blk[a + bit / 32] >> (bit % 32)) & (blk[row + bit / 32] >> (bit % 32)) & 1) return bit;
  return kNoHit;
}

static void test_first_meet(std::mt19937& rng) {
  for (uint32_t W = 1; W <= 6; ++W) {
    int none = 0, last = 0;
    for (int iter = 0; iter < 600; ++iter) {
      std::vector<uint32_t> blk(64, 0);
      const uint32_t a = 2 * (rng() % 8), row = 32 + 2 * (rng() % 8);  // 8-byte aligned, apart
      const int kind = iter % 3;  // 0: sparse random masks, 1: no shared bit, 2: shared only in the last word
      for (uint32_t i = 0; i < 2 * W; ++i) {
        blk[a + i] = (uint32_t)rng() & (uint32_t)rng() & (uint32_t)rng();
        blk[row + i] = (uint32_t)rng() & (uint32_t)rng();
        if (kind) blk[row + i] &= ~blk[a + i];
      }
      if (kind == 2) {
        const uint32_t bit = 64 * (W - 1) + rng() % 64;
        blk[a + bit / 32] |= 1u << (bit % 32);
        blk[row + bit / 32] |= 1u << (bit % 32);
      }
      const uint32_t want = ref_meet(blk, a, row, W);
      none += want == kNoHit;
      last += want != kNoHit && want >= 64 * (W - 1);
      if (kind == 1) CHECK(want == kNoHit, "no shared bit");
      if (kind == 2) CHECK(want != kNoHit && want / 64 == W - 1, "last word only");
      const uint32_t g1 = first_meet(blk.data(), a, row, W), g2 = first_meet_loop(blk.data(), a, row, W);
      CHECK(g1 == want && g2 == want, "first_meet W=%u kind=%d: %u %u, want %u", W, kind, g1, g2, want);
    }
    CHECK(none >= 200 && last >= 200, "W=%u cases: %d none, %d last", W, none, last);
  }
}

static void test_remote_row(std::mt19937& rng) {
  // direct array: identities base .. base + len - 1 → u16 rows
  for (int iter = 0; iter < 200; ++iter) {
    std::vector<uint32_t> blk(256);
    for (auto& c : blk) c = (uint32_t)rng();
    HttpProg pg{};
    pg.flags = kProgRemoteDirect;
    pg.rdir_base = 1000 + rng() % 1000;
    pg.rdir_len = 1 + rng() % 100;
    pg.rdir_off = 4 * (rng() % 8);
    pg.default_remote = 7777;
    const uint16_t* arr = reinterpret_cast<const uint16_t*>(blk.data() + pg.rdir_off);
    const uint32_t in = pg.rdir_base + rng() % pg.rdir_len;
    CHECK(remote_row(blk.data(), pg, in) == arr[in - pg.rdir_base], "direct, in range");
    CHECK(remote_row(blk.data(), pg, pg.rdir_base + pg.rdir_len - 1) == arr[pg.rdir_len - 1], "direct, last");
    CHECK(remote_row(blk.data(), pg, pg.rdir_base + pg.rdir_len) == 7777, "direct, one past");
    CHECK(remote_row(blk.data(), pg, pg.rdir_base + pg.rdir_len + rng() % 100000) == 7777, "direct, above");
    CHECK(remote_row(blk.data(), pg, pg.rdir_base - 1) == 7777, "direct, below: d wraps");
    CHECK(remote_row(blk.data(), pg, rng() % pg.rdir_base) == 7777, "direct, below: d wraps");
  }
  // remote table: every slot empty (an identity outside the table, the
  // default row), then one identity in its first or second bucket, or nowhere
  for (int iter = 0; iter < 600; ++iter) {
    HttpProg pg{};
    pg.rtab_nb = 1 + rng() % 40;
    pg.rtab_off = 4 * (rng() % 4);  // buckets 16-byte aligned (http.cc)
    pg.default_remote = 4242;
    const uint32_t empty = 0xFFFFFFF0u;
    alignas(16) static uint32_t blk[16 + 8 * 40];
    for (uint32_t k = 0; k < pg.rtab_nb; ++k)
      for (uint32_t s = 0; s < 4; ++s) {
        blk[pg.rtab_off + 8 * k + s] = empty;
        blk[pg.rtab_off + 8 * k + 4 + s] = pg.default_remote;
      }
    uint32_t id;
    do id = (uint32_t)rng() % 100000; while (pg.rtab_nb > 1 && rtab_b1(id, pg.rtab_nb) == rtab_b2(id, pg.rtab_nb));
    const int where = iter % 3;  // bucket 1, bucket 2, absent
    const uint32_t bk = where == 0 ? rtab_b1(id, pg.rtab_nb) : rtab_b2(id, pg.rtab_nb), slot = rng() % 4;
    CHECK(bk < pg.rtab_nb, "bucket in range");
    if (where < 2) {
      blk[pg.rtab_off + 8 * bk + slot] = id;
      blk[pg.rtab_off + 8 * bk + 4 + slot] = 100 + iter;
    }
    const uint32_t want = where < 2 ? 100u + iter : pg.default_remote;
    CHECK(remote_row(blk, pg, id) == want, "table where=%d", where);
    CHECK(remote_row_hashed((const uint32_t*)blk, pg, id) == want, "table (hashed) where=%d", where);
    CHECK(remote_row(blk, pg, id + 1) == pg.default_remote, "another identity");
  }
}

static void test_walk_overflow() {
  // byte mode: D = 300; S0 = 600 goes to S1 = 900 on 'a', both default to
  // themselves; no other cell matches any state
  std::vector<uint32_t> cells(1200, 0xFFFFFFFFu);
  const uint32_t D = 300, S0 = 600, S1 = 900;
  cells[S0 + 'a'] = S0 | S1 << 16;
  alignas(16) uint8_t arena[64] = {0};
  const uint32_t len = 12;  // entry at 16: length, "a" and 11 bytes that change nothing; ends at 32
  memcpy(arena + 16, &len, 4);
  memset(arena + 20, 'z', len);
  arena[20] = 'a';
  const uint2 m = make_uint2(0, 1u | CG_HTTP_F_OVERFLOW << 24);  // offset 16 / 16
  CHECK(walk_overflow<false>(cells.data(), D, S0, arena, 64, m, false) == S0, "not an overflow slot");
  CHECK(walk_overflow<false>(cells.data(), D, S0, arena, 64, m, true) == S1, "walked");
  CHECK(walk_overflow<false>(cells.data(), D, S0, arena, 32, m, true) == S1, "an entry ending at arena_bytes is walked");
  CHECK(walk_overflow<false>(cells.data(), D, S0, arena, 31, m, true) == D, "aoff + 4 + len > arena_bytes");
  CHECK(walk_overflow<false>(cells.data(), D, S0, arena, 20, m, true) == D, "only the length fits");
  CHECK(walk_overflow<false>(cells.data(), D, S0, arena, 19, m, true) == D, "aoff + 4 > arena_bytes");
  CHECK(walk_overflow<false>(cells.data(), D, S0, arena, 0, m, true) == D, "no arena");
  const uint2 far = make_uint2(0, 0xFFFFFFu | CG_HTTP_F_OVERFLOW << 24);
  CHECK(walk_overflow<false>(cells.data(), D, S0, arena, 64, far, true) == D, "offset far past the arena");
  // class mode: the same table with states as byte offsets, 'a' as class 5
  std::vector<uint32_t> ccells(1200, 0xFFFFFFFFu);
  ccells[S0 + 5] = 4 * S0 | (4 * S1) << 16;
  arena[20] = 4 * 5;
  memset(arena + 21, 4 * 9, len - 1);
  CHECK(walk_overflow<true>(ccells.data(), 4 * D, 4 * S0, arena, 32, m, true) == 4 * S1, "class mode, walked");
  CHECK(walk_overflow<true>(ccells.data(), 4 * D, 4 * S0, arena, 31, m, true) == 4 * D, "class mode, past the arena");
}

int main() {
  std::mt19937 rng(20261019);
  test_steps(rng);
  test_first_meet(rng);
  test_remote_row(rng);
  test_walk_overflow();
  if (bad) {
    fprintf(stderr, "%d checks failed\n", bad);
    return 1;
  }
  printf("http_walk ok\n");
  return 0;
}
