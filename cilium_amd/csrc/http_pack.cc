// http_pack.cc — program-grouped request batches and the host table walker.
//
// The packer resolves each request's program on the host (the lookup the
// reference does per request in PortNetworkPolicy::Matches,
// envoy/cilium_network_policy.h:169-192), groups requests by program and
// pads every group to whole 64-request tiles, so each chunk of tiles has one
// program whose comb table a workgroup stages in LDS.  A tile holds the meta
// unit and only as many 16-byte string units as its longest string needs
// (the tile table gives each tile's offset and unit count), so the batch is
// as large as its strings, not as the 128-byte slot.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <vector>
#include <exception>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <type_traits>
#include <atomic>
#include <cstddef>
#include <array>
#include <cstring>
#include <map>
#include <string>

#include "comb.h"
#include "http.h"
#include "http_walk.h"

namespace cg {

namespace {

constexpr uint8_t kSep = 0x00;
constexpr uint8_t kAbsent = 0x01;
constexpr uint8_t kRestAbsent = 0x02;  // every remaining field absent (http.cc)

// A header value byte Envoy's HTTP/1 codec rejects (http_parser's
// IS_HEADER_CHAR: control bytes other than HTAB, and DEL); the request never
// reaches the L7 filter.
inline bool codec_rejects(uint8_t c) { return (c < 0x20 && c != 0x09) || c == 0x7F; }
constexpr size_t kUnitBytes = (size_t)CG_HTTP_TILE * 16;  // one string unit of a tile: 1 KiB
constexpr size_t kMetaBytes = (size_t)CG_HTTP_TILE * CG_HTTP_META_BYTES;  // the tile's meta block: 512 B
constexpr size_t kGranule = 512;  // tile offsets count 512-byte granules
constexpr size_t kMaxTileBytes = kMetaBytes + (size_t)(CG_HTTP_UNITS - 1) * kUnitBytes;

// byte offset of unit u (0 = meta block) of tile t, lane l (its last unit
// a half unit of 8 bytes per lane when tile_half)
inline size_t tile_unit_at(const HttpTile& t, uint32_t u, size_t lane) {
  const bool half = u && u == tile_units(t) && tile_half(t);
  return (size_t)t.at * kGranule +
         (u ? kMetaBytes + (size_t)(u - 1) * kUnitBytes + lane * (half ? 8 : 16) : lane * CG_HTTP_META_BYTES);
}

bool name_eq_ci(const uint8_t* a, size_t an, const std::string& lower_b) {
  if (an != lower_b.size()) return false;
  for (size_t i = 0; i < an; ++i) {
    uint8_t c = a[i];
    if (c >= 'A' && c <= 'Z') c = c - 'A' + 'a';
    if (c != (uint8_t)lower_b[i]) return false;
  }
  return true;
}

size_t max_groups(const HttpSnapshot& s, size_t n) { return std::min(n, s.progs.size() + 2); }

// chunk table, then the tile table, then (1 KiB aligned) the tile data
size_t ttab_off(size_t max_tiles) { return sizeof(HttpBatchHeader) + sizeof(HttpChunk) * max_tiles; }
size_t header_bytes(size_t max_tiles) {
  size_t b = ttab_off(max_tiles) + sizeof(HttpTile) * max_tiles;
  return (b + 1023) & ~(size_t)1023;
}

}  // namespace

size_t http_batch_slots(const HttpSnapshot& s, size_t n) {
  return ((n + CG_HTTP_TILE - 1) / CG_HTTP_TILE + max_groups(s, n)) * CG_HTTP_TILE;
}

size_t http_batch_bytes(const HttpSnapshot& s, size_t n) {
  size_t tiles = http_batch_slots(s, n) / CG_HTTP_TILE;
  return header_bytes(tiles) + tiles * kMaxTileBytes;
}

namespace {

// Worker threads for the packer: CILIUM_GPU_PACK_THREADS, else the hardware
// threads (at most 16); small batches stay on the calling thread.
unsigned pack_threads(size_t n) {
  if (n < 16384) return 1;
  static const unsigned t = [] {
    if (const char* e = getenv("CILIUM_GPU_PACK_THREADS")) {
      const long v = strtol(e, nullptr, 10);
      if (v >= 1 && v <= 256) return (unsigned)v;
    }
    return std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  }();
  return t;
}

// fn(begin, end, worker) over [0, n) in `nt` contiguous ranges.
template <class F>
void parallel_ranges(size_t n, unsigned nt, F&& fn) {
  if (nt <= 1 || n == 0) {
    fn((size_t)0, n, 0u);
    return;
  }
  std::vector<std::thread> th;
  std::exception_ptr err;
  std::mutex mu;
  for (unsigned t = 0; t < nt; ++t) {
    const size_t a = n * t / nt, b = n * (t + 1) / nt;
    th.emplace_back([&, a, b, t] {
      try {
        fn(a, b, t);
      } catch (...) {
        std::lock_guard<std::mutex> lk(mu);
        if (!err) err = std::current_exception();
      }
    });
  }
  for (auto& x : th) x.join();
  if (err) std::rethrow_exception(err);
}

// fn(item) for items [0, n) taken dynamically by `nt` workers.
template <class F>
void parallel_items(size_t n, unsigned nt, F&& fn) {
  std::atomic<size_t> next{0};
  parallel_ranges(nt, nt, [&](size_t, size_t, unsigned) {
    for (size_t i; (i = next.fetch_add(1)) < n;) fn(i);
  });
}

}  // namespace

void http_pack(const HttpSnapshot& s, size_t n, const uint32_t* policy, const uint8_t* ingress,
               const uint16_t* port, const uint32_t* remote, const uint8_t* hdr_blob,
               const uint64_t* hdr_off, void* batch, size_t batch_cap, uint32_t* order, size_t* nslots_out,
               uint8_t* arena, size_t arena_cap, size_t* arena_used) {
  const unsigned nt = pack_threads(n);
  const bool build = batch || arena_used;
  const bool dbg = getenv("CILIUM_GPU_PACK_DEBUG") != nullptr;
  auto t0 = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!dbg) return;
    auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[pack] %-10s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  };
  // program groups are laid out in ascending program id, the two special
  // ids (allow, deny) last: group index gi
  const size_t np = s.progs.size();
  auto group_of = [&](uint32_t p) -> size_t { return p < np ? p : np + (p == kProgAllow ? 0 : 1); };
  auto prog_of_group = [&](size_t g) -> uint32_t { return g < np ? (uint32_t)g : g == np ? kProgAllow : kProgDeny; };
  // ---- per request (parallel): program, walked string (field values in
  // field order, SEP-terminated, class-coded for class-mode programs),
  // codec verdict.  Each worker appends its strings to its own buffer.
  const size_t F = s.fields.size();
  std::vector<std::vector<uint8_t>> sbuf(nt);
  std::vector<uint32_t> prog(n), soff(n), slen(n);
  std::vector<uint8_t> malformed(n, 0);
  std::vector<std::vector<size_t>> gcount(nt, std::vector<size_t>(np + 2, 0));
  // fields by name length: a header name is compared with same-length fields only
  std::vector<std::vector<uint32_t>> by_len;
  for (size_t f = 0; f < F; ++f) {
    const size_t L = s.fields[f].size();
    if (by_len.size() <= L) by_len.resize(L + 1);
    by_len[L].push_back((uint32_t)f);
  }
  // literal tokens (HttpSnapshot::prog_tokens) by their first code: per
  // program, tok_first[code / 4] heads a list through tok_next of the tokens
  // that start with the code, longest first (-1 ends it).
  // CILIUM_GPU_PACK_TOKENS=0 packs plain class codes against the same tables.
  const char* tok_env = getenv("CILIUM_GPU_PACK_TOKENS");
  const bool tokens = !(tok_env && tok_env[0] == '0' && !tok_env[1]);
  std::vector<std::vector<int16_t>> tok_first(np), tok_next(np);
  for (size_t p = 0; p < np && p < s.prog_tokens.size() && tokens && build; ++p) {
    const auto& toks = s.prog_tokens[p];
    if (toks.empty()) continue;
    std::vector<int16_t> asc(toks.size());
    for (size_t t = 0; t < toks.size(); ++t) asc[t] = (int16_t)t;
    std::stable_sort(asc.begin(), asc.end(),
                     [&](int16_t a, int16_t b) { return toks[a].seq.size() < toks[b].seq.size(); });
    tok_first[p].assign(64, -1);
    tok_next[p].assign(toks.size(), -1);
    for (int16_t t : asc) {  // shortest first, each pushed at the head
      int16_t& head = tok_first[p][toks[t].seq[0] >> 2];
      tok_next[p][t] = head;
      head = t;
    }
  }
  auto worker_of = [&](size_t i) -> unsigned {
    // parallel_ranges splits [0, n) at n*t/nt
    unsigned t = (unsigned)((i * nt) / n);
    while (t + 1 < nt && i >= n * (t + 1) / nt) ++t;
    while (t > 0 && i < n * t / nt) --t;
    return t;
  };
  parallel_ranges(n, nt, [&](size_t a, size_t b, unsigned t) {
    std::vector<uint8_t>& strs = sbuf[t];
    if (build) strs.reserve((b - a) * 64);
    std::vector<const uint8_t*> vp(F);
    std::vector<size_t> vl(F);
    for (size_t i = a; i < b; ++i) {
      prog[i] = policy[i] >= s.npolicies ? kProgDeny : s.lookup_prog(policy[i], ingress[i] != 0, port[i]);
      gcount[t][group_of(prog[i])]++;
      if (!build) continue;
      std::fill(vp.begin(), vp.end(), nullptr);
      const uint8_t* p = hdr_blob + hdr_off[i];
      const uint8_t* e = hdr_blob + hdr_off[i + 1];
      while (p < e) {
        const uint8_t* nm = p;
        while (p < e && *p) ++p;
        size_t nl = p - nm;
        if (p < e) ++p;
        const uint8_t* v = p;
        while (p < e && *p) ++p;
        size_t vlen = p - v;
        if (p < e) ++p;
        if (s.raw_values) {
          // escaped proxylib value: no raw byte <= 0x02, and 0x03 only as
          // the first byte of an escape pair
          for (size_t k = 0; k < vlen; ++k) {
            if (v[k] <= 0x02) malformed[i] = 1;
            if (v[k] == 0x03) {
              // an escape pair, or the list-item separator pair {0x03, 0x14}
              if (k + 1 >= vlen || v[k + 1] < 0x10 || v[k + 1] > 0x14) malformed[i] = 1;
              ++k;
            }
          }
        } else {
          for (size_t k = 0; k < vlen; ++k)
            if (codec_rejects(v[k])) malformed[i] = 1;
        }
        if (nl < by_len.size())
          for (uint32_t f : by_len[nl])
            if (!vp[f] && name_eq_ci(nm, nl, s.fields[f])) {  // first value wins (HeaderMap::get)
              vp[f] = v;
              vl[f] = vlen;
            }
      }
      const size_t o = strs.size();
      size_t last = 0;  // fields [last, F) are all absent
      for (size_t f = 0; f < F; ++f)
        if (vp[f]) last = f + 1;
      for (size_t f = 0; f < last; ++f) {
        if (!vp[f]) strs.push_back(kAbsent);
        else strs.insert(strs.end(), vp[f], vp[f] + vl[f]);
        strs.push_back(kSep);
      }
      if (last < F) strs.push_back(kRestAbsent);
      if (strs.size() - o > 0xFFFFFFFFull) fail(CG_INVALID_ARGUMENT, "request string beyond 4 GiB");
      soff[i] = (uint32_t)o;  // offsets within one worker's buffer stay below 4 GiB per worker
      slen[i] = (uint32_t)(strs.size() - o);
      if (strs.size() > 0xFFFFFFFFull) fail(CG_INVALID_ARGUMENT, "packer buffer beyond 4 GiB per worker");
      if (prog[i] < np && (s.progs[prog[i]].flags & kProgClass)) {
        const auto& code = s.prog_code[prog[i]];
        for (size_t k = o; k < strs.size(); ++k) strs[k] = code[strs[k]];
        // literal tokens, left to right, the longest match first.  A string
        // for the overflow arena (by its untokenized length) stays as it is.
        if (tokens && slen[i] <= CG_HTTP_SLOT_BYTES && !tok_first[prog[i]].empty()) {
          const auto& first = tok_first[prog[i]];
          const auto& toks = s.prog_tokens[prog[i]];
          uint8_t* q = strs.data() + o;
          const size_t L = slen[i];
          size_t w = 0;
          for (size_t r = 0; r < L;) {
            size_t hit = 0;
            uint8_t sym = q[r];
            for (int16_t t = first[q[r] >> 2]; t >= 0; t = tok_next[prog[i]][t]) {
              const auto& sq = toks[t].seq;
              if (sq.size() <= L - r && memcmp(q + r, sq.data(), sq.size()) == 0) {
                hit = sq.size();
                sym = toks[t].code;
                break;
              }
            }
            q[w++] = sym;
            r += hit ? hit : 1;
          }
          strs.resize(o + w);
          slen[i] = (uint32_t)w;
        }
      }
    }
  });
  // string pointers (the workers' buffers no longer grow)
  std::vector<const uint8_t*> sp(build ? n : 0);
  if (build)
    parallel_ranges(n, nt, [&](size_t a, size_t b, unsigned t) {
      for (size_t i = a; i < b; ++i) sp[i] = sbuf[t].data() + soff[i];
    });
  lap("strings");
  auto str_ptr = [&](size_t i) -> const uint8_t* { return sp[i]; };
  auto str_len = [&](size_t i) -> size_t { return build ? slen[i] : 0; };
  // string units a request needs in its tile: 0 when the kernel does not
  // walk the slot string (malformed, or spilled to the overflow arena)
  auto walked_units = [&](size_t i) -> uint32_t {
    const size_t len = str_len(i);
    if (malformed[i] || len > CG_HTTP_SLOT_BYTES) return 0;
    return (uint32_t)((len + 15) / 16);
  };
  // ---- groups, their first slots and chunks
  std::vector<size_t> count(np + 2, 0);
  for (unsigned t = 0; t < nt; ++t)
    for (size_t g = 0; g < np + 2; ++g) count[g] += gcount[t][g];
  std::vector<size_t> first_slot(np + 2, 0);
  std::vector<HttpChunk> chunks;
  size_t tiles = 0;
  for (size_t g = 0; g < np + 2; ++g) {
    if (!count[g]) continue;
    first_slot[g] = tiles * CG_HTTP_TILE;
    size_t t = (count[g] + CG_HTTP_TILE - 1) / CG_HTTP_TILE;
    for (size_t k = 0; k < t; k += kChunkTiles)
      chunks.push_back({prog_of_group(g), (uint32_t)(tiles + k), (uint32_t)std::min<size_t>(kChunkTiles, t - k), 0});
    tiles += t;
  }
  const size_t nslots = tiles * CG_HTTP_TILE;
  if (nslots_out) *nslots_out = nslots;
  // ---- slot assignment: within a program group, requests ordered by the
  // number of 16-byte units their string spans, so the lanes of a tile end
  // their walks together, then by the string itself, so neighbouring lanes
  // share DFA states for as long as their strings share a prefix (their LDS
  // reads then broadcast instead of conflicting).  A counting sort into
  // (group, units) buckets, then each bucket sorted by content in parallel.
  constexpr size_t kKeys = CG_HTTP_UNITS + 2;
  auto key_of = [&](size_t i) -> size_t {
    const size_t len = str_len(i);
    return len > CG_HTTP_SLOT_BYTES ? CG_HTTP_UNITS + 1 : (len + 15) / 16;
  };
  std::vector<size_t> bstart((np + 2) * kKeys + 1, 0);
  for (size_t i = 0; i < n; ++i) bstart[group_of(prog[i]) * kKeys + key_of(i) + 1]++;
  for (size_t k = 1; k < bstart.size(); ++k) bstart[k] += bstart[k - 1];
  lap("buckets");
  std::vector<uint32_t> idx(n);
  {
    std::vector<size_t> fill(bstart.begin(), bstart.end() - 1);
    for (size_t i = 0; i < n; ++i) idx[fill[group_of(prog[i]) * kKeys + key_of(i)]++] = (uint32_t)i;
  }
  lap("idx");
  if (build) {
    // each bucket (one program, one unit count) ordered by string length,
    // so a tile's lanes end together (the last-unit tail is tight), then by
    // the first 32 bytes and a hash of the rest: lanes with a common prefix
    // sit together and walk the same DFA states (their LDS reads broadcast)
    // for that long, identical strings all the way.  Keys are local
    // records: no string compares in the sort.
    struct Rec {
      uint32_t len, i;
      uint64_t pre[4];  // bytes 0..31, big-endian, zero-padded
      uint64_t rest;    // FNV-1a of bytes 32..
    };
    std::vector<size_t> buckets;
    for (size_t k = 0; k + 1 < bstart.size(); ++k)
      if (bstart[k + 1] - bstart[k] > 1) buckets.push_back(k);
    // largest buckets first
    std::sort(buckets.begin(), buckets.end(),
              [&](size_t a, size_t b) { return bstart[a + 1] - bstart[a] > bstart[b + 1] - bstart[b]; });
    parallel_items(buckets.size(), nt, [&](size_t bi) {
      const size_t k = buckets[bi];
      std::vector<Rec> r(bstart[k + 1] - bstart[k]);
      for (size_t j = 0; j < r.size(); ++j) {
        const uint32_t i = idx[bstart[k] + j];
        const uint8_t* q = sp[i];
        const size_t L = slen[i];
        Rec& e = r[j];
        for (int w = 0; w < 4; ++w) {
          uint64_t x = 0;
          for (size_t c = 8 * w; c < 8 * w + 8; ++c) x = x << 8 | (c < L ? q[c] : 0);
          e.pre[w] = x;
        }
        uint64_t h = 1469598103934665603ull;
        for (size_t c = 32; c < L; ++c) h = (h ^ q[c]) * 1099511628211ull;
        e.rest = h;
        e.i = i;
        e.len = (uint32_t)L;
      }
      std::sort(r.begin(), r.end(), [](const Rec& a, const Rec& b) {
        if (a.len != b.len) return a.len < b.len;
        for (int w = 0; w < 4; ++w)
          if (a.pre[w] != b.pre[w]) return a.pre[w] < b.pre[w];
        if (a.rest != b.rest) return a.rest < b.rest;
        return a.i < b.i;
      });
      for (size_t j = 0; j < r.size(); ++j) idx[bstart[k] + j] = r[j].i;
    });
  }
  lap("sort");
  std::vector<uint32_t> slot_of(n);
  std::vector<uint32_t> req_of_slot(nslots, 0xFFFFFFFFu);
  for (size_t g = 0; g < np + 2; ++g) {
    size_t pos = first_slot[g];
    for (size_t r = bstart[g * kKeys]; r < bstart[(g + 1) * kKeys]; ++r) {
      slot_of[idx[r]] = (uint32_t)pos;
      req_of_slot[pos] = idx[r];
      ++pos;
    }
  }
  // ---- tile table: each tile's string units = its longest walked string,
  // and the bytes its lanes hold in that last unit (padding past the longest
  // one need not be walked: comb.h, padding never changes a label)
  std::vector<HttpTile> ttab(tiles);
  // half last units only in tiles of programs http_kernel walks one part at
  // a time from LDS (one_part_tiles; its other walkers read whole units)
  std::vector<uint8_t> half_ok(tiles, 0);
  for (const HttpChunk& c : chunks) {
    const bool ok = c.prog < np && !(s.progs[c.prog].flags & kProgAllowAll) && s.progs[c.prog].part_count == 1 &&
                    (s.progs[c.prog].flags & kProgRebased) && s.progs[c.prog].cell_count <= kMaxLdsCells;
    std::fill(half_ok.begin() + c.first_tile, half_ok.begin() + c.first_tile + c.ntiles, (uint8_t)ok);
  }
  parallel_ranges(tiles, nt, [&](size_t a, size_t b, unsigned) {
    for (size_t k = a; k < b; ++k) {
      uint32_t units = 0, tail = 0;
      for (size_t l = 0; l < CG_HTTP_TILE; ++l) {
        const uint32_t i = req_of_slot[k * CG_HTTP_TILE + l];
        if (i != 0xFFFFFFFFu) units = std::max(units, walked_units(i));
      }
      for (size_t l = 0; l < CG_HTTP_TILE && units; ++l) {
        const uint32_t i = req_of_slot[k * CG_HTTP_TILE + l];
        if (i != 0xFFFFFFFFu && walked_units(i) == units)
          tail = std::max<uint32_t>(tail, (uint32_t)(str_len(i) - 16 * (units - 1)));
      }
      if (units && !tail) tail = 16;
      // a last unit holding at most 8 bytes of any lane is stored as a half
      // unit: 512 B less per tile (config 5: 6.7% of the batch)
      ttab[k].units = units | (units && tail <= 8 && half_ok[k] ? kTileHalfLast : 0u) | tail << 16;
    }
  });
  lap("ttab");
  uint64_t gran = 0;
  for (auto& t : ttab) {
    if (gran > 0xFFFFFFFFull) fail(CG_INVALID_ARGUMENT, "batch beyond 2 TiB");
    t.at = (uint32_t)gran;
    gran += tile_granules(t);
  }
  const size_t max_tiles = http_batch_slots(s, n) / CG_HTTP_TILE;
  const size_t hdr = header_bytes(max_tiles);
  const size_t need = hdr + gran * kGranule;
  if (batch && need > batch_cap) fail(CG_INVALID_ARGUMENT, "batch buffer too small");
  uint8_t* data = batch ? (uint8_t*)batch + hdr : nullptr;
  auto unit_ptr = [&](size_t slot, uint32_t u) {
    return data + tile_unit_at(ttab[slot / CG_HTTP_TILE], u, slot % CG_HTTP_TILE);
  };
  // overflow arena entries in request order: u32 length then the string,
  // 16-byte aligned
  std::vector<uint64_t> aoff(n, ~0ull);
  size_t used = 0;
  for (size_t i = 0; i < n && build; ++i) {
    const size_t len = str_len(i);
    if (len <= CG_HTTP_SLOT_BYTES) continue;
    if (used / 16 >= (1u << 24)) fail(CG_INVALID_ARGUMENT, "overflow arena beyond 256 MiB");
    aoff[i] = used;
    used += (4 + len + 15) & ~(size_t)15;
  }
  if (batch) {
    HttpBatchHeader h{};
    h.magic = kBatchMagic;
    h.epoch = s.epoch;
    h.nchunks = (uint32_t)chunks.size();
    h.ntiles = (uint32_t)tiles;
    h.tiles_off = hdr;
    h.nslots = nslots;
    h.ttab_off = ttab_off(max_tiles);
    h.total_bytes = need;
    h.arena_bytes = used;
    memcpy(batch, &h, sizeof(h));
    memcpy((uint8_t*)batch + sizeof(h), chunks.data(), chunks.size() * sizeof(HttpChunk));
    memcpy((uint8_t*)batch + h.ttab_off, ttab.data(), ttab.size() * sizeof(HttpTile));
  }
  if (order)
    for (size_t sl = 0; sl < nslots; ++sl) order[sl] = req_of_slot[sl];
  // ---- tiles (parallel): meta block, string units, padding slots
  if (batch || (arena && build)) {
    parallel_ranges(tiles, nt, [&](size_t a, size_t b, unsigned) {
      for (size_t k = a; k < b; ++k) {
        if (batch) memset(data + (size_t)ttab[k].at * kGranule, 0, (size_t)tile_granules(ttab[k]) * kGranule);
        for (size_t l = 0; l < CG_HTTP_TILE; ++l) {
          const size_t sl = k * CG_HTTP_TILE + l;
          const uint32_t i = req_of_slot[sl];
          if (i == 0xFFFFFFFFu) {
            if (batch) unit_ptr(sl, 0)[7] = CG_HTTP_F_PAD;
            continue;
          }
          const uint8_t* str = str_ptr(i);
          const uint32_t len = (uint32_t)str_len(i);
          // meta (CG_HTTP_META_BYTES = 8): [0..3] remote identity, [4..6]
          // overflow arena offset / 16, [7] flags
          uint8_t meta[CG_HTTP_META_BYTES] = {0};
          memcpy(meta, &remote[i], 4);
          uint8_t flags = ingress[i] ? CG_HTTP_F_INGRESS : 0;
          if (malformed[i]) flags |= CG_HTTP_F_MALFORMED;
          if (len > CG_HTTP_SLOT_BYTES) {
            flags |= CG_HTTP_F_OVERFLOW;
            const uint64_t o = aoff[i];
            if (arena && o + 4 + len <= arena_cap) {
              memcpy(arena + o, &len, 4);
              memcpy(arena + o + 4, str, len);
            }
            const uint32_t off16 = (uint32_t)(o / 16);
            meta[4] = off16 & 0xFF;
            meta[5] = (off16 >> 8) & 0xFF;
            meta[6] = (off16 >> 16) & 0xFF;
          }
          meta[7] = flags;
          if (batch) {
            memcpy(unit_ptr(sl, 0), meta, CG_HTTP_META_BYTES);
            const uint32_t wu = walked_units(i);
            const HttpTile& tt = ttab[k];
            for (uint32_t u = 0; u < wu; ++u) {
              // (a half unit holds the tile's last ≤ 8 bytes of every lane)
              const size_t cap = u + 1 == tile_units(tt) && tile_half(tt) ? 8 : 16;
              memcpy(unit_ptr(sl, u + 1), str + u * 16, std::min<size_t>(cap, len - u * 16));
            }
          }
        }
      }
    });
  }
  lap("write");
  if (arena_used) *arena_used = used;
  if (arena && used > arena_cap) fail(CG_INVALID_ARGUMENT, "overflow arena too small");
}

// Every slot as one lane of http_kernel_global takes it (kernels_http.hip
// http_chunks, then http_tiles<1>), over host_view() and through the functions
// the kernels run (http_walk.h).  A lane's loads are made the same way: the
// slot's meta pair, its 16-byte units (a half last unit as 8 bytes and zeros,
// as ld_nt_unit gives it).  Leaving a slot once its verdict is settled (not
// counted; the dead state, which is absorbing) is loop structure: the kernel
// walks on and gets the same.
void http_eval_host(const HttpSnapshot& s, const uint8_t* batch, size_t nslots, const uint8_t* arena,
                    size_t arena_len, uint8_t* out, uint32_t* rule) {
  using namespace walk;
  const HttpDev T = s.host_view();
  HttpBatchHeader h;
  memcpy(&h, batch, sizeof(h));
  // Host-only checks, in front of the walk.  A stale batch, or
  // one of more slots than given: the kernel denies every slot and counts
  // it; here it is the caller's error.
  if (h.magic != kBatchMagic || h.epoch != T.epoch) fail(CG_INVALID_ARGUMENT, "batch packed for another snapshot");
  if ((size_t)h.ntiles * CG_HTTP_TILE > nslots) fail(CG_INVALID_ARGUMENT, "batch of more slots than given");
  // No read past the batch: its length is not an argument, so the header's
  // total_bytes bounds the chunk table, the tile table and every tile.
  const HttpChunk* chunks = (const HttpChunk*)(batch + sizeof(h));
  const HttpTile* ttab = (const HttpTile*)(batch + h.ttab_off);
  bool inside = sizeof(h) + (uint64_t)h.nchunks * sizeof(HttpChunk) <= h.total_bytes &&
                h.ttab_off <= h.total_bytes && h.tiles_off <= h.total_bytes &&
                (uint64_t)h.ntiles * sizeof(HttpTile) <= h.total_bytes - h.ttab_off;
  for (uint32_t t = 0; inside && t < h.ntiles; ++t)
    inside = ((uint64_t)ttab[t].at + tile_granules(ttab[t])) * kGranule <= h.total_bytes - h.tiles_off;
  if (!inside) fail(CG_INVALID_ARGUMENT, "batch tables or tiles past its end");
  // No read past the arena: the kernel's bound is the header's arena_bytes.
  const uint64_t arena_bytes = std::min<uint64_t>(h.arena_bytes, arena_len);

  // a slot no chunk reaches keeps what the verdict buffer held: 0
  std::fill(out, out + nslots, (uint8_t)0);
  if (rule) std::fill(rule, rule + nslots, kNoHit);
  for (uint32_t c = 0; c < h.nchunks; ++c) {
    const HttpChunk ch = chunks[c];
    if (!chunk_ok(ch, h.ntiles)) continue;  // malformed chunk
    const uint32_t prog = ch.prog;
    const bool real = prog < T.nprogs;
    HttpProg pg{};
    if (real) pg = T.progs[prog];
    const bool walkp = prog_walked(real, pg);
    // http_kernel's straight-line walker (a one-part program in LDS) reads a
    // half last unit and at most 8 units; every other walked program goes
    // through http_tiles, which denies a half tile unwalked
    const bool generic = !(prog_in_lds(T, pg, walkp) && pg.part_count == 1);
    const uint32_t* blk = T.cells + pg.cell_begin;
    const bool rebased = pg.flags & kProgRebased;
    const uint32_t W = pg.mask_words;
    for (uint32_t t = ch.first_tile; t < ch.first_tile + ch.ntiles; ++t) {
      const HttpTile tt = ttab[t];
      const uint8_t* tile = batch + h.tiles_off + (size_t)tt.at * kGranule;
      const bool half = tile_half(tt);
      const uint32_t units = generic ? tile_units(tt) : std::min<uint32_t>(tile_units(tt), CG_HTTP_UNITS - 1);
      for (uint32_t lane = 0; lane < CG_HTTP_TILE; ++lane) {
        const size_t sl = (size_t)t * CG_HTTP_TILE + lane;
        uint2 meta;
        memcpy(&meta, tile + lane * CG_HTTP_META_BYTES, sizeof(meta));
        const bool counted = slot_counted(meta.y);
        if (!walkp) out[sl] = counted && trivial_allows(prog, real);
        if (!walkp || !counted || (generic && half)) continue;
        const uint32_t row = remote_row(blk, pg, meta.x);
        // a part's walk of the slot: the first rule its end state's label allows
        auto part_hit = [&](auto cls, const HttpPart& pt, const uint32_t* cells) {
          constexpr bool kCls = decltype(cls)::value;
          uint32_t st = pt.start;
          for (uint32_t u = 0; u < units && st != pt.dead; ++u) {
            const uint8_t* up = tile + kMetaBytes + (size_t)u * kUnitBytes;
            uint4 unit = make_uint4(0, 0, 0, 0);
            if (half && u + 1 == units) memcpy(&unit, up + lane * 8, 8);
            else unit = load16(up + lane * 16);
            for (int k = 0; k < 16; ++k) st = step<kCls>(cells, pt.dead, st, get_byte(unit, k));
          }
          if (slot_overflow(meta.y)) st = walk_overflow<kCls>(cells, pt.dead, pt.start, arena, arena_bytes, meta, true);
          const uint32_t lab = state_label<kCls>(cells, st);
          return lab != 0xFFFFu ? first_meet(blk, pt.acc_off + lab * 2 * W, row, W) : kNoHit;
        };
        uint32_t hit = kNoHit;
        for (uint32_t pi = 0; pi < pg.part_count; ++pi) {
          const HttpPart pt = T.parts[pg.part_begin + pi];
          const uint32_t* cells = rebased ? blk : T.cells + pt.walk_off;
          hit = std::min(hit, pt.mode == kPartClass ? part_hit(std::true_type{}, pt, cells)
                                                    : part_hit(std::false_type{}, pt, cells));
        }
        if (pg.flags & kProgHasAlways) hit = std::min(hit, first_meet(blk, pg.always_off, row, W));
        out[sl] = hit != kNoHit;
        if (rule && hit != kNoHit) rule[sl] = pg.rule_base + hit;
      }
    }
  }
}

}  // namespace cg

// The packer's worker count for a large batch (what cg_http_pack uses).
extern "C" uint32_t cg_http_pack_threads(void) { return cg::pack_threads((size_t)1 << 20); }
