// selcache.cc — host compile of the selector cache (selcache.h): strings to
// interned ids, CSR tables, validation; the host walkers; the device publish.
#include "selcache.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <thread>

#include "kernels.h"

namespace cg {

namespace {

constexpr size_t kMaxValues = 1u << 24;  // ScReq.op_nv holds the count in 24 bits

// "source:key" → (source, key); no colon: source "any" (labels.ParseLabel's
// default, pkg/labels/labels.go).
void split_key(const std::string& full, std::string* src, std::string* key) {
  const size_t c = full.find(':');
  if (c == std::string::npos) {
    *src = "any";
    *key = full;
  } else {
    *src = full.substr(0, c);
    *key = full.substr(c + 1);
  }
}

void check_off64(const uint64_t* off, size_t n, const char* what) {
  if (off[0] != 0) fail(CG_INVALID_ARGUMENT, std::string(what) + ": offsets must start at 0");
  for (size_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) fail(CG_INVALID_ARGUMENT, std::string(what) + ": offsets decrease");
}

void check_off32(const uint32_t* off, size_t n, const char* what) {
  if (off[0] != 0) fail(CG_INVALID_ARGUMENT, std::string(what) + ": offsets must start at 0");
  for (size_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) fail(CG_INVALID_ARGUMENT, std::string(what) + ": offsets decrease");
}

std::string str_at(const uint8_t* blob, const uint64_t* off, size_t i) {
  return off[i + 1] == off[i] ? std::string() : std::string((const char*)blob + off[i], off[i + 1] - off[i]);
}

// Ids of the identities' strings start at 1; "any" is kScAny.
uint32_t intern(std::unordered_map<std::string, uint32_t>& dict, const std::string& s) {
  if (s == "any") return kScAny;
  auto it = dict.find(s);
  if (it != dict.end()) return it->second;
  if (dict.size() >= 0xFFFFFFF0u) fail(CG_MAP_FULL, "selector cache: too many distinct strings");
  const uint32_t id = (uint32_t)dict.size() + 1;
  dict.emplace(s, id);
  return id;
}

template <class F>
void run_threads(size_t items, uint32_t threads, F&& f) {
  const size_t t = std::max<size_t>(1, std::min<size_t>(threads ? threads : 1, items));
  if (t == 1) {
    f(0, items);
    return;
  }
  std::vector<std::thread> pool;
  const size_t per = (items + t - 1) / t;
  for (size_t k = 0; k < t; ++k) {
    const size_t lo = k * per, hi = std::min(items, lo + per);
    if (lo < hi) pool.emplace_back([&f, lo, hi] { f(lo, hi); });
  }
  for (auto& th : pool) th.join();
}

// ---- the label format of a prefix (pkg/labels/cidr.go:23-45)
// net.IP.String() of a 16-byte address that To4() refuses: lower-case hex
// groups without leading zeros, the first longest run of two or more zero
// groups as "::".
std::string go_ip6_string(const uint8_t p[16]) {
  int e0 = -1, e1 = -1;
  for (int i = 0; i < 16; i += 2) {
    int j = i;
    while (j < 16 && p[j] == 0 && p[j + 1] == 0) j += 2;
    if (j > i && j - i > e1 - e0) {
      e0 = i;
      e1 = j;
      i = j;
    }
  }
  if (e1 - e0 <= 2) e0 = e1 = -1;
  static const char* hex = "0123456789abcdef";
  std::string out;
  for (int i = 0; i < 16; i += 2) {
    if (i == e0) {
      out += "::";
      i = e1;
      if (i >= 16) break;
    } else if (i > 0) {
      out += ':';
    }
    const uint32_t g = ((uint32_t)p[i] << 8) | p[i + 1];
    bool on = false;
    for (int sh = 12; sh >= 0; sh -= 4) {
      const uint32_t d = (g >> sh) & 15u;
      if (d || on || sh == 0) {
        out += hex[d];
        on = true;
      }
    }
  }
  return out;
}

bool is_mapped4(const uint8_t p[16]) {  // net.IP.To4 on 16 bytes
  for (int i = 0; i < 10; ++i)
    if (p[i]) return false;
  return p[10] == 0xFF && p[11] == 0xFF;
}

std::string dotted(const uint8_t* p) {
  return std::to_string(p[0]) + "." + std::to_string(p[1]) + "." + std::to_string(p[2]) + "." + std::to_string(p[3]);
}

// maskedIPToLabelString without the "cidr:" source.
std::string label_key_of(uint32_t family, const uint8_t addr[16], uint32_t len) {
  std::string ip = family == 4 ? dotted(addr) : is_mapped4(addr) ? dotted(addr + 12) : go_ip6_string(addr);
  for (char& c : ip)
    if (c == ':') c = '-';
  if (ip.front() == '-') ip.insert(ip.begin(), '0');
  if (ip.back() == '-') ip.push_back('0');
  return ip + "/" + std::to_string(len);
}

bool parse_dec(const std::string& s, size_t lo, size_t hi, uint32_t max, uint32_t* out) {
  if (hi <= lo || hi - lo > 3) return false;
  uint32_t v = 0;
  for (size_t i = lo; i < hi; ++i) {
    if (s[i] < '0' || s[i] > '9') return false;
    v = v * 10 + (uint32_t)(s[i] - '0');
  }
  *out = v;
  return v <= max;
}

bool parse_ip4(const std::string& s, uint8_t out[4]) {
  size_t at = 0;
  for (int k = 0; k < 4; ++k) {
    size_t dot = k < 3 ? s.find('.', at) : s.size();
    uint32_t v;
    if (dot == std::string::npos || !parse_dec(s, at, dot, 255, &v)) return false;
    out[k] = (uint8_t)v;
    at = dot + 1;
  }
  return true;
}

// Hex groups and at most one "::"; no embedded dotted quad (the label format
// never prints one inside an IPv6 text).
bool parse_ip6(const std::string& s, uint8_t out[16]) {
  uint16_t g[8];
  int ng = 0, ell = -1;
  size_t i = 0;
  const size_t n = s.size();
  if (n >= 2 && s[0] == ':' && s[1] == ':') {
    ell = 0;
    i = 2;
  } else if (n == 0 || s[0] == ':') {
    return false;
  }
  while (i < n) {
    uint32_t v = 0;
    size_t d = 0;
    for (; i < n && d < 4; ++i, ++d) {
      const char c = s[i];
      const int x = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
      if (x < 0) break;
      v = v * 16 + (uint32_t)x;
    }
    if (d == 0 || ng == 8) return false;
    g[ng++] = (uint16_t)v;
    if (i == n) break;
    if (s[i] != ':' || ++i == n) return false;
    if (s[i] == ':') {
      if (ell >= 0) return false;
      ell = ng;
      ++i;
    }
  }
  if (ell < 0 ? ng != 8 : ng > 7) return false;
  uint16_t full[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int head = ell < 0 ? ng : ell;
  for (int k = 0; k < head; ++k) full[k] = g[k];
  for (int k = head; k < ng; ++k) full[8 - (ng - k)] = g[k];
  for (int k = 0; k < 8; ++k) {
    out[2 * k] = (uint8_t)(full[k] >> 8);
    out[2 * k + 1] = (uint8_t)full[k];
  }
  return true;
}

uint32_t mask_word(uint32_t len, uint32_t k) {  // bits of word k among the first `len`
  const uint32_t b = len > 32 * k ? std::min<uint32_t>(len - 32 * k, 32) : 0;
  return b ? 0xFFFFFFFFu << (32 - b) : 0u;
}

uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

}  // namespace

std::string sc_cidr_label_key(const ScCidr& p) {
  uint8_t addr[16];
  for (int k = 0; k < 4; ++k)
    for (int b = 0; b < 4; ++b) addr[4 * k + b] = (uint8_t)(p.a[k] >> (24 - 8 * b));
  return label_key_of(p.family, addr, p.len);
}

std::shared_ptr<const ScCidrSnap> sc_compile_cidrs(const uint32_t* ids, const cg_cidr* prefixes, size_t n) {
  auto s = std::make_shared<ScCidrSnap>();
  if (n == 0) return s;
  if (!ids || !prefixes) fail(CG_INVALID_ARGUMENT, "selector cache: NULL prefix identity arrays");
  if (n > 0xFFFFFFC0u) fail(CG_MAP_FULL, "selector cache: too many identities");
  s->ids.assign(ids, ids + n);
  s->recs.resize(n);
  for (size_t i = 0; i < n; ++i) {
    const cg_cidr& c = prefixes[i];
    if (c.family != 4 && c.family != 6)
      fail(CG_INVALID_ARGUMENT, "prefix identity " + std::to_string(i) + ": family is neither 4 nor 6");
    if (c.prefixlen > (c.family == 4 ? 32u : 128u))
      fail(CG_INVALID_ARGUMENT, "prefix identity " + std::to_string(i) + ": prefix length past the family's");
    ScCidr r{};
    const uint32_t nw = c.family == 4 ? 1 : 4;
    for (uint32_t k = 0; k < nw; ++k) r.a[k] = be32(c.addr + 4 * k) & mask_word(c.prefixlen, k);
    r.len = c.prefixlen;
    r.family = c.family;
    s->recs[i] = r;
  }
  return s;
}

ScReqCidr sc_classify_req(const std::string& src, const std::string& key, const std::vector<std::string>& vals) {
  ScReqCidr q{};
  q.kind = kScCidrAbsent;
  for (const auto& v : vals) q.has_empty |= v.empty() ? 1u : 0u;
  if (key == "world" && (src == "reserved" || src == "any")) {
    q.kind = kScCidrWorld;
    return q;
  }
  if (src != "cidr" && src != "any") return q;
  const size_t slash = key.rfind('/');
  uint32_t len;
  if (slash == std::string::npos || !parse_dec(key, slash + 1, key.size(), 128, &len)) return q;
  std::string ip = key.substr(0, slash);
  uint8_t addr[16] = {0};
  uint32_t family;
  if (ip.find('.') != std::string::npos) {
    uint8_t v4[4];
    if (!parse_ip4(ip, v4)) return q;
    if (len <= 32) {
      family = 4;
      std::copy(v4, v4 + 4, addr);
    } else if (len >= 96) {  // the text of an IPv4-mapped IPv6 prefix
      family = 6;
      addr[10] = addr[11] = 0xFF;
      std::copy(v4, v4 + 4, addr + 12);
    } else {
      return q;
    }
  } else {
    for (char& c : ip)
      if (c == '-') c = ':';
    if (!parse_ip6(ip, addr)) return q;
    family = 6;
  }
  const uint32_t nw = family == 4 ? 1 : 4;
  for (uint32_t k = 0; k < nw; ++k) {
    q.a[k] = be32(addr + 4 * k);
    q.mask[k] = mask_word(len, k);
    if (q.a[k] & ~q.mask[k]) return q;  // host bits set: no label is printed that way
  }
  if (label_key_of(family, addr, len) != key) return q;
  q.len = len;
  q.family = family;
  q.kind = kScCidrPrefix;
  return q;
}

std::shared_ptr<const ScIdentSnap> sc_compile_identities(const uint32_t* ids, size_t n, const uint32_t* label_off,
                                                         const uint8_t* key_blob, const uint64_t* key_off,
                                                         const uint8_t* val_blob, const uint64_t* val_off) {
  auto s = std::make_shared<ScIdentSnap>();
  if (n == 0) return s;
  if (!ids || !label_off) fail(CG_INVALID_ARGUMENT, "selector cache: NULL identity arrays");
  if (n > 0xFFFFFFC0u) fail(CG_MAP_FULL, "selector cache: too many identities");
  check_off32(label_off, n, "identity labels");
  const size_t nl = label_off[n];
  if (nl && (!key_off || !val_off)) fail(CG_INVALID_ARGUMENT, "selector cache: NULL label strings");
  if (nl) {
    check_off64(key_off, nl, "label keys");
    check_off64(val_off, nl, "label values");
    if ((key_off[nl] && !key_blob) || (val_off[nl] && !val_blob))
      fail(CG_INVALID_ARGUMENT, "selector cache: NULL label blob");
  }
  s->ids.assign(ids, ids + n);
  s->lab_off.assign(label_off, label_off + n + 1);
  s->labels.resize(nl);
  std::string src, key;
  for (size_t l = 0; l < nl; ++l) {
    split_key(str_at(key_blob, key_off, l), &src, &key);
    s->labels[l] = ScLabel{intern(s->dict, key), intern(s->dict, src), intern(s->dict, str_at(val_blob, val_off, l)),
                           0};
  }
  s->n = (uint32_t)n;
  return s;
}

std::vector<ScSelSrc> sc_parse_selectors(const cg_selector_table& t) {
  std::vector<ScSelSrc> out(t.n_selectors);
  if (t.n_selectors == 0) return out;
  if (t.n_selectors > 0x7FFFFFFFu) fail(CG_MAP_FULL, "selector table: too many selectors");
  if (!t.req_off) fail(CG_INVALID_ARGUMENT, "selector table: NULL req_off");
  check_off32(t.req_off, t.n_selectors, "selector requirements");
  const size_t nr = t.req_off[t.n_selectors];
  size_t nv = 0;
  if (nr) {
    if (!t.ops || !t.key_off || !t.val_off) fail(CG_INVALID_ARGUMENT, "selector table: NULL requirement arrays");
    check_off64(t.key_off, nr, "requirement keys");
    check_off32(t.val_off, nr, "requirement values");
    if (t.key_off[nr] && !t.key_blob) fail(CG_INVALID_ARGUMENT, "selector table: NULL key blob");
    nv = t.val_off[nr];
    if (nv) {
      if (!t.val_str_off) fail(CG_INVALID_ARGUMENT, "selector table: NULL value offsets");
      check_off64(t.val_str_off, nv, "requirement value strings");
      if (t.val_str_off[nv] && !t.val_blob) fail(CG_INVALID_ARGUMENT, "selector table: NULL value blob");
    }
  }
  for (size_t s = 0; s < t.n_selectors; ++s) {
    ScSelSrc& sel = out[s];
    sel.always = t.req_off[s + 1] == t.req_off[s];  // selector.go:307-310: the wildcard
    for (size_t r = t.req_off[s]; r < t.req_off[s + 1]; ++r) {
      ScSelSrc::Req q;
      q.op = t.ops[r];
      if (q.op > CG_SEL_DOES_NOT_EXIST)
        fail(CG_POLICY_REJECTED, "selector " + std::to_string(s) + ": unknown operator " + std::to_string(q.op));
      const std::string full = str_at(t.key_blob, t.key_off, r);
      // selector.go:284-289: reserved:all among the matchLabels selects everything
      if (q.op == CG_SEL_MATCH_LABEL && full == "reserved:all") sel.always = true;
      split_key(full, &q.src, &q.key);
      const size_t v0 = t.val_off[r], v1 = t.val_off[r + 1];
      if (v1 - v0 >= kMaxValues) fail(CG_MAP_FULL, "selector table: too many values in one requirement");
      if (q.op == CG_SEL_MATCH_LABEL && v1 - v0 != 1)
        fail(CG_INVALID_ARGUMENT, "selector table: a matchLabels requirement has exactly one value");
      for (size_t v = v0; v < v1; ++v) q.vals.push_back(str_at(t.val_blob, t.val_str_off, v));
      sel.reqs.push_back(std::move(q));
    }
  }
  return out;
}

std::shared_ptr<const ScRuleSrc> sc_parse_rules(const cg_selector_table& sels, const cg_selcache_rules& rules) {
  auto out = std::make_shared<ScRuleSrc>();
  out->sels = sc_parse_selectors(sels);
  const size_t n = rules.n_rules, S = out->sels.size();
  if (n > 0x7FFFFFFFu) fail(CG_MAP_FULL, "selector cache: too many rules");
  if (n && (!rules.subject || !rules.dir_flags)) fail(CG_INVALID_ARGUMENT, "rule set: NULL subject/dir_flags");
  out->n = (uint32_t)n;
  for (size_t r = 0; r < n; ++r) {
    if (rules.subject[r] >= S) fail(CG_INVALID_ARGUMENT, "rule set: subject selector out of range");
    if (rules.dir_flags[r] & ~3u) fail(CG_INVALID_ARGUMENT, "rule set: unknown dir_flags bits");
  }
  if (n) {
    out->subject.assign(rules.subject, rules.subject + n);
    out->flags.assign(rules.dir_flags, rules.dir_flags + n);
  }
  for (int d = 0; d < 2; ++d) {
    const uint32_t* offs[2] = {rules.req_off[d], rules.allow_off[d]};
    const uint32_t* idxs[2] = {rules.req_idx[d], rules.allow_idx[d]};
    std::vector<uint32_t>* o_off[2] = {&out->req_off[d], &out->allow_off[d]};
    std::vector<uint32_t>* o_idx[2] = {&out->req_idx[d], &out->allow_idx[d]};
    for (int k = 0; k < 2; ++k) {
      if (n == 0) {
        o_off[k]->assign(1, 0);
        continue;
      }
      if (!offs[k]) fail(CG_INVALID_ARGUMENT, "rule set: NULL list offsets");
      check_off32(offs[k], n, "rule lists");
      const size_t m = offs[k][n];
      if (m && !idxs[k]) fail(CG_INVALID_ARGUMENT, "rule set: NULL list indices");
      for (size_t x = 0; x < m; ++x)
        if (idxs[k][x] >= S) fail(CG_INVALID_ARGUMENT, "rule set: selector index out of range");
      o_off[k]->assign(offs[k], offs[k] + n + 1);
      if (m) o_idx[k]->assign(idxs[k], idxs[k] + m);
    }
  }
  return out;
}

ScSelTab sc_compile_selectors(const ScIdentSnap& idents, const std::vector<ScSelSrc>& sels) {
  ScSelTab t;
  // strings no identity carries: ids past the dictionary's, so that they
  // equal no label's id and each other only when the strings are equal
  std::unordered_map<std::string, uint32_t> extra;
  const uint32_t base = (uint32_t)idents.dict.size() + 1;
  auto id_of = [&](const std::string& s) -> uint32_t {
    if (s == "any") return kScAny;
    auto it = idents.dict.find(s);
    if (it != idents.dict.end()) return it->second;
    auto jt = extra.find(s);
    if (jt != extra.end()) return jt->second;
    if ((uint64_t)base + extra.size() >= 0xFFFFFFF0ull) fail(CG_MAP_FULL, "selector cache: too many distinct strings");
    const uint32_t id = base + (uint32_t)extra.size();
    extra.emplace(s, id);
    return id;
  };
  t.sels.reserve(sels.size());
  for (const ScSelSrc& s : sels) {
    if (t.reqs.size() + s.reqs.size() > 0x7FFFFFFFu) fail(CG_MAP_FULL, "selector table: too many requirements");
    t.sels.push_back(ScSel{(uint32_t)t.reqs.size(), (uint32_t)s.reqs.size() | (s.always ? kScAlways : 0u)});
    for (const auto& q : s.reqs) {
      if (t.vals.size() + q.vals.size() > 0xFFFFFFF0u) fail(CG_MAP_FULL, "selector table: too many values");
      t.reqs.push_back(ScReq{id_of(q.key), id_of(q.src), (uint32_t)q.op | ((uint32_t)q.vals.size() << 8),
                             (uint32_t)t.vals.size()});
      t.creqs.push_back(sc_classify_req(q.src, q.key, q.vals));
      for (const auto& v : q.vals) t.vals.push_back(id_of(v));
    }
  }
  return t;
}

void sc_match_host(const ScIdentDev& I, const ScSelDev& T, uint64_t* bits, uint32_t threads) {
  const size_t W = I.words;
  run_threads((size_t)T.n * W, threads, [&](size_t lo, size_t hi) {
    for (size_t c = lo; c < hi; ++c) {
      const uint32_t s = (uint32_t)(c / W), w = (uint32_t)(c % W);
      uint64_t word = 0;
      const uint32_t i1 = std::min<uint64_t>((uint64_t)I.n + I.nc, 64ull * w + 64);
      for (uint32_t i = 64 * w; i < i1; ++i)
        word |= (uint64_t)(i < I.n ? sc_matches(I, T, s, i) : sc_cidr_matches(I, T, s, i - I.n)) << (i & 63u);
      bits[c] = word;
    }
  });
}

void sc_reach_host(const ScRuleDev& R, uint32_t n_ids, uint32_t words, const uint32_t* eps, size_t n, uint64_t* ing,
                   uint64_t* eg, uint8_t* flags, uint32_t threads) {
  const uint64_t valid_last = (n_ids & 63u) ? (1ull << (n_ids & 63u)) - 1ull : ~0ull;
  run_threads(n, threads, [&](size_t lo, size_t hi) {
    std::vector<uint32_t> selected;
    for (size_t k = lo; k < hi; ++k) {
      const uint32_t e = eps[k];
      selected.clear();
      uint32_t fl = 0;
      for (uint32_t r = 0; r < R.n; ++r)
        if ((R.M[(size_t)R.subject[r] * words + (e >> 6)] >> (e & 63u)) & 1ull) {
          selected.push_back(r);
          fl |= R.flags[r];
        }
      flags[k] = (uint8_t)fl;
      uint64_t* out[2] = {ing + k * words, eg + k * words};
      for (int d = 0; d < 2; ++d) {
        for (uint32_t w = 0; w < words; ++w) {
          uint64_t allow = 0, deny = 0;
          for (uint32_t r : selected) {
            for (uint32_t x = R.req_off[d][r]; x < R.req_off[d][r + 1]; ++x)
              deny |= ~R.M[(size_t)R.req_idx[d][x] * words + w];
            for (uint32_t x = R.allow_off[d][r]; x < R.allow_off[d][r + 1]; ++x)
              allow |= R.M[(size_t)R.allow_idx[d][x] * words + w];
          }
          out[d][w] = allow & ~deny & (w == words - 1 ? valid_last : ~0ull);
        }
      }
    }
  });
}

ScExpTab sc_compile_expand(const cg_expand_table& t, size_t src_rows) {
  ScExpTab out;
  const size_t n = t.n_rows;
  if (n == 0) return out;
  if (n > 0x7FFFFFFFu) fail(CG_MAP_FULL, "expansion table: too many rows");
  if (!t.rows || !t.src_off) fail(CG_INVALID_ARGUMENT, "expansion table: NULL rows/src_off");
  check_off32(t.src_off, n, "expansion sources");
  const size_t m = t.src_off[n];
  if (m && !t.src_idx) fail(CG_INVALID_ARGUMENT, "expansion table: NULL src_idx");
  for (size_t x = 0; x < m; ++x)
    if (t.src_idx[x] >= src_rows) fail(CG_INVALID_ARGUMENT, "expansion table: source row index out of range");
  out.rows.resize(n);
  for (size_t r = 0; r < n; ++r) {
    const cg_expand_row& in = t.rows[r];
    if (in.flags & ~(uint32_t)CG_EXP_ALL) fail(CG_INVALID_ARGUMENT, "expansion table: unknown row flags");
    out.rows[r] = ScExpRow{t.src_off[r], t.src_off[r + 1] - t.src_off[r],
                           (uint32_t)in.dport | ((uint32_t)in.protocol << 16) | ((uint32_t)in.egress << 24),
                           in.proxy_port, (uint16_t)in.flags};
  }
  if (m) out.src_idx.assign(t.src_idx, t.src_idx + m);
  return out;
}

void sc_expand_host(const ScExpDev& X, uint64_t* row_off, cg_policy_key* keys, uint16_t* proxy, uint64_t cap,
                    uint64_t* total, uint32_t threads) {
  const size_t R = X.n_rows;
  std::vector<uint64_t> cnt(R, 0);
  run_threads(R, threads, [&](size_t lo, size_t hi) {
    for (size_t r = lo; r < hi; ++r)
      for (uint32_t w = 0; w < X.words; ++w) cnt[r] += (uint64_t)__builtin_popcountll(sc_exp_word(X, X.rows[r], w));
  });
  uint64_t sum = 0;
  for (size_t r = 0; r < R; ++r) {
    row_off[r] = sum;
    sum += cnt[r];
  }
  row_off[R] = sum;
  *total = sum;
  if (sum > cap) return;
  run_threads(R, threads, [&](size_t lo, size_t hi) {
    for (size_t r = lo; r < hi; ++r) {
      const ScExpRow& row = X.rows[r];
      uint64_t at = row_off[r];
      for (uint32_t w = 0; w < X.words; ++w) {
        uint64_t word = sc_exp_word(X, row, w);
        while (word) {
          const uint32_t b = (uint32_t)__builtin_ctzll(word);
          word &= word - 1;
          cg_policy_key k;
          k.sec_label = X.ids[64u * w + b];
          k.dport = (uint16_t)row.tmpl;
          k.protocol = (uint8_t)(row.tmpl >> 16);
          k.egress = (uint8_t)(row.tmpl >> 24);
          keys[at] = k;
          proxy[at++] = row.proxy_be;
        }
      }
    }
  });
}

ScRuleDev ScPublished::host_rules() const {
  ScRuleDev r{};
  r.subject = rules->subject.data();
  r.flags = rules->flags.data();
  for (int d = 0; d < 2; ++d) {
    r.req_off[d] = rules->req_off[d].data();
    r.req_idx[d] = rules->req_idx[d].data();
    r.allow_off[d] = rules->allow_off[d].data();
    r.allow_idx[d] = rules->allow_idx[d].data();
  }
  r.M = reinterpret_cast<const unsigned long long*>(host_m.data());
  r.n = rules->n;
  return r;
}

// Compile the rule selectors against the current identities and publish a
// fresh snapshot; on a GPU handle upload it and compute M = the match matrix
// of the rule selectors, which every reach launch reads.  Anything that
// fails leaves the previous snapshot published.
void SelcacheState::rebuild(Engine& e) {
  auto p = std::make_shared<ScPublished>();
  p->idents = idents;
  p->cidrs = cidrs;
  p->rules = rules;
  const uint64_t total = (uint64_t)idents->n + cidrs->recs.size();
  if (total > 0xFFFFFFC0ull) fail(CG_MAP_FULL, "selector cache: too many identities");
  p->n = (uint32_t)total;
  p->words = (uint32_t)((total + 63) / 64);
  p->ids = idents->ids;
  p->ids.insert(p->ids.end(), cidrs->ids.begin(), cidrs->ids.end());
  p->seltab = sc_compile_selectors(*idents, rules->sels);
  if (e.has_gpu()) {
    e.set_device();
    auto tab = std::make_shared<DevTables>();
    p->dI = ScIdentDev{tab->add(idents->lab_off), tab->add(idents->labels), idents->n, p->words,
                       tab->add(cidrs->recs),     (uint32_t)cidrs->recs.size()};
    p->d_ids = tab->add(p->ids);
    p->dT = ScSelDev{tab->add(p->seltab.sels), tab->add(p->seltab.reqs), tab->add(p->seltab.vals),
                     (uint32_t)p->seltab.sels.size(), tab->add(p->seltab.creqs)};
    ScRuleDev r{};
    r.subject = tab->add(rules->subject);
    r.flags = tab->add(rules->flags);
    for (int d = 0; d < 2; ++d) {
      r.req_off[d] = tab->add(rules->req_off[d]);
      r.req_idx[d] = tab->add(rules->req_idx[d]);
      r.allow_off[d] = tab->add(rules->allow_off[d]);
      r.allow_idx[d] = tab->add(rules->allow_idx[d]);
    }
    r.n = rules->n;
    tab->bufs.emplace_back();
    tab->bufs.back().alloc((size_t)p->dT.n * p->words * sizeof(uint64_t));
    unsigned long long* M = tab->bufs.back().as<unsigned long long>();
    r.M = M;
    hip_check(launch_selcache_match(p->dI, p->dT, M, e.stream, e.cus), "selcache match kernel launch");
    dev_sync(e, nullptr);
    p->dR = r;
    p->tab = std::move(tab);
  }
  pub = std::move(p);
  dirty = false;
}

}  // namespace cg
