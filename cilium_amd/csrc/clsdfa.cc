// clsdfa.cc — Hopcroft minimization over byte classes.
#include "clsdfa.h"

#include <algorithm>
#include <deque>
#include <map>
#include <numeric>
#include <set>
#include <string>
#include <unordered_map>

#include "common.h"

namespace cg {

namespace {

// Refinable partition (Valmari-style): elements of a block are contiguous in
// `elems`; marking moves an element into the block's marked prefix.
struct Partition {
  std::vector<int> elems, loc, blk, first, end, mid;
  std::vector<int> touched;

  explicit Partition(int n) : elems(n), loc(n), blk(n, 0) {
    std::iota(elems.begin(), elems.end(), 0);
    std::iota(loc.begin(), loc.end(), 0);
  }
  int nblocks() const { return (int)first.size(); }
  void mark(int e) {
    int b = blk[e];
    int i = loc[e], j = mid[b];
    if (i < j) return;  // already marked
    std::swap(elems[i], elems[j]);
    loc[elems[i]] = i;
    loc[elems[j]] = j;
    if (mid[b]++ == first[b]) touched.push_back(b);
  }
};

}  // namespace

ClsDfa minimize_cls(const ClsDfa& d) {
  const int n = d.size();
  const int k = d.ncls;
  // initial partition by label (dead state shares block with other label-0 states)
  Partition P(n);
  {
    std::vector<std::pair<uint32_t, int>> v(n);
    for (int s = 0; s < n; ++s) v[s] = {d.label[s], s};
    std::stable_sort(v.begin(), v.end());
    for (int i = 0; i < n; ++i) {
      int s = v[i].second;
      P.elems[i] = s;
      P.loc[s] = i;
      if (i == 0 || v[i].first != v[i - 1].first) {
        P.first.push_back(i);
        if (i > 0) P.end.push_back(i);
      }
      P.blk[s] = (int)P.first.size() - 1;
    }
    P.end.push_back(n);
    P.mid = P.first;
  }
  // inverse transitions, CSR per (class, target)
  std::vector<int> inv_off((size_t)k * n + 1, 0);
  std::vector<int> inv((size_t)n * k);
  for (int s = 0; s < n; ++s)
    for (int c = 0; c < k; ++c) inv_off[(size_t)c * n + d.trans[(size_t)s * k + c] + 1]++;
  for (size_t i = 1; i < inv_off.size(); ++i) inv_off[i] += inv_off[i - 1];
  {
    std::vector<int> fill(inv_off.begin(), inv_off.end() - 1);
    for (int s = 0; s < n; ++s)
      for (int c = 0; c < k; ++c) inv[fill[(size_t)c * n + d.trans[(size_t)s * k + c]]++] = s;
  }
  std::vector<uint8_t> in_w(P.nblocks(), 1);
  std::vector<int> W;
  for (int b = 0; b < P.nblocks(); ++b) W.push_back(b);
  std::vector<int> splitter;
  while (!W.empty()) {
    int A = W.back();
    W.pop_back();
    in_w[A] = 0;
    splitter.assign(P.elems.begin() + P.first[A], P.elems.begin() + P.end[A]);
    for (int c = 0; c < k; ++c) {
      for (int t : splitter) {
        size_t o = (size_t)c * n + t;
        for (int i = inv_off[o]; i < inv_off[o + 1]; ++i) P.mark(inv[i]);
      }
      for (int b : P.touched) {
        if (P.mid[b] == P.end[b]) {  // every element marked: no split
          P.mid[b] = P.first[b];
          continue;
        }
        // split: marked [first, mid) becomes new block nb
        int nb = P.nblocks();
        P.first.push_back(P.first[b]);
        P.end.push_back(P.mid[b]);
        P.mid.push_back(P.first[b]);
        P.first[b] = P.mid[b];
        P.mid[b] = P.first[b];
        for (int i = P.first[nb]; i < P.end[nb]; ++i) P.blk[P.elems[i]] = nb;
        in_w.push_back(0);
        int sz_nb = P.end[nb] - P.first[nb], sz_b = P.end[b] - P.first[b];
        if (in_w[b]) {
          W.push_back(nb);
          in_w[nb] = 1;
        } else if (sz_nb <= sz_b) {
          W.push_back(nb);
          in_w[nb] = 1;
        } else {
          W.push_back(b);
          in_w[b] = 1;
        }
      }
      P.touched.clear();
    }
  }
  // quotient with canonical BFS order
  const int nb = P.nblocks();
  std::vector<int> rep(nb);
  for (int b = 0; b < nb; ++b) rep[b] = P.elems[P.first[b]];
  std::vector<int> newid(nb, -1);
  std::vector<int> order;
  int dead_b = P.blk[0];
  newid[dead_b] = 0;
  order.push_back(dead_b);
  ClsDfa out;
  int start_b = P.blk[1];
  if (start_b != dead_b) {
    newid[start_b] = 1;
    order.push_back(start_b);
    for (size_t qi = 1; qi < order.size(); ++qi) {
      int s = rep[order[qi]];
      for (int c = 0; c < k; ++c) {
        int t = P.blk[d.trans[(size_t)s * k + c]];
        if (newid[t] < 0) {
          newid[t] = (int)order.size();
          order.push_back(t);
        }
      }
    }
  } else {
    order.push_back(dead_b);  // language empty: start == a copy of dead
  }
  const int m = (int)order.size();
  // recompress classes: classes with identical columns merge
  std::vector<int> col_id(k);
  std::vector<int> col_rep;
  {
    std::map<std::vector<int>, int> cols;
    std::vector<int> col(m);
    for (int c = 0; c < k; ++c) {
      for (int i = 0; i < m; ++i) {
        int t = (i == 1 && start_b == dead_b) ? 0 : newid[P.blk[d.trans[(size_t)rep[order[i]] * k + c]]];
        col[i] = (i == 0) ? 0 : t;
      }
      auto it = cols.emplace(col, (int)cols.size());
      col_id[c] = it.first->second;
      if (it.second) col_rep.push_back(c);
    }
  }
  out.ncls = (int)col_rep.size();
  for (int b = 0; b < 256; ++b) out.clsmap[b] = (uint8_t)col_id[d.clsmap[b]];
  out.trans.assign((size_t)m * out.ncls, 0);
  out.label.assign(m, 0);
  for (int i = 1; i < m; ++i) {
    if (start_b == dead_b) break;
    int s = rep[order[i]];
    out.label[i] = d.label[s];
    for (int c = 0; c < out.ncls; ++c)
      out.trans[(size_t)i * out.ncls + c] = newid[P.blk[d.trans[(size_t)s * k + col_rep[c]]]];
  }
  return out;
}

int run_classes(const ClsDfa& d, int s, const uint8_t* seq, size_t n) {
  for (size_t i = 0; i < n && s != 0 && !d.label[s]; ++i) s = d.trans[(size_t)s * d.ncls + seq[i]];
  return s;
}

ClsDfa with_token_columns(const ClsDfa& d, const std::vector<ClsSeq>& toks) {
  ClsDfa o = d;
  const int k = d.ncls, k2 = k + (int)toks.size();
  o.ncls = k2;
  o.trans.assign((size_t)d.size() * k2, 0);
  for (int s = 0; s < d.size(); ++s) {
    std::copy(d.trans.begin() + (size_t)s * k, d.trans.begin() + (size_t)(s + 1) * k, o.trans.begin() + (size_t)s * k2);
    if (s == 0 || d.label[s]) continue;  // dead and accepting rows have no live transition
    for (size_t t = 0; t < toks.size(); ++t)
      o.trans[(size_t)s * k2 + k + t] = run_classes(d, s, toks[t].data(), toks[t].size());
  }
  return o;
}

std::vector<ClsSeq> pick_tokens(const ClsDfa& d, const std::vector<std::vector<uint64_t>>& label_masks,
                                int max_tokens, size_t cell_budget) {
  std::vector<ClsSeq> picked;
  const int n = d.size(), k = d.ncls;
  if (max_tokens <= 0 || n < 3 || label_masks.empty()) return picked;
  const size_t W = label_masks[0].size();
  auto tr = [&](int s, int c) { return d.trans[(size_t)s * k + c]; };
  // forced states: not accepting, one live class, and that one leaves the state
  std::vector<int> fcls(n, -1);
  for (int s = 1; s < n; ++s) {
    if (d.label[s]) continue;
    int live = 0, c1 = -1;
    for (int c = 0; c < k; ++c)
      if (tr(s, c) != 0) {
        ++live;
        c1 = c;
      }
    if (live == 1 && tr(s, c1) != s) fcls[s] = c1;
  }
  // rule tags reachable from each state (a fixpoint; states are numbered
  // breadth-first, so a descending sweep settles most of it at once)
  std::vector<uint64_t> reach((size_t)n * W, 0);
  for (int s = 1; s < n; ++s)
    if (d.label[s] && d.label[s] - 1 < label_masks.size())
      std::copy(label_masks[d.label[s] - 1].begin(), label_masks[d.label[s] - 1].end(), reach.begin() + (size_t)s * W);
  for (bool changed = true; changed;) {
    changed = false;
    for (int s = n - 1; s >= 1; --s)
      for (int c = 0; c < k; ++c) {
        const int t = tr(s, c);
        if (t == 0 || t == s) continue;
        for (size_t w = 0; w < W; ++w) {
          const uint64_t v = reach[(size_t)s * W + w] | reach[(size_t)t * W + w];
          if (v != reach[(size_t)s * W + w]) {
            reach[(size_t)s * W + w] = v;
            changed = true;
          }
        }
      }
  }
  std::vector<uint32_t> tags(n, 0);
  for (int s = 0; s < n; ++s)
    for (size_t w = 0; w < W; ++w) tags[s] += (uint32_t)__builtin_popcountll(reach[(size_t)s * W + w]);
  // chains by spelling, with the tags behind each symbol summed over the
  // chains that spell it.  A chain starts on a live edge of a branching state
  // (or of the start state) into a forced state and follows the forced run.
  constexpr size_t kChainMax = 64;
  std::map<std::string, std::vector<uint64_t>> chains;
  for (int s = 1; s < n; ++s) {
    if (d.label[s] || (fcls[s] >= 0 && s != 1)) continue;
    for (int c = 0; c < k; ++c) {
      const int t = tr(s, c);
      if (t == 0 || t == s || fcls[t] < 0) continue;
      std::string sp(1, (char)c);
      std::vector<uint64_t> w{tags[t]};
      for (int cur = t; fcls[cur] >= 0 && sp.size() < kChainMax;) {
        sp.push_back((char)fcls[cur]);
        cur = tr(cur, fcls[cur]);
        w.push_back(tags[cur]);
      }
      auto& acc = chains[sp];
      acc.resize(w.size(), 0);
      for (size_t i = 0; i < w.size(); ++i) acc[i] += w[i];
    }
  }
  // what a token's column costs: a cell in every row it leaves off the row's
  // default (comb.h; the default is the commoner of "dead" and "stay")
  std::vector<uint8_t> self_row(n, 0);
  for (int s = 1; s < n; ++s) {
    int self_n = 0, dead_n = 0;
    for (int c = 0; c < k; ++c) {
      self_n += tr(s, c) == s;
      dead_n += tr(s, c) == 0;
    }
    self_row[s] = !d.label[s] && self_n > dead_n;
  }
  auto cells_of = [&](const std::string& t) {
    size_t cells = 0;
    for (int s = 1; s < n; ++s)
      if (!d.label[s]) cells += run_classes(d, s, (const uint8_t*)t.data(), t.size()) != (self_row[s] ? s : 0);
    return cells;
  };
  // First the tokens that cost a cell in at most an eighth of the rows; the
  // dear ones (a token that holds a field separator takes a cell in every
  // self-looping row, to save two symbols more than its halves) only for the
  // codes those leave free.
  size_t column_cap = std::max<size_t>((size_t)n / 8, 16);
  std::vector<std::string> toks;
  std::set<std::string> too_dear;  // candidates turned down
  std::vector<uint8_t> covered;
  for (int round = 0; round < max_tokens && cell_budget; ++round) {
    std::unordered_map<std::string, uint64_t> score;
    for (const auto& [sp, w] : chains) {
      // the chain as the packer would read it: at each symbol the longest
      // picked token that matches, else the symbol itself
      covered.assign(sp.size(), 0);
      for (size_t i = 0; i < sp.size();) {
        size_t best = 0;
        for (const std::string& t : toks)
          if (t.size() > best && sp.compare(i, t.size(), t) == 0) best = t.size();
        if (best) std::fill(covered.begin() + i, covered.begin() + i + best, 1);
        i += best ? best : 1;
      }
      for (size_t i = 0; i < sp.size(); ++i) {
        if (covered[i]) continue;
        for (size_t len = 2; len <= (size_t)kTokenMaxLen && i + len <= sp.size() && !covered[i + len - 1]; ++len)
          score[sp.substr(i, len)] += (uint64_t)(len - 1) * w[i + len - 1];
      }
    }
    // best score first; ties: the longer, then the smaller spelling (no
    // iteration order in the result).  The best one the budget still takes.
    std::vector<std::pair<uint64_t, const std::string*>> cand;
    for (const auto& [sp, sc] : score)
      if (sc && !too_dear.count(sp)) cand.push_back({sc, &sp});
    std::sort(cand.begin(), cand.end(), [](const auto& a, const auto& b) {
      if (a.first != b.first) return a.first > b.first;
      if (a.second->size() != b.second->size()) return a.second->size() > b.second->size();
      return *a.second < *b.second;
    });
    const std::string* best = nullptr;
    for (const auto& c : cand) {
      const size_t cells = cells_of(*c.second);
      if (cells <= cell_budget && cells <= column_cap) {
        best = c.second;
        cell_budget -= cells;
        break;
      }
      too_dear.insert(*c.second);
    }
    if (!best) {
      if (column_cap == SIZE_MAX) break;
      column_cap = SIZE_MAX;
      too_dear.clear();
      --round;
      continue;
    }
    toks.push_back(*best);
  }
  for (const std::string& t : toks) picked.emplace_back(t.begin(), t.end());
  return picked;
}

}  // namespace cg
