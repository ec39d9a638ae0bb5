// clsdfa.h — byte-class-compressed DFA with per-state accept labels, and its
// Hopcroft minimization.  Used for the per-program union automata.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace cg {

struct ClsDfa {
  int ncls = 1;
  uint8_t clsmap[256] = {0};
  std::vector<int32_t> trans;   // size() * ncls; state 0 = dead, 1 = start
  std::vector<uint32_t> label;  // 0 = non-accepting, else an accept-set id
  int size() const { return (int)label.size(); }
  int next(int s, uint8_t b) const { return trans[(size_t)s * ncls + clsmap[b]]; }
};

// Hopcroft partition refinement (initial partition by label), quotient,
// canonical BFS renumbering from the start state (dead → 0, start → 1, then
// breadth-first in class order) and re-compression of byte classes.
ClsDfa minimize_cls(const ClsDfa& d);

// Literal tokens.  A token is a sequence of 2..kTokenMaxLen byte classes that
// gets a class column of its own: δ(S, tok) = δ*(S, classes of tok) for every
// state S, so a string walks to the same state whichever of its literals are
// written as one token symbol.  No byte maps to a token column (clsmap stays
// byte → class); only a packer that knows the sequences emits them.
constexpr int kTokenMaxLen = 16;
using ClsSeq = std::vector<uint8_t>;

// δ*(s, seq), seq in classes of d.  An accepting state absorbs, as it does in
// the comb tables (comb.h).
int run_classes(const ClsDfa& d, int s, const uint8_t* seq, size_t n);

// Up to `max_tokens` sequences, best first, chosen from the literals the DFA
// spells: its forced chains (runs of states that are dead but for one class),
// each entered over a live edge of a branching state, and every sub-sequence
// of them.  A candidate scores (length - 1) x the rule tags still reachable
// behind it (label_masks[label - 1], bit = tag), summed over the chains that
// spell it; after each pick the chains are re-read with the picked tokens
// taken out (greedy, longest first, as the packer reads a string).  A
// token's column costs a cell in every row it moves off the row's default, so
// one that holds a field separator costs every self-looping row a cell.  A
// candidate that would take more cells than `cell_budget` has left is passed
// over for good (its sub-sequences stay candidates), and one that takes a
// cell in more than an eighth of the rows waits until no cheaper one is left.
std::vector<ClsSeq> pick_tokens(const ClsDfa& d, const std::vector<std::vector<uint64_t>>& label_masks,
                                int max_tokens, size_t cell_budget);

// `d` widened by one column per token (column d.ncls + i for toks[i]).
ClsDfa with_token_columns(const ClsDfa& d, const std::vector<ClsSeq>& toks);

}  // namespace cg
