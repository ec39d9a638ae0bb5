// selcache.h — the selector cache: the identity cache and a rule set's
// selectors compiled to interned-id tables (dev_types.h Sc*), so that
// "which identities does this selector select" (getSecurityIdentities,
// pkg/endpoint/policy.go:93-106) and "which identities may this endpoint
// reach at L3" (computeDesiredL3PolicyMapEntries, :298-371) are bitset
// kernels (kernels_selcache.hip) instead of per-identity label walks.
#pragma once

#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "dev_types.h"
#include "engine.h"

namespace cg {

// The identity cache, compiled: CSR label records in the given order and the
// string → id dictionary that selectors are interned against.
struct ScIdentSnap {
  std::vector<uint32_t> ids;
  std::vector<uint32_t> lab_off{0};
  std::vector<ScLabel> labels;
  std::unordered_map<std::string, uint32_t> dict;  // ids from 1; "any" is kScAny and not stored
  uint32_t n = 0;
};

// The prefix section: identities that are a CIDR prefix, as 24-byte records
// in the given order (cg_selcache_set_cidr_identities); their bits follow the
// label identities'.
struct ScCidrSnap {
  std::vector<uint32_t> ids;
  std::vector<ScCidr> recs;
};

// Selectors as given (strings), kept so they can be interned again when the
// identity cache — and with it the dictionary — is replaced.
struct ScSelSrc {
  struct Req {
    std::string key, src;  // "source:key" split; src "any" when there is no colon
    uint8_t op;
    std::vector<std::string> vals;
  };
  std::vector<Req> reqs;
  bool always = false;  // the empty selector, or matchLabels holds reserved:all
};

struct ScSelTab {
  std::vector<ScSel> sels;
  std::vector<ScReq> reqs;
  std::vector<uint32_t> vals;
  std::vector<ScReqCidr> creqs;  // parallel to reqs: what each requirement selects in a prefix identity
  ScSelDev view() const { return {sels.data(), reqs.data(), vals.data(), (uint32_t)sels.size(), creqs.data()}; }
};

struct ScRuleSrc {
  std::vector<ScSelSrc> sels;
  std::vector<uint32_t> subject;
  std::vector<uint8_t> flags;
  std::vector<uint32_t> req_off[2], req_idx[2], allow_off[2], allow_idx[2];
  uint32_t n = 0;
};

// Validating compilers of the C ABI's arguments (fail with CG_INVALID_ARGUMENT
// on malformed offsets or indices, CG_POLICY_REJECTED on an unknown operator).
std::shared_ptr<const ScIdentSnap> sc_compile_identities(const uint32_t* ids, size_t n, const uint32_t* label_off,
                                                         const uint8_t* key_blob, const uint64_t* key_off,
                                                         const uint8_t* val_blob, const uint64_t* val_off);
// Validates family and prefix length (CG_INVALID_ARGUMENT) and masks the
// address bits below the prefix.
std::shared_ptr<const ScCidrSnap> sc_compile_cidrs(const uint32_t* ids, const cg_cidr* prefixes, size_t n);
// What a requirement on `src:key` with `vals` selects in a prefix identity:
// the key must be the exact image of a prefix under the label format
// (maskedIPToLabelString, pkg/labels/cidr.go:23-45) — inverted, re-serialised
// as Go's net.IP.String() prints it and compared as strings — or `world`.
ScReqCidr sc_classify_req(const std::string& src, const std::string& key, const std::vector<std::string>& vals);
// The key part of the label cidr:<P>/<m> of a (masked) prefix record.
std::string sc_cidr_label_key(const ScCidr& p);
std::vector<ScSelSrc> sc_parse_selectors(const cg_selector_table& t);
std::shared_ptr<const ScRuleSrc> sc_parse_rules(const cg_selector_table& sels, const cg_selcache_rules& rules);
// Interns against the identities' dictionary; a string no identity carries
// gets an id past the dictionary's.  Each requirement is also classified for
// the prefix section (sc_classify_req).
ScSelTab sc_compile_selectors(const ScIdentSnap& idents, const std::vector<ScSelSrc>& sels);

// Host walkers over the compiled tables (cg_diag_selcache_*): what the
// kernels compute, on `threads` CPU threads.
void sc_match_host(const ScIdentDev& I, const ScSelDev& T, uint64_t* bits, uint32_t threads);
void sc_reach_host(const ScRuleDev& R, uint32_t n_ids, uint32_t words, const uint32_t* eps, size_t n, uint64_t* ing,
                   uint64_t* eg, uint8_t* flags, uint32_t threads);

// A cg_expand_table compiled to device records (dev_types.h ScExpRow).
struct ScExpTab {
  std::vector<ScExpRow> rows;
  std::vector<uint32_t> src_idx;
};
// Validates offsets and that every source index is < src_rows
// (CG_INVALID_ARGUMENT otherwise).
ScExpTab sc_compile_expand(const cg_expand_table& t, size_t src_rows);
// What the three expansion kernels compute: row_off[R + 1], *total, and —
// unless *total > cap — keys[*total] / proxy[*total], rows on `threads` threads.
void sc_expand_host(const ScExpDev& X, uint64_t* row_off, cg_policy_key* keys, uint16_t* proxy, uint64_t cap,
                    uint64_t* total, uint32_t threads);

// One published build: the host tables and, on a GPU handle, their device
// copies with the rule selectors' match matrix M already computed.
struct ScPublished {
  std::shared_ptr<const ScIdentSnap> idents;
  std::shared_ptr<const ScCidrSnap> cidrs;
  std::shared_ptr<const ScRuleSrc> rules;
  std::vector<uint32_t> ids;      // both sections' identity numbers, in bit order
  uint32_t n = 0, words = 0;      // identities of both sections; ceil(n / 64)
  ScIdentDev host_idents() const {
    return {idents->lab_off.data(), idents->labels.data(), idents->n, words, cidrs->recs.data(),
            (uint32_t)cidrs->recs.size()};
  }
  ScSelTab seltab;                // rules->sels interned against idents
  std::vector<uint64_t> host_m;   // M on the host, filled by the first diag reach
  std::shared_ptr<DevTables> tab; // device copies (engine.h)
  ScIdentDev dI{};
  ScSelDev dT{};
  ScRuleDev dR{};
  const uint32_t* d_ids = nullptr;  // ids on the device: what expansion writes as sec_label
  ScRuleDev host_rules() const;   // over host_m
};

struct SelcacheState {
  std::shared_ptr<const ScIdentSnap> idents = std::make_shared<ScIdentSnap>();
  std::shared_ptr<const ScCidrSnap> cidrs = std::make_shared<ScCidrSnap>();
  std::shared_ptr<const ScRuleSrc> rules = std::make_shared<ScRuleSrc>();
  bool dirty = true;
  std::shared_ptr<ScPublished> pub;
  void rebuild(Engine& e);
};

}  // namespace cg
