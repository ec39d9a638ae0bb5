// kafka_walk.h — kafkaRedirect.canAccess → RequestMessage.MatchesRule
// (pkg/proxy/kafka.go:117-153, pkg/kafka/policy.go:144-225) for one request
// over the tables of dev_types.h.  kafka_kernel (kernels.hip) issues its loads
// phase by phase for several requests of a lane; these are the decisions
// between the loads and the slow walk, taking what a phase loaded, so
// kafka_eval_host loads the same words through host_view() and calls them in
// the same order.  No counters here.
#pragma once

#include "dev_types.h"

namespace cg {

// isTopicAPIKey (pkg/kafka/policy.go:27-52) as a bitmask over 0..37
constexpr unsigned long long kKfTopicKeys =
    (1ULL << 0) | (1ULL << 1) | (1ULL << 2) | (1ULL << 3) | (1ULL << 4) | (1ULL << 5) | (1ULL << 6) | (1ULL << 8) |
    (1ULL << 9) | (1ULL << 19) | (1ULL << 20) | (1ULL << 21) | (1ULL << 23) | (1ULL << 24) | (1ULL << 27) |
    (1ULL << 28) | (1ULL << 34) | (1ULL << 35) | (1ULL << 37);
CG_HDI bool kf_is_topic_key(int k) { return k >= 0 && k < 64 && ((kKfTopicKeys >> k) & 1); }

// A request's class by the kind of request ReadRequest produced (the
// ruleMatches switch): 0 typed, 1 consumer-metadata, 2 nil.
CG_HDI uint32_t kf_class(uint32_t kind) {
  return kind == CG_KAFKA_K_TYPED ? 0 : kind == CG_KAFKA_K_CONSUMER_METADATA ? 1 : 2;
}
// Its apiKey bucket: the key for 0..63, 64 for any other.
CG_HDI uint32_t kf_bucket(int key) { return (key >= 0 && key < 64) ? (uint32_t)key : 64u; }
// Its summary: group g, context (nt topics: with / without), apiKey bucket.
CG_HDI uint32_t kf_sum_index(uint32_t g, uint32_t nt, int key) {
  return g * kKfSumsPerGroup + (nt == 0 ? kKfBuckets : 0) + kf_bucket(key);
}

// The verdict the summary settles with two bit tests: any = its `any` word,
// vm = its version mask of class c.
CG_HDI uint32_t kf_fast(uint32_t any, unsigned long long vm, uint32_t c, int ver) {
  return ((any >> c) & 1) | ((ver >= 0 && ver < 64) ? (uint32_t)((vm >> ver) & 1) : 0u);
}
// Whether a request kf_fast did not allow has anything left to try: clientID
// rules (typed requests), exception rules, topics.  tail = {any, x_off, x_cnt, pad}.
CG_HDI bool kf_needs_slow(uint4 tail, uint32_t c, uint32_t nt) {
  return (c == 0 && (tail.x & kKfSumHasClients)) || tail.z != 0 || nt != 0;
}

// The group of (redirect, identity): dflt, the redirect's group for unlisted
// identities, unless the identity has a slot.  e = the first probed slot, at
// hh = kf_hash(red << 32 | ident) & ghash_mask.
CG_HDI uint32_t kf_group(const KafkaDev& T, uint32_t dflt, uint4 e, uint32_t hh, uint32_t ident, uint32_t red) {
  if (ident == 0) return dflt;
  if (e.x == ident && e.y == red) return e.z;
  if (e.x == ~0u && e.y == ~0u) return dflt;
  // collision: linear probing from the next slot (a separate loop, so the
  // first probe's registers are not turned into a pointer phi)
  uint32_t slot = hh;
  for (uint32_t probe = 1; probe <= T.ghash_mask; ++probe) {
    slot = (slot + 1) & T.ghash_mask;
    const uint4 x = load16(T.ghash + slot);
    if (x.x == ident && x.y == red) return x.z;
    if (x.x == ~0u && x.y == ~0u) break;
  }
  return dflt;
}

// ruleMatches, pkg/kafka/policy.go:144-195
CG_HDI bool kf_rule_matches(const KafkaRuleDev& r, int key, int ver, uint32_t kind, uint32_t client) {
  if (!(r.flags & kKfKeyWild)) {
    if (key < 0 || key >= 64 || !((r.keys >> key) & 1)) return false;
  }
  if (!(r.flags & kKfVerWild) && r.version != ver) return false;
  const bool has_client = r.flags & kKfHasClient;
  const bool has_topic = r.flags & kKfHasTopic;
  if (!has_topic && !has_client) return true;
  if (kind == CG_KAFKA_K_TYPED) return !has_client || r.client_id == client;
  if (kind == CG_KAFKA_K_CONSUMER_METADATA) return true;
  return !(has_topic && kf_is_topic_key(key));  // matchNonTopicRequests
}

// Slow part of one request: clientID table (typed requests against clientID
// rules), exception rules, then per topic the (group, topic) rule list.
// tids = the record's 12 topic words; si, tail, c as above.
CG_HDI uint32_t kf_slow(const KafkaDev& T, const uint32_t* tids, const uint32_t* __restrict__ arena, uint32_t g,
                        uint32_t si, uint4 tail, int key, int ver, uint32_t kind, uint32_t c, uint32_t nt,
                        uint32_t client) {
  const bool vin = ver >= 0 && ver < 64;
  if (c == 0 && (tail.x & kKfSumHasClients)) {
    const unsigned long long k = ((unsigned long long)si << 32) | client;
    uint32_t hh = kf_hash(k) & T.chash_mask;
    for (uint32_t probe = 0; probe <= T.chash_mask; ++probe) {
      const KafkaClientDev* e = T.chash + hh;
      const uint4 a = load16(e);
      const unsigned long long kk = (unsigned long long)a.x | ((unsigned long long)a.y << 32);
      if (kk == k) {
        const unsigned long long cvm = (unsigned long long)a.z | ((unsigned long long)a.w << 32);
        if (e->any != 0 || (vin && ((cvm >> ver) & 1))) return 1;
        break;
      }
      if (kk == ~0ULL) break;
      hh = (hh + 1) & T.chash_mask;
    }
  }
  for (uint32_t j = 0; j < tail.z; ++j)
    if (kf_rule_matches(T.rules[tail.y + j], key, ver, kind, client)) return 1;
  if (nt == 0) return 0;
  // topic ids re-read from the record, or its topic tail (cached)
  const uint32_t* tsrc = nt > CG_KAFKA_MAX_TOPICS ? arena + tids[0] : tids;
  if (nt == CG_KAFKA_TOPICS_IN_ARENA) nt = tids[1];
  for (uint32_t t = 0; t < nt; ++t) {
    const unsigned long long k = ((unsigned long long)g << 32) | tsrc[t];
    uint32_t hh = kf_hash(k) & T.thash_mask;
    bool cov = false;
    for (uint32_t probe = 0; probe <= T.thash_mask; ++probe) {
      const KafkaTopicDev e = T.thash[hh];
      if (e.key == k) {
        for (uint32_t j = 0; j < e.cnt && !cov; ++j)
          cov = kf_rule_matches(T.rules[e.off + j], key, ver, kind, client);
        break;
      }
      if (e.key == ~0ULL) break;
      hh = (hh + 1) & T.thash_mask;
    }
    if (!cov) return 0;
  }
  return 1;
}

}  // namespace cg
