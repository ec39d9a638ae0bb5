// l4_array.h — the policy program array: cilium_policy[lxc_id] → one
// endpoint's policy map (bpf/lib/maps.h:44-62, tail-called at l3.h:99,130).
#pragma once

#include <map>
#include <memory>
#include <vector>

#include "dev_types.h"
#include "engine.h"

namespace cg {

// One published upload of an array: the slot words and the members' L4Dev
// records (own), and the members' table sets those records point into.  A
// launch holds the whole thing and records own.fence; members is declared
// first, so it is released last — after own's fence has waited for every
// queued kernel that reads the records, the members' tables or their counters.
struct L4ArrTables {
  std::vector<std::shared_ptr<DevTables>> members;  // in refs order
  DevTables own;
};

struct PolicyArrayState {
  std::vector<uint32_t> slot_map = std::vector<uint32_t>(CG_POLICY_ARRAY_SLOTS, 0u);  // map id, 0 = empty
  std::map<uint32_t, uint32_t> refs;  // member map id -> slots that name it
  bool slots_changed = true;          // a slot changed since the last upload

  std::shared_ptr<L4ArrTables> tab;  // the published upload
  L4ArrDev dev{};                    // view of tab; copy it together with tab

  // Endpoint program headers (cg_endpoint_header), independent of the slots'
  // maps.  Their upload is a table set of its own, built when an egress call
  // first asks for it and after every change, under the same hold of the
  // handle lock that takes the array's snapshot; a launch holds both.
  std::map<uint16_t, cg_endpoint_header> headers;
  bool headers_changed = true;
  std::shared_ptr<DevTables> hdr_tab;
  EpHdrDev hdr_dev{};

  // The headers as the egress kernel reads them (dev_types.h EpHdrDev).
  void header_tables(std::vector<uint32_t>* idx, std::vector<uint4>* recs) const {
    idx->assign(CG_POLICY_ARRAY_SLOTS, 0u);
    recs->clear();
    for (const auto& kv : headers) {
      (*idx)[kv.first] = (uint32_t)(recs->size() / 4) + 1;
      uint4 w[4];
      memcpy(w, &kv.second, sizeof(w));
      recs->insert(recs->end(), w, w + 4);
    }
    if (recs->empty()) recs->resize(4);  // never read: every index word is 0
  }

  void put(uint32_t lxc_id, uint32_t map_id) {  // map_id 0 empties the slot
    uint32_t& s = slot_map[lxc_id];
    if (s == map_id) return;
    if (s) {
      auto it = refs.find(s);
      if (--it->second == 0) refs.erase(it);
    }
    if (map_id) ++refs[map_id];
    s = map_id;
    slots_changed = true;
  }
  void drop_map(uint32_t map_id) {  // the map is being destroyed
    auto it = refs.find(map_id);
    if (it == refs.end()) return;
    for (uint32_t& s : slot_map)
      if (s == map_id) s = 0;
    refs.erase(it);
    slots_changed = true;
  }
};

}  // namespace cg
