// endpoint_map.h — the endpoint map, cilium_lxc (bpf/lib/maps.h, struct
// endpoint_key / endpoint_info bpf/lib/common.h:147-173; Go side
// pkg/maps/lxcmap/lxcmap.go): a local endpoint's address → {lxc_id, flags},
// and its device form, the exact tables of dev_types.h EpMapDev.
#pragma once

#include <array>
#include <map>
#include <memory>
#include <vector>

#include "dev_types.h"
#include "engine.h"
#include "ipcache.h"

namespace cg {

struct EndpointMapState {
  uint32_t max_entries = 65535;  // lxcmap.go:33 MaxEntries
  using Key = std::pair<uint8_t, std::array<uint8_t, 16>>;  // family, address (network order)
  std::map<Key, cg_endpoint_info> entries;
  bool dirty = true;

  // host copies of the device tables (also walked by cg_diag_l4_frames_eval_host)
  std::vector<uint32_t> ex4;
  std::vector<uint64_t> ex6;
  uint32_t ex4_mask = 0, ex6_mask = 0, ex4_probes = 0, ex6_probes = 0;
  std::shared_ptr<DevTables> tab;  // the published device tables (engine.h)
  EpMapDev dev{};                  // view of tab; copy it together with tab

  void build_tables() {
    std::vector<std::pair<uint32_t, uint64_t>> x4;
    std::vector<std::pair<std::pair<uint64_t, uint64_t>, uint64_t>> x6;
    for (const auto& [k, v] : entries) {
      const uint64_t e = (uint64_t)v.flags << 32 | v.lxc_id;
      const auto& a = k.second;
      if (k.first == 4) {
        x4.emplace_back((uint32_t)a[0] << 24 | a[1] << 16 | a[2] << 8 | a[3], e);
      } else {
        uint64_t hi = 0, lo = 0;
        for (int i = 0; i < 8; ++i) hi = hi << 8 | a[i];
        for (int i = 8; i < 16; ++i) lo = lo << 8 | a[i];
        x6.push_back({{hi, lo}, e});
      }
    }
    build_exact4(x4, &ex4, &ex4_mask, &ex4_probes);
    build_exact6(x6, &ex6, &ex6_mask, &ex6_probes);
  }
  template <class Ptr>
  EpMapDev view(Ptr ptr) const {
    EpMapDev d{};
    d.ex4 = ptr(ex4);
    d.ex6 = ptr(ex6);
    d.ex4_mask = ex4_mask;
    d.ex6_mask = ex6_mask;
    d.ex4_probes = ex4_probes;
    d.ex6_probes = ex6_probes;
    return d;
  }
  EpMapDev host_view() const { return view(HostPtr{}); }
  void rebuild(Engine& e) {
    build_tables();
    if (e.has_gpu()) {
      e.set_device();
      auto t = std::make_shared<DevTables>();
      const EpMapDev d = view([&](const auto& v) { return t->add(v); });
      tab = std::move(t);  // publish (the caller holds the handle lock)
      dev = d;
    }
    dirty = false;
  }
};

}  // namespace cg
