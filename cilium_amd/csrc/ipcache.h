// ipcache.h — the IP → security-identity map (cilium_ipcache,
// bpf/lib/maps.h:135-159; Go side pkg/maps/ipcache/ipcache.go:36-130) and its
// device longest-prefix structures (dev_types.h IpcacheDev).
#pragma once

#include <algorithm>
#include <map>
#include <memory>
#include <vector>

#include "dev_types.h"
#include "engine.h"
#include "lpm.h"

namespace cg {

// The exact tables of dev_types.h (ex4_find / ex6_find) from {address, entry}
// pairs, for the ipcache's full-length prefixes and the endpoint map: open
// addressing at load <= 1/4 (a lookup's first slot is nearly always the
// answer or empty), linear probing; the longest probe sequence bounds every
// lookup.  v4 addresses in host order, v6 as (high word, low word).
inline void build_exact4(const std::vector<std::pair<uint32_t, uint64_t>>& x4, std::vector<uint32_t>* tab,
                         uint32_t* mask, uint32_t* probes) {
  uint32_t cap = 16;
  while (cap < 4 * x4.size()) cap <<= 1;
  tab->assign(4 * (size_t)cap, 0);
  *mask = cap - 1;
  *probes = 0;
  for (const auto& [a, e] : x4) {
    uint32_t p = 0;
    while ((*tab)[4 * (size_t)((ipc_ex4_hash(a) + p) & *mask) + 1]) ++p;
    uint32_t* sl = &(*tab)[4 * (size_t)((ipc_ex4_hash(a) + p) & *mask)];
    sl[0] = a;
    sl[1] = 1;
    sl[2] = (uint32_t)e;
    sl[3] = (uint32_t)(e >> 32);
    *probes = std::max(*probes, p);
  }
}
inline void build_exact6(const std::vector<std::pair<std::pair<uint64_t, uint64_t>, uint64_t>>& x6,
                         std::vector<uint64_t>* tab, uint32_t* mask, uint32_t* probes) {
  uint32_t cap = 16;
  while (cap < 4 * x6.size()) cap <<= 1;
  tab->assign(4 * (size_t)cap, 0);
  *mask = cap - 1;
  *probes = 0;
  for (const auto& [k, e] : x6) {
    const uint32_t h = ipc_ex6_hash(k.first, k.second);
    uint32_t p = 0;
    while ((*tab)[4 * (size_t)((h + p) & *mask) + 3]) ++p;
    uint64_t* sl = &(*tab)[4 * (size_t)((h + p) & *mask)];
    sl[0] = k.first;
    sl[1] = k.second;
    sl[2] = e;
    sl[3] = 1;
    *probes = std::max(*probes, p);
  }
}

struct IpcacheState {
  uint32_t max_entries = 512000;  // ipcache.go:36 MaxEntries, node_config.h:61
  // key {family, prefixlen, masked address} → RemoteEndpointInfo {sec_label, tunnel_endpoint}
  std::map<CidrKey, IpcVal> entries;
  bool dirty = true;

  // host copies of the device tables (also walked by cg_diag_ipcache_eval_host)
  std::vector<uint64_t> l16, chunks, runs6, code6;  // l16: the /16 level while building
  std::vector<uint32_t> l16x, ent6;
  std::vector<uint8_t> crowd6;
  std::vector<uint32_t> ex4;  // exact /32 slots (dev_types.h IpcacheDev)
  std::vector<uint64_t> ex6;  // exact /128 slots
  uint32_t ex4_mask = 0, ex6_mask = 0, ex4_probes = 0, ex6_probes = 0;
  uint32_t v6_bits = 16;
  std::shared_ptr<DevTables> tab;  // the published device tables (engine.h)
  IpcacheDev dev{};                // view of tab; copy it together with tab

  void build_tables();
  // The kernels' view (ptr as in PolicyMapState::view).
  template <class Ptr>
  IpcacheDev view(Ptr ptr) const {
    IpcacheDev d{};
    d.l16x = ptr(l16x);
    d.chunks = ptr(chunks);
    d.code6 = ptr(code6);
    d.ent6 = ptr(ent6);
    d.crowd6 = ptr(crowd6);
    d.runs6 = ptr(runs6);
    d.v6_bits = v6_bits;
    d.nruns6 = (uint32_t)(runs6.size() / 4);
    d.ex4 = ptr(ex4);
    d.ex6 = ptr(ex6);
    d.ex4_mask = ex4_mask;
    d.ex6_mask = ex6_mask;
    d.ex4_probes = ex4_probes;
    d.ex6_probes = ex6_probes;
    return d;
  }
  IpcacheDev host_view() const { return view(HostPtr{}); }
  void rebuild(Engine& e);
};

}  // namespace cg
