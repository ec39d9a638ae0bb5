// capi.cc — the extern "C" boundary (include/cilium_gpu.h).  Every entry
// point catches internal errors and returns a cg_result code.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <exception>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "ct_map.h"
#include "endpoint_map.h"
#include "engine.h"
#include "frame_progs.h"
#include "frame_walk.h"
#include "http.h"
#include "kafka.h"
#include "kafka_wire.h"
#include "kernels.h"
#include "l4.h"
#include "l4_array.h"
#include "l4_walk.h"
#include "lb_map.h"
#include "ipcache.h"
#include "lpm.h"
#include "lpm_walk.h"
#include "regex.h"
#include "ring.h"
#include "selcache.h"

using namespace cg;

namespace {

std::mutex g_handles_mu;
std::map<uint64_t, std::shared_ptr<Engine>> g_handles;
uint64_t g_next_handle = 1;
// Bumped (after the change is published) by everything that changes what a
// ring call resolves to: cg_close, ring open / close, an HTTP policy publish.
// cg_http_ring_verdicts keeps its handle, ring and snapshot per calling thread
// while this is unchanged, so Envoy's workers take no lock and touch no
// shared reference count per request.
std::atomic<uint64_t> g_epoch{1};
void bump_epoch() { g_epoch.fetch_add(1, std::memory_order_acq_rel); }

std::shared_ptr<Engine> get(uint64_t h) {
  std::lock_guard<std::mutex> lk(g_handles_mu);
  auto it = g_handles.find(h);
  if (it == g_handles.end()) fail(CG_INVALID_INSTANCE, "unknown handle");
  return it->second;
}

template <class F>
int guarded(F&& f) {
  try {
    f();
    return CG_OK;
  } catch (const Error& e) {
    set_error(e.msg);
    return e.code;
  } catch (const std::bad_alloc&) {
    set_error("out of host memory");
    return CG_UNKNOWN_ERROR;
  } catch (const std::exception& e) {
    set_error(e.what());
    return CG_UNKNOWN_ERROR;
  } catch (...) {
    set_error("unknown error");
    return CG_UNKNOWN_ERROR;
  }
}

PolicyMapState& get_map(Engine& e, uint32_t id) {
  auto it = e.maps.find(id);
  if (it == e.maps.end()) fail(CG_NOT_FOUND, "unknown policy map id");
  return *it->second;
}

PolicyArrayState& get_arr(Engine& e, uint32_t id) {
  auto it = e.arrays.find(id);
  if (it == e.arrays.end()) fail(CG_NOT_FOUND, "unknown policy array id");
  return *it->second;
}

EndpointMapState& get_ep(Engine& e, uint32_t id) {
  auto it = e.epmaps.find(id);
  if (it == e.epmaps.end()) fail(CG_NOT_FOUND, "unknown endpoint map id");
  return *it->second;
}

CtMapState& get_ct(Engine& e, uint32_t id) {
  auto it = e.ctmaps.find(id);
  if (it == e.ctmaps.end()) fail(CG_NOT_FOUND, "unknown conntrack map id");
  return *it->second;
}

LbMapState& get_lb(Engine& e, uint32_t id) {
  auto it = e.lbmaps.find(id);
  if (it == e.lbmaps.end()) fail(CG_NOT_FOUND, "unknown service map id");
  return *it->second;
}

IpcacheState& get_ipc(Engine& e, uint32_t id) {
  auto it = e.ipcaches.find(id);
  if (it == e.ipcaches.end()) fail(CG_NOT_FOUND, "unknown ipcache id");
  return *it->second;
}

SelcacheState& get_sc(Engine& e, uint32_t id) {
  auto it = e.selcaches.find(id);
  if (it == e.selcaches.end()) fail(CG_NOT_FOUND, "unknown selector cache id");
  return *it->second;
}

PrefilterState& get_pf(Engine& e, uint32_t id) {
  auto it = e.prefilters.find(id);
  if (it == e.prefilters.end()) fail(CG_NOT_FOUND, "unknown prefilter id");
  return *it->second;
}

void* stream_of(Engine& e, void* s) { return s ? s : e.stream; }

void check_launch(int err, const char* what) { hip_check(err, what); }

// A queued launch on `stream` reads this table set: record it on the set's
// retirement fence (engine.h LaunchFence).
void fence(const std::shared_ptr<DevTables>& t, void* stream) {
  if (t) t->fence.record(stream);
}

CidrKey make_cidr(const cg_cidr& c) {
  CidrKey k;
  if (c.family != 4 && c.family != 6) fail(CG_INVALID_ADDRESS, "cidr family must be 4 or 6");
  int bits = c.family == 4 ? 32 : 128;
  if (c.prefixlen > bits) fail(CG_INVALID_ADDRESS, "prefix length out of range");
  k.family = c.family;
  k.plen = c.prefixlen;
  k.net.fill(0);
  int bytes = bits / 8;
  for (int i = 0; i < bytes; ++i) {
    int keep = std::max(0, std::min(8, (int)c.prefixlen - 8 * i));
    uint8_t mask = keep == 0 ? 0 : (uint8_t)(0xFF << (8 - keep));
    k.net[i] = c.addr[i] & mask;  // net.ParseCIDR returns the masked network
  }
  return k;
}

// selectMap (prefilter.go:108-122)
int select_map(const CidrKey& k) {
  if (k.family == 4) return k.plen == 32 ? 1 : 0;
  return k.plen == 128 ? 3 : 2;
}

}  // namespace

extern "C" {

const char* cg_last_error(void) { return get_error().c_str(); }

const char* cg_version(void) { return "libciliumgpu gfx950 r1"; }

uint64_t cg_open(const cg_kv* params, size_t n, uint8_t debug) {
  uint64_t out = 0;
  int rc = guarded([&] {
    auto e = std::make_shared<Engine>();
    e->debug = debug;
    int dev = 0;
    for (size_t i = 0; i < n; ++i)
      if (params[i].key && params[i].value && strcmp(params[i].key, "device") == 0) dev = atoi(params[i].value);
    e->device = dev;
    if (dev >= 0) {
      int count = 0;
      if (hipGetDeviceCount(&count) != hipSuccess || dev >= count)
        fail(CG_NO_DEVICE, "no HIP device " + std::to_string(dev));
      hipDeviceProp_t prop;
      hip_check(hipGetDeviceProperties(&prop, dev), "hipGetDeviceProperties");
      if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        fail(CG_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
      e->cus = prop.multiProcessorCount;
      hip_check(hipSetDevice(dev), "hipSetDevice");
      hipStream_t s;
      hip_check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
      e->stream = s;
    }
    std::lock_guard<std::mutex> lk(g_handles_mu);
    out = g_next_handle++;
    g_handles[out] = e;
  });
  return rc == CG_OK ? out : 0;
}

void cg_close(uint64_t h) {
  std::shared_ptr<Engine> e;
  {
    std::lock_guard<std::mutex> lk(g_handles_mu);
    auto it = g_handles.find(h);
    if (it == g_handles.end()) return;
    e = it->second;
    g_handles.erase(it);
  }
  bump_epoch();
  if (e->has_gpu()) {
    (void)hipSetDevice(e->device);
    {
      std::shared_ptr<HttpRing> r;
      {
        std::lock_guard<std::mutex> lk(e->ring_mu);
        r = std::move(e->ring);
      }
      if (r) r->close();
    }
    (void)hipStreamSynchronize((hipStream_t)e->stream);
    e->arrays.clear();
    e->maps.clear();
    e->prefilters.clear();
    e->ipcaches.clear();
    e->epmaps.clear();
    e->ctmaps.clear();
    e->lbmaps.clear();
    e->selcaches.clear();
    e->http.reset();
    e->kafka.reset();
    (void)hipStreamDestroy((hipStream_t)e->stream);
  }
}

int cg_sync(uint64_t h) {
  return guarded([&] {
    auto e = get(h);
    if (e->has_gpu()) dev_sync(*e, nullptr);
  });
}

// ------------------------------------------------------------------ L4 ----
int cg_policymap_create(uint64_t h, uint32_t max_entries, uint32_t* map_id) {
  return guarded([&] {
    auto e = get(h);
    if (!map_id) fail(CG_INVALID_ARGUMENT, "map_id is NULL");
    if (max_entries == 0) max_entries = 16384;  // policymap.go:37 MaxEntries
    if (max_entries > 65536) fail(CG_INVALID_ARGUMENT, "max_entries > 65536");
    std::lock_guard<std::mutex> lk(e->mu);
    auto m = std::make_unique<PolicyMapState>();
    m->max_entries = max_entries;
    uint32_t id = e->next_id++;
    e->maps[id] = std::move(m);
    *map_id = id;
  });
}

int cg_policymap_destroy(uint64_t h, uint32_t map_id) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    get_map(*e, map_id);
    if (e->has_gpu()) dev_sync(*e, nullptr);
    e->maps.erase(map_id);
    for (auto& arr : e->arrays) arr.second->drop_map(map_id);  // its slots are empty from now on
  });
}

int cg_policymap_allow(uint64_t h, uint32_t map_id, const cg_policy_key* keys, const uint16_t* ports_be,
                       size_t n) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PolicyMapState& m = get_map(*e, map_id);
    if (n && (!keys || !ports_be)) fail(CG_INVALID_ARGUMENT, "NULL keys/ports");
    size_t fresh = 0;
    std::map<uint64_t, int> seen;
    for (size_t i = 0; i < n; ++i) {
      uint64_t k = l4_key(keys[i]);
      if (k == kL4EmptyKey) fail(CG_INVALID_ARGUMENT, "reserved all-ones policy key");
      if (!m.entries.count(k) && seen.emplace(k, 1).second) ++fresh;
    }
    if (m.entries.size() + fresh > m.max_entries) fail(CG_MAP_FULL, "policy map full (E2BIG)");
    for (size_t i = 0; i < n; ++i) {
      uint64_t k = l4_key(keys[i]);
      auto it = m.entries.find(k);
      if (it != m.entries.end()) {
        it->second.proxy_port_be = ports_be[i];
      } else {
        uint32_t id;
        if (!m.free_ids.empty()) {
          id = m.free_ids.back();
          m.free_ids.pop_back();
        } else {
          id = m.next_id++;
        }
        m.zero_counter(*e, id);
        m.entries[k] = {ports_be[i], id};
        m.order.push_back(k);
      }
    }
    m.dirty = true;
  });
}

int cg_policymap_delete(uint64_t h, uint32_t map_id, const cg_policy_key* keys, size_t n) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PolicyMapState& m = get_map(*e, map_id);
    for (size_t i = 0; i < n; ++i)
      if (!m.entries.count(l4_key(keys[i]))) fail(CG_NOT_FOUND, "policy key not found (ENOENT)");
    for (size_t i = 0; i < n; ++i) {
      uint64_t k = l4_key(keys[i]);
      auto it = m.entries.find(k);
      if (it == m.entries.end()) continue;  // duplicate in the batch
      m.free_ids.push_back(it->second.id);
      m.entries.erase(it);
      m.order.erase(std::find(m.order.begin(), m.order.end(), k));
    }
    m.dirty = true;
  });
}

int cg_policymap_lookup(uint64_t h, uint32_t map_id, const cg_policy_key* key, cg_policy_entry* entry) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PolicyMapState& m = get_map(*e, map_id);
    auto it = m.entries.find(l4_key(*key));
    if (it == m.entries.end()) fail(CG_NOT_FOUND, "policy key not found");
    if (entry) {
      memset(entry, 0, sizeof(*entry));
      entry->proxy_port = it->second.proxy_port_be;
      // counters include every verdict call queued on this device so far
      if (e->has_gpu()) {
        e->set_device();
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
      }
      m.read_counters(*e, it->second.id, &entry->packets, &entry->bytes);
    }
  });
}

int cg_policymap_dump(uint64_t h, uint32_t map_id, cg_policy_key* keys, cg_policy_entry* entries, size_t cap,
                      size_t* n) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PolicyMapState& m = get_map(*e, map_id);
    if (n) *n = m.order.size();
    std::vector<uint64_t> ctr;
    if (e->has_gpu() && m.d_counters) {
      e->set_device();
      hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
      ctr.resize((size_t)m.max_entries * 2);
      hip_check(hipMemcpy(ctr.data(), m.d_counters->get(), ctr.size() * 8, hipMemcpyDeviceToHost), "D2H counters");
    }
    size_t i = 0;
    for (uint64_t k : m.order) {
      if (i >= cap) break;
      if (keys) keys[i] = l4_unkey(k);
      if (entries) {
        memset(&entries[i], 0, sizeof(cg_policy_entry));
        const auto& en = m.entries[k];
        entries[i].proxy_port = en.proxy_port_be;
        if (!ctr.empty()) {
          entries[i].packets = ctr[(size_t)en.id * 2];
          entries[i].bytes = ctr[(size_t)en.id * 2 + 1];
        }
      }
      ++i;
    }
  });
}

int cg_policymap_flush(uint64_t h, uint32_t map_id) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PolicyMapState& m = get_map(*e, map_id);
    for (auto& [k, en] : m.entries) m.free_ids.push_back(en.id);
    m.entries.clear();
    m.order.clear();
    m.dirty = true;
  });
}

int cg_policymap_sync(uint64_t h, uint32_t map_id, const cg_policy_key* keys, const uint16_t* ports_be, size_t n,
                      size_t* added, size_t* deleted) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PolicyMapState& m = get_map(*e, map_id);
    if (n && (!keys || !ports_be)) fail(CG_INVALID_ARGUMENT, "NULL keys/ports");
    // the wanted state: distinct keys in first-appearance order, last value
    std::unordered_map<uint64_t, uint16_t> want;
    std::vector<uint64_t> seq;
    want.reserve(n);
    for (size_t i = 0; i < n; ++i) {
      const uint64_t k = l4_key(keys[i]);
      if (k == kL4EmptyKey) fail(CG_INVALID_ARGUMENT, "reserved all-ones policy key");
      auto [it, fresh] = want.emplace(k, ports_be[i]);
      if (fresh)
        seq.push_back(k);
      else
        it->second = ports_be[i];
    }
    if (want.size() > m.max_entries) fail(CG_MAP_FULL, "policy map full (E2BIG)");
    // nothing below fails: deletes first, so that their counter slots are free
    size_t n_del = 0, n_add = 0;
    std::vector<uint64_t> order;
    order.reserve(want.size());
    for (uint64_t k : m.order) {
      if (want.count(k)) {
        order.push_back(k);
        continue;
      }
      auto it = m.entries.find(k);
      m.free_ids.push_back(it->second.id);
      m.entries.erase(it);
      ++n_del;
    }
    std::vector<uint32_t> fresh_ids;
    for (uint64_t k : seq) {
      const uint16_t port = want[k];
      auto it = m.entries.find(k);
      if (it != m.entries.end()) {
        if (it->second.proxy_port_be != port) {
          it->second.proxy_port_be = port;
          ++n_add;
        }
        continue;
      }
      uint32_t id;
      if (!m.free_ids.empty()) {
        id = m.free_ids.back();
        m.free_ids.pop_back();
      } else {
        id = m.next_id++;
      }
      fresh_ids.push_back(id);
      m.entries[k] = {port, id};
      order.push_back(k);
      ++n_add;
    }
    m.order = std::move(order);
    if (n_add || n_del) m.dirty = true;
    if (added) *added = n_add;
    if (deleted) *deleted = n_del;
    // new keys count from zero: clear their slots, one memset per run of ids
    std::sort(fresh_ids.begin(), fresh_ids.end());
    for (size_t i = 0; i < fresh_ids.size();) {
      size_t j = i + 1;
      while (j < fresh_ids.size() && fresh_ids[j] == fresh_ids[j - 1] + 1) ++j;
      m.zero_counters(*e, fresh_ids[i], (uint32_t)(j - i));
      i = j;
    }
  });
}

// A map's published tables, copied under the handle lock and held while the
// launch is enqueued (engine.h DevTables).
struct L4View {
  std::shared_ptr<DevTables> keep;
  L4Dev dev;
};
static L4View l4_view(Engine& e, uint32_t map_id) {
  std::lock_guard<std::mutex> lk(e.mu);
  PolicyMapState& m = get_map(e, map_id);
  if (m.dirty) m.rebuild(e);
  return {m.tab, m.dev};
}
struct IpcView {
  std::shared_ptr<DevTables> keep;
  IpcacheDev dev;
};
static IpcView ipc_view(Engine& e, uint32_t ipc_id) {
  std::lock_guard<std::mutex> lk(e.mu);
  IpcacheState& p = get_ipc(e, ipc_id);
  if (p.dirty) p.rebuild(e);
  return {p.tab, p.dev};
}

static uint32_t check_l4_mode(uint32_t mode) {
  if ((mode & ~(3u | CG_L4_IGNORE_DROP)) || (mode & 3u) == 3u) fail(CG_INVALID_ARGUMENT, "unknown L4 verdict mode");
  return mode;
}

static void l4_dev(Engine& e, uint32_t map_id, uint32_t mode, const cg_l4_tuple* d_t, size_t n, int32_t* d_out,
                   void* s) {
  e.require_gpu();
  const L4View v = l4_view(e, map_id);
  e.set_device();
  check_launch(launch_l4(v.dev, d_t, n, d_out, mode, stream_of(e, s), e.cus), "l4 kernel launch");
  fence(v.keep, stream_of(e, s));
}

static void l4_host(Engine& e, uint32_t map_id, uint32_t mode, const cg_l4_tuple* t, size_t n, int32_t* out) {
  e.require_gpu();
  if (n && (!t || !out)) fail(CG_INVALID_ARGUMENT, "NULL tuples/verdicts");
  const L4View v = l4_view(e, map_id);
  host_pipeline(e, n, {{t, sizeof(cg_l4_tuple)}}, {{out, sizeof(int32_t)}},
                [&](void* const* din, void* const* dout, size_t cnt, void* st) {
                  check_launch(launch_l4(v.dev, din[0], cnt, (int32_t*)dout[0], mode, st, e.cus), "l4 kernel launch");
                });
}

int cg_l4_verdicts_dev(uint64_t h, uint32_t map_id, const cg_l4_tuple* d_tuples, size_t n, int32_t* d_verdicts,
                       void* stream) {
  return guarded([&] { l4_dev(*get(h), map_id, CG_L4_CAN_ACCESS, d_tuples, n, d_verdicts, stream); });
}

int cg_l4_verdicts_host(uint64_t h, uint32_t map_id, const cg_l4_tuple* tuples, size_t n, int32_t* verdicts) {
  return guarded([&] { l4_host(*get(h), map_id, CG_L4_CAN_ACCESS, tuples, n, verdicts); });
}

int cg_l4_policy_verdicts_dev(uint64_t h, uint32_t map_id, uint32_t mode, const cg_l4_tuple* d_tuples, size_t n,
                              int32_t* d_verdicts, void* stream) {
  return guarded([&] { l4_dev(*get(h), map_id, check_l4_mode(mode), d_tuples, n, d_verdicts, stream); });
}

int cg_l4_policy_verdicts_host(uint64_t h, uint32_t map_id, uint32_t mode, const cg_l4_tuple* tuples, size_t n,
                               int32_t* verdicts) {
  return guarded([&] { l4_host(*get(h), map_id, check_l4_mode(mode), tuples, n, verdicts); });
}

// The egress flow with identities from the ipcache (bpf_lxc.c:509-527 v4,
// :205-220 v6): policy_can_egress{4,6} semantics.
static void l4_ipc_dev(Engine& e, uint32_t map_id, uint32_t ipc_id, int family, const void* d_addr,
                       const cg_l4_tuple* d_t, size_t n, int32_t* d_out, void* s) {
  e.require_gpu();
  const L4View v = l4_view(e, map_id);
  const IpcView iv = ipc_view(e, ipc_id);
  e.set_device();
  check_launch(launch_l4_ipcache(v.dev, iv.dev, family, d_addr, d_t, n, d_out, CG_L4_EGRESS, stream_of(e, s), e.cus),
               "l4 (ipcache) kernel launch");
  fence(v.keep, stream_of(e, s));
  fence(iv.keep, stream_of(e, s));
}

static void l4_ipc_host(Engine& e, uint32_t map_id, uint32_t ipc_id, int family, const void* addr,
                        const cg_l4_tuple* t, size_t n, int32_t* out) {
  e.require_gpu();
  if (n && (!addr || !t || !out)) fail(CG_INVALID_ARGUMENT, "NULL addresses/tuples/verdicts");
  const L4View v = l4_view(e, map_id);
  const IpcView iv = ipc_view(e, ipc_id);
  host_pipeline(e, n, {{addr, family == 6 ? 16u : 4u}, {t, sizeof(cg_l4_tuple)}}, {{out, sizeof(int32_t)}},
                [&](void* const* din, void* const* dout, size_t cnt, void* st) {
                  check_launch(launch_l4_ipcache(v.dev, iv.dev, family, din[0], din[1], cnt, (int32_t*)dout[0],
                                                 CG_L4_EGRESS, st, e.cus),
                               "l4 (ipcache) kernel launch");
                });
}

int cg_l4_verdicts_ipcache_dev(uint64_t h, uint32_t map_id, uint32_t ipc_id, const uint32_t* d_remote_v4,
                               const cg_l4_tuple* d_tuples, size_t n, int32_t* d_verdicts, void* stream) {
  return guarded([&] { l4_ipc_dev(*get(h), map_id, ipc_id, 4, d_remote_v4, d_tuples, n, d_verdicts, stream); });
}

int cg_l4_verdicts_ipcache_host(uint64_t h, uint32_t map_id, uint32_t ipc_id, const uint32_t* remote_v4,
                                const cg_l4_tuple* tuples, size_t n, int32_t* verdicts) {
  return guarded([&] { l4_ipc_host(*get(h), map_id, ipc_id, 4, remote_v4, tuples, n, verdicts); });
}

int cg_l4_verdicts_ipcache6_dev(uint64_t h, uint32_t map_id, uint32_t ipc_id, const uint8_t* d_remote_v6,
                                const cg_l4_tuple* d_tuples, size_t n, int32_t* d_verdicts, void* stream) {
  return guarded([&] { l4_ipc_dev(*get(h), map_id, ipc_id, 6, d_remote_v6, d_tuples, n, d_verdicts, stream); });
}

int cg_l4_verdicts_ipcache6_host(uint64_t h, uint32_t map_id, uint32_t ipc_id, const uint8_t* remote_v6,
                                 const cg_l4_tuple* tuples, size_t n, int32_t* verdicts) {
  return guarded([&] { l4_ipc_host(*get(h), map_id, ipc_id, 6, remote_v6, tuples, n, verdicts); });
}

// ----------------------------------------------- policy program array ----
// cilium_policy[lxc_id] (bpf/lib/maps.h:44-62): slots naming policy maps, and
// verdict entries that take each tuple's lxc_id (l4_array.h, kernels_l4_array.hip).
int cg_policy_array_create(uint64_t h, uint32_t* arr_id) {
  return guarded([&] {
    auto e = get(h);
    if (!arr_id) fail(CG_INVALID_ARGUMENT, "arr_id is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    const uint32_t id = e->next_id++;
    e->arrays[id] = std::make_unique<PolicyArrayState>();
    *arr_id = id;
  });
}

int cg_policy_array_destroy(uint64_t h, uint32_t arr_id) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    get_arr(*e, arr_id);
    if (e->has_gpu()) dev_sync(*e, nullptr);
    e->arrays.erase(arr_id);
  });
}

int cg_policy_array_set(uint64_t h, uint32_t arr_id, const uint16_t* lxc_ids, const uint32_t* map_ids, size_t n) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PolicyArrayState& a = get_arr(*e, arr_id);
    if (n && (!lxc_ids || !map_ids)) fail(CG_INVALID_ARGUMENT, "NULL lxc_ids/map_ids");
    for (size_t i = 0; i < n; ++i) get_map(*e, map_ids[i]);  // all checked before any slot changes
    for (size_t i = 0; i < n; ++i) a.put(lxc_ids[i], map_ids[i]);
  });
}

int cg_policy_array_clear(uint64_t h, uint32_t arr_id, const uint16_t* lxc_ids, size_t n) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PolicyArrayState& a = get_arr(*e, arr_id);
    if (n && !lxc_ids) fail(CG_INVALID_ARGUMENT, "NULL lxc_ids");
    for (size_t i = 0; i < n; ++i) a.put(lxc_ids[i], 0);
  });
}

int cg_policy_array_get(uint64_t h, uint32_t arr_id, uint16_t lxc_id, uint32_t* map_id) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PolicyArrayState& a = get_arr(*e, arr_id);
    if (!map_id) fail(CG_INVALID_ARGUMENT, "map_id is NULL");
    *map_id = a.slot_map[lxc_id];
  });
}

// Endpoint program headers: the from-container program's compile-time
// constants per slot (l4_array.h), independent of the slots' maps.
int cg_policy_array_set_headers(uint64_t h, uint32_t arr_id, const uint16_t* lxc_ids,
                                const cg_endpoint_header* headers, size_t n) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PolicyArrayState& a = get_arr(*e, arr_id);
    if (n && (!lxc_ids || !headers)) fail(CG_INVALID_ARGUMENT, "NULL lxc_ids/headers");
    constexpr uint32_t known = CG_EPH_F_IPV4 | CG_EPH_F_NO_SMAC | CG_EPH_F_NO_DMAC | CG_EPH_F_NO_SIP;
    for (size_t i = 0; i < n; ++i) {  // all checked before any header changes
      if (headers[i].flags & ~known) fail(CG_INVALID_ARGUMENT, "unknown endpoint header flags");
      if (headers[i].pad[0] | headers[i].pad[1]) fail(CG_INVALID_ARGUMENT, "endpoint header pad must be 0");
    }
    for (size_t i = 0; i < n; ++i) a.headers[lxc_ids[i]] = headers[i];
    if (n) a.headers_changed = true;
  });
}

int cg_policy_array_clear_headers(uint64_t h, uint32_t arr_id, const uint16_t* lxc_ids, size_t n) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PolicyArrayState& a = get_arr(*e, arr_id);
    if (n && !lxc_ids) fail(CG_INVALID_ARGUMENT, "NULL lxc_ids");
    for (size_t i = 0; i < n; ++i) a.headers_changed |= a.headers.erase(lxc_ids[i]) != 0;
  });
}

int cg_policy_array_get_header(uint64_t h, uint32_t arr_id, uint16_t lxc_id, cg_endpoint_header* out) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PolicyArrayState& a = get_arr(*e, arr_id);
    if (!out) fail(CG_INVALID_ARGUMENT, "out is NULL");
    auto it = a.headers.find(lxc_id);
    if (it == a.headers.end()) fail(CG_NOT_FOUND, "policy array: the slot has no header");
    *out = it->second;
  });
}

// One snapshot of the whole array, taken under the handle lock: dirty members
// are rebuilt, and the slot words and records are uploaded again only if a
// slot or a member's published tables changed since the last upload.  The
// holder keeps every member's tables and counters alive (l4_array.h).
struct L4ArrView {
  std::shared_ptr<L4ArrTables> keep;
  L4ArrDev dev;
};
static L4ArrView l4_array_view_locked(Engine& e, uint32_t arr_id) {  // the caller holds e.mu
  PolicyArrayState& a = get_arr(e, arr_id);
  std::vector<std::shared_ptr<DevTables>> members;
  std::vector<L4Dev> recs;
  bool changed = a.slots_changed || !a.tab;
  for (const auto& ref : a.refs) {
    PolicyMapState& m = get_map(e, ref.first);  // a destroyed map has left refs (cg_policymap_destroy)
    if (m.dirty) m.rebuild(e);
    if (!changed && a.tab->members[members.size()] != m.tab) changed = true;
    members.push_back(m.tab);
    recs.push_back(m.dev);
  }
  if (changed) {
    std::map<uint32_t, uint32_t> word;  // map id -> 1 + record index
    for (const auto& ref : a.refs) word.emplace(ref.first, (uint32_t)word.size() + 1);
    std::vector<uint32_t> slot(CG_POLICY_ARRAY_SLOTS, 0u);
    for (uint32_t s = 0; s < CG_POLICY_ARRAY_SLOTS; ++s)
      if (a.slot_map[s]) slot[s] = word[a.slot_map[s]];
    if (recs.empty()) recs.push_back(L4Dev{});  // never read: every slot word is 0
    e.set_device();
    auto t = std::make_shared<L4ArrTables>();
    t->members = std::move(members);
    L4ArrDev d{};
    d.slot = t->own.add(slot);
    d.recs = t->own.add(recs);
    a.tab = std::move(t);  // publish
    a.dev = d;
    a.slots_changed = false;
  }
  return {a.tab, a.dev};
}
static L4ArrView l4_array_view(Engine& e, uint32_t arr_id) {
  std::lock_guard<std::mutex> lk(e.mu);
  return l4_array_view_locked(e, arr_id);
}

static void l4_array_dev(Engine& e, uint32_t arr_id, const IpcView* iv, uint32_t mode, int family, const void* d_addr,
                         const uint16_t* d_lxc, const cg_l4_tuple* d_t, size_t n, int32_t* d_out, void* s) {
  e.require_gpu();
  const L4ArrView v = l4_array_view(e, arr_id);
  e.set_device();
  check_launch(launch_l4_array(v.dev, iv ? iv->dev : IpcacheDev{}, family, d_addr, d_lxc, d_t, n, d_out, mode,
                               stream_of(e, s), e.cus),
               "l4 array kernel launch");
  v.keep->own.fence.record(stream_of(e, s));
  if (iv) fence(iv->keep, stream_of(e, s));
}

static void l4_array_host(Engine& e, uint32_t arr_id, const IpcView* iv, uint32_t mode, int family, const void* addr,
                          const uint16_t* lxc, const cg_l4_tuple* t, size_t n, int32_t* out) {
  e.require_gpu();
  if (n && (!lxc || !t || !out || (family && !addr))) fail(CG_INVALID_ARGUMENT, "NULL lxc_ids/tuples/verdicts");
  const L4ArrView v = l4_array_view(e, arr_id);
  std::vector<HostIn> ins = {{lxc, sizeof(uint16_t)}, {t, sizeof(cg_l4_tuple)}};
  if (family) ins.push_back({addr, family == 6 ? 16u : 4u});
  host_pipeline(e, n, ins, {{out, sizeof(int32_t)}}, [&](void* const* din, void* const* dout, size_t cnt, void* st) {
    check_launch(launch_l4_array(v.dev, iv ? iv->dev : IpcacheDev{}, family, family ? din[2] : nullptr,
                                 (const uint16_t*)din[0], din[1], cnt, (int32_t*)dout[0], mode, st, e.cus),
                 "l4 array kernel launch");
  });
}

static void check_family(int family) {
  if (family != 4 && family != 6) fail(CG_INVALID_ARGUMENT, "family must be 4 or 6");
}

int cg_l4_array_verdicts_dev(uint64_t h, uint32_t arr_id, uint32_t mode, const uint16_t* d_lxc_ids,
                             const cg_l4_tuple* d_tuples, size_t n, int32_t* d_verdicts, void* stream) {
  return guarded([&] {
    l4_array_dev(*get(h), arr_id, nullptr, check_l4_mode(mode), 0, nullptr, d_lxc_ids, d_tuples, n, d_verdicts, stream);
  });
}

int cg_l4_array_verdicts_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint16_t* lxc_ids,
                              const cg_l4_tuple* tuples, size_t n, int32_t* verdicts) {
  return guarded([&] {
    l4_array_host(*get(h), arr_id, nullptr, check_l4_mode(mode), 0, nullptr, lxc_ids, tuples, n, verdicts);
  });
}

int cg_l4_array_verdicts_ipcache_dev(uint64_t h, uint32_t arr_id, uint32_t ipc_id, uint32_t mode, int family,
                                     const void* d_remote, const uint16_t* d_lxc_ids, const cg_l4_tuple* d_tuples,
                                     size_t n, int32_t* d_verdicts, void* stream) {
  return guarded([&] {
    auto e = get(h);
    check_l4_mode(mode);
    check_family(family);
    e->require_gpu();
    const IpcView iv = ipc_view(*e, ipc_id);
    l4_array_dev(*e, arr_id, &iv, mode, family, d_remote, d_lxc_ids, d_tuples, n, d_verdicts, stream);
  });
}

int cg_l4_array_verdicts_ipcache_host(uint64_t h, uint32_t arr_id, uint32_t ipc_id, uint32_t mode, int family,
                                      const void* remote, const uint16_t* lxc_ids, const cg_l4_tuple* tuples, size_t n,
                                      int32_t* verdicts) {
  return guarded([&] {
    auto e = get(h);
    check_l4_mode(mode);
    check_family(family);
    e->require_gpu();
    const IpcView iv = ipc_view(*e, ipc_id);
    l4_array_host(*e, arr_id, &iv, mode, family, remote, lxc_ids, tuples, n, verdicts);
  });
}

// ----------------------------------------------------- endpoint map ----
// cilium_lxc with its values (endpoint_map.h), the control-plane calls of
// pkg/maps/lxcmap.
static EndpointMapState::Key make_ep_key(const cg_endpoint_key& k) {
  if (k.family != 4 && k.family != 6) fail(CG_INVALID_ADDRESS, "endpoint key family must be 4 or 6");
  EndpointMapState::Key out;
  out.first = k.family;
  out.second.fill(0);
  memcpy(out.second.data(), k.addr, k.family == 4 ? 4 : 16);
  return out;
}

int cg_endpoint_map_create(uint64_t h, uint32_t max_entries, uint32_t* ep_id) {
  return guarded([&] {
    auto e = get(h);
    if (!ep_id) fail(CG_INVALID_ARGUMENT, "ep_id is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    auto p = std::make_unique<EndpointMapState>();
    if (max_entries) p->max_entries = max_entries;
    const uint32_t id = e->next_id++;
    e->epmaps[id] = std::move(p);
    *ep_id = id;
  });
}

int cg_endpoint_map_destroy(uint64_t h, uint32_t ep_id) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    get_ep(*e, ep_id);
    if (e->has_gpu()) dev_sync(*e, nullptr);
    e->epmaps.erase(ep_id);
  });
}

int cg_endpoint_map_update(uint64_t h, uint32_t ep_id, const cg_endpoint_key* keys, const cg_endpoint_info* values,
                           size_t n) {
  return guarded([&] {
    auto e = get(h);
    if (n && (!keys || !values)) fail(CG_INVALID_ARGUMENT, "NULL keys/values");
    std::lock_guard<std::mutex> lk(e->mu);
    EndpointMapState& p = get_ep(*e, ep_id);
    // a key given twice in one batch keeps its last value, as sequential updates would
    std::map<EndpointMapState::Key, cg_endpoint_info> batch;
    for (size_t i = 0; i < n; ++i) batch[make_ep_key(keys[i])] = cg_endpoint_info{values[i].lxc_id, 0, values[i].flags};
    size_t fresh = 0;
    for (const auto& kv : batch) fresh += !p.entries.count(kv.first);
    if (p.entries.size() + fresh > p.max_entries) fail(CG_MAP_FULL, "endpoint map full (max_entries)");
    for (const auto& kv : batch) p.entries[kv.first] = kv.second;
    p.dirty = true;
  });
}

int cg_endpoint_map_delete(uint64_t h, uint32_t ep_id, const cg_endpoint_key* keys, size_t n) {
  return guarded([&] {
    auto e = get(h);
    if (n && !keys) fail(CG_INVALID_ARGUMENT, "NULL keys");
    std::lock_guard<std::mutex> lk(e->mu);
    EndpointMapState& p = get_ep(*e, ep_id);
    std::vector<EndpointMapState::Key> ks;
    for (size_t i = 0; i < n; ++i) {
      ks.push_back(make_ep_key(keys[i]));
      if (!p.entries.count(ks.back())) fail(CG_NOT_FOUND, "endpoint map: no entry for key");
    }
    for (const auto& k : ks) p.entries.erase(k);
    p.dirty = true;
  });
}

int cg_endpoint_map_lookup(uint64_t h, uint32_t ep_id, const cg_endpoint_key* key, cg_endpoint_info* value) {
  return guarded([&] {
    auto e = get(h);
    if (!key || !value) fail(CG_INVALID_ARGUMENT, "NULL key/value");
    std::lock_guard<std::mutex> lk(e->mu);
    EndpointMapState& p = get_ep(*e, ep_id);
    auto it = p.entries.find(make_ep_key(*key));
    if (it == p.entries.end()) fail(CG_NOT_FOUND, "endpoint map: no entry for key");
    *value = it->second;
  });
}

int cg_endpoint_map_dump(uint64_t h, uint32_t ep_id, cg_endpoint_key* keys, cg_endpoint_info* values, size_t cap,
                         size_t* n) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    EndpointMapState& p = get_ep(*e, ep_id);
    size_t i = 0;
    for (const auto& [k, v] : p.entries) {
      if (i >= cap) break;
      if (keys) {
        memset(&keys[i], 0, sizeof(cg_endpoint_key));
        keys[i].family = k.first;
        memcpy(keys[i].addr, k.second.data(), 16);
      }
      if (values) values[i] = v;
      ++i;
    }
    if (n) *n = p.entries.size();
  });
}

// -------------------------------------------------- conntrack maps ----
// cilium_ct{4,6}_* / cilium_ct_any{4,6}_* with their values (ct_map.h).
static CtMapState::Key make_ct_key(const cg_ct_key& k, bool global) {
  if (k.family != 4 && k.family != 6) fail(CG_INVALID_ADDRESS, "conntrack key family must be 4 or 6");
  if (k.kind != CG_CT_MAP_TCP && k.kind != CG_CT_MAP_ANY) fail(CG_INVALID_ARGUMENT, "conntrack key kind must be TCP or ANY");
  if (k.flags & ~0x07u) fail(CG_INVALID_ARGUMENT, "conntrack key flags above TUPLE_F_SERVICE");
  if (global && k.scope) fail(CG_INVALID_ARGUMENT, "a global conntrack map holds scope 0 only");
  if (k.family == 4)
    for (int i = 4; i < 16; ++i)
      if (k.daddr[i] | k.saddr[i]) fail(CG_INVALID_ARGUMENT, "an IPv4 conntrack key uses address bytes 0..3");
  return CtMapState::make_key(k);
}

int cg_ct_map_create(uint64_t h, uint32_t max_entries, uint32_t flags, uint32_t* ct_id) {
  return guarded([&] {
    auto e = get(h);
    if (!ct_id) fail(CG_INVALID_ARGUMENT, "ct_id is NULL");
    if (flags & ~CG_CT_MAP_F_GLOBAL) fail(CG_INVALID_ARGUMENT, "unknown conntrack map flags");
    std::lock_guard<std::mutex> lk(e->mu);
    auto p = std::make_unique<CtMapState>();
    if (max_entries) p->max_entries = max_entries;
    p->global = flags & CG_CT_MAP_F_GLOBAL;
    const uint32_t id = e->next_id++;
    e->ctmaps[id] = std::move(p);
    *ct_id = id;
  });
}

int cg_ct_map_destroy(uint64_t h, uint32_t ct_id) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    get_ct(*e, ct_id);
    if (e->has_gpu()) dev_sync(*e, nullptr);
    e->ctmaps.erase(ct_id);
  });
}

int cg_ct_map_update(uint64_t h, uint32_t ct_id, const cg_ct_key* keys, const cg_ct_entry* values, size_t n) {
  return guarded([&] {
    auto e = get(h);
    if (n && (!keys || !values)) fail(CG_INVALID_ARGUMENT, "NULL keys/values");
    std::lock_guard<std::mutex> lk(e->mu);
    CtMapState& p = get_ct(*e, ct_id);
    std::map<CtMapState::Key, cg_ct_entry> batch;
    for (size_t i = 0; i < n; ++i) batch[make_ct_key(keys[i], p.global)] = values[i];
    size_t fresh = 0;
    for (const auto& kv : batch) fresh += !p.entries.count(kv.first);
    if (p.entries.size() + fresh > p.max_entries) fail(CG_MAP_FULL, "conntrack map full (max_entries)");
    for (const auto& kv : batch) p.entries[kv.first] = kv.second;
    p.dirty = true;
  });
}

int cg_ct_map_delete(uint64_t h, uint32_t ct_id, const cg_ct_key* keys, size_t n) {
  return guarded([&] {
    auto e = get(h);
    if (n && !keys) fail(CG_INVALID_ARGUMENT, "NULL keys");
    std::lock_guard<std::mutex> lk(e->mu);
    CtMapState& p = get_ct(*e, ct_id);
    std::vector<CtMapState::Key> ks;
    for (size_t i = 0; i < n; ++i) {
      ks.push_back(make_ct_key(keys[i], p.global));
      if (!p.entries.count(ks.back())) fail(CG_NOT_FOUND, "conntrack map: no entry for key");
    }
    for (const auto& k : ks) p.entries.erase(k);
    p.dirty = true;
  });
}

int cg_ct_map_lookup(uint64_t h, uint32_t ct_id, const cg_ct_key* key, cg_ct_entry* value) {
  return guarded([&] {
    auto e = get(h);
    if (!key || !value) fail(CG_INVALID_ARGUMENT, "NULL key/value");
    std::lock_guard<std::mutex> lk(e->mu);
    CtMapState& p = get_ct(*e, ct_id);
    auto it = p.entries.find(make_ct_key(*key, p.global));
    if (it == p.entries.end()) fail(CG_NOT_FOUND, "conntrack map: no entry for key");
    *value = it->second;
  });
}

int cg_ct_map_dump(uint64_t h, uint32_t ct_id, cg_ct_key* keys, cg_ct_entry* values, size_t cap, size_t* n) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    CtMapState& p = get_ct(*e, ct_id);
    size_t i = 0;
    for (const auto& [k, v] : p.entries) {
      if (i >= cap) break;
      if (keys) keys[i] = CtMapState::key_of(k);
      if (values) values[i] = v;
      ++i;
    }
    if (n) *n = p.entries.size();
  });
}

int cg_ct_map_apply(uint64_t h, uint32_t ct_id, const cg_ct_record* records, size_t n, const uint32_t* pkt_len,
                    const uint32_t* src_labels, int32_t* results) {
  return guarded([&] {
    auto e = get(h);
    if (n && !records) fail(CG_INVALID_ARGUMENT, "NULL records");
    std::lock_guard<std::mutex> lk(e->mu);
    CtMapState& p = get_ct(*e, ct_id);
    // every record is checked before any is carried out
    for (size_t i = 0; i < n; ++i) {
      if (records[i].op > CG_CT_OP_UPDATE_SLAVE) fail(CG_INVALID_ARGUMENT, "unknown conntrack op");
      if (records[i].op != CG_CT_OP_NONE) make_ct_key(records[i].key, p.global);
    }
    for (size_t i = 0; i < n; ++i) {
      const cg_ct_record& r = records[i];
      if (results) results[i] = 0;
      if (r.op == CG_CT_OP_NONE) continue;
      const CtMapState::Key k = CtMapState::make_key(r.key);
      if (r.op == CG_CT_OP_DELETE) {
        p.dirty |= p.entries.erase(k) != 0;
        continue;
      }
      if (r.op == CG_CT_OP_UPDATE_SLAVE) {  // ct_update{4,6}_slave: a missing entry is left alone
        auto it = p.entries.find(k);
        if (it != p.entries.end()) {
          it->second.slave = r.pad1;
          p.dirty = true;
        }
        continue;
      }
      cg_ct_key rel = r.key;  // the ICMP / ICMPv6 entry that relates errors to the flow
      rel.nexthdr = r.key.family == 4 ? 1 : 58;
      rel.sport = rel.dport = 0;
      rel.flags = r.key.flags | CG_TUPLE_F_RELATED;
      const CtMapState::Key kr = CtMapState::make_key(rel);
      // ct_create4's second entry for a ct_state with addr (conntrack.h:725-753), dir != CT_INGRESS
      const bool second = r.key.family == 4 && r.pad0 == 1 && r.pad2[1] != 0;
      cg_ct_key two = r.key;
      if (second) {
        memcpy(two.daddr, &r.pad2[1], 4);
        if (r.loopback) {
          two.flags = CG_TUPLE_F_IN;
          memcpy(two.saddr, &r.pad3, 4);
        }
      }
      const CtMapState::Key k2 = CtMapState::make_key(two);
      std::vector<CtMapState::Key> fresh;
      for (const CtMapState::Key* c : {&k, &kr, &k2})
        if (!p.entries.count(*c) && std::find(fresh.begin(), fresh.end(), *c) == fresh.end()) fresh.push_back(*c);
      if (p.entries.size() + fresh.size() > p.max_entries) {
        if (results) results[i] = CG_DROP_CT_CREATE_FAILED;
        continue;
      }
      cg_ct_entry en{};
      if (r.pad0 != 0) {  // dir != CT_INGRESS (conntrack.h:706-712): tx; CT_EGRESS has SECLABEL in the record
        en.tx_packets = 1;
        en.tx_bytes = pkt_len ? pkt_len[i] : 0;
        en.src_sec_id = r.pad0 == 1 ? r.pad2[0] : 0;
      } else {
        en.rx_packets = 1;
        en.rx_bytes = pkt_len ? pkt_len[i] : 0;
        en.src_sec_id = src_labels ? src_labels[i] : 0;
      }
      en.rev_nat_index = r.rev_nat_index;
      en.slave = r.pad1;
      if (r.loopback) en.flags |= CG_CT_E_LB_LOOPBACK;
      p.entries[k] = en;
      if (second) p.entries[k2] = en;
      en.flags |= CG_CT_E_SEEN_NON_SYN;
      p.entries[kr] = en;
      p.dirty = true;
    }
  });
}

// ------------------------------------------------------ service maps ----
// cilium_lb{4,6}_services / cilium_lb{4,6}_reverse_nat (lb_map.h).
static void check_lb_addr(uint8_t family, const uint8_t* addr, const char* what) {
  if (family != 4 && family != 6) fail(CG_INVALID_ADDRESS, "service map family must be 4 or 6");
  if (family == 4)
    for (int i = 4; i < 16; ++i)
      if (addr[i]) fail(CG_INVALID_ARGUMENT, what);
}
static LbMapState::Key make_lb_key(const cg_lb_key& k) {
  check_lb_addr(k.family, k.address, "an IPv4 service key uses address bytes 0..3");
  if (k.pad[0] | k.pad[1] | k.pad[2]) fail(CG_INVALID_ARGUMENT, "service key pad must be 0");
  return LbMapState::make_key(k);
}
static std::pair<uint8_t, uint16_t> make_rn_key(const cg_lb_revnat_key& k) {
  if (k.family != 4 && k.family != 6) fail(CG_INVALID_ADDRESS, "service map family must be 4 or 6");
  if (k.pad) fail(CG_INVALID_ARGUMENT, "reverse NAT key pad must be 0");
  return {k.family, k.index};
}

int cg_lb_map_create(uint64_t h, uint32_t max_entries, uint32_t ipv4_loopback, uint32_t* lb_id) {
  return guarded([&] {
    auto e = get(h);
    if (!lb_id) fail(CG_INVALID_ARGUMENT, "lb_id is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    auto p = std::make_unique<LbMapState>();
    if (max_entries) p->max_entries = max_entries;
    p->loopback = ipv4_loopback;
    const uint32_t id = e->next_id++;
    e->lbmaps[id] = std::move(p);
    *lb_id = id;
  });
}

int cg_lb_map_destroy(uint64_t h, uint32_t lb_id) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    get_lb(*e, lb_id);
    if (e->has_gpu()) dev_sync(*e, nullptr);
    e->lbmaps.erase(lb_id);
  });
}

int cg_lb_map_set_loopback(uint64_t h, uint32_t lb_id, uint32_t ipv4_loopback) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    LbMapState& p = get_lb(*e, lb_id);
    p.loopback = ipv4_loopback;
    p.dirty = true;
  });
}

int cg_lb_map_service_update(uint64_t h, uint32_t lb_id, const cg_lb_key* keys, const cg_lb_service* values, size_t n) {
  return guarded([&] {
    auto e = get(h);
    if (n && (!keys || !values)) fail(CG_INVALID_ARGUMENT, "NULL keys/values");
    std::lock_guard<std::mutex> lk(e->mu);
    LbMapState& p = get_lb(*e, lb_id);
    std::map<LbMapState::Key, cg_lb_service> batch;
    for (size_t i = 0; i < n; ++i) {
      check_lb_addr(keys[i].family, values[i].target, "an IPv4 service value uses target bytes 0..3");
      batch[make_lb_key(keys[i])] = values[i];
    }
    size_t fresh[2] = {0, 0};
    for (const auto& kv : batch) fresh[kv.first[0] == 6] += !p.services.count(kv.first);
    if (p.count_services(4) + fresh[0] > p.max_entries || p.count_services(6) + fresh[1] > p.max_entries)
      fail(CG_MAP_FULL, "service map full (max_entries)");
    for (const auto& kv : batch) p.services[kv.first] = kv.second;
    p.dirty = true;
  });
}

int cg_lb_map_service_delete(uint64_t h, uint32_t lb_id, const cg_lb_key* keys, size_t n) {
  return guarded([&] {
    auto e = get(h);
    if (n && !keys) fail(CG_INVALID_ARGUMENT, "NULL keys");
    std::lock_guard<std::mutex> lk(e->mu);
    LbMapState& p = get_lb(*e, lb_id);
    std::vector<LbMapState::Key> ks;
    for (size_t i = 0; i < n; ++i) {
      ks.push_back(make_lb_key(keys[i]));
      if (!p.services.count(ks.back())) fail(CG_NOT_FOUND, "service map: no entry for key");
    }
    for (const auto& k : ks) p.services.erase(k);
    p.dirty = true;
  });
}

int cg_lb_map_service_lookup(uint64_t h, uint32_t lb_id, const cg_lb_key* key, cg_lb_service* value) {
  return guarded([&] {
    auto e = get(h);
    if (!key || !value) fail(CG_INVALID_ARGUMENT, "NULL key/value");
    std::lock_guard<std::mutex> lk(e->mu);
    LbMapState& p = get_lb(*e, lb_id);
    auto it = p.services.find(make_lb_key(*key));
    if (it == p.services.end()) fail(CG_NOT_FOUND, "service map: no entry for key");
    *value = it->second;
  });
}

int cg_lb_map_service_dump(uint64_t h, uint32_t lb_id, cg_lb_key* keys, cg_lb_service* values, size_t cap, size_t* n) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    LbMapState& p = get_lb(*e, lb_id);
    size_t i = 0;
    for (const auto& [k, v] : p.services) {
      if (i >= cap) break;
      if (keys) keys[i] = LbMapState::key_of(k);
      if (values) values[i] = v;
      ++i;
    }
    if (n) *n = p.services.size();
  });
}

int cg_lb_map_revnat_update(uint64_t h, uint32_t lb_id, const cg_lb_revnat_key* keys, const cg_lb_revnat* values,
                            size_t n) {
  return guarded([&] {
    auto e = get(h);
    if (n && (!keys || !values)) fail(CG_INVALID_ARGUMENT, "NULL keys/values");
    std::lock_guard<std::mutex> lk(e->mu);
    LbMapState& p = get_lb(*e, lb_id);
    std::map<std::pair<uint8_t, uint16_t>, cg_lb_revnat> batch;
    for (size_t i = 0; i < n; ++i) {
      check_lb_addr(keys[i].family, values[i].address, "an IPv4 reverse NAT value uses address bytes 0..3");
      if (values[i].pad) fail(CG_INVALID_ARGUMENT, "reverse NAT value pad must be 0");
      batch[make_rn_key(keys[i])] = values[i];
    }
    size_t fresh[2] = {0, 0};
    for (const auto& kv : batch) fresh[kv.first.first == 6] += !p.revnat.count(kv.first);
    if (p.count_revnat(4) + fresh[0] > p.max_entries || p.count_revnat(6) + fresh[1] > p.max_entries)
      fail(CG_MAP_FULL, "reverse NAT map full (max_entries)");
    for (const auto& kv : batch) p.revnat[kv.first] = kv.second;
    p.dirty = true;
  });
}

int cg_lb_map_revnat_delete(uint64_t h, uint32_t lb_id, const cg_lb_revnat_key* keys, size_t n) {
  return guarded([&] {
    auto e = get(h);
    if (n && !keys) fail(CG_INVALID_ARGUMENT, "NULL keys");
    std::lock_guard<std::mutex> lk(e->mu);
    LbMapState& p = get_lb(*e, lb_id);
    std::vector<std::pair<uint8_t, uint16_t>> ks;
    for (size_t i = 0; i < n; ++i) {
      ks.push_back(make_rn_key(keys[i]));
      if (!p.revnat.count(ks.back())) fail(CG_NOT_FOUND, "reverse NAT map: no entry for index");
    }
    for (const auto& k : ks) p.revnat.erase(k);
    p.dirty = true;
  });
}

int cg_lb_map_revnat_lookup(uint64_t h, uint32_t lb_id, const cg_lb_revnat_key* key, cg_lb_revnat* value) {
  return guarded([&] {
    auto e = get(h);
    if (!key || !value) fail(CG_INVALID_ARGUMENT, "NULL key/value");
    std::lock_guard<std::mutex> lk(e->mu);
    LbMapState& p = get_lb(*e, lb_id);
    auto it = p.revnat.find(make_rn_key(*key));
    if (it == p.revnat.end()) fail(CG_NOT_FOUND, "reverse NAT map: no entry for index");
    *value = it->second;
  });
}

int cg_lb_map_revnat_dump(uint64_t h, uint32_t lb_id, cg_lb_revnat_key* keys, cg_lb_revnat* values, size_t cap,
                          size_t* n) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    LbMapState& p = get_lb(*e, lb_id);
    size_t i = 0;
    for (const auto& [k, v] : p.revnat) {
      if (i >= cap) break;
      if (keys) keys[i] = cg_lb_revnat_key{k.second, k.first, 0};
      if (values) values[i] = v;
      ++i;
    }
    if (n) *n = p.revnat.size();
  });
}

// ------------------------------------------- L4 verdicts from frames ----
// What an entry of the route names beside its batch.  ep_id: 0 when lxc_ids
// name the endpoints; ct_id: NULL without a conntrack map; egress: the
// from-container program over the array's headers, else the ingress one.
struct FramesReq {
  uint32_t arr_id, ep_id, ipc_id;
  const uint32_t* ct_id;
  bool egress;
  // the from-container program over a services map: the map, and the per-frame arrays only that program has
  const uint32_t* lb_id = nullptr;
  const uint32_t* hash = nullptr;
  cg_ct_record* svc_recs = nullptr;
  cg_lb_xlate* xlate = nullptr;
};
static void check_frames_args(uint32_t mode, const void* lxc, uint32_t ep_id, const void* labels, uint32_t ipc_id) {
  if ((mode & ~CG_L4_IGNORE_DROP) != CG_L4_INGRESS)
    fail(CG_INVALID_ARGUMENT, "frame verdicts run the ingress program: mode is CG_L4_INGRESS [| CG_L4_IGNORE_DROP]");
  if ((lxc != nullptr) == (ep_id != 0)) fail(CG_INVALID_ARGUMENT, "give lxc_ids or an endpoint map, not both or neither");
  if ((labels != nullptr) == (ipc_id != 0))
    fail(CG_INVALID_ARGUMENT, "give src_labels or an ipcache, not both or neither");
}
static void check_egress_args(uint32_t mode, const void* lxc, const void* labels, uint32_t ipc_id, uint32_t ct_id,
                              const void* recs) {
  if ((mode & ~CG_L4_IGNORE_DROP) != CG_L4_EGRESS)
    fail(CG_INVALID_ARGUMENT, "egress frame verdicts run the from-container program: mode is CG_L4_EGRESS [| CG_L4_IGNORE_DROP]");
  if (!lxc) fail(CG_INVALID_ARGUMENT, "lxc_ids is mandatory: the program hangs on the endpoint's own device");
  if ((labels != nullptr) == (ipc_id != 0))
    fail(CG_INVALID_ARGUMENT, "give dst_labels or an ipcache, not both or neither");
  if (recs && !ct_id) fail(CG_INVALID_ARGUMENT, "records need a conntrack map");
}
// The checks of every entry, in their order.  gpu: the entry launches; host: raw is read here (or staged from here).
static void check_frames(Engine& e, const FramesReq& q, const FramesBatch& b, bool gpu, bool host) {
  if (q.lb_id && (!q.ct_id || !q.ipc_id || b.labels))
    fail(CG_INVALID_ARGUMENT, "the service steps need a conntrack map and the ipcache; dst_labels cannot name a backend");
  if (q.egress) check_egress_args(b.mode, b.lxc, b.labels, q.ipc_id, q.ct_id ? *q.ct_id : 0, b.recs);
  else check_frames_args(b.mode, b.lxc, q.ep_id, b.labels, q.ipc_id);
  if (gpu) e.require_gpu();
  if (!b.off || (b.n && !b.out)) fail(CG_INVALID_ARGUMENT, "NULL raw_off/verdicts");
  if (host && b.off[b.n] > b.off[0] && !b.raw) fail(CG_INVALID_ARGUMENT, "NULL raw");
}

// One snapshot of the policy array and of what the request names beside it (the endpoint map or the array's
// headers, the ipcache, the conntrack map), taken under one hold of the handle lock; the launch holds all of them.
struct FramesView {
  L4ArrView arr;
  std::shared_ptr<DevTables> ep_keep, hdr_keep, ipc_keep, ct_keep, lb_keep;
  LbMapDev lb{};
  EpMapDev ep{};
  EpHdrDev hdr{};
  IpcacheDev ipc{};
  CtMapDev ct{};
};
static FramesView frames_view(Engine& e, const FramesReq& q) {
  std::lock_guard<std::mutex> lk(e.mu);
  FramesView v;
  if (q.ct_id) {
    CtMapState& p = get_ct(e, *q.ct_id);
    if (p.dirty) p.rebuild(e);
    v.ct_keep = p.tab;
    v.ct = p.dev;
  }
  if (q.lb_id) {
    LbMapState& p = get_lb(e, *q.lb_id);
    if (p.dirty) p.rebuild(e);
    v.lb_keep = p.tab;
    v.lb = p.dev;
  }
  v.arr = l4_array_view_locked(e, q.arr_id);
  if (q.ep_id) {
    EndpointMapState& p = get_ep(e, q.ep_id);
    if (p.dirty) p.rebuild(e);
    v.ep_keep = p.tab;
    v.ep = p.dev;
  }
  if (q.egress) {
    PolicyArrayState& a = get_arr(e, q.arr_id);
    if (a.headers_changed || !a.hdr_tab) {
      std::vector<uint32_t> idx;
      std::vector<uint4> recs;
      a.header_tables(&idx, &recs);
      e.set_device();
      auto t = std::make_shared<DevTables>();
      EpHdrDev d{};
      d.idx = t->add(idx);
      d.recs = t->add(recs);
      a.hdr_tab = std::move(t);  // publish
      a.hdr_dev = d;
      a.headers_changed = false;
    }
    v.hdr_keep = a.hdr_tab;
    v.hdr = a.hdr_dev;
  }
  if (q.ipc_id) {
    IpcacheState& p = get_ipc(e, q.ipc_id);
    if (p.dirty) p.rebuild(e);
    v.ipc_keep = p.tab;
    v.ipc = p.dev;
  }
  return v;
}
// The launch over device buffers d: the from-container program when the view holds headers, the one with the
// service steps when it holds a service map (x: that program's per-frame device arrays).
struct SvcArrays {
  const uint32_t* hash = nullptr;
  cg_ct_record* svc_recs = nullptr;
  cg_lb_xlate* xlate = nullptr;
};
static void frames_launch(Engine& e, const FramesView& v, const FramesBatch& d, const SvcArrays& x, void* st) {
  const IpcacheDev* ipc = v.ipc_keep ? &v.ipc : nullptr;
  const CtMapDev* ct = v.ct_keep ? &v.ct : nullptr;
  if (v.lb_keep)
    check_launch(launch_l4_frames_egress_svc(v.arr.dev, EpHdrSvcDev{v.hdr, v.lb, x.hash, (uint4*)x.svc_recs, (uint4*)x.xlate},
                                             v.ipc, v.ct, d, st, e.cus),
                 "l4 frames egress service kernel launch");
  else if (v.hdr_keep)
    check_launch(launch_l4_frames_egress(v.arr.dev, v.hdr, ipc, ct, d, st, e.cus), "l4 frames egress kernel launch");
  else
    check_launch(launch_l4_frames(v.arr.dev, v.ep_keep ? &v.ep : nullptr, ipc, ct, d, st, e.cus),
                 ct ? "l4 frames conntrack kernel launch" : "l4 frames kernel launch");
  fence(v.ct_keep, st);
  fence(v.lb_keep, st);
  v.arr.keep->own.fence.record(st);
  fence(v.ep_keep, st);
  fence(v.hdr_keep, st);
  fence(v.ipc_keep, st);
}

static void frames_dev(uint64_t h, const FramesReq& q, const FramesBatch& d, void* stream) {
  auto e = get(h);
  check_frames(*e, q, d, true, false);
  const FramesView v = frames_view(*e, q);
  e->set_device();
  frames_launch(*e, v, d, SvcArrays{q.hash, q.svc_recs, q.xlate}, stream_of(*e, stream));
}

static void* stage_in(StagingSlot& sl, int i, const void* src, size_t bytes);

// The host entries' staging: the blob's window [raw_off[0], raw_off[n]), the offsets and the per-frame inputs go
// up, the launch runs over the device copies, the results come back.
static void frames_staged(Engine& e, const FramesView& v, const FramesReq& q, const FramesBatch& b) {
  const size_t n = b.n;
  const uint64_t lo = b.off[0], bytes = b.off[n] > lo ? b.off[n] - lo : 0;
  e.set_device();
  auto lease = e.staging.acquire(e.device);
  const auto st = (hipStream_t)lease->stream;
  FramesBatch d = b;
  // the kernel adds the offsets to d.raw
  const uint8_t* d_win = (const uint8_t*)stage_in(*lease, 0, b.raw + lo, bytes);
  d.raw = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_win) - lo);
  d.off = (const uint64_t*)stage_in(*lease, 1, b.off, (n + 1) * 8);
  if (b.lxc) d.lxc = (const uint16_t*)stage_in(*lease, 2, b.lxc, n * 2);
  if (b.labels) d.labels = (const uint32_t*)stage_in(*lease, 3, b.labels, n * 4);
  if (b.pkt_len) d.pkt_len = (const uint32_t*)stage_in(*lease, 4, b.pkt_len, n * 4);
  d.out = (int32_t*)lease->dev_buf(5, n * 4);
  if (b.info) d.info = (cg_l4_frame_info*)lease->dev_buf(6, n * sizeof(cg_l4_frame_info));
  if (b.recs) d.recs = (cg_ct_record*)lease->dev_buf(7, n * sizeof(cg_ct_record));
  SvcArrays x;
  if (q.hash) x.hash = (const uint32_t*)stage_in(*lease, 29, q.hash, n * 4);
  if (q.svc_recs) x.svc_recs = (cg_ct_record*)lease->dev_buf(30, n * sizeof(cg_ct_record));
  if (q.xlate) x.xlate = (cg_lb_xlate*)lease->dev_buf(31, n * sizeof(cg_lb_xlate));
  frames_launch(e, v, d, x, (void*)st);
  int32_t* h_out = (int32_t*)lease->host_buf(5, n * 4);
  hip_check(hipMemcpyAsync(h_out, d.out, n * 4, hipMemcpyDeviceToHost, st), "D2H");
  void* h_info = b.info ? lease->host_buf(6, n * sizeof(cg_l4_frame_info)) : nullptr;
  if (b.info) hip_check(hipMemcpyAsync(h_info, d.info, n * sizeof(cg_l4_frame_info), hipMemcpyDeviceToHost, st), "D2H");
  void* h_recs = b.recs ? lease->host_buf(7, n * sizeof(cg_ct_record)) : nullptr;
  if (b.recs) hip_check(hipMemcpyAsync(h_recs, d.recs, n * sizeof(cg_ct_record), hipMemcpyDeviceToHost, st), "D2H");
  void* h_srecs = q.svc_recs ? lease->host_buf(30, n * sizeof(cg_ct_record)) : nullptr;
  if (q.svc_recs)
    hip_check(hipMemcpyAsync(h_srecs, x.svc_recs, n * sizeof(cg_ct_record), hipMemcpyDeviceToHost, st), "D2H");
  void* h_xl = q.xlate ? lease->host_buf(31, n * sizeof(cg_lb_xlate)) : nullptr;
  if (q.xlate) hip_check(hipMemcpyAsync(h_xl, x.xlate, n * sizeof(cg_lb_xlate), hipMemcpyDeviceToHost, st), "D2H");
  hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  memcpy(b.out, h_out, n * 4);
  if (b.info) memcpy(b.info, h_info, n * sizeof(cg_l4_frame_info));
  if (b.recs) memcpy(b.recs, h_recs, n * sizeof(cg_ct_record));
  if (q.svc_recs) memcpy(q.svc_recs, h_srecs, n * sizeof(cg_ct_record));
  if (q.xlate) memcpy(q.xlate, h_xl, n * sizeof(cg_lb_xlate));
}

static void frames_host(uint64_t h, const FramesReq& q, const FramesBatch& b) {
  auto e = get(h);
  check_frames(*e, q, b, true, true);
  const FramesView v = frames_view(*e, q);
  if (b.n) frames_staged(*e, v, q, b);
}

int cg_l4_frames_verdicts_dev(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* d_raw,
                              const uint64_t* d_raw_off, size_t n, const uint16_t* d_lxc_ids, uint32_t ep_id,
                              const uint32_t* d_src_labels, uint32_t ipc_id, const uint32_t* d_pkt_len,
                              int32_t* d_verdicts, cg_l4_frame_info* d_info, void* stream) {
  return guarded([&] {
    frames_dev(h, {arr_id, ep_id, ipc_id, nullptr, false},
               {d_raw, d_raw_off, n, d_lxc_ids, d_src_labels, d_pkt_len, d_verdicts, d_info, nullptr, mode}, stream);
  });
}

int cg_l4_frames_ct_verdicts_dev(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* d_raw,
                                 const uint64_t* d_raw_off, size_t n, const uint16_t* d_lxc_ids, uint32_t ep_id,
                                 const uint32_t* d_src_labels, uint32_t ipc_id, const uint32_t* d_pkt_len,
                                 uint32_t ct_id, int32_t* d_verdicts, cg_l4_frame_info* d_info,
                                 cg_ct_record* d_records, void* stream) {
  return guarded([&] {
    frames_dev(h, {arr_id, ep_id, ipc_id, &ct_id, false},
               {d_raw, d_raw_off, n, d_lxc_ids, d_src_labels, d_pkt_len, d_verdicts, d_info, d_records, mode}, stream);
  });
}

int cg_l4_frames_egress_verdicts_dev(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* d_raw,
                                     const uint64_t* d_raw_off, size_t n, const uint16_t* d_lxc_ids,
                                     const uint32_t* d_dst_labels, uint32_t ipc_id, const uint32_t* d_pkt_len,
                                     uint32_t ct_id, int32_t* d_verdicts, cg_l4_frame_info* d_info,
                                     cg_ct_record* d_records, void* stream) {
  return guarded([&] {
    frames_dev(h, {arr_id, 0, ipc_id, ct_id ? &ct_id : nullptr, true},
               {d_raw, d_raw_off, n, d_lxc_ids, d_dst_labels, d_pkt_len, d_verdicts, d_info, d_records, mode}, stream);
  });
}

int cg_l4_frames_verdicts_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                               const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids, uint32_t ep_id,
                               const uint32_t* src_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                               int32_t* verdicts, cg_l4_frame_info* info) {
  return guarded([&] {
    frames_host(h, {arr_id, ep_id, ipc_id, nullptr, false},
                {raw, raw_off, n, lxc_ids, src_labels, pkt_len, verdicts, info, nullptr, mode});
  });
}

int cg_l4_frames_ct_verdicts_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                                  const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids, uint32_t ep_id,
                                  const uint32_t* src_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                                  uint32_t ct_id, int32_t* verdicts, cg_l4_frame_info* info, cg_ct_record* records) {
  return guarded([&] {
    frames_host(h, {arr_id, ep_id, ipc_id, &ct_id, false},
                {raw, raw_off, n, lxc_ids, src_labels, pkt_len, verdicts, info, records, mode});
  });
}

int cg_l4_frames_egress_verdicts_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                                      const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids,
                                      const uint32_t* dst_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                                      uint32_t ct_id, int32_t* verdicts, cg_l4_frame_info* info,
                                      cg_ct_record* recs) {
  return guarded([&] {
    frames_host(h, {arr_id, 0, ipc_id, ct_id ? &ct_id : nullptr, true},
                {raw, raw_off, n, lxc_ids, dst_labels, pkt_len, verdicts, info, recs, mode});
  });
}

static FramesReq svc_req(uint32_t arr_id, uint32_t ipc_id, const uint32_t* ct_id, const uint32_t* lb_id,
                         const uint32_t* hash, cg_ct_record* svc_recs, cg_lb_xlate* xlate) {
  FramesReq q{arr_id, 0, ipc_id, *ct_id ? ct_id : nullptr, true};
  q.lb_id = lb_id;
  q.hash = hash;
  q.svc_recs = svc_recs;
  q.xlate = xlate;
  return q;
}

int cg_l4_frames_egress_svc_verdicts_dev(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* d_raw,
                                         const uint64_t* d_raw_off, size_t n, const uint16_t* d_lxc_ids,
                                         const uint32_t* d_dst_labels, uint32_t ipc_id, const uint32_t* d_pkt_len,
                                         uint32_t ct_id, uint32_t lb_id, const uint32_t* d_hash, int32_t* d_verdicts,
                                         cg_l4_frame_info* d_info, cg_ct_record* d_records,
                                         cg_ct_record* d_svc_records, cg_lb_xlate* d_xlate, void* stream) {
  return guarded([&] {
    frames_dev(h, svc_req(arr_id, ipc_id, &ct_id, &lb_id, d_hash, d_svc_records, d_xlate),
               {d_raw, d_raw_off, n, d_lxc_ids, d_dst_labels, d_pkt_len, d_verdicts, d_info, d_records, mode}, stream);
  });
}

int cg_l4_frames_egress_svc_verdicts_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                                          const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids,
                                          const uint32_t* dst_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                                          uint32_t ct_id, uint32_t lb_id, const uint32_t* hash, int32_t* verdicts,
                                          cg_l4_frame_info* info, cg_ct_record* records, cg_ct_record* svc_records,
                                          cg_lb_xlate* xlate) {
  return guarded([&] {
    frames_host(h, svc_req(arr_id, ipc_id, &ct_id, &lb_id, hash, svc_records, xlate),
                {raw, raw_off, n, lxc_ids, dst_labels, pkt_len, verdicts, info, records, mode});
  });
}

// ----------------------------------------------------------------- LPM ----
int cg_prefilter_create(uint64_t h, uint32_t config, uint32_t max_lpm, uint32_t max_hash, uint32_t* pf_id) {
  return guarded([&] {
    auto e = get(h);
    if (!pf_id) fail(CG_INVALID_ARGUMENT, "pf_id is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    auto p = std::make_unique<PrefilterState>();
    p->config = config;
    if (max_lpm) p->max_lpm = max_lpm;
    if (max_hash) p->max_hash = max_hash;
    uint32_t id = e->next_id++;
    e->prefilters[id] = std::move(p);
    *pf_id = id;
  });
}

int cg_prefilter_destroy(uint64_t h, uint32_t pf_id) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    get_pf(*e, pf_id);
    if (e->has_gpu()) dev_sync(*e, nullptr);
    e->prefilters.erase(pf_id);
  });
}

int cg_prefilter_insert(uint64_t h, uint32_t pf_id, int64_t revision, const cg_cidr* cidrs, size_t n,
                        int64_t* revision_out) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PrefilterState& p = get_pf(*e, pf_id);
    if (revision != 0 && p.revision != revision)
      fail(CG_REVISION_MISMATCH,
           "Latest revision is " + std::to_string(p.revision) + " not " + std::to_string(revision));
    std::vector<std::pair<int, CidrKey>> undo;
    int err = 0;
    std::string msg;
    for (size_t i = 0; i < n && !err; ++i) {
      CidrKey k = make_cidr(cidrs[i]);
      int which = select_map(k);
      if (!p.enabled(which)) {
        err = CG_NO_MAP;
        msg = "No map enabled for CIDR string";
        break;
      }
      uint32_t cap = (which == 0 || which == 2) ? p.max_lpm : p.max_hash;
      if (p.maps[which].count(k)) {
        // BPF_ANY update of an existing key succeeds, and Insert still queues
        // it for undo: a later failure deletes it (prefilter.go:141-158).
        undo.push_back({which, k});
        continue;
      }
      if (p.maps[which].size() >= cap) {
        err = CG_MAP_FULL;
        msg = "Error inserting CIDR string: map full";
        break;
      }
      p.maps[which].insert(k);
      undo.push_back({which, k});
    }
    if (err) {
      for (auto& [w, k] : undo) p.maps[w].erase(k);
      fail(err, msg);
    }
    p.revision++;
    p.dirty = true;
    if (revision_out) *revision_out = p.revision;
  });
}

int cg_prefilter_delete(uint64_t h, uint32_t pf_id, int64_t revision, const cg_cidr* cidrs, size_t n,
                        int64_t* revision_out) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PrefilterState& p = get_pf(*e, pf_id);
    if (revision != 0 && p.revision != revision)
      fail(CG_REVISION_MISMATCH,
           "Latest revision is " + std::to_string(p.revision) + " not " + std::to_string(revision));
    std::vector<CidrKey> ks;
    for (size_t i = 0; i < n; ++i) {
      CidrKey k = make_cidr(cidrs[i]);
      int which = select_map(k);
      if (!p.enabled(which)) fail(CG_NO_MAP, "No map enabled for CIDR string");
      if (!p.maps[which].count(k)) fail(CG_NOT_FOUND, "No map entry for CIDR string");
      ks.push_back(k);
    }
    for (auto& k : ks) p.maps[select_map(k)].erase(k);
    p.revision++;
    p.dirty = true;
    if (revision_out) *revision_out = p.revision;
  });
}

int cg_prefilter_dump(uint64_t h, uint32_t pf_id, cg_cidr* out, size_t cap, size_t* n, int64_t* revision) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PrefilterState& p = get_pf(*e, pf_id);
    size_t i = 0, total = 0;
    for (int w = 0; w < 4; ++w) {  // prefixesV4Dyn .. prefixesV6Fix order (prefilter.go:102)
      for (const auto& k : p.maps[w]) {
        if (out && i < cap) {
          memset(&out[i], 0, sizeof(cg_cidr));
          out[i].family = k.family;
          out[i].prefixlen = k.plen;
          memcpy(out[i].addr, k.net.data(), 16);
          ++i;
        }
        ++total;
      }
    }
    if (n) *n = total;
    if (revision) *revision = p.revision;
  });
}

int cg_prefilter_set_endpoints(uint64_t h, uint32_t pf_id, const uint32_t* v4, size_t n4, const uint8_t* v6,
                               size_t n6) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PrefilterState& p = get_pf(*e, pf_id);
    p.ep4.assign(v4, v4 + n4);
    p.ep6.resize(n6);
    for (size_t i = 0; i < n6; ++i) memcpy(p.ep6[i].data(), v6 + 16 * i, 16);
    p.dirty = true;
  });
}

struct LpmView {
  std::shared_ptr<DevTables> keep;
  LpmDev dev;
  bool v4f, v6f;
};
static LpmView lpm_view(Engine& e, uint32_t pf_id) {
  std::lock_guard<std::mutex> lk(e.mu);
  PrefilterState& p = get_pf(e, pf_id);
  if (p.dirty) p.rebuild(e);
  return {p.tab, p.dev, p.v4_filter, p.v6_filter};
}

int cg_prefilter_verdicts_dev(uint64_t h, uint32_t pf_id, const uint32_t* d_v4, size_t n4, uint8_t* d_out4,
                              const uint8_t* d_v6, size_t n6, uint8_t* d_out6, void* stream) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    const LpmView v = lpm_view(*e, pf_id);
    e->set_device();
    check_launch(launch_lpm(v.dev, v.v4f, v.v6f, d_v4, n4, d_out4, d_v6, n6, d_out6, stream_of(*e, stream), e->cus),
                 "lpm kernel launch");
    fence(v.keep, stream_of(*e, stream));
  });
}

int cg_prefilter_verdicts_host(uint64_t h, uint32_t pf_id, const uint32_t* v4, size_t n4, uint8_t* out4,
                               const uint8_t* v6, size_t n6, uint8_t* out6) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    if ((n4 && (!v4 || !out4)) || (n6 && (!v6 || !out6))) fail(CG_INVALID_ARGUMENT, "NULL address/verdict arrays");
    const LpmView v = lpm_view(*e, pf_id);
    host_pipeline(*e, n4, {{v4, 8}}, {{out4, 1}}, [&](void* const* din, void* const* dout, size_t cnt, void* st) {
      check_launch(launch_lpm(v.dev, v.v4f, v.v6f, (const uint32_t*)din[0], cnt, (uint8_t*)dout[0], nullptr, 0,
                              nullptr, st, e->cus),
                   "lpm kernel launch");
    });
    host_pipeline(*e, n6, {{v6, 32}}, {{out6, 1}}, [&](void* const* din, void* const* dout, size_t cnt, void* st) {
      check_launch(launch_lpm(v.dev, v.v4f, v.v6f, nullptr, 0, nullptr, (const uint8_t*)din[0], cnt,
                              (uint8_t*)dout[0], st, e->cus),
                   "lpm kernel launch");
    });
  });
}

// ------------------------------------------------------------- ipcache ----
int cg_ipcache_create(uint64_t h, uint32_t max_entries, uint32_t* ipc_id) {
  return guarded([&] {
    auto e = get(h);
    if (!ipc_id) fail(CG_INVALID_ARGUMENT, "ipc_id is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    auto p = std::make_unique<IpcacheState>();
    if (max_entries) p->max_entries = max_entries;
    uint32_t id = e->next_id++;
    e->ipcaches[id] = std::move(p);
    *ipc_id = id;
  });
}

int cg_ipcache_destroy(uint64_t h, uint32_t ipc_id) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    get_ipc(*e, ipc_id);
    if (e->has_gpu()) dev_sync(*e, nullptr);
    e->ipcaches.erase(ipc_id);
  });
}

int cg_ipcache_update(uint64_t h, uint32_t ipc_id, const cg_cidr* keys, const cg_remote_endpoint_info* values,
                      size_t n) {
  return guarded([&] {
    auto e = get(h);
    if (n && (!keys || !values)) fail(CG_INVALID_ARGUMENT, "NULL keys/values");
    std::lock_guard<std::mutex> lk(e->mu);
    IpcacheState& p = get_ipc(*e, ipc_id);
    std::map<CidrKey, IpcVal> batch;
    for (size_t i = 0; i < n; ++i) batch[make_cidr(keys[i])] = IpcVal{values[i].sec_label, values[i].tunnel_endpoint};
    size_t fresh = 0;
    for (const auto& kv : batch) fresh += !p.entries.count(kv.first);
    if (p.entries.size() + fresh > p.max_entries) fail(CG_MAP_FULL, "ipcache: map full (max_entries)");
    // a key given twice in one batch keeps its last value, as sequential updates would
    for (size_t i = 0; i < n; ++i) p.entries[make_cidr(keys[i])] = IpcVal{values[i].sec_label, values[i].tunnel_endpoint};
    p.dirty = true;
  });
}

int cg_ipcache_delete(uint64_t h, uint32_t ipc_id, const cg_cidr* keys, size_t n) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    IpcacheState& p = get_ipc(*e, ipc_id);
    std::vector<CidrKey> ks;
    for (size_t i = 0; i < n; ++i) {
      CidrKey k = make_cidr(keys[i]);
      if (!p.entries.count(k)) fail(CG_NOT_FOUND, "ipcache: no entry for key");
      ks.push_back(k);
    }
    for (auto& k : ks) p.entries.erase(k);
    p.dirty = true;
  });
}

int cg_ipcache_lookup(uint64_t h, uint32_t ipc_id, const cg_cidr* key, cg_remote_endpoint_info* value) {
  return guarded([&] {
    auto e = get(h);
    if (!key || !value) fail(CG_INVALID_ARGUMENT, "NULL key/value");
    std::lock_guard<std::mutex> lk(e->mu);
    IpcacheState& p = get_ipc(*e, ipc_id);
    auto it = p.entries.find(make_cidr(*key));
    if (it == p.entries.end()) fail(CG_NOT_FOUND, "ipcache: no entry for key");
    value->sec_label = it->second.identity;
    value->tunnel_endpoint = it->second.tunnel;
  });
}

int cg_ipcache_dump(uint64_t h, uint32_t ipc_id, cg_cidr* keys, cg_remote_endpoint_info* values, size_t cap,
                    size_t* n) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    IpcacheState& p = get_ipc(*e, ipc_id);
    size_t i = 0;
    for (const auto& [k, v] : p.entries) {
      if (i >= cap) break;
      if (keys) {
        memset(&keys[i], 0, sizeof(cg_cidr));
        keys[i].family = k.family;
        keys[i].prefixlen = k.plen;
        memcpy(keys[i].addr, k.net.data(), 16);
      }
      if (values) values[i] = cg_remote_endpoint_info{v.identity, v.tunnel};
      ++i;
    }
    if (n) *n = p.entries.size();
  });
}

int cg_ipcache_resolve_dev(uint64_t h, uint32_t ipc_id, const uint32_t* d_v4, size_t n4,
                           cg_remote_endpoint_info* d_out4, const uint8_t* d_v6, size_t n6,
                           cg_remote_endpoint_info* d_out6, void* stream) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    const IpcView v = ipc_view(*e, ipc_id);
    e->set_device();
    check_launch(launch_ipcache(v.dev, d_v4, n4, (IpcVal*)d_out4, d_v6, n6, (IpcVal*)d_out6, stream_of(*e, stream),
                                e->cus),
                 "ipcache kernel launch");
    fence(v.keep, stream_of(*e, stream));
  });
}

int cg_ipcache_resolve_host(uint64_t h, uint32_t ipc_id, const uint32_t* v4, size_t n4,
                            cg_remote_endpoint_info* out4, const uint8_t* v6, size_t n6,
                            cg_remote_endpoint_info* out6) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    if ((n4 && (!v4 || !out4)) || (n6 && (!v6 || !out6))) fail(CG_INVALID_ARGUMENT, "NULL address/result arrays");
    const IpcView v = ipc_view(*e, ipc_id);
    host_pipeline(*e, n4, {{v4, 4}}, {{out4, 8}}, [&](void* const* din, void* const* dout, size_t cnt, void* st) {
      check_launch(launch_ipcache(v.dev, (const uint32_t*)din[0], cnt, (IpcVal*)dout[0], nullptr, 0, nullptr, st,
                                  e->cus),
                   "ipcache kernel launch");
    });
    host_pipeline(*e, n6, {{v6, 16}}, {{out6, 8}}, [&](void* const* din, void* const* dout, size_t cnt, void* st) {
      check_launch(launch_ipcache(v.dev, nullptr, 0, nullptr, (const uint8_t*)din[0], cnt, (IpcVal*)dout[0], st,
                                  e->cus),
                   "ipcache kernel launch");
    });
  });
}

// The ipcache tables walked on the host exactly as ipcache_kernel does.
int cg_diag_ipcache_eval_host(uint64_t h, uint32_t ipc_id, const uint32_t* v4, size_t n4,
                              cg_remote_endpoint_info* out4, const uint8_t* v6, size_t n6,
                              cg_remote_endpoint_info* out6) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    IpcacheState& p = get_ipc(*e, ipc_id);
    if (p.dirty) p.rebuild(*e);
    const IpcacheDev t = p.host_view();
    for (size_t i = 0; i < n4; ++i) {
      const uint64_t v = ipc_v4_value(t, __builtin_bswap32(v4[i]));
      out4[i] = cg_remote_endpoint_info{(uint32_t)v, (uint32_t)(v >> 32)};
    }
    for (size_t i = 0; i < n6; ++i) {
      uint64_t hi = 0, lo = 0;
      for (int k = 0; k < 8; ++k) hi = hi << 8 | v6[16 * i + k];
      for (int k = 8; k < 16; ++k) lo = lo << 8 | v6[16 * i + k];
      const uint32_t tb = (uint32_t)(hi >> (64 - t.v6_bits));
      uint32_t k, L, R;
      uint64_t v = kIpcMiss;
      if (ipc_v6_bucket(t.code6[tb >> 5], tb, &k)) {
        L = t.ent6[4 * (size_t)k];
        R = t.ent6[4 * (size_t)k + 1];
        const uint32_t crowd = t.ent6[4 * (size_t)k + 2];
        uint64_t xv;
        if (t.ent6[4 * (size_t)k + 3] && ipc_ex6_find(t, hi, lo, ipc_ex6_hash(hi, lo) & t.ex6_mask, &xv)) {
          v = xv;  // a /128 entry
        } else {
          v = t.runs6[4 * (size_t)R + 2];
          if (!le128(t.runs6[4 * (size_t)R], t.runs6[4 * (size_t)R + 1], hi, lo))
            v = ipc_v6_search_value(t, hi, lo, L, R, crowd);
        }
      }
      out6[i] = cg_remote_endpoint_info{(uint32_t)v, (uint32_t)(v >> 32)};
    }
  });
}

// ------------------------------------------------------- selector cache ----
// The published snapshot, copied under the handle lock and held for the call.
static std::shared_ptr<ScPublished> sc_pub(Engine& e, uint32_t sc_id) {
  std::lock_guard<std::mutex> lk(e.mu);
  SelcacheState& s = get_sc(e, sc_id);
  if (s.dirty || !s.pub) s.rebuild(e);
  return s.pub;
}

// The selector table of a match call: the caller's, interned against the
// snapshot's identities, or (sels == NULL) the rule set's.
static const ScSelTab& sc_table_of(const ScPublished& p, const cg_selector_table* sels, ScSelTab* own) {
  if (!sels) return p.seltab;
  *own = sc_compile_selectors(*p.idents, sc_parse_selectors(*sels));
  return *own;
}

static void sc_check_cap(const ScPublished& p, const ScSelTab& t, const void* bits, size_t cap_words) {
  const size_t need = t.sels.size() * (size_t)p.words;
  if (need && !bits) fail(CG_INVALID_ARGUMENT, "selcache match: NULL bits");
  if (cap_words < need) fail(CG_INVALID_ARGUMENT, "selcache match: bits holds fewer than S * W words");
}

int cg_selcache_create(uint64_t h, uint32_t* sc_id) {
  return guarded([&] {
    auto e = get(h);
    if (!sc_id) fail(CG_INVALID_ARGUMENT, "sc_id is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    const uint32_t id = e->next_id++;
    e->selcaches[id] = std::make_unique<SelcacheState>();
    *sc_id = id;
  });
}

int cg_selcache_destroy(uint64_t h, uint32_t sc_id) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    get_sc(*e, sc_id);
    if (e->has_gpu()) dev_sync(*e, nullptr);
    e->selcaches.erase(sc_id);
  });
}

int cg_selcache_set_identities(uint64_t h, uint32_t sc_id, const uint32_t* ids, size_t n, const uint32_t* label_off,
                               const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob,
                               const uint64_t* val_off) {
  return guarded([&] {
    auto e = get(h);
    auto snap = sc_compile_identities(ids, n, label_off, key_blob, key_off, val_blob, val_off);
    std::lock_guard<std::mutex> lk(e->mu);
    SelcacheState& s = get_sc(*e, sc_id);
    if ((uint64_t)n + s.cidrs->recs.size() > 0xFFFFFFC0ull) fail(CG_MAP_FULL, "selector cache: too many identities");
    s.idents = std::move(snap);
    s.dirty = true;
  });
}

int cg_selcache_set_cidr_identities(uint64_t h, uint32_t sc_id, const uint32_t* ids, const cg_cidr* prefixes,
                                    size_t n) {
  return guarded([&] {
    auto e = get(h);
    auto snap = sc_compile_cidrs(ids, prefixes, n);
    std::lock_guard<std::mutex> lk(e->mu);
    SelcacheState& s = get_sc(*e, sc_id);
    if ((uint64_t)s.idents->n + n > 0xFFFFFFC0ull) fail(CG_MAP_FULL, "selector cache: too many identities");
    s.cidrs = std::move(snap);
    s.dirty = true;
  });
}

int cg_selcache_set_rules(uint64_t h, uint32_t sc_id, const cg_selector_table* sels, const cg_selcache_rules* rules) {
  return guarded([&] {
    auto e = get(h);
    if (!sels || !rules) fail(CG_INVALID_ARGUMENT, "selcache rules: NULL tables");
    auto src = sc_parse_rules(*sels, *rules);
    std::lock_guard<std::mutex> lk(e->mu);
    SelcacheState& s = get_sc(*e, sc_id);
    s.rules = std::move(src);
    s.dirty = true;
  });
}

int cg_selcache_info(uint64_t h, uint32_t sc_id, size_t* n_identities, size_t* words, size_t* n_selectors,
                     size_t* n_rules) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    SelcacheState& s = get_sc(*e, sc_id);
    const size_t total = (size_t)s.idents->n + s.cidrs->recs.size();
    if (n_identities) *n_identities = total;
    if (words) *words = (total + 63) / 64;
    if (n_selectors) *n_selectors = s.rules->sels.size();
    if (n_rules) *n_rules = s.rules->n;
  });
}

// An ad-hoc selector table's device copy lives until the kernel reading it
// has finished: its DevTables fence waits when the last holder lets go.
static ScSelDev sc_upload_table(const ScSelTab& t, DevTables& tab) {
  return ScSelDev{tab.add(t.sels), tab.add(t.reqs), tab.add(t.vals), (uint32_t)t.sels.size(), tab.add(t.creqs)};
}

int cg_selcache_match_dev(uint64_t h, uint32_t sc_id, const cg_selector_table* sels, uint64_t* d_bits,
                          size_t cap_words, void* stream) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    const auto p = sc_pub(*e, sc_id);
    ScSelTab own;
    const ScSelTab& t = sc_table_of(*p, sels, &own);
    sc_check_cap(*p, t, d_bits, cap_words);
    e->set_device();
    void* st = stream_of(*e, stream);
    auto tmp = std::make_shared<DevTables>();
    const ScSelDev dT = sels ? sc_upload_table(t, *tmp) : p->dT;
    check_launch(launch_selcache_match(p->dI, dT, (unsigned long long*)d_bits, st, e->cus),
                 "selcache match kernel launch");
    fence(p->tab, st);
    if (sels) fence(tmp, st);
  });
}

int cg_selcache_match_host(uint64_t h, uint32_t sc_id, const cg_selector_table* sels, uint64_t* bits,
                           size_t cap_words) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    const auto p = sc_pub(*e, sc_id);
    ScSelTab own;
    const ScSelTab& t = sc_table_of(*p, sels, &own);
    sc_check_cap(*p, t, bits, cap_words);
    const size_t need = t.sels.size() * (size_t)p->words;
    if (!need) return;
    e->set_device();
    DevTables tmp;
    const ScSelDev dT = sels ? sc_upload_table(t, tmp) : p->dT;
    DevMem out;
    out.alloc(need * sizeof(uint64_t));
    check_launch(launch_selcache_match(p->dI, dT, out.as<unsigned long long>(), e->stream, e->cus),
                 "selcache match kernel launch");
    fence(p->tab, e->stream);
    dev_sync(*e, nullptr);
    hip_check(hipMemcpy(bits, out.get(), need * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
  });
}

int cg_selcache_reach_dev(uint64_t h, uint32_t sc_id, const uint32_t* d_endpoints, size_t n, uint64_t* d_ing,
                          uint64_t* d_eg, uint8_t* d_flags, void* stream) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    if (n && (!d_endpoints || !d_ing || !d_eg || !d_flags)) fail(CG_INVALID_ARGUMENT, "selcache reach: NULL arrays");
    const auto p = sc_pub(*e, sc_id);
    e->set_device();
    void* st = stream_of(*e, stream);
    check_launch(launch_selcache_reach(p->dR, p->n, p->words, d_endpoints, n,
                                       (unsigned long long*)d_ing, (unsigned long long*)d_eg, d_flags, st),
                 "selcache reach kernel launch");
    fence(p->tab, st);
  });
}

static void sc_check_endpoints(const ScPublished& p, const uint32_t* eps, size_t n, const void* ing, const void* eg,
                               const void* flags) {
  if (n && (!eps || !ing || !eg || !flags)) fail(CG_INVALID_ARGUMENT, "selcache reach: NULL arrays");
  for (size_t i = 0; i < n; ++i)
    if (eps[i] >= p.n) fail(CG_INVALID_ARGUMENT, "selcache reach: endpoint index outside the identity table");
}

int cg_selcache_reach_host(uint64_t h, uint32_t sc_id, const uint32_t* endpoints, size_t n, uint64_t* ing,
                           uint64_t* eg, uint8_t* flags) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    const auto p = sc_pub(*e, sc_id);
    sc_check_endpoints(*p, endpoints, n, ing, eg, flags);
    if (!n) return;
    e->set_device();
    const size_t W = p->words, row = n * W * sizeof(uint64_t);
    DevMem d_ep, d_ing, d_eg, d_fl;
    d_ep.upload(endpoints, n * sizeof(uint32_t));
    d_ing.alloc(row);
    d_eg.alloc(row);
    d_fl.alloc(n);
    check_launch(launch_selcache_reach(p->dR, p->n, p->words, d_ep.as<uint32_t>(), n,
                                       d_ing.as<unsigned long long>(), d_eg.as<unsigned long long>(),
                                       d_fl.as<uint8_t>(), e->stream),
                 "selcache reach kernel launch");
    fence(p->tab, e->stream);
    dev_sync(*e, nullptr);
    if (row) {
      hip_check(hipMemcpy(ing, d_ing.get(), row, hipMemcpyDeviceToHost), "hipMemcpy D2H");
      hip_check(hipMemcpy(eg, d_eg.get(), row, hipMemcpyDeviceToHost), "hipMemcpy D2H");
    }
    hip_check(hipMemcpy(flags, d_fl.get(), n, hipMemcpyDeviceToHost), "hipMemcpy D2H");
  });
}

// The compiled tables walked on the host, as the kernels walk them.
int cg_diag_selcache_match_host(uint64_t h, uint32_t sc_id, const cg_selector_table* sels, uint64_t* bits,
                                size_t cap_words, uint32_t threads) {
  return guarded([&] {
    auto e = get(h);
    const auto p = sc_pub(*e, sc_id);
    ScSelTab own;
    const ScSelTab& t = sc_table_of(*p, sels, &own);
    sc_check_cap(*p, t, bits, cap_words);
    sc_match_host(p->host_idents(), t.view(), bits, threads);
  });
}

// The rule selectors' matrix on the host, once per snapshot.
static void sc_ensure_host_m(Engine& e, ScPublished& p, uint32_t threads) {
  std::lock_guard<std::mutex> lk(e.mu);
  const size_t need = p.seltab.sels.size() * (size_t)p.words;
  if (p.host_m.size() != need || !need) {
    p.host_m.assign(std::max<size_t>(need, 1), 0);
    sc_match_host(p.host_idents(), p.seltab.view(), p.host_m.data(), threads);
    if (!need) p.host_m.resize(1);
  }
}

int cg_diag_selcache_reach_host(uint64_t h, uint32_t sc_id, const uint32_t* endpoints, size_t n, uint64_t* ing,
                                uint64_t* eg, uint8_t* flags, uint32_t threads) {
  return guarded([&] {
    auto e = get(h);
    const auto p = sc_pub(*e, sc_id);
    sc_check_endpoints(*p, endpoints, n, ing, eg, flags);
    sc_ensure_host_m(*e, *p, threads);
    sc_reach_host(p->host_rules(), p->n, p->words, endpoints, n, ing, eg, flags, threads);
  });
}

// ---- expansion into policy-map entries
static void sc_check_expand_out(const cg_expand_table* table, const void* row_off, const void* keys,
                                const void* proxy, size_t cap) {
  if (!table) fail(CG_INVALID_ARGUMENT, "selcache expand: NULL table");
  if (!row_off) fail(CG_INVALID_ARGUMENT, "selcache expand: NULL row_off");
  if (cap && (!keys || !proxy)) fail(CG_INVALID_ARGUMENT, "selcache expand: NULL keys/proxy");
  if (cap > (1ull << 40)) fail(CG_INVALID_ARGUMENT, "selcache expand: cap_entries out of range");
}

static ScExpDev sc_exp_view(const ScPublished& p, const ScExpRow* rows, const uint32_t* src_idx, size_t n_rows,
                            const uint32_t* ids, const uint64_t* src) {
  ScExpDev X{};
  X.rows = rows;
  X.src_idx = src_idx;
  X.ids = ids;
  X.src = reinterpret_cast<const unsigned long long*>(src);
  X.n_rows = (uint32_t)n_rows;
  X.n_ids = p.n;
  X.words = p.words;
  return X;
}

int cg_selcache_expand_dev(uint64_t h, uint32_t sc_id, const cg_expand_table* table, const uint64_t* d_src,
                           size_t src_rows, uint64_t* d_row_off, cg_policy_key* d_keys, uint16_t* d_proxy,
                           size_t cap_entries, uint64_t* d_total, void* stream) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    sc_check_expand_out(table, d_row_off, d_keys, d_proxy, cap_entries);
    if ((uintptr_t)d_keys & 7u) fail(CG_INVALID_ARGUMENT, "selcache expand: d_keys is not 8-byte aligned");
    const auto p = sc_pub(*e, sc_id);
    const ScExpTab t = sc_compile_expand(*table, src_rows);
    if (!t.src_idx.empty() && p->words && !d_src) fail(CG_INVALID_ARGUMENT, "selcache expand: NULL source matrix");
    e->set_device();
    void* st = stream_of(*e, stream);
    auto tmp = std::make_shared<DevTables>();
    const ScExpDev X = sc_exp_view(*p, tmp->add(t.rows), tmp->add(t.src_idx), t.rows.size(), p->d_ids, d_src);
    check_launch(launch_selcache_expand(X, (unsigned long long*)d_row_off, d_keys, d_proxy, cap_entries,
                                        (unsigned long long*)d_total, st, e->cus),
                 "selcache expand kernel launch");
    fence(p->tab, st);
    fence(tmp, st);
  });
}

// Rows, offsets and (when they fit) entries back to the host after the
// expansion queued on the handle's stream.
static void sc_expand_copy_back(Engine& e, size_t n_rows, const DevMem& d_off, const DevMem& d_keys,
                                const DevMem& d_proxy, uint64_t* row_off, cg_policy_key* keys, uint16_t* proxy,
                                size_t cap, uint64_t* total) {
  hipStream_t st = (hipStream_t)e.stream;
  hip_check(hipMemcpyAsync(row_off, d_off.get(), (n_rows + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st),
            "hipMemcpy D2H");
  dev_sync(e, nullptr);
  const uint64_t n = row_off[n_rows];
  if (total) *total = n;
  if (n && n <= cap) {
    hip_check(hipMemcpyAsync(keys, d_keys.get(), n * sizeof(cg_policy_key), hipMemcpyDeviceToHost, st), "hipMemcpy D2H");
    hip_check(hipMemcpyAsync(proxy, d_proxy.get(), n * sizeof(uint16_t), hipMemcpyDeviceToHost, st), "hipMemcpy D2H");
    dev_sync(e, nullptr);
  }
}

int cg_selcache_expand_host(uint64_t h, uint32_t sc_id, const cg_expand_table* table, const uint64_t* src,
                            size_t src_rows, uint64_t* row_off, cg_policy_key* keys, uint16_t* proxy,
                            size_t cap_entries, uint64_t* total) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    sc_check_expand_out(table, row_off, keys, proxy, cap_entries);
    const auto p = sc_pub(*e, sc_id);
    const ScExpTab t = sc_compile_expand(*table, src_rows);
    const size_t src_bytes = src_rows * (size_t)p->words * sizeof(uint64_t);
    if (src_bytes && !src) fail(CG_INVALID_ARGUMENT, "selcache expand: NULL source matrix");
    e->set_device();
    DevTables tmp;
    DevMem d_src, d_off, d_keys, d_proxy;
    d_src.upload(src, src_bytes);
    d_off.alloc((t.rows.size() + 1) * sizeof(uint64_t));
    d_keys.alloc(cap_entries * sizeof(cg_policy_key));
    d_proxy.alloc(cap_entries * sizeof(uint16_t));
    const ScExpDev X = sc_exp_view(*p, tmp.add(t.rows), tmp.add(t.src_idx), t.rows.size(), p->d_ids, d_src.as<uint64_t>());
    check_launch(launch_selcache_expand(X, d_off.as<unsigned long long>(), d_keys.get(), d_proxy.as<uint16_t>(),
                                        cap_entries, nullptr, e->stream, e->cus),
                 "selcache expand kernel launch");
    fence(p->tab, e->stream);
    sc_expand_copy_back(*e, t.rows.size(), d_off, d_keys, d_proxy, row_off, keys, proxy, cap_entries, total);
  });
}

static void sc_check_entries_args(const ScPublished& p, const uint32_t* eps, size_t n, const void* flags) {
  if (n && (!eps || !flags)) fail(CG_INVALID_ARGUMENT, "selcache entries: NULL endpoints/flags");
  if (n > 0x3FFFFFFFu) fail(CG_MAP_FULL, "selcache entries: too many endpoints");
  for (size_t i = 0; i < n; ++i)
    if (eps[i] >= p.n) fail(CG_INVALID_ARGUMENT, "selcache entries: endpoint index outside the identity table");
}

int cg_selcache_entries_host(uint64_t h, uint32_t sc_id, const cg_selector_table* sels, const uint32_t* endpoints,
                             size_t n_endpoints, const cg_expand_table* table, uint64_t* row_off,
                             cg_policy_key* keys, uint16_t* proxy, size_t cap_entries, uint64_t* total,
                             uint8_t* flags) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    sc_check_expand_out(table, row_off, keys, proxy, cap_entries);
    const auto p = sc_pub(*e, sc_id);
    sc_check_entries_args(*p, endpoints, n_endpoints, flags);
    ScSelTab own;
    if (sels) own = sc_compile_selectors(*p->idents, sc_parse_selectors(*sels));
    const size_t S = own.sels.size(), E = n_endpoints, W = p->words;
    const ScExpTab t = sc_compile_expand(*table, S + 2 * E);
    e->set_device();
    DevTables tmp;
    DevMem d_src, d_ep, d_fl, d_off, d_keys, d_proxy;
    d_src.alloc((S + 2 * E) * W * sizeof(uint64_t));
    d_off.alloc((t.rows.size() + 1) * sizeof(uint64_t));
    d_keys.alloc(cap_entries * sizeof(cg_policy_key));
    d_proxy.alloc(cap_entries * sizeof(uint16_t));
    unsigned long long* src = d_src.as<unsigned long long>();
    if (S)
      check_launch(launch_selcache_match(p->dI, sc_upload_table(own, tmp), src, e->stream, e->cus),
                   "selcache match kernel launch");
    if (E) {
      d_ep.upload(endpoints, E * sizeof(uint32_t));
      d_fl.alloc(E);
      check_launch(launch_selcache_reach(p->dR, p->n, p->words, d_ep.as<uint32_t>(), E, src + S * W,
                                         src + (S + E) * W, d_fl.as<uint8_t>(), e->stream),
                   "selcache reach kernel launch");
      hip_check(hipMemcpyAsync(flags, d_fl.get(), E, hipMemcpyDeviceToHost, (hipStream_t)e->stream), "hipMemcpy D2H");
    }
    const ScExpDev X = sc_exp_view(*p, tmp.add(t.rows), tmp.add(t.src_idx), t.rows.size(), p->d_ids, d_src.as<uint64_t>());
    check_launch(launch_selcache_expand(X, d_off.as<unsigned long long>(), d_keys.get(), d_proxy.as<uint16_t>(),
                                        cap_entries, nullptr, e->stream, e->cus),
                 "selcache expand kernel launch");
    fence(p->tab, e->stream);
    sc_expand_copy_back(*e, t.rows.size(), d_off, d_keys, d_proxy, row_off, keys, proxy, cap_entries, total);
  });
}

int cg_diag_selcache_expand_host(uint64_t h, uint32_t sc_id, const cg_expand_table* table, const uint64_t* src,
                                 size_t src_rows, uint64_t* row_off, cg_policy_key* keys, uint16_t* proxy,
                                 size_t cap_entries, uint64_t* total, uint32_t threads) {
  return guarded([&] {
    auto e = get(h);
    sc_check_expand_out(table, row_off, keys, proxy, cap_entries);
    const auto p = sc_pub(*e, sc_id);
    const ScExpTab t = sc_compile_expand(*table, src_rows);
    if (src_rows * (size_t)p->words && !src) fail(CG_INVALID_ARGUMENT, "selcache expand: NULL source matrix");
    uint64_t n = 0;
    sc_expand_host(sc_exp_view(*p, t.rows.data(), t.src_idx.data(), t.rows.size(), p->ids.data(), src),
                   row_off, keys, proxy, cap_entries, &n, threads);
    if (total) *total = n;
  });
}

int cg_diag_selcache_entries_host(uint64_t h, uint32_t sc_id, const cg_selector_table* sels,
                                  const uint32_t* endpoints, size_t n_endpoints, const cg_expand_table* table,
                                  uint64_t* row_off, cg_policy_key* keys, uint16_t* proxy, size_t cap_entries,
                                  uint64_t* total, uint8_t* flags, uint32_t threads) {
  return guarded([&] {
    auto e = get(h);
    sc_check_expand_out(table, row_off, keys, proxy, cap_entries);
    const auto p = sc_pub(*e, sc_id);
    sc_check_entries_args(*p, endpoints, n_endpoints, flags);
    ScSelTab own;
    if (sels) own = sc_compile_selectors(*p->idents, sc_parse_selectors(*sels));
    const size_t S = own.sels.size(), E = n_endpoints, W = p->words;
    const ScExpTab t = sc_compile_expand(*table, S + 2 * E);
    std::vector<uint64_t> src(std::max<size_t>((S + 2 * E) * W, 1), 0);
    if (S) sc_match_host(p->host_idents(), own.view(), src.data(), threads);
    if (E) {
      sc_ensure_host_m(*e, *p, threads);
      sc_reach_host(p->host_rules(), p->n, p->words, endpoints, E, src.data() + S * W,
                    src.data() + (S + E) * W, flags, threads);
    }
    uint64_t n = 0;
    sc_expand_host(sc_exp_view(*p, t.rows.data(), t.src_idx.data(), t.rows.size(), p->ids.data(), src.data()),
                   row_off, keys, proxy, cap_entries, &n, threads);
    if (total) *total = n;
  });
}

// ---------------------------------------------------------------- HTTP ----
int cg_http_policy_update(uint64_t h, const char* json, size_t len) {
  return guarded([&] {
    auto e = get(h);
    if (!json) fail(CG_INVALID_ARGUMENT, "NULL policy");
    std::shared_ptr<HttpSnapshot> snap = http_compile(json, len);
    if (e->has_gpu()) {
      e->set_device();
      snap->upload(*e);
    }
    {
      std::lock_guard<std::mutex> lk(e->mu);
      e->http = snap;  // publish
    }
    bump_epoch();
  });
}

int cg_http_policy_update_npds(uint64_t h, const uint8_t* resp, size_t len) {
  std::string json;
  const int rc = guarded([&] {
    if (!resp && len) fail(CG_INVALID_ARGUMENT, "NULL DiscoveryResponse");
    json = npds_pb_to_json(resp, len, true);  // Envoy: proto3 strings must be UTF-8
  });
  if (rc != CG_OK) return rc;
  return cg_http_policy_update(h, json.data(), json.size());
}

static std::shared_ptr<HttpSnapshot> http_snap(Engine& e);

int cg_http_policy_export(uint64_t h, void* buf, size_t cap, size_t* len) {
  return guarded([&] {
    auto e = get(h);
    const std::vector<uint8_t> img = http_image_export(*http_snap(*e));
    if (len) *len = img.size();
    if (buf && cap >= img.size()) memcpy(buf, img.data(), img.size());
    else if (buf) fail(CG_INVALID_ARGUMENT, "policy image buffer too small");
  });
}

int cg_http_policy_import(uint64_t h, const void* buf, size_t len) {
  return guarded([&] {
    auto e = get(h);
    std::shared_ptr<HttpSnapshot> snap = http_image_import(static_cast<const uint8_t*>(buf), len);
    if (e->has_gpu()) {
      e->set_device();
      snap->upload(*e);
    }
    {
      std::lock_guard<std::mutex> lk(e->mu);
      e->http = snap;  // publish
    }
    bump_epoch();
  });
}

static std::shared_ptr<HttpSnapshot> http_snap(Engine& e) {
  std::lock_guard<std::mutex> lk(e.mu);
  if (!e.http) fail(CG_NOT_FOUND, "no HTTP policy installed");
  return e.http;
}

int cg_http_policy_index(uint64_t h, const char* name, uint32_t* index) {
  return guarded([&] {
    auto e = get(h);
    auto s = http_snap(*e);
    auto it = s->policy_index.find(name ? name : "");
    if (it == s->policy_index.end()) fail(CG_NOT_FOUND, "no policy named " + std::string(name ? name : ""));
    *index = it->second;
  });
}

int cg_http_rule_info_get(uint64_t h, cg_http_rule_info* out, size_t cap, size_t* n) {
  return guarded([&] {
    auto e = get(h);
    auto s = http_snap(*e);
    if (n) *n = s->rule_info.size();
    if (out) memcpy(out, s->rule_info.data(), std::min(cap, s->rule_info.size()) * sizeof(cg_http_rule_info));
  });
}

int cg_http_policy_stats(uint64_t h, uint64_t* out, size_t n) {
  return guarded([&] {
    auto e = get(h);
    auto s = http_snap(*e);
    uint64_t max_prog_cells = 0, lds_progs = 0;
    for (const auto& pg : s->progs) {
      if (pg.flags & kProgAllowAll) continue;
      max_prog_cells = std::max<uint64_t>(max_prog_cells, pg.cell_count);
      lds_progs += (pg.flags & kProgRebased) && pg.cell_count <= kMaxLdsCells;
    }
    uint64_t v[14] = {s->progs.size(),
                     s->parts.size(),
                     s->total_states,
                     s->cells.size() * 4,
                     s->fields.size(),
                     s->total_rules,
                     s->npolicies,
                     s->total_remote_slots,
                     s->total_exceptions,
                     s->cells.size(),
                     max_prog_cells,
                     lds_progs,
                     s->total_tokens,
                     s->total_token_cells};
    for (size_t i = 0; i < n && i < 14; ++i) out[i] = v[i];
  });
}

int cg_diag_http_tokens(uint64_t h, uint32_t prog, uint8_t* code_map, uint8_t* out, size_t cap, size_t* used) {
  return guarded([&] {
    auto e = get(h);
    auto s = http_snap(*e);
    if (prog >= s->progs.size()) fail(CG_INVALID_ARGUMENT, "no such HTTP program");
    const bool cls = s->progs[prog].flags & kProgClass;
    if (code_map)
      for (int b = 0; b < 256; ++b) code_map[b] = cls ? s->prog_code[prog][b] : (uint8_t)b;
    size_t at = 0;
    for (const auto& t : s->prog_tokens[prog]) {
      if (out && at + 2 + t.seq.size() <= cap) {
        out[at] = t.code;
        out[at + 1] = (uint8_t)t.seq.size();
        memcpy(out + at + 2, t.seq.data(), t.seq.size());
      }
      at += 2 + t.seq.size();
    }
    if (used) *used = at;
  });
}

size_t cg_http_batch_bytes(uint64_t h, size_t n) {
  size_t v = 0;
  guarded([&] {
    auto e = get(h);
    v = http_batch_bytes(*http_snap(*e), n);
  });
  return v;
}

size_t cg_http_batch_slots(uint64_t h, size_t n) {
  size_t v = 0;
  guarded([&] {
    auto e = get(h);
    v = http_batch_slots(*http_snap(*e), n);
  });
  return v;
}

int cg_http_pack(uint64_t h, size_t n, const uint32_t* policy, const uint8_t* ingress, const uint16_t* port,
                 const uint32_t* remote, const uint8_t* hdr_blob, const uint64_t* hdr_off, void* batch,
                 size_t batch_cap, uint32_t* order, size_t* nslots, uint8_t* arena, size_t arena_cap,
                 size_t* arena_used) {
  return guarded([&] {
    auto e = get(h);
    auto s = http_snap(*e);
    http_pack(*s, n, policy, ingress, port, remote, hdr_blob, hdr_off, batch, batch_cap, order, nslots, arena,
              arena_cap, arena_used);
  });
}

static size_t batch_used_bytes(const void* batch) {
  HttpBatchHeader hdr;
  memcpy(&hdr, batch, sizeof(hdr));
  if (hdr.magic != kBatchMagic) fail(CG_INVALID_ARGUMENT, "not a packed HTTP batch");
  return hdr.total_bytes;
}

int cg_http_verdicts_dev(uint64_t h, const void* d_batch, size_t nslots, const uint8_t* d_arena, uint8_t* d_out,
                         void* stream) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    auto s = http_snap(*e);
    e->set_device();
    check_launch(launch_http(s->dev, d_batch, nslots, d_arena, d_out, stream_of(*e, stream), e->cus),
                 "http kernel launch");
    s->fence.record(stream_of(*e, stream));
  });
}

int cg_http_verdicts_rules_dev(uint64_t h, const void* d_batch, size_t nslots, const uint8_t* d_arena, uint8_t* d_out,
                               uint32_t* d_rule, void* stream) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    auto s = http_snap(*e);
    if (nslots && !d_rule) fail(CG_INVALID_ARGUMENT, "NULL rule array");
    e->set_device();
    check_launch(launch_http(s->dev, d_batch, nslots, d_arena, d_out, stream_of(*e, stream), e->cus, nullptr, d_rule),
                 "http kernel launch");
    s->fence.record(stream_of(*e, stream));
  });
}

int cg_http_verdicts_raw_dev(uint64_t h, const uint8_t* d_raw, const uint64_t* d_raw_off, size_t n,
                             const uint32_t* d_policy, const uint8_t* d_ingress, const uint16_t* d_port,
                             const uint32_t* d_remote, uint8_t* d_out, void* stream) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    auto s = http_snap(*e);
    if (n && (!d_raw_off || !d_policy || !d_ingress || !d_port || !d_remote || !d_out))
      fail(CG_INVALID_ARGUMENT, "NULL device array");
    e->set_device();
    auto lease = e->staging.acquire(e->device);
    http_verdicts_raw_on(*s, *lease, e->cus, RawInput::Heads, d_raw, d_raw_off, n, d_policy, d_ingress, d_port,
                         d_remote, d_out, stream_of(*e, stream));
    // the device-layout sequence returns with its kernels still queued on
    // the stream, reading the snapshot's tables: keep the snapshot alive
    s->fence.record(stream_of(*e, stream));
    // no stream given: the handle's, waited for (a caller that wants the
    // call asynchronous names its stream)
    if (!stream) hip_check(hipStreamSynchronize((hipStream_t)stream_of(*e, stream)), "hipStreamSynchronize");
  });
}

int cg_http_verdicts_fields_dev(uint64_t h, const uint8_t* d_hdr_blob, const uint64_t* d_hdr_off, size_t n,
                                const uint32_t* d_policy, const uint8_t* d_ingress, const uint16_t* d_port,
                                const uint32_t* d_remote, uint8_t* d_out, void* stream) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    auto s = http_snap(*e);
    if (n && (!d_hdr_off || !d_policy || !d_ingress || !d_port || !d_remote || !d_out))
      fail(CG_INVALID_ARGUMENT, "NULL device array");
    e->set_device();
    auto lease = e->staging.acquire(e->device);
    http_verdicts_raw_on(*s, *lease, e->cus, RawInput::Lists, d_hdr_blob, d_hdr_off, n, d_policy, d_ingress, d_port,
                         d_remote, d_out, stream_of(*e, stream));
    s->fence.record(stream_of(*e, stream));  // as cg_http_verdicts_raw_dev
    if (!stream) hip_check(hipStreamSynchronize((hipStream_t)stream_of(*e, stream)), "hipStreamSynchronize");
  });
}

// Copy a host array into the lease's pinned buffer i and DMA it to its
// device buffer i (async on the lease's stream).
static void* stage_in(StagingSlot& sl, int i, const void* src, size_t bytes) {
  void* d = sl.dev_buf(i, bytes);
  if (!bytes) return d;
  void* hb = sl.host_buf(i, bytes);
  memcpy(hb, src, bytes);
  hip_check(hipMemcpyAsync(d, hb, bytes, hipMemcpyHostToDevice, (hipStream_t)sl.stream), "H2D");
  return d;
}

static void http_verdicts_host_impl(uint64_t h, const void* batch, size_t nslots, const uint32_t* order,
                                    size_t n, const uint8_t* arena, size_t arena_len, uint8_t* out, uint32_t* rule);

int cg_http_verdicts_host(uint64_t h, const void* batch, size_t nslots, const uint32_t* order, size_t n,
                          const uint8_t* arena, size_t arena_len, uint8_t* out) {
  return guarded([&] { http_verdicts_host_impl(h, batch, nslots, order, n, arena, arena_len, out, nullptr); });
}

int cg_http_verdicts_rules_host(uint64_t h, const void* batch, size_t nslots, const uint32_t* order, size_t n,
                                const uint8_t* arena, size_t arena_len, uint8_t* out, uint32_t* rule) {
  return guarded([&] {
    if (n && !rule) fail(CG_INVALID_ARGUMENT, "NULL rule array");
    http_verdicts_host_impl(h, batch, nslots, order, n, arena, arena_len, out, rule);
  });
}

static void http_verdicts_host_impl(uint64_t h, const void* batch, size_t nslots, const uint32_t* order,
                                    size_t n, const uint8_t* arena, size_t arena_len, uint8_t* out, uint32_t* rule) {
  {
    auto e = get(h);
    e->require_gpu();
    auto s = http_snap(*e);
    if (!batch || (n && (!order || !out))) fail(CG_INVALID_ARGUMENT, "NULL batch/order/out");
    HttpBatchHeader hdr;
    memcpy(&hdr, batch, sizeof(hdr));
    if (hdr.magic != kBatchMagic || hdr.epoch != s->epoch)
      fail(CG_INVALID_ARGUMENT, "batch was packed against another policy snapshot");
    if (hdr.nslots != nslots) fail(CG_INVALID_ARGUMENT, "nslots differs from the packed batch");
    if (hdr.arena_bytes && (!arena || arena_len < hdr.arena_bytes))
      fail(CG_INVALID_ARGUMENT, "overflow arena shorter than the packed batch needs");
    e->set_device();
    auto lease = e->staging.acquire(e->device);
    void* dr = stage_in(*lease, 0, batch, batch_used_bytes(batch));
    void* da = stage_in(*lease, 1, arena, hdr.arena_bytes);
    void* dout = lease->dev_buf(2, nslots + 1);
    uint32_t* drule = rule ? (uint32_t*)lease->dev_buf(3, (nslots + 1) * 4) : nullptr;
    check_launch(launch_http(s->dev, dr, nslots, (const uint8_t*)da, (uint8_t*)dout, lease->stream, e->cus, nullptr,
                             drule),
                 "http kernel launch");
    uint8_t* slots = (uint8_t*)lease->host_buf(2, nslots + 1);
    uint32_t* rslots = rule ? (uint32_t*)lease->host_buf(3, (nslots + 1) * 4) : nullptr;
    if (nslots)
      hip_check(hipMemcpyAsync(slots, dout, nslots, hipMemcpyDeviceToHost, (hipStream_t)lease->stream), "D2H");
    if (nslots && rule)
      hip_check(hipMemcpyAsync(rslots, drule, nslots * 4, hipMemcpyDeviceToHost, (hipStream_t)lease->stream), "D2H");
    hip_check(hipStreamSynchronize((hipStream_t)lease->stream), "hipStreamSynchronize");
    for (size_t i = 0; i < nslots; ++i)
      if (order[i] < n) {
        out[order[i]] = slots[i];
        if (rule) rule[order[i]] = rslots[i];
      }
  }
}

// --------------------------------------------------------------- Kafka ----
int cg_kafka_policy_update(uint64_t h, const char* json, size_t len) {
  return guarded([&] {
    auto e = get(h);
    if (!json) fail(CG_INVALID_ARGUMENT, "NULL policy");
    auto snap = kafka_compile(json, len);
    if (e->has_gpu()) {
      e->set_device();
      snap->upload(*e);
    }
    std::lock_guard<std::mutex> lk(e->mu);
    e->kafka = snap;
  });
}

static std::shared_ptr<KafkaSnapshot> kafka_snap(Engine& e) {
  std::lock_guard<std::mutex> lk(e.mu);
  if (!e.kafka) fail(CG_NOT_FOUND, "no Kafka policy installed");
  return e.kafka;
}

int cg_kafka_policy_index(uint64_t h, const char* name, uint32_t* index) {
  return guarded([&] {
    auto e = get(h);
    auto s = kafka_snap(*e);
    auto it = s->redirect_index.find(name ? name : "");
    if (it == s->redirect_index.end()) fail(CG_NOT_FOUND, "no Kafka redirect named " + std::string(name ? name : ""));
    *index = it->second;
  });
}

int cg_kafka_intern(uint64_t h, uint32_t what, const char* str, size_t len, uint32_t* id) {
  return guarded([&] {
    auto e = get(h);
    auto s = kafka_snap(*e);
    const auto& m = what == 0 ? s->topic_ids : s->client_ids;
    auto it = m.find(std::string(str ? str : "", len));
    *id = it == m.end() ? CG_KAFKA_UNKNOWN_STR : it->second;
  });
}

int cg_kafka_verdicts_dev(uint64_t h, const cg_kafka_request* d_reqs, size_t n, const uint32_t* d_arena,
                          uint8_t* d_out, void* stream) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    auto s = kafka_snap(*e);
    e->set_device();
    check_launch(launch_kafka(s->dev, d_reqs, n, d_arena, d_out, stream_of(*e, stream), e->cus),
                 "kafka kernel launch");
    s->fence.record(stream_of(*e, stream));
  });
}

int cg_kafka_verdicts_split_dev(uint64_t h, const cg_kafka_request_head* d_heads, const uint32_t* d_topics,
                                size_t n, const uint32_t* d_arena, uint8_t* d_out, void* stream) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    auto s = kafka_snap(*e);
    if (n && (!d_heads || !d_topics || !d_out)) fail(CG_INVALID_ARGUMENT, "NULL heads/topics/out");
    e->set_device();
    check_launch(launch_kafka(s->dev, d_heads, n, d_arena, d_out, stream_of(*e, stream), e->cus, d_topics),
                 "kafka kernel launch");
    s->fence.record(stream_of(*e, stream));
  });
}

int cg_kafka_verdicts_host(uint64_t h, const cg_kafka_request* reqs, size_t n, const uint32_t* arena,
                           size_t arena_len, uint8_t* out) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    auto s = kafka_snap(*e);
    if (n && (!reqs || !out)) fail(CG_INVALID_ARGUMENT, "NULL requests/out");
    e->set_device();
    // the topic arena is shared by every chunk: one copy on its own lease
    auto lease = e->staging.acquire(e->device);
    const uint32_t* da = (const uint32_t*)stage_in(*lease, 0, arena, arena ? arena_len * 4 : 0);
    hip_check(hipStreamSynchronize((hipStream_t)lease->stream), "hipStreamSynchronize");
    host_pipeline(*e, n, {{reqs, sizeof(cg_kafka_request)}}, {{out, 1}},
                  [&](void* const* din, void* const* dout, size_t cnt, void* st) {
                    check_launch(launch_kafka(s->dev, din[0], cnt, da, (uint8_t*)dout[0], st, e->cus),
                                 "kafka kernel launch");
                  });
  });
}

// ------------------------------------------------------- Kafka decode ----
// The GPU decode of n staged requests on `st`, then the host decode of the
// requests the device deferred (gzip / snappy message payloads): their bytes
// come back, kafka_decode_host_one rewrites their record and status, and
// their long topic lists go after the device's arena entries.  Returns the
// arena entries used (may exceed arena_cap: nothing written beyond it).
static size_t kafka_decode_on(Engine& e, const KafkaSnapshot& s, StagingSlot& sl, const uint8_t* d_raw,
                              const uint64_t* d_off, size_t n, const uint16_t* d_red, const uint32_t* d_rem,
                              cg_kafka_request* d_reqs, uint32_t* d_arena, size_t arena_cap, uint8_t* d_status,
                              hipStream_t st) {
  // counters: topic arena entries, requests the decode kernel deferred,
  // inflate bytes reserved, payloads inflated on the device, requests the
  // inflate kernel deferred (to the host), payloads it deferred without a
  // reservation (arena full, impossible size)
  auto* ctr = (unsigned long long*)sl.dev_buf(7, 48);
  hip_check(hipMemsetAsync(ctr, 0, 48, st), "hipMemsetAsync");
  // the decode kernel's deferred requests (compressed sets) and the
  // payloads' decoded bytes (grow-only; a payload past it goes to the host)
  auto* dlist = (uint32_t*)sl.dev_buf(28, n * 4);
  uint8_t* zarena = (uint8_t*)sl.dev_buf(27, kKafkaInflateArena);
  check_launch(launch_kafka_decode(s.ddict[0], s.ddict[1], d_raw, d_off, n, d_red, d_rem, d_reqs, d_arena,
                                   arena_cap, ctr, d_status, st, e.cus, dlist, zarena, kKafkaInflateArena),
               "kafka decode kernel launch");
  auto* hc = (unsigned long long*)sl.host_buf(7, 48);
  hip_check(hipMemcpyAsync(hc, ctr, 48, hipMemcpyDeviceToHost, st), "D2H");
  hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  size_t used = (size_t)hc[0];
  e.kafka_inflated.fetch_add(hc[3]);
  e.kafka_deferred.fetch_add(hc[4]);
  e.kafka_arena_full.fetch_add(hc[5]);
  if (hc[4] == 0) return used;
  std::vector<uint8_t> status(n);
  std::vector<uint64_t> off(n + 1);
  hip_check(hipMemcpy(status.data(), d_status, n, hipMemcpyDeviceToHost), "D2H");
  hip_check(hipMemcpy(off.data(), d_off, (n + 1) * 8, hipMemcpyDeviceToHost), "D2H");
  std::vector<uint8_t> bytes;
  std::vector<uint32_t> spill;
  for (size_t i = 0; i < n; ++i) {
    if (status[i] != 2) continue;  // kKwDefer
    const uint64_t len = off[i + 1] > off[i] ? off[i + 1] - off[i] : 0;
    bytes.resize(len);
    if (len) hip_check(hipMemcpy(bytes.data(), d_raw + off[i], len, hipMemcpyDeviceToHost), "D2H");
    cg_kafka_request q;
    hip_check(hipMemcpy(&q, d_reqs + i, sizeof(q), hipMemcpyDeviceToHost), "D2H");
    const size_t base = spill.size();
    const uint8_t rc = kafka_decode_host_one(s, bytes.data(), len, q.policy, q.remote, &q, &spill);
    if (rc == CG_KAFKA_DECODE_OK && q.n_topics > CG_KAFKA_MAX_TOPICS) q.topic_ids[0] = (uint32_t)(used + base);
    hip_check(hipMemcpy(d_reqs + i, &q, sizeof(q), hipMemcpyHostToDevice), "H2D");
    hip_check(hipMemcpy(d_status + i, &rc, 1, hipMemcpyHostToDevice), "H2D");
  }
  if (!spill.empty() && used + spill.size() <= arena_cap)
    hip_check(hipMemcpy(d_arena + used, spill.data(), spill.size() * 4, hipMemcpyHostToDevice), "H2D");
  return used + spill.size();
}

static void check_offsets(const uint64_t* off, size_t n) {
  if (!off) fail(CG_INVALID_ARGUMENT, "NULL raw_off");
  for (size_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) fail(CG_INVALID_ARGUMENT, "raw_off must be non-decreasing");
}

int cg_kafka_decode_stats(uint64_t h, uint64_t* device_inflated, uint64_t* host_deferred) {
  return guarded([&] {
    auto e = get(h);
    if (device_inflated) *device_inflated = e->kafka_inflated.load();
    if (host_deferred) *host_deferred = e->kafka_deferred.load();
  });
}

int cg_kafka_inflate_stats(uint64_t h, uint64_t* unreserved) {
  return guarded([&] {
    auto e = get(h);
    if (unreserved) *unreserved = e->kafka_arena_full.load();
  });
}

int cg_kafka_decode_dev(uint64_t h, const uint8_t* d_raw, const uint64_t* d_raw_off, size_t n,
                        const uint16_t* d_redirect, const uint32_t* d_remote, cg_kafka_request* d_reqs,
                        uint32_t* d_arena, size_t arena_cap, size_t* arena_used, uint8_t* d_status, void* stream) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    auto s = kafka_snap(*e);
    if (!arena_used) fail(CG_INVALID_ARGUMENT, "NULL arena_used");
    *arena_used = 0;
    if (!n) return;
    e->set_device();
    auto lease = e->staging.acquire(e->device);
    const size_t used = kafka_decode_on(*e, *s, *lease, d_raw, d_raw_off, n, d_redirect, d_remote, d_reqs, d_arena,
                                        d_arena ? arena_cap : 0, d_status, (hipStream_t)stream_of(*e, stream));
    *arena_used = used;
    if (used > (d_arena ? arena_cap : 0)) fail(CG_MAP_FULL, "Kafka topic arena too small");
  });
}

// Stage raw requests, offsets, redirects and remotes on a lease (buffers
// 0..3) and decode them into lease buffers 4 (records), 5 (statuses), 6 (arena).
struct KafkaStaged {
  cg_kafka_request* reqs;
  uint8_t* status;
  uint32_t* arena;
  size_t used;
};
static KafkaStaged kafka_stage_decode(Engine& e, const KafkaSnapshot& s, StagingSlot& sl, const uint8_t* raw,
                                      const uint64_t* raw_off, size_t n, const uint16_t* redirect,
                                      const uint32_t* remote, size_t arena_cap) {
  check_offsets(raw_off, n);
  if (!redirect || !remote || (raw_off[n] && !raw)) fail(CG_INVALID_ARGUMENT, "NULL raw/redirect/remote");
  const auto st = (hipStream_t)sl.stream;
  const uint8_t* d_raw = (const uint8_t*)stage_in(sl, 0, raw, raw_off[n]);
  const uint64_t* d_off = (const uint64_t*)stage_in(sl, 1, raw_off, (n + 1) * 8);
  const uint16_t* d_red = (const uint16_t*)stage_in(sl, 2, redirect, n * 2);
  const uint32_t* d_rem = (const uint32_t*)stage_in(sl, 3, remote, n * 4);
  KafkaStaged k;
  k.reqs = (cg_kafka_request*)sl.dev_buf(4, n * sizeof(cg_kafka_request));
  k.status = (uint8_t*)sl.dev_buf(5, n);
  k.arena = (uint32_t*)sl.dev_buf(6, std::max<size_t>(arena_cap, 1) * 4);
  k.used = kafka_decode_on(e, s, sl, d_raw, d_off, n, d_red, d_rem, k.reqs, k.arena, arena_cap, k.status, st);
  return k;
}

int cg_kafka_decode_host(uint64_t h, const uint8_t* raw, const uint64_t* raw_off, size_t n, const uint16_t* redirect,
                         const uint32_t* remote, cg_kafka_request* reqs, uint32_t* arena, size_t arena_cap,
                         size_t* arena_used, uint8_t* status) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    auto s = kafka_snap(*e);
    if (!arena_used || (n && (!reqs || !status))) fail(CG_INVALID_ARGUMENT, "NULL reqs/status/arena_used");
    *arena_used = 0;
    if (!n) return;
    if (!arena) arena_cap = 0;
    e->set_device();
    auto lease = e->staging.acquire(e->device);
    const KafkaStaged k = kafka_stage_decode(*e, *s, *lease, raw, raw_off, n, redirect, remote, arena_cap);
    *arena_used = k.used;
    if (k.used > arena_cap) fail(CG_MAP_FULL, "Kafka topic arena too small");
    const auto st = (hipStream_t)lease->stream;
    hip_check(hipMemcpyAsync(reqs, k.reqs, n * sizeof(cg_kafka_request), hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipMemcpyAsync(status, k.status, n, hipMemcpyDeviceToHost, st), "D2H");
    if (k.used) hip_check(hipMemcpyAsync(arena, k.arena, k.used * 4, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  });
}

int cg_kafka_verdicts_raw_host(uint64_t h, const uint8_t* raw, const uint64_t* raw_off, size_t n,
                               const uint16_t* redirect, const uint32_t* remote, uint8_t* out) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    auto s = kafka_snap(*e);
    if (n && !out) fail(CG_INVALID_ARGUMENT, "NULL out");
    if (!n) return;
    check_offsets(raw_off, n);
    e->set_device();
    auto lease = e->staging.acquire(e->device);
    // a request's topic list needs at least 2 bytes per topic
    const size_t cap = (size_t)(raw_off[n] - raw_off[0]) / 2 + 16;
    const KafkaStaged k = kafka_stage_decode(*e, *s, *lease, raw, raw_off, n, redirect, remote, cap);
    if (k.used > cap) fail(CG_UNKNOWN_ERROR, "Kafka topic arena bound exceeded");
    const auto st = (hipStream_t)lease->stream;
    uint8_t* d_v = (uint8_t*)lease->dev_buf(0, n + 16);  // the raw bytes are no longer needed
    check_launch(launch_kafka(s->dev, k.reqs, n, k.arena, d_v, st, e->cus), "kafka kernel launch");
    uint8_t* hv = (uint8_t*)lease->host_buf(4, 2 * n);
    hip_check(hipMemcpyAsync(hv, d_v, n, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipMemcpyAsync(hv + n, k.status, n, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
    for (size_t i = 0; i < n; ++i) out[i] = hv[n + i] == CG_KAFKA_DECODE_OK ? hv[i] : CG_KAFKA_V_CLOSE;
  });
}

// Requests from host memory through the device path.  A large call runs in
// chunks of ~kHostChunkBytes on two workers, each with its own lease
// (pinned buffers + stream): while one worker copies its chunk into pinned
// memory (several threads) the other's chunk is on the bus or the GPU.
// 32 MiB: 0.351 / 0.340 G requests/s on config 5's 8M header lists against
// 0.299 / 0.331 at 160 MiB and 0.280 / 0.262 at 16 (profiles/r05aa_host_chunks.txt)
constexpr size_t kHostChunkBytes = (size_t)32 << 20;

static void run_host_chunk(const HttpSnapshot& s, Engine& e, StagingSlot& sl, RawInput in, const uint8_t* raw,
                           const uint64_t* raw_off, size_t a, size_t b, const uint32_t* policy,
                           const uint8_t* ingress, const uint16_t* port, const uint32_t* remote, uint8_t* out,
                           unsigned copy_threads) {
  const size_t m = b - a;
  const uint64_t base = raw_off[a], bytes = raw_off[b] - base;
  const auto st = (hipStream_t)sl.stream;
  uint8_t* h_raw = (uint8_t*)sl.host_buf(0, bytes);
  uint64_t* h_off = (uint64_t*)sl.host_buf(1, (m + 1) * 8);
  uint32_t* h_pol = (uint32_t*)sl.host_buf(2, m * 4);
  uint8_t* h_ing = (uint8_t*)sl.host_buf(3, m);
  uint16_t* h_port = (uint16_t*)sl.host_buf(4, m * 2);
  uint32_t* h_rem = (uint32_t*)sl.host_buf(5, m * 4);
  // the copies, split over threads by request ranges
  auto copy = [&](size_t i0, size_t i1) {
    const uint64_t b0 = raw_off[a + i0] - base, b1 = raw_off[a + i1] - base;
    if (b1 > b0) memcpy(h_raw + b0, raw + base + b0, b1 - b0);
    for (size_t i = i0; i < i1; ++i) h_off[i] = raw_off[a + i] - base;  // rebased to the staged bytes
    memcpy(h_pol + i0, policy + a + i0, (i1 - i0) * 4);
    memcpy(h_ing + i0, ingress + a + i0, i1 - i0);
    memcpy(h_port + i0, port + a + i0, (i1 - i0) * 2);
    memcpy(h_rem + i0, remote + a + i0, (i1 - i0) * 4);
  };
  const unsigned nt = m < 65536 ? 1u : copy_threads;
  if (nt <= 1) {
    copy(0, m);
  } else {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back(copy, m * t / nt, m * (t + 1) / nt);
    for (auto& x : th) x.join();
  }
  h_off[m] = bytes;
  auto h2d = [&](int i, const void* hsrc, size_t nb) {
    void* d = sl.dev_buf(i, nb);
    if (nb) hip_check(hipMemcpyAsync(d, hsrc, nb, hipMemcpyHostToDevice, st), "H2D");
    return d;
  };
  const uint8_t* d_raw = (const uint8_t*)h2d(0, h_raw, bytes);
  const uint64_t* d_off = (const uint64_t*)h2d(1, h_off, (m + 1) * 8);
  const uint32_t* d_pol = (const uint32_t*)h2d(2, h_pol, m * 4);
  const uint8_t* d_ing = (const uint8_t*)h2d(3, h_ing, m);
  const uint16_t* d_port = (const uint16_t*)h2d(4, h_port, m * 2);
  const uint32_t* d_rem = (const uint32_t*)h2d(5, h_rem, m * 4);
  uint8_t* d_out = (uint8_t*)sl.dev_buf(6, m);
  http_verdicts_raw_on(s, sl, e.cus, in, d_raw, d_off, m, d_pol, d_ing, d_port, d_rem, d_out, st);
  uint8_t* ho = (uint8_t*)sl.host_buf(6, m);
  hip_check(hipMemcpyAsync(ho, d_out, m, hipMemcpyDeviceToHost, st), "D2H");
  hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  memcpy(out + a, ho, m);
}

static void verdicts_raw_from_host(uint64_t h, RawInput in, const uint8_t* raw, const uint64_t* raw_off, size_t n,
                                   const uint32_t* policy, const uint8_t* ingress, const uint16_t* port,
                                   const uint32_t* remote, uint8_t* out) {
  auto e = get(h);
  e->require_gpu();
  auto s = http_snap(*e);
  if (!n) return;
  check_offsets(raw_off, n);
  if (!policy || !ingress || !port || !remote || !out || (raw_off[n] != raw_off[0] && !raw))
    fail(CG_INVALID_ARGUMENT, "NULL raw/policy/ingress/port/remote/out");
  if (in == RawInput::Lists)  // the 16-bit value spans (the device path would deny it)
    for (size_t i = 0; i < n; ++i)
      if (raw_off[i + 1] - raw_off[i] > 0xFFFFu) fail(CG_INVALID_ARGUMENT, "header list longer than 64 KiB");
  const uint64_t total = raw_off[n] - raw_off[0] + 19 * (uint64_t)n;
  // (CILIUM_GPU_HOST_CHUNK_MB: another chunk size, for measurements)
  size_t chunk_bytes = kHostChunkBytes;
  if (const char* v = getenv("CILIUM_GPU_HOST_CHUNK_MB")) chunk_bytes = std::max<size_t>(1, strtoull(v, nullptr, 10)) << 20;
  const size_t nchunks = (size_t)std::max<uint64_t>(1, std::min<uint64_t>(n / 4096 + 1, total / chunk_bytes + 1));
  const unsigned nw = nchunks > 1 ? 2u : 1u;
  const unsigned copy_threads = std::max(1u, cg_http_pack_threads() / nw);
  std::exception_ptr err;
  std::mutex mu;
  auto worker = [&](unsigned w) {
    try {
      e->set_device();
      auto lease = e->staging.acquire(e->device);
      for (size_t k = w; k < nchunks; k += nw) {
        {
          std::lock_guard<std::mutex> lk(mu);
          if (err) return;
        }
        run_host_chunk(*s, *e, *lease, in, raw, raw_off, n * k / nchunks, n * (k + 1) / nchunks, policy, ingress,
                       port, remote, out, copy_threads);
      }
    } catch (...) {
      std::lock_guard<std::mutex> lk(mu);
      if (!err) err = std::current_exception();
    }
  };
  if (nw == 1) {
    worker(0);
  } else {
    std::thread t1(worker, 1u);
    worker(0);
    t1.join();
  }
  if (err) std::rethrow_exception(err);
}

int cg_http_verdicts_raw_host(uint64_t h, const uint8_t* raw, const uint64_t* raw_off, size_t n,
                              const uint32_t* policy, const uint8_t* ingress, const uint16_t* port,
                              const uint32_t* remote, uint8_t* out) {
  return guarded([&] { verdicts_raw_from_host(h, RawInput::Heads, raw, raw_off, n, policy, ingress, port, remote, out); });
}

// ---- small header-list calls: the host packer on the calling thread ----
// Envoy decides one request per decodeHeaders (cilium_l7policy.cc:127-182),
// from many worker threads at once.  For a call of at most kSmallLists lists
// the host packer (one pass, no device layout step) + one staged copy in +
// one http_kernel launch + one copy out is the fastest sequence: 29.5 us per
// single-request call, 90K calls/s from 16 threads, each call on its own
// staging lease (profiles/r05g_http_latency.jsonl).  Combining concurrent
// calls into one batch was measured and lost (80K calls/s at 8 calls per
// batch: the flusher serializes the packing and the wake-ups).
constexpr size_t kSmallLists = 1024;

static void small_lists_host(Engine& e, const uint8_t* blob, const uint64_t* off, size_t n, const uint32_t* pol,
                             const uint8_t* ing, const uint16_t* port, const uint32_t* rem, uint8_t* out) {
  auto s = http_snap(e);
  const size_t bytes = off[n] - off[0];
  // the overflow arena holds the strings past a slot: bounded by the list
  // bytes plus each request's separators
  const size_t arena_cap = bytes + n * (2 * s->fields.size() + 24) + 64;
  e.set_device();
  auto lease = e.staging.acquire(e.device);
  const size_t bcap = http_batch_bytes(*s, n), scap = http_batch_slots(*s, n) + 1;
  uint8_t* hb = (uint8_t*)lease->host_buf(0, bcap);
  uint8_t* ha = (uint8_t*)lease->host_buf(1, arena_cap);
  std::vector<uint32_t> order(scap);
  size_t nslots = 0, aused = 0;
  http_pack(*s, n, pol, ing, port, rem, blob, off, hb, bcap, order.data(), &nslots, ha, arena_cap, &aused);
  HttpBatchHeader hdr;
  memcpy(&hdr, hb, sizeof(hdr));
  const hipStream_t st = (hipStream_t)lease->stream;
  void* dr = lease->dev_buf(0, bcap);
  void* da = lease->dev_buf(1, arena_cap);
  hip_check(hipMemcpyAsync(dr, hb, hdr.total_bytes, hipMemcpyHostToDevice, st), "H2D");
  if (hdr.arena_bytes) hip_check(hipMemcpyAsync(da, ha, hdr.arena_bytes, hipMemcpyHostToDevice, st), "H2D");
  void* dout = lease->dev_buf(2, nslots + 1);
  check_launch(launch_http(s->dev, dr, nslots, (const uint8_t*)da, (uint8_t*)dout, st, e.cus), "http kernel launch");
  uint8_t* slots = (uint8_t*)lease->host_buf(2, nslots + 1);
  if (nslots) hip_check(hipMemcpyAsync(slots, dout, nslots, hipMemcpyDeviceToHost, st), "D2H");
  hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  memset(out, 0, n);
  for (size_t i = 0; i < nslots; ++i)
    if (order[i] < n) out[order[i]] = slots[i];
}

int cg_http_verdicts_fields_host(uint64_t h, const uint8_t* hdr_blob, const uint64_t* hdr_off, size_t n,
                                 const uint32_t* policy, const uint8_t* ingress, const uint16_t* port,
                                 const uint32_t* remote, uint8_t* out) {
  return guarded([&] {
    // small calls, and any call on a snapshot the device packer does not
    // take (more than kRawMaxFields header fields): the host packer, in
    // pieces of kHostPackLists, so a snapshot works or fails the same way
    // whatever the batch size
    bool host_pack = n && n <= kSmallLists;
    if (n && !host_pack) {
      auto e = get(h);
      host_pack = !http_snap(*e)->lists_ok;
    }
    if (host_pack) {
      auto e = get(h);
      e->require_gpu();
      (void)http_snap(*e);  // CG_NOT_FOUND first
      check_offsets(hdr_off, n);
      if (!policy || !ingress || !port || !remote || !out || (hdr_off[n] != hdr_off[0] && !hdr_blob))
        fail(CG_INVALID_ARGUMENT, "NULL hdr_blob/policy/ingress/port/remote/out");
      for (size_t i = 0; i < n; ++i)  // the packer's limit (16-bit value spans), before the batch is shared
        if (hdr_off[i + 1] - hdr_off[i] > 0xFFFFu) fail(CG_INVALID_ARGUMENT, "header list longer than 64 KiB");
      constexpr size_t kHostPackLists = (size_t)1 << 20;
      for (size_t a = 0; a < n; a += kHostPackLists) {
        const size_t m = std::min(kHostPackLists, n - a);
        small_lists_host(*e, hdr_blob, hdr_off + a, m, policy + a, ingress + a, port + a, remote + a, out + a);
      }
      return;
    }
    verdicts_raw_from_host(h, RawInput::Lists, hdr_blob, hdr_off, n, policy, ingress, port, remote, out);
  });
}

// ------------------------------------------------------ verdict ring ----
int cg_http_ring_open(uint64_t h, uint32_t workgroups, uint32_t slots) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    std::lock_guard<std::mutex> lk(e->ring_mu);
    if (e->ring) fail(CG_INVALID_ARGUMENT, "the handle's ring is open");
    auto r = std::make_shared<HttpRing>();
    r->open(*e, workgroups, slots);
    e->ring = std::move(r);
    bump_epoch();
  });
}

// A calling thread's handle, ring and snapshot as of epoch `epoch` (g_epoch).
struct RingCallCache {
  uint64_t h = 0, epoch = 0;
  std::shared_ptr<Engine> e;
  std::shared_ptr<HttpRing> r;
  std::shared_ptr<HttpSnapshot> s;
};
thread_local RingCallCache t_ring_call;

int cg_http_ring_verdicts(uint64_t h, const uint8_t* hdr_blob, const uint64_t* hdr_off, size_t n,
                          const uint32_t* policy, const uint8_t* ingress, const uint16_t* port,
                          const uint32_t* remote, uint8_t* out) {
  bool other = false;
  const int rc = guarded([&] {
    RingCallCache& c = t_ring_call;
    const uint64_t ep = g_epoch.load(std::memory_order_acquire);
    if (c.h != h || c.epoch != ep || !c.e) {  // the locked lookups, once per thread and epoch
      c = RingCallCache{};
      auto e = get(h);
      e->require_gpu();
      std::shared_ptr<HttpRing> r;
      {
        std::lock_guard<std::mutex> lk(e->ring_mu);
        r = e->ring;
      }
      if (!r) fail(CG_NOT_FOUND, "no ring open (cg_http_ring_open)");
      auto s = http_snap(*e);
      c = RingCallCache{h, ep, std::move(e), std::move(r), std::move(s)};
    }
    Engine* e = c.e.get();
    HttpRing* r = c.r.get();
    const std::shared_ptr<HttpSnapshot>& s = c.s;
    if (!n) return;
    check_offsets(hdr_off, n);
    if (!policy || !ingress || !port || !remote || !out || (hdr_off[n] != hdr_off[0] && !hdr_blob))
      fail(CG_INVALID_ARGUMENT, "NULL hdr_blob/policy/ingress/port/remote/out");
    for (size_t i = 0; i < n; ++i)  // the packer's limit (16-bit value spans)
      if (hdr_off[i + 1] - hdr_off[i] > 0xFFFFu) fail(CG_INVALID_ARGUMENT, "header list longer than 64 KiB");
    if (n > kRingReqs || hdr_off[n] - hdr_off[0] > kRingBlob || !s->lists_ok) {
      other = true;  // past a slot: the staged entry
      return;
    }
    r->verdicts(*e, s, hdr_blob, hdr_off, n, policy, ingress, port, remote, out);
  });
  if (rc == CG_OK && other)
    return cg_http_verdicts_fields_host(h, hdr_blob, hdr_off, n, policy, ingress, port, remote, out);
  return rc;
}

int cg_http_ring_stats(uint64_t h, uint64_t* served, uint64_t* launches) {
  return guarded([&] {
    auto e = get(h);
    std::shared_ptr<HttpRing> r;
    {
      std::lock_guard<std::mutex> lk(e->ring_mu);
      r = e->ring;
    }
    if (!r) fail(CG_NOT_FOUND, "no ring open (cg_http_ring_open)");
    r->stats(served, launches);
  });
}

int cg_http_ring_close(uint64_t h) {
  return guarded([&] {
    auto e = get(h);
    std::shared_ptr<HttpRing> r;
    {
      std::lock_guard<std::mutex> lk(e->ring_mu);
      r = std::move(e->ring);
    }
    bump_epoch();
    if (!r) fail(CG_NOT_FOUND, "no ring open (cg_http_ring_open)");
    r->close();
  });
}

// ------------------------------------------------------------ counters ----
static void counters_loc(Engine& e, uint32_t what, uint32_t id, void** p, size_t* n) {
  *p = nullptr;
  *n = 0;
  if (what == CG_CTR_HTTP_PROGRAMS || what == CG_CTR_HTTP_RULES || what == CG_CTR_HTTP_ALLREDUCE) {
    auto s = http_snap(e);
    uint64_t* base = s->d_counters.as<uint64_t>();
    const size_t np = s->progs.size() * 2, nr = s->rule_info.size();
    if (what == CG_CTR_HTTP_PROGRAMS) {
      *p = base;
      *n = np;
    } else if (what == CG_CTR_HTTP_RULES) {
      *p = base ? base + np + 1 : nullptr;
      *n = nr;
    } else {
      *p = base;
      *n = np + 1 + nr;
    }
  } else if (what == 1) {
    auto s = kafka_snap(e);
    *p = s->d_counters.get();
    *n = s->dflt_group.size() * 2;
  } else if (what == 2) {
    std::lock_guard<std::mutex> lk(e.mu);
    PrefilterState& pf = get_pf(e, id);
    *p = pf.d_counters ? pf.d_counters->get() : nullptr;
    *n = pf.d_counters ? 2 : 0;
  } else {
    fail(CG_INVALID_ARGUMENT, "unknown counter set");
  }
}

int cg_read_counters(uint64_t h, uint32_t what, uint32_t id, uint64_t* out, size_t cap, size_t* n) {
  return guarded([&] {
    auto e = get(h);
    void* p;
    size_t cnt;
    counters_loc(*e, what, id, &p, &cnt);
    if (n) *n = cnt;
    size_t k = std::min(cap, cnt);
    if (k && p && e->has_gpu()) {
      e->set_device();
      hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
      hip_check(hipMemcpy(out, p, k * 8, hipMemcpyDeviceToHost), "D2H counters");
    } else if (k) {
      memset(out, 0, k * 8);
    }
  });
}

int cg_counters_device_ptr(uint64_t h, uint32_t what, uint32_t id, void** d_ptr, size_t* n) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    counters_loc(*e, what, id, d_ptr, n);
  });
}

int cg_counters_copy_dev(uint64_t h, uint32_t what, uint32_t id, void* d_dst, size_t n, void* stream) {
  return guarded([&] {
    auto e = get(h);
    e->require_gpu();
    void* p;
    size_t cnt;
    counters_loc(*e, what, id, &p, &cnt);
    size_t k = std::min(n, cnt);
    e->set_device();
    if (k)
      hip_check(hipMemcpyAsync(d_dst, p, k * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream_of(*e, stream)),
                "D2D counters");
  });
}

int cg_reset_counters(uint64_t h) {
  return guarded([&] {
    auto e = get(h);
    if (!e->has_gpu()) return;
    e->set_device();
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->http) e->http->d_counters.zero();
    if (e->kafka) e->kafka->d_counters.zero();
    for (auto& [id, p] : e->prefilters)
      if (p->d_counters) p->d_counters->zero();
    for (auto& [id, m] : e->maps)
      if (m->d_counters) m->d_counters->zero();
  });
}

// ------------------------------------------------------ regex syntax ----
int cg_regex_validate(const char* re, size_t re_len, uint32_t flavour) {
  return guarded([&] {
    std::string err;
    const RegexFlavour f = flavour == CG_REGEX_GO ? RegexFlavour::Go : RegexFlavour::Ecma;
    if (flavour > CG_REGEX_GO) fail(CG_INVALID_ARGUMENT, "unknown regex flavour");
    if (!regex_syntax_ok(std::string(re, re_len), &err, f)) fail(CG_POLICY_REJECTED, err);
  });
}

// ------------------------------------------------------- diagnostics ----
// Host-side walkers of the compiled tables and the regex compiler, for the
// CPU test-suite only.  No verdict entry point calls them.
int cg_diag_regex_match(const char* re, size_t re_len, const uint8_t* s, size_t len, uint32_t search,
                        uint8_t* result) {
  return guarded([&] {
    // the last compiled patterns are kept: tests run one pattern on many strings
    static std::mutex mu;
    static std::map<std::pair<std::string, bool>, std::shared_ptr<const ByteDfa>> cache;
    const auto key = std::make_pair(std::string(re, re_len), search != 0);
    std::shared_ptr<const ByteDfa> d;
    {
      std::lock_guard<std::mutex> g(mu);
      auto it = cache.find(key);
      if (it != cache.end()) d = it->second;
    }
    if (!d) {
      d = std::make_shared<const ByteDfa>(
          compile_regex(key.first, ByteSet::all(), search ? MatchMode::Search : MatchMode::Full));
      std::lock_guard<std::mutex> g(mu);
      if (cache.size() >= 64) cache.clear();
      cache.emplace(key, d);
    }
    *result = dfa_run(*d, std::string((const char*)s, len)) ? 1 : 0;
  });
}

int cg_diag_http_rules_host(uint64_t h, const void* batch, size_t nslots, const uint32_t* order, size_t n,
                            const uint8_t* arena, size_t arena_len, uint32_t* rule) {
  return guarded([&] {
    auto e = get(h);
    auto s = http_snap(*e);
    std::vector<uint8_t> slots(nslots);
    std::vector<uint32_t> r(nslots);
    http_eval_host(*s, (const uint8_t*)batch, nslots, arena, arena_len, slots.data(), r.data());
    for (size_t i = 0; i < nslots; ++i)
      if (order[i] < n) rule[order[i]] = r[i];
  });
}

int cg_diag_http_eval_host(uint64_t h, const void* batch, size_t nslots, const uint32_t* order, size_t n,
                           const uint8_t* arena, size_t arena_len, uint8_t* out) {
  return guarded([&] {
    auto e = get(h);
    auto s = http_snap(*e);
    std::vector<uint8_t> slots(nslots);
    http_eval_host(*s, (const uint8_t*)batch, nslots, arena, arena_len, slots.data());
    for (size_t i = 0; i < nslots; ++i)
      if (order[i] < n) out[order[i]] = slots[i];
  });
}

// The L4, prefilter and Kafka host evaluators run the kernels' own per-item
// functions (l4_walk.h, lpm_walk.h, kafka_walk.h) over host_view(), each item
// loaded as the kernel's load phases load it.

// Per tuple as l4_kernel does it, with plain CG_L4_CAN_ACCESS semantics.
int cg_diag_l4_eval_host(uint64_t h, uint32_t map_id, const cg_l4_tuple* t, size_t n, int32_t* out) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PolicyMapState& m = get_map(*e, map_id);
    if (m.dirty) m.rebuild(*e);
    const L4Dev T = m.host_view();
    for (size_t i = 0; i < n; ++i) {
      uint32_t w[3];  // identity, dport | proto << 16 | flags << 24, len
      memcpy(w, &t[i], sizeof(w));
      const uint32_t w1 = l4_mode_word(w[1], CG_L4_CAN_ACCESS);
      uint32_t val = 0;
      const int which = l4_resolve(T, [&](uint32_t b) { return T.fp[b]; }, w[0], w1,
                                   (w1 >> 24) & CG_L4_F_FRAGMENT, &val);
      out[i] = l4_wrap(l4_verdict(which, val, w1 >> 24), CG_L4_CAN_ACCESS);
    }
  });
}

// Per tuple as l4_array_kernel does it: the slot's map, then l4_kernel's walk
// with `mode`; an empty slot is the missed tail call.
int cg_diag_l4_array_eval_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint16_t* lxc, const cg_l4_tuple* t,
                               size_t n, int32_t* out) {
  return guarded([&] {
    auto e = get(h);
    check_l4_mode(mode);
    std::lock_guard<std::mutex> lk(e->mu);
    PolicyArrayState& a = get_arr(*e, arr_id);
    if (n && (!lxc || !t || !out)) fail(CG_INVALID_ARGUMENT, "NULL lxc_ids/tuples/verdicts");
    std::map<uint32_t, L4Dev> views;
    for (const auto& ref : a.refs) {
      PolicyMapState& m = get_map(*e, ref.first);
      if (m.dirty) m.rebuild(*e);
      views.emplace(ref.first, m.host_view());
    }
    for (size_t i = 0; i < n; ++i) {
      const uint32_t map_id = a.slot_map[lxc[i]];
      if (!map_id) {
        out[i] = CG_DROP_MISSED_TAIL_CALL;
        continue;
      }
      const L4Dev& T = views.find(map_id)->second;
      uint32_t w[3];  // identity, dport | proto << 16 | flags << 24, len
      memcpy(w, &t[i], sizeof(w));
      const uint32_t w1 = l4_mode_word(w[1], mode);
      uint32_t val = 0;
      const int which = l4_resolve(T, [&](uint32_t b) { return T.fp[b]; }, w[0], w1,
                                   (w1 >> 24) & CG_L4_F_FRAGMENT, &val);
      out[i] = l4_wrap(l4_verdict(which, val, w1 >> 24), mode);
    }
  });
}

// The array as the frames kernels see it, over the members' host views (the caller holds e.mu): slot words, and
// one record per member map.
struct L4ArrHostView {
  std::vector<uint32_t> slot = std::vector<uint32_t>(CG_POLICY_ARRAY_SLOTS, 0u);
  std::vector<L4Dev> recs;
  L4ArrHostView(Engine& e, PolicyArrayState& a) {
    std::map<uint32_t, uint32_t> word;
    for (const auto& ref : a.refs) {
      PolicyMapState& m = get_map(e, ref.first);
      if (m.dirty) m.rebuild(e);
      word.emplace(ref.first, (uint32_t)recs.size() + 1);
      recs.push_back(m.host_view());
    }
    for (uint32_t s = 0; s < CG_POLICY_ARRAY_SLOTS; ++s)
      if (a.slot_map[s]) slot[s] = word[a.slot_map[s]];
    if (recs.empty()) recs.push_back(L4Dev{});
  }
  L4ArrDev dev() const { return L4ArrDev{slot.data(), recs.data()}; }
};

// Per frame as l4_frames_kernel does it: the request's program (frame_progs.h)
// over the host views of the array, the endpoint map or the array's headers,
// the ipcache and the conntrack map.  No device, no counters.  l4_off (may be
// NULL): the L4 offset the walk found, 0 where it did not get that far.
static void frames_eval_host(uint64_t h, const FramesReq& q, const FramesBatch& b, uint32_t* l4_off) {
  auto e = get(h);
  check_frames(*e, q, b, false, true);
  std::lock_guard<std::mutex> lk(e->mu);
  PolicyArrayState& a = get_arr(*e, q.arr_id);
  const L4ArrHostView av(*e, a);
  const L4ArrDev A = av.dev();
  std::vector<uint32_t> hidx;
  std::vector<uint4> hrecs;
  if (q.egress) a.header_tables(&hidx, &hrecs);
  const EpHdrDev H{hidx.data(), hrecs.data()};
  EpMapDev E{};
  IpcacheDev ipc{};
  CtMapDev C{};
  LbMapDev L{};
  if (q.lb_id) {
    LbMapState& p = get_lb(*e, *q.lb_id);
    if (p.dirty) p.rebuild(*e);
    L = p.host_view();
  }
  if (q.ep_id) {
    EndpointMapState& p = get_ep(*e, q.ep_id);
    if (p.dirty) p.rebuild(*e);
    E = p.host_view();
  }
  if (q.ipc_id) {
    IpcacheState& p = get_ipc(*e, q.ipc_id);
    if (p.dirty) p.rebuild(*e);
    ipc = p.host_view();
  }
  if (q.ct_id) {
    CtMapState& p = get_ct(*e, *q.ct_id);
    if (p.dirty) p.rebuild(*e);
    C = p.host_view();
  }
  const uint64_t wlo = b.off[0], whi = b.off[b.n];
  const uint8_t* lo = b.raw + wlo;
  const uint8_t* hi = whi > wlo ? b.raw + whi : lo;
  // prog: a program type's value, T: its table
  auto loop = [&](auto prog, const auto& T) {
    using P = decltype(prog);
    for (size_t i = 0; i < b.n; ++i) {
      uint64_t start;
      const uint32_t len = frame_range(b.off[i], b.off[i + 1], wlo, whi, &start);
      const uint8_t* base = b.raw + start;
      auto ld = [&](uint32_t o) {
        uint32_t v = 0;
        for (int k = 0; k < 4; ++k) {
          const uint8_t* p = base + o + k;
          if (p >= lo && p < hi) v |= (uint32_t)*p << (8 * k);
        }
        return v;
      };
      auto count = [](const L4Dev&, uint32_t) {};
      const uint32_t plen = b.pkt_len ? b.pkt_len[i] : len;
      const uint32_t lxc = b.lxc ? b.lxc[i] : 0u, label = b.labels ? b.labels[i] : 0u;
      cg_l4_frame_info fi;
      CtRecWords r;
      uint32_t lo4 = 0;
      if constexpr (HasExtra<P>::value) {
        typename P::Extra ex;
        b.out[i] = P::run(A, T, ipc, C, ld, len, lxc, label, plen, b.mode, &fi, &lo4, &r, count, i, &ex);
        P::store(T, i, ex);
      } else {
        b.out[i] = P::run(A, T, ipc, C, ld, len, lxc, label, plen, b.mode, &fi, &lo4, &r, count);
      }
      if (b.info) b.info[i] = fi;
      if (P::kRecs && b.recs) memcpy(&b.recs[i], r.w, sizeof(cg_ct_record));
      if (l4_off) l4_off[i] = lo4;
    }
  };
  if (q.lb_id)
    loop(EgressSvcProg{}, EpHdrSvcDev{H, L, q.hash, (uint4*)q.svc_recs, (uint4*)q.xlate});
  else if (q.egress)
    with_bools([&](auto kIpc, auto kCt) { loop(EgressProg<kIpc, kCt>{}, H); }, q.ipc_id != 0, q.ct_id != nullptr);
  else
    with_bools([&](auto kEp, auto kIpc, auto kCt) { loop(IngressProg<kEp, kIpc, kCt>{}, E); }, q.ep_id != 0,
               q.ipc_id != 0, q.ct_id != nullptr);
}

int cg_diag_l4_frames_eval_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                                const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids, uint32_t ep_id,
                                const uint32_t* src_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                                int32_t* verdicts, cg_l4_frame_info* info, uint32_t* l4_off) {
  return guarded([&] {
    frames_eval_host(h, {arr_id, ep_id, ipc_id, nullptr, false},
                     {raw, raw_off, n, lxc_ids, src_labels, pkt_len, verdicts, info, nullptr, mode}, l4_off);
  });
}

int cg_diag_l4_frames_ct_eval_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                                   const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids, uint32_t ep_id,
                                   const uint32_t* src_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                                   uint32_t ct_id, int32_t* verdicts, cg_l4_frame_info* info,
                                   cg_ct_record* records, uint32_t* l4_off) {
  return guarded([&] {
    frames_eval_host(h, {arr_id, ep_id, ipc_id, &ct_id, false},
                     {raw, raw_off, n, lxc_ids, src_labels, pkt_len, verdicts, info, records, mode}, l4_off);
  });
}

int cg_diag_l4_frames_egress_eval_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                                       const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids,
                                       const uint32_t* dst_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                                       uint32_t ct_id, int32_t* verdicts, cg_l4_frame_info* info,
                                       cg_ct_record* ct_recs, uint32_t* l4_off) {
  return guarded([&] {
    frames_eval_host(h, {arr_id, 0, ipc_id, ct_id ? &ct_id : nullptr, true},
                     {raw, raw_off, n, lxc_ids, dst_labels, pkt_len, verdicts, info, ct_recs, mode}, l4_off);
  });
}

int cg_diag_l4_frames_egress_svc_eval_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                                           const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids,
                                           const uint32_t* dst_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                                           uint32_t ct_id, uint32_t lb_id, const uint32_t* hash, int32_t* verdicts,
                                           cg_l4_frame_info* info, cg_ct_record* records, cg_ct_record* svc_records,
                                           cg_lb_xlate* xlate, uint32_t* l4_off) {
  return guarded([&] {
    frames_eval_host(h, svc_req(arr_id, ipc_id, &ct_id, &lb_id, hash, svc_records, xlate),
                     {raw, raw_off, n, lxc_ids, dst_labels, pkt_len, verdicts, info, records, mode}, l4_off);
  });
}

int cg_diag_ct_hash(const cg_ct_key* keys, size_t n, uint32_t* hashes) {
  return guarded([&] {
    if (n && (!keys || !hashes)) fail(CG_INVALID_ARGUMENT, "NULL keys/hashes");
    for (size_t i = 0; i < n; ++i) {
      const CtMapState::Key k = make_ct_key(keys[i], false);
      hashes[i] = keys[i].family == 4 ? ct_hash(CtMapState::dev_key<kCt4Words>(k))
                                      : ct_hash(CtMapState::dev_key<kCt6Words>(k));
    }
  });
}

int cg_diag_ct_map_info(uint64_t h, uint32_t ct_id, uint32_t buckets[2], uint32_t probes[2]) {
  return guarded([&] {
    auto e = get(h);
    if (!buckets || !probes) fail(CG_INVALID_ARGUMENT, "NULL buckets/probes");
    std::lock_guard<std::mutex> lk(e->mu);
    CtMapState& p = get_ct(*e, ct_id);
    if (p.dirty) p.rebuild(*e);
    buckets[0] = p.mask4 + 1;
    buckets[1] = p.mask6 + 1;
    probes[0] = p.probes4;
    probes[1] = p.probes6;
  });
}

// Per packet as lpm_kernel does it.
int cg_diag_prefilter_eval_host(uint64_t h, uint32_t pf_id, const uint32_t* v4, size_t n4, uint8_t* out4,
                                const uint8_t* v6, size_t n6, uint8_t* out6) {
  return guarded([&] {
    auto e = get(h);
    std::lock_guard<std::mutex> lk(e->mu);
    PrefilterState& p = get_pf(*e, pf_id);
    if (p.dirty) p.rebuild(*e);
    const LpmDev t = p.host_view();
    const bool v4f = p.v4_filter, v6f = p.v6_filter;  // as the launch passes them
    for (size_t i = 0; i < n4; ++i) {
      const uint32_t s = __builtin_bswap32(v4[2 * i]), a = v4[2 * i + 1];
      const uint32_t w = v4f ? t.top[s >> 20] : 0u;
      const uint32_t eh = ep_hash32(a) & t.ep4_mask, ek = t.ep4_keys[eh];
      bool drop = v4_covered(t, s, w);
      if (!drop) drop = !ep4_has(t, a, ek, eh);
      out4[i] = drop ? CG_XDP_DROP : CG_XDP_PASS;
    }
    for (size_t i = 0; i < n6; ++i) {
      const uint4 a = load16(v6 + 32 * i), b = load16(v6 + 32 * i + 16);
      const uint64_t sh = __builtin_bswap64(u64_of(a.x, a.y)), sl = __builtin_bswap64(u64_of(a.z, a.w));
      const uint64_t dh = __builtin_bswap64(u64_of(b.x, b.y)), dl = __builtin_bswap64(u64_of(b.z, b.w));
      const uint64_t cw = v6f ? t.v6_code[sh >> (68 - t.v6_bits)] : 0;
      const uint32_t eh = ep_hash128(dh, dl) & t.ep6_mask;
      const uint4 ek = load16(t.ep6_keys + 2 * (size_t)eh);
      // level 2, then the top two candidates of a mixed bucket
      uint32_t m;
      const uint32_t code = v6_code_of(cw, (uint32_t)(sh >> (64 - t.v6_bits)), &m);
      const bool mixed = code == kLpmPartial;
      const V6Window win = v6_window(t.v6_mix[mixed ? m : 0], mixed);
      const int64_t r1 = mixed ? win.R : 0, r0 = mixed && win.R - 1 >= win.L ? win.R - 1 : r1;
      bool drop = code == 1;
      if (mixed)
        drop = v6_covered(t, sh, sl, win, load16(t.v6_iv + 4 * r1), load16(t.v6_iv + 4 * r1 + 2),
                          load16(t.v6_iv + 4 * r0), load16(t.v6_iv + 4 * r0 + 2));
      if (!drop) drop = !ep6_has(t, dh, dl, ek, eh);
      out6[i] = drop ? CG_XDP_DROP : CG_XDP_PASS;
    }
  });
}

int cg_diag_kafka_eval_host(uint64_t h, const cg_kafka_request* reqs, size_t n, const uint32_t* arena,
                            size_t arena_len, uint8_t* out) {
  return guarded([&] {
    auto e = get(h);
    auto s = kafka_snap(*e);
    for (size_t i = 0; i < n; ++i) out[i] = kafka_eval_host(*s, reqs[i], arena, arena_len);
  });
}

int cg_diag_kafka_decode_host(uint64_t h, const uint8_t* raw, const uint64_t* raw_off, size_t n,
                              const uint16_t* redirect, const uint32_t* remote, cg_kafka_request* reqs,
                              uint32_t* arena, size_t arena_cap, size_t* arena_used, uint8_t* status) {
  return guarded([&] {
    auto e = get(h);
    auto s = kafka_snap(*e);
    if (!arena_used || (n && (!reqs || !status || !redirect || !remote))) fail(CG_INVALID_ARGUMENT, "NULL argument");
    *arena_used = 0;
    if (!n) return;
    check_offsets(raw_off, n);
    std::vector<uint32_t> spill;
    for (size_t i = 0; i < n; ++i)
      status[i] = kafka_decode_host_one(*s, raw + raw_off[i], raw_off[i + 1] - raw_off[i], redirect[i], remote[i],
                                        &reqs[i], &spill);
    *arena_used = spill.size();
    if (spill.size() > (arena ? arena_cap : 0)) fail(CG_MAP_FULL, "Kafka topic arena too small");
    if (!spill.empty()) memcpy(arena, spill.data(), spill.size() * 4);
  });
}

}  // extern "C"
