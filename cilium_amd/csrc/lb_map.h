// lb_map.h — the service maps, cilium_lb{4,6}_services and
// cilium_lb{4,6}_reverse_nat (pkg/maps/lbmap; struct lb{4,6}_key / lb{4,6}_service
// / lb{4,6}_reverse_nat bpf/lib/common.h:408-462), of one node: the host tables
// and their device form, the slot tables and dense arrays of lb_walk.h.
#pragma once

#include <array>
#include <map>
#include <memory>
#include <vector>

#include "engine.h"
#include "lb_walk.h"

namespace cg {

struct LbMapState {
  uint32_t max_entries = CG_LB_MAP_MAX_ENTRIES;  // of each of the four maps
  uint32_t loopback = 0;                         // IPV4_LOOPBACK, network order
  // {family, address, dport's bytes as stored, slave (big-endian)}: the map's order is the dump's
  using Key = std::array<uint8_t, 21>;
  std::map<Key, cg_lb_service> services;
  std::map<std::pair<uint8_t, uint16_t>, cg_lb_revnat> revnat;  // {family, index}
  bool dirty = true;

  // host copies of the device tables (also walked by cg_diag_l4_frames_egress_svc_eval_host)
  std::vector<uint32_t> s4, s6, rn4, rn6;
  uint32_t mask4 = 0, mask6 = 0, probes4 = 0, probes6 = 0;
  std::shared_ptr<DevTables> tab;  // the published device tables (engine.h)
  LbMapDev dev{};                  // view of tab; copy it together with tab

  static Key make_key(const cg_lb_key& k) {
    Key out;
    out[0] = k.family;
    memcpy(&out[1], k.address, 16);
    memcpy(&out[17], &k.dport, 2);
    out[19] = (uint8_t)(k.slave >> 8);
    out[20] = (uint8_t)k.slave;
    return out;
  }
  static cg_lb_key key_of(const Key& in) {
    cg_lb_key k{};
    k.family = in[0];
    memcpy(k.address, &in[1], 16);
    memcpy(&k.dport, &in[17], 2);
    k.slave = (uint16_t)(in[19] << 8 | in[20]);
    return k;
  }
  size_t count_services(uint8_t family) const {
    size_t n = 0;
    for (const auto& kv : services) n += kv.first[0] == family;
    return n;
  }
  size_t count_revnat(uint8_t family) const {
    size_t n = 0;
    for (const auto& kv : revnat) n += kv.first.first == family;
    return n;
  }

  // One family's services into slots of lb_slot_words(A) words, at most half of them used.
  template <int A>
  void build_family(uint8_t family, std::vector<uint32_t>* t, uint32_t* mask, uint32_t* probes) const {
    constexpr int SW = lb_slot_words(A);
    const size_t n = count_services(family);
    size_t nb = 1;
    while (nb < 2 * n) nb <<= 1;
    t->assign(nb * SW, 0u);
    *mask = (uint32_t)(nb - 1);
    *probes = 0;
    for (const auto& [key, v] : services) {
      if (key[0] != family) continue;
      LbKey<A> k;
      memcpy(k.a, &key[1], 4 * A);
      uint16_t dport;
      memcpy(&dport, &key[17], 2);
      k.ds = dport | (uint32_t)(key[19] << 8 | key[20]) << 16;
      const uint32_t h = lb_hash(k) & *mask;
      for (uint32_t p = 0;; ++p) {
        uint32_t* s = t->data() + (size_t)((h + p) & *mask) * SW;
        const int used = A == 1 ? 2 : 5;
        if (s[used]) continue;  // nb >= 2 n: a free slot exists
        const uint32_t pc = v.port | (uint32_t)v.count << 16, rw = v.rev_nat_index | (uint32_t)v.weight << 16;
        if constexpr (A == 1) {
          s[0] = k.a[0];
          s[1] = k.ds;
          s[2] = 1;
          s[3] = pc;
          memcpy(&s[4], v.target, 4);
          s[5] = rw;
        } else {
          memcpy(&s[0], k.a, 16);
          s[4] = k.ds;
          s[5] = 1;
          s[6] = pc;
          s[7] = rw;
          memcpy(&s[8], v.target, 16);
        }
        if (p > *probes) *probes = p;
        break;
      }
    }
  }
  void build_tables() {
    build_family<1>(4, &s4, &mask4, &probes4);
    build_family<4>(6, &s6, &mask6, &probes6);
    size_t n4 = 0, n6 = 0;
    for (const auto& kv : revnat) {
      size_t& n = kv.first.first == 4 ? n4 : n6;
      if ((size_t)kv.first.second + 1 > n) n = (size_t)kv.first.second + 1;
    }
    rn4.assign(2 * (n4 ? n4 : 1), 0u);
    rn6.assign(8 * (n6 ? n6 : 1), 0u);
    for (const auto& [k, v] : revnat) {
      if (k.first == 4) {
        memcpy(&rn4[2 * (size_t)k.second], v.address, 4);
        rn4[2 * (size_t)k.second + 1] = v.port | 1u << 16;
      } else {
        memcpy(&rn6[8 * (size_t)k.second], v.address, 16);
        rn6[8 * (size_t)k.second + 4] = v.port | 1u << 16;
      }
    }
  }
  template <class Ptr>
  LbMapDev view(Ptr ptr) const {
    LbMapDev d{};
    d.s4 = ptr(s4);
    d.s6 = ptr(s6);
    d.mask4 = mask4;
    d.mask6 = mask6;
    d.probes4 = probes4;
    d.probes6 = probes6;
    d.rn4 = ptr(rn4);
    d.rn6 = ptr(rn6);
    d.nrn4 = (uint32_t)(rn4.size() / 2);
    d.nrn6 = (uint32_t)(rn6.size() / 8);
    d.loopback = loopback;
    return d;
  }
  LbMapDev host_view() const { return view(HostPtr{}); }
  void rebuild(Engine& e) {
    build_tables();
    if (e.has_gpu()) {
      e.set_device();
      auto t = std::make_shared<DevTables>();
      const LbMapDev d = view([&](const auto& v) { return t->add(v); });
      tab = std::move(t);  // publish (the caller holds the handle lock)
      dev = d;
    }
    dirty = false;
  }
};

}  // namespace cg
