// ct_map.h — the conntrack maps, cilium_ct{4,6}_* and cilium_ct_any{4,6}_*
// (pkg/maps/ctmap; struct ipv{4,6}_ct_tuple / ct_entry bpf/lib/common.h:338-406),
// of one scope set: the host table with the whole ct_entry per key, and its
// device form, the bucket tables of ct_walk.h.
#pragma once

#include <array>
#include <map>
#include <memory>
#include <vector>

#include "ct_walk.h"
#include "engine.h"

namespace cg {

struct CtMapState {
  uint32_t max_entries = 1u << 20;
  bool global = false;
  // {scope (big-endian), kind, family, the tuple's 38 bytes as stored}: the map's order is the dump's
  using Key = std::array<uint8_t, 42>;
  std::map<Key, cg_ct_entry> entries;
  bool dirty = true;

  // host copies of the device tables (also walked by cg_diag_l4_frames_ct_eval_host)
  std::vector<uint32_t> t4, t6;
  uint32_t mask4 = 0, mask6 = 0, probes4 = 0, probes6 = 0;
  std::shared_ptr<DevTables> tab;  // the published device tables (engine.h)
  CtMapDev dev{};                  // view of tab; copy it together with tab

  static Key make_key(const cg_ct_key& k) {
    Key out;
    out[0] = (uint8_t)(k.scope >> 8);
    out[1] = (uint8_t)k.scope;
    out[2] = k.kind;
    out[3] = k.family;
    memcpy(&out[4], k.daddr, 16);
    memcpy(&out[20], k.saddr, 16);
    memcpy(&out[36], &k.dport, 2);
    memcpy(&out[38], &k.sport, 2);
    out[40] = k.nexthdr;
    out[41] = k.flags;
    return out;
  }
  static cg_ct_key key_of(const Key& in) {
    cg_ct_key k{};
    k.scope = (uint16_t)(in[0] << 8 | in[1]);
    k.kind = in[2];
    k.family = in[3];
    memcpy(k.daddr, &in[4], 16);
    memcpy(k.saddr, &in[20], 16);
    memcpy(&k.dport, &in[36], 2);
    memcpy(&k.sport, &in[38], 2);
    k.nexthdr = in[40];
    k.flags = in[41];
    return k;
  }
  // The key's words as frame_ct_verdict builds them.
  template <int W>
  static CtKey<W> dev_key(const Key& in) {
    constexpr int A = (W - 2) / 2;
    CtKey<W> k;
    memcpy(&k.w[0], &in[4], 4 * A);
    memcpy(&k.w[A], &in[20], 4 * A);
    memcpy(&k.w[W - 2], &in[36], 4);
    k.w[W - 1] = in[40] | (uint32_t)(in[41] | (in[2] == CG_CT_MAP_ANY ? kCtKindBit : 0u)) << 8 |
                 (uint32_t)(in[0] << 8 | in[1]) << 16;
    return k;
  }

  // `n` keys of one family into buckets of S slots, at most S / 2 per bucket on average.
  template <int W, int S>
  void build_family(uint8_t family, std::vector<uint32_t>* t, uint32_t* mask, uint32_t* probes) const {
    size_t n = 0;
    for (const auto& kv : entries) n += kv.first[3] == family;
    size_t nb = 1;
    while (nb * (S / 2 ? S / 2 : 1) < n) nb <<= 1;
    if (S == kCt6Slots)  // three slots: one key per bucket on average
      while (nb < n) nb <<= 1;
    t->assign(nb * kCtLineWords, 0u);
    *mask = (uint32_t)(nb - 1);
    *probes = 0;
    for (const auto& kv : entries) {
      if (kv.first[3] != family) continue;
      const CtKey<W> k = dev_key<W>(kv.first);
      const uint32_t h = ct_hash(k) & *mask;
      for (uint32_t p = 0;; ++p) {
        uint32_t* line = t->data() + (size_t)((h + p) & *mask) * kCtLineWords;
        const uint32_t cnt = (line[31] >> 16) & 0xFF;
        if (cnt == (uint32_t)S) continue;  // nb * S > n: a bucket with room exists
        for (int i = 0; i < W; ++i) line[W * cnt + i] = k.w[i];
        // a TUPLE_F_SERVICE key is created with rev_nat_index 0 (lb.h:714-715 runs before :750): its 16 bits
        // hold the entry's slave, which lb*_local reads (lb_walk.h)
        const uint16_t v16 = kv.first[41] & CG_TUPLE_F_SERVICE ? kv.second.slave : kv.second.rev_nat_index;
        line[W * S + cnt / 2] |= (uint32_t)v16 << (16 * (cnt & 1));
        line[31] += 1u << 16;
        if (kv.second.flags & CG_CT_E_LB_LOOPBACK) line[31] |= 1u << (24 + cnt);
        if (p > *probes) *probes = p;
        break;
      }
    }
  }
  void build_tables() {
    build_family<kCt4Words, kCt4Slots>(4, &t4, &mask4, &probes4);
    build_family<kCt6Words, kCt6Slots>(6, &t6, &mask6, &probes6);
  }
  template <class Ptr>
  CtMapDev view(Ptr ptr) const {
    CtMapDev d{};
    d.t4 = ptr(t4);
    d.t6 = ptr(t6);
    d.mask4 = mask4;
    d.mask6 = mask6;
    d.probes4 = probes4;
    d.probes6 = probes6;
    d.global = global;
    return d;
  }
  CtMapDev host_view() const { return view(HostPtr{}); }
  void rebuild(Engine& e) {
    build_tables();
    if (e.has_gpu()) {
      e.set_device();
      auto t = std::make_shared<DevTables>();
      const CtMapDev d = view([&](const auto& v) { return t->add(v); });
      tab = std::move(t);  // publish (the caller holds the handle lock)
      dev = d;
    }
    dirty = false;
  }
};

}  // namespace cg
