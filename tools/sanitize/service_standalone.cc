// service_standalone.cc — the host side of service load-balancing on the egress
// frames route (cg_lb_map_*, cg_diag_l4_frames_egress_svc_eval_host → egress_walk.h
// and lb_walk.h over the host views, cg_ct_map_apply on service and egress
// records), driven through the C API from a program of its own, so that it can
// be linked with AddressSanitizer + UBSan and run as it is
// (tools/sanitize/service_standalone.py builds it, writes the worlds and runs
// it).  No GPU: the handle is host-only.
//
// Input: a file of sections {u32 name length, name, u64 bytes, data} holding a
// world (maps, slots, headers, ipcache, conntrack entries, service and
// reverse-NAT entries), a frame batch with its hashes, and the verdicts, info,
// both record arrays and the translation records the Python oracle expects.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "cilium_gpu.h"

namespace {

using Bytes = std::vector<uint8_t>;
std::map<std::string, Bytes> load(const char* path) {
  std::map<std::string, Bytes> out;
  FILE* f = fopen(path, "rb");
  if (!f) return out;
  uint32_t nl;
  while (fread(&nl, 4, 1, f) == 1) {
    std::string name(nl, '\0');
    uint64_t n = 0;
    if (fread(&name[0], 1, nl, f) != nl || fread(&n, 8, 1, f) != 1) break;
    Bytes b(n);
    if (n && fread(b.data(), 1, n, f) != n) break;
    out[name] = std::move(b);
  }
  fclose(f);
  return out;
}

int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
      ++failures;                   \
    }                               \
  } while (0)
#define OK(call) CHECK((call) == CG_OK, "%s: %s", #call, cg_last_error())

template <class T>
const T* as(const Bytes& b) {
  return reinterpret_cast<const T*>(b.data());
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s world.bin...\n", argv[0]);
    return 2;
  }
  for (int a = 1; a < argc; ++a) {
    auto S = load(argv[a]);
    if (!S.count("raw")) {
      fprintf(stderr, "%s: not a world file\n", argv[a]);
      return 2;
    }
    const cg_kv params[] = {{"device", "-1"}};
    const uint64_t h = cg_open(params, 1, 0);
    CHECK(h != 0, "cg_open: %s", cg_last_error());
    const uint32_t n_maps = *as<uint32_t>(S["n_maps"]);
    std::vector<uint32_t> map_ids(n_maps);
    for (uint32_t m = 0; m < n_maps; ++m) {
      const std::string p = "map" + std::to_string(m);
      OK(cg_policymap_create(h, *as<uint32_t>(S[p + "_max"]), &map_ids[m]));
      const Bytes& k = S[p + "_keys"];
      if (!k.empty())
        OK(cg_policymap_allow(h, map_ids[m], as<cg_policy_key>(k), as<uint16_t>(S[p + "_ports"]),
                              k.size() / sizeof(cg_policy_key)));
    }
    uint32_t arr = 0, ipc = 0, ct = 0, lb = 0;
    OK(cg_policy_array_create(h, &arr));
    const size_t n_slots = S["slots"].size() / 2;
    std::vector<uint32_t> slot_maps(n_slots);
    for (size_t i = 0; i < n_slots; ++i) slot_maps[i] = map_ids[as<uint32_t>(S["slot_maps"])[i]];
    OK(cg_policy_array_set(h, arr, as<uint16_t>(S["slots"]), slot_maps.data(), n_slots));
    const size_t n_hdr = S["hdr_slots"].size() / 2;
    OK(cg_policy_array_set_headers(h, arr, as<uint16_t>(S["hdr_slots"]), as<cg_endpoint_header>(S["hdrs"]), n_hdr));
    OK(cg_ipcache_create(h, 0, &ipc));
    OK(cg_ipcache_update(h, ipc, as<cg_cidr>(S["ipc_keys"]), as<cg_remote_endpoint_info>(S["ipc_vals"]),
                         S["ipc_keys"].size() / sizeof(cg_cidr)));
    OK(cg_ct_map_create(h, 0, 0, &ct));
    const size_t n_ct = S["ct_keys"].size() / sizeof(cg_ct_key);
    if (n_ct) OK(cg_ct_map_update(h, ct, as<cg_ct_key>(S["ct_keys"]), as<cg_ct_entry>(S["ct_vals"]), n_ct));
    // the service map: raw ops, dump order, all-or-nothing
    OK(cg_lb_map_create(h, 0, 0, &lb));
    OK(cg_lb_map_set_loopback(h, lb, *as<uint32_t>(S["loopback"])));
    const size_t n_svc = S["svc_keys"].size() / sizeof(cg_lb_key), n_rn = S["rn_keys"].size() / sizeof(cg_lb_revnat_key);
    if (n_svc) OK(cg_lb_map_service_update(h, lb, as<cg_lb_key>(S["svc_keys"]), as<cg_lb_service>(S["svc_vals"]), n_svc));
    if (n_rn) OK(cg_lb_map_revnat_update(h, lb, as<cg_lb_revnat_key>(S["rn_keys"]), as<cg_lb_revnat>(S["rn_vals"]), n_rn));
    size_t total = 0;
    OK(cg_lb_map_service_dump(h, lb, nullptr, nullptr, 0, &total));
    CHECK(total == n_svc, "service dump counts %zu of %zu", total, n_svc);
    std::vector<cg_lb_key> dk(total);
    std::vector<cg_lb_service> dv(total);
    OK(cg_lb_map_service_dump(h, lb, dk.data(), dv.data(), total, &total));
    for (size_t i = 0; i < total; ++i) {
      cg_lb_service one;
      OK(cg_lb_map_service_lookup(h, lb, &dk[i], &one));
      CHECK(!memcmp(&one, &dv[i], sizeof(one)), "service %zu: lookup and dump differ", i);
      if (i) {
        const int c = dk[i - 1].family != dk[i].family ? (dk[i - 1].family < dk[i].family ? -1 : 1)
                                                       : memcmp(dk[i - 1].address, dk[i].address, 16);
        CHECK(c <= 0, "service dump out of order at %zu", i);
      }
    }
    if (total) {
      cg_lb_key two[2] = {dk[0], dk[0]};
      two[1].slave = 65535;  // absent: nothing is deleted
      CHECK(cg_lb_map_service_delete(h, lb, two, 2) == CG_NOT_FOUND, "a delete with an absent key went through");
      OK(cg_lb_map_service_delete(h, lb, &dk[0], 1));
      cg_lb_service gone;
      CHECK(cg_lb_map_service_lookup(h, lb, &dk[0], &gone) == CG_NOT_FOUND, "a deleted key is still there");
      OK(cg_lb_map_service_update(h, lb, &dk[0], &dv[0], 1));
    }
    OK(cg_lb_map_revnat_dump(h, lb, nullptr, nullptr, 0, &total));
    CHECK(total == n_rn, "reverse NAT dump counts %zu of %zu", total, n_rn);
    std::vector<cg_lb_revnat_key> rk(total);
    std::vector<cg_lb_revnat> rv(total);
    OK(cg_lb_map_revnat_dump(h, lb, rk.data(), rv.data(), total, &total));
    for (size_t i = 0; i < total; ++i) {
      cg_lb_revnat one;
      OK(cg_lb_map_revnat_lookup(h, lb, &rk[i], &one));
      CHECK(!memcmp(&one, &rv[i], sizeof(one)), "reverse NAT %zu: lookup and dump differ", i);
    }
    // the batch
    const uint8_t* raw = S["raw"].data();
    const uint64_t* off = as<uint64_t>(S["off"]);
    const size_t n = S["off"].size() / 8 - 1;
    const uint16_t* lxc = as<uint16_t>(S["lxc"]);
    const uint32_t* hash = as<uint32_t>(S["hash"]);
    const uint32_t* plen = S["plen"].empty() ? nullptr : as<uint32_t>(S["plen"]);
    std::vector<int32_t> v(n);
    std::vector<cg_l4_frame_info> info(n);
    std::vector<cg_ct_record> rec(n), srec(n);
    std::vector<cg_lb_xlate> xl(n);
    std::vector<uint32_t> l4o(n);
    for (int use_hash = 0; use_hash < 2; ++use_hash)
      for (int ign = 0; ign < 2; ++ign) {
        const std::string tag = std::string(use_hash ? "hash" : "null") + (ign ? "_ign" : "");
        if (!S.count("v_" + tag)) continue;
        const uint32_t mode = CG_L4_EGRESS | (ign ? CG_L4_IGNORE_DROP : 0);
        // the whole batch, then windows that start past 0 and end before the blob does
        const size_t sizes[] = {n, 1, 63, 64, 65, 1000}, firsts[] = {0, 3, 5, 7, 11, 13};
        for (size_t k = 0; k < 6; ++k) {
          const size_t first = firsts[k], cnt = sizes[k];
          if (first + cnt > n) continue;
          OK(cg_diag_l4_frames_egress_svc_eval_host(h, arr, mode, raw, off + first, cnt, lxc + first, nullptr, ipc,
                                                    plen ? plen + first : nullptr, ct, lb,
                                                    use_hash ? hash + first : nullptr, v.data(), info.data(), rec.data(),
                                                    srec.data(), xl.data(), l4o.data()));
          const struct {
            const char* what;
            const void* got;
            std::string want;
            size_t elem;
          } outs[] = {{"verdicts", v.data(), "v_", 4},
                      {"info", info.data(), "info_", sizeof(cg_l4_frame_info)},
                      {"records", rec.data(), "rec_", sizeof(cg_ct_record)},
                      {"service records", srec.data(), "srec_", sizeof(cg_ct_record)},
                      {"translation records", xl.data(), "xl_", sizeof(cg_lb_xlate)}};
          for (const auto& o : outs)
            CHECK(!memcmp(o.got, S[o.want + tag].data() + first * o.elem, cnt * o.elem), "%s %s n=%zu: %s differ", argv[a],
                  tag.c_str(), cnt, o.what);
        }
        // optional outputs left out
        OK(cg_diag_l4_frames_egress_svc_eval_host(h, arr, mode, raw, off, n, lxc, nullptr, ipc, plen, ct, lb, nullptr,
                                                  v.data(), nullptr, nullptr, nullptr, nullptr, nullptr));
      }
    CHECK(cg_diag_l4_frames_egress_svc_eval_host(h, arr, CG_L4_EGRESS, raw, off, n, lxc, nullptr, ipc, plen, 0, lb, nullptr,
                                                 v.data(), nullptr, nullptr, nullptr, nullptr,
                                                 nullptr) == CG_INVALID_ARGUMENT,
          "a service map without a conntrack map went through");
    // apply: the service records, then the egress records, twice (a duplicate CREATE leaves the map as it is)
    if (S.count("v_hash_ign")) {
      OK(cg_diag_l4_frames_egress_svc_eval_host(h, arr, CG_L4_EGRESS | CG_L4_IGNORE_DROP, raw, off, n, lxc, nullptr, ipc,
                                                plen, ct, lb, hash, v.data(), nullptr, rec.data(), srec.data(), nullptr,
                                                nullptr));
      uint32_t fresh = 0, small = 0;
      OK(cg_ct_map_create(h, 0, 0, &fresh));
      OK(cg_ct_map_create(h, 2, 0, &small));
      std::vector<int32_t> res(n);
      size_t after[2] = {0, 0};
      for (int round = 0; round < 2; ++round) {
        OK(cg_ct_map_apply(h, fresh, srec.data(), n, plen, nullptr, res.data()));
        OK(cg_ct_map_apply(h, fresh, rec.data(), n, plen, nullptr, res.data()));
        OK(cg_ct_map_dump(h, fresh, nullptr, nullptr, 0, &after[round]));
      }
      CHECK(after[0] == after[1], "a second apply changed the map: %zu then %zu keys", after[0], after[1]);
      OK(cg_ct_map_apply(h, small, srec.data(), n, plen, nullptr, res.data()));
      OK(cg_ct_map_apply(h, small, rec.data(), n, plen, nullptr, res.data()));
      std::vector<cg_ct_key> keys(after[1]);
      std::vector<cg_ct_entry> vals(after[1]);
      OK(cg_ct_map_dump(h, fresh, keys.data(), vals.data(), after[1], &after[1]));
      size_t service_keys = 0;
      for (size_t i = 0; i < after[1]; ++i) {
        CHECK(vals[i].tx_packets == 1 && vals[i].rx_packets == 0, "a service or egress entry counts rx");
        service_keys += (keys[i].flags & CG_TUPLE_F_SERVICE) != 0;
        if (keys[i].flags & CG_TUPLE_F_SERVICE) CHECK(vals[i].rev_nat_index == 0, "a service entry with rev_nat_index");
      }
      size_t creates = 0;
      for (size_t i = 0; i < n; ++i) creates += srec[i].op == CG_CT_OP_CREATE;
      CHECK(creates == 0 || service_keys > 0, "apply wrote no service key");
      OK(cg_ct_map_destroy(h, fresh));
      OK(cg_ct_map_destroy(h, small));
    }
    OK(cg_lb_map_destroy(h, lb));
    OK(cg_ct_map_destroy(h, ct));
    OK(cg_ipcache_destroy(h, ipc));
    OK(cg_policy_array_destroy(h, arr));
    for (uint32_t id : map_ids) OK(cg_policymap_destroy(h, id));
    cg_close(h);
    printf("%s: %zu frames, %s\n", argv[a], n, failures ? "FAILED" : "ok");
  }
  return failures ? 1 : 0;
}
