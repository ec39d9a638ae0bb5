// egress_standalone.cc — the host evaluator path of the egress frames route
// (cg_diag_l4_frames_egress_eval_host → egress_walk.h over the host views),
// the endpoint headers' calls and cg_ct_map_apply on egress records, driven
// through the C API from a program of its own, so that it can be linked with
// AddressSanitizer + UBSan and run as it is (tools/sanitize/egress_standalone.py
// builds it, writes the worlds and runs it).  No GPU: the handle is host-only.
//
// Input: a file of sections {u32 name length, name, u64 bytes, data} holding a
// world (maps, slots, headers, ipcache, conntrack keys), a frame batch and the
// verdicts, info and records the Python oracle expects for it.
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
    // maps, the array and its headers
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
    uint32_t arr = 0, ipc = 0, ct = 0;
    OK(cg_policy_array_create(h, &arr));
    const size_t n_slots = S["slots"].size() / 2;
    std::vector<uint32_t> slot_maps(n_slots);
    for (size_t i = 0; i < n_slots; ++i) slot_maps[i] = map_ids[as<uint32_t>(S["slot_maps"])[i]];
    OK(cg_policy_array_set(h, arr, as<uint16_t>(S["slots"]), slot_maps.data(), n_slots));
    const size_t n_hdr = S["hdr_slots"].size() / 2;
    OK(cg_policy_array_set_headers(h, arr, as<uint16_t>(S["hdr_slots"]), as<cg_endpoint_header>(S["hdrs"]), n_hdr));
    for (size_t i = 0; i < n_hdr; ++i) {
      cg_endpoint_header back;
      OK(cg_policy_array_get_header(h, arr, as<uint16_t>(S["hdr_slots"])[i], &back));
      CHECK(!memcmp(&back, as<cg_endpoint_header>(S["hdrs"]) + i, sizeof(back)), "header %zu reads back differently", i);
    }
    cg_endpoint_header bad = as<cg_endpoint_header>(S["hdrs"])[0];
    bad.flags = 0x100;
    CHECK(cg_policy_array_set_headers(h, arr, as<uint16_t>(S["hdr_slots"]), &bad, 1) == CG_INVALID_ARGUMENT,
          "unknown header flags accepted");
    OK(cg_ipcache_create(h, 0, &ipc));
    OK(cg_ipcache_update(h, ipc, as<cg_cidr>(S["ipc_keys"]), as<cg_remote_endpoint_info>(S["ipc_vals"]),
                         S["ipc_keys"].size() / sizeof(cg_cidr)));
    OK(cg_ct_map_create(h, 0, 0, &ct));
    const size_t n_ct = S["ct_keys"].size() / sizeof(cg_ct_key);
    if (n_ct) OK(cg_ct_map_update(h, ct, as<cg_ct_key>(S["ct_keys"]), as<cg_ct_entry>(S["ct_vals"]), n_ct));
    // the batch
    const uint8_t* raw = S["raw"].data();
    const uint64_t* off = as<uint64_t>(S["off"]);
    const size_t n = S["off"].size() / 8 - 1;
    const uint16_t* lxc = as<uint16_t>(S["lxc"]);
    const uint32_t* labels = as<uint32_t>(S["labels"]);
    const uint32_t* plen = S["plen"].empty() ? nullptr : as<uint32_t>(S["plen"]);
    std::vector<int32_t> v(n);
    std::vector<cg_l4_frame_info> info(n);
    std::vector<cg_ct_record> rec(n);
    std::vector<uint32_t> l4o(n);
    for (int use_ipc = 0; use_ipc < 2; ++use_ipc)
      for (int use_ct = 0; use_ct < 2; ++use_ct)
        for (int ign = 0; ign < 2; ++ign) {
          const std::string tag = std::string(use_ipc ? "ipc" : "lab") + (use_ct ? "_ct" : "_noct") + (ign ? "_ign" : "");
          if (!S.count("v_" + tag)) continue;
          const uint32_t mode = CG_L4_EGRESS | (ign ? CG_L4_IGNORE_DROP : 0);
          // the whole batch, then windows that start past 0 and end before the blob does
          const size_t sizes[] = {n, 1, 63, 64, 65, 1000};
          for (size_t k = 0; k < 6; ++k) {
            const size_t first = k ? 5 * k : 0, cnt = sizes[k];
            if (first + cnt > n) continue;
            OK(cg_diag_l4_frames_egress_eval_host(h, arr, mode, raw, off + first, cnt, lxc + first,
                                                  use_ipc ? nullptr : labels + first, use_ipc ? ipc : 0,
                                                  plen ? plen + first : nullptr, use_ct ? ct : 0, v.data(), info.data(),
                                                  use_ct ? rec.data() : nullptr, l4o.data()));
            CHECK(!memcmp(v.data(), as<int32_t>(S["v_" + tag]) + first, cnt * 4), "%s %s n=%zu: verdicts differ",
                  argv[a], tag.c_str(), cnt);
            CHECK(!memcmp(info.data(), as<cg_l4_frame_info>(S["info_" + tag]) + first, cnt * sizeof(cg_l4_frame_info)),
                  "%s %s n=%zu: info differs", argv[a], tag.c_str(), cnt);
            if (use_ct)
              CHECK(!memcmp(rec.data(), as<cg_ct_record>(S["rec_" + tag]) + first, cnt * sizeof(cg_ct_record)),
                    "%s %s n=%zu: records differ", argv[a], tag.c_str(), cnt);
          }
        }
    // apply the last records (egress: dir 1) to a fresh map and to one that is too small
    if (S.count("v_lab_ct")) {
      OK(cg_diag_l4_frames_egress_eval_host(h, arr, CG_L4_EGRESS, raw, off, n, lxc, labels, 0, plen, ct, v.data(), nullptr,
                                            rec.data(), nullptr));
      uint32_t fresh = 0, small = 0;
      OK(cg_ct_map_create(h, 0, 0, &fresh));
      OK(cg_ct_map_create(h, 3, 0, &small));
      std::vector<int32_t> res(n);
      OK(cg_ct_map_apply(h, fresh, rec.data(), n, plen, nullptr, res.data()));
      OK(cg_ct_map_apply(h, small, rec.data(), n, plen, labels, res.data()));
      size_t total = 0;
      OK(cg_ct_map_dump(h, fresh, nullptr, nullptr, 0, &total));
      std::vector<cg_ct_key> keys(total);
      std::vector<cg_ct_entry> vals(total);
      OK(cg_ct_map_dump(h, fresh, keys.data(), vals.data(), total, &total));
      size_t creates = 0;
      for (size_t i = 0; i < n; ++i) creates += rec[i].op == CG_CT_OP_CREATE;
      CHECK(creates == 0 || total > 0, "apply wrote nothing");
      for (size_t i = 0; i < total; ++i)
        CHECK(vals[i].tx_packets == 1 && vals[i].rx_packets == 0, "an egress entry counts rx");
      OK(cg_ct_map_destroy(h, fresh));
      OK(cg_ct_map_destroy(h, small));
    }
    OK(cg_policy_array_clear_headers(h, arr, as<uint16_t>(S["hdr_slots"]), n_hdr));
    OK(cg_ct_map_destroy(h, ct));
    OK(cg_ipcache_destroy(h, ipc));
    OK(cg_policy_array_destroy(h, arr));
    for (uint32_t id : map_ids) OK(cg_policymap_destroy(h, id));
    cg_close(h);
    printf("%s: %zu frames, %s\n", argv[a], n, failures ? "FAILED" : "ok");
  }
  return failures ? 1 : 0;
}
