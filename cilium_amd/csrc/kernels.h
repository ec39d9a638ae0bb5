// kernels.h — host-callable launchers of the gfx950 kernels (kernels.hip).
#pragma once

#include <cstddef>
#include <cstdint>

#include "ct_walk.h"
#include "dev_types.h"
#include "lb_walk.h"

namespace cg {

// All launchers enqueue on `stream` (hipStream_t) and return the hipError_t
// of the launch.  n == 0 launches nothing.
// mode: CG_L4_CAN_ACCESS / CG_L4_INGRESS / CG_L4_EGRESS [| CG_L4_IGNORE_DROP].
int launch_l4(const L4Dev& t, const void* tuples, size_t n, int32_t* out, uint32_t mode, void* stream, int cus);
// launch_l4 with each tuple's identity taken from the ipcache resolution of
// addrs[i] (remote address, network order: u32 for family 4, 16 bytes for 6).
int launch_l4_ipcache(const L4Dev& t, const IpcacheDev& ipc, int family, const void* addrs, const void* tuples,
                      size_t n, int32_t* out, uint32_t mode, void* stream, int cus);
// The policy program array (kernels_l4_array.hip): tuple i is judged by the
// map in slot lxc[i] of A, CG_DROP_MISSED_TAIL_CALL for an empty slot.
// family 0: the tuple's own identity; 4 / 6: the ipcache resolution of
// addrs[i], as launch_l4_ipcache.
int launch_l4_array(const L4ArrDev& A, const IpcacheDev& ipc, int family, const void* addrs, const uint16_t* lxc,
                    const void* tuples, size_t n, int32_t* out, uint32_t mode, void* stream, int cus);
// L4 verdicts from raw frames (kernels_l4_frames.hip): frame i of a batch is
// raw[off[i] .. off[i+1]).  A launcher takes device buffers; capi.cc carries
// an entry's host buffers in the same struct up to the staging.
struct FramesBatch {
  const uint8_t* raw;
  const uint64_t* off;
  size_t n;
  const uint16_t* lxc;
  const uint32_t* labels;
  const uint32_t* pkt_len;  // may be NULL
  int32_t* out;
  cg_l4_frame_info* info;  // may be NULL
  cg_ct_record* recs;      // may be NULL; not written without a conntrack map
  uint32_t mode;
};
// The ingress program per frame (frame_walk.h).  E: the endpoint map that names
// each frame's endpoint by destination address, or NULL and lxc[i] names it;
// ipc: the ipcache that resolves the source address, or NULL and labels[i] is
// the source identity; C: the conntrack map of the lookup in front of the
// policy (ct_walk.h), or NULL and the kernel without the lookup runs.
int launch_l4_frames(const L4ArrDev& A, const EpMapDev* E, const IpcacheDev* ipc, const CtMapDev* C,
                     const FramesBatch& b, void* stream, int cus);
// The from-container program per frame (egress_walk.h): lxc is mandatory, H the
// array's endpoint headers; ipc NULL: labels are the destination identities.
int launch_l4_frames_egress(const L4ArrDev& A, const EpHdrDev& H, const IpcacheDev* ipc, const CtMapDev* C,
                            const FramesBatch& b, void* stream, int cus);
// The same program over a services map (lb_walk.h): T carries the headers, the
// service tables and the per-frame hash / svc_records / xlate arrays.
int launch_l4_frames_egress_svc(const L4ArrDev& A, const EpHdrSvcDev& T, const IpcacheDev& ipc, const CtMapDev& C,
                                const FramesBatch& b, void* stream, int cus);
int launch_lpm(const LpmDev& t, bool v4_filter, bool v6_filter, const uint32_t* v4, size_t n4,
               uint8_t* out4, const uint8_t* v6, size_t n6, uint8_t* out6, void* stream, int cus);
// order (optional): out[order[slot]] instead of out[slot] (request order;
// an entry >= nout, e.g. 0xFFFFFFFF = padding, writes nothing) — the
// raw-request batches.
// rule (optional): per slot (or order[slot]) the first matching rule's
// counter index, 0xFFFFFFFF when no rule allows.
// codes (optional): the batch's strings are raw bytes (the device-layout raw
// path writes them uncoded) and class-mode programs code them through these
// per-program 256-byte maps (HttpRawDev.codes) as they walk.
int launch_http(const HttpDev& t, const void* records, size_t n, const uint8_t* arena, uint8_t* out,
                void* stream, int cus, const uint32_t* order = nullptr, uint32_t* rule = nullptr,
                uint32_t nout = 0xFFFFFFFFu, const uint8_t* codes = nullptr);
int launch_ipcache(const IpcacheDev& t, const uint32_t* v4, size_t n4, IpcVal* out4, const uint8_t* v6, size_t n6,
                   IpcVal* out6, void* stream, int cus);
// tails (optional): the split layout — reqs holds 16-byte heads, tails the
// 48-byte topic ids of each request (cg_kafka_verdicts_split_*).
int launch_kafka(const KafkaDev& t, const void* reqs, size_t n, const uint32_t* arena, uint8_t* out,
                 void* stream, int cus, const void* tails = nullptr);
// Kafka wire decode (kernels_kafka.hip): records + statuses (kKwDefer for the
// host to finish); ctr[0] arena entries reserved, ctr[1] deferred requests
// (both zeroed by the caller).
int launch_kafka_decode(const KafkaDictDev& topics, const KafkaDictDev& clients, const uint8_t* raw,
                        const uint64_t* off, size_t n, const uint16_t* redirect, const uint32_t* remote, void* recs,
                        uint32_t* arena, size_t arena_cap, unsigned long long* ctr, uint8_t* status, void* stream,
                        int cus, uint32_t* defer_list, uint8_t* zarena, size_t zcap);

// Raw HTTP/1 heads → batch (kernels_http_raw.hip; sequences in http_raw.cc).
// Both sequences take the requests as a RawReqs (dev_types.h) and start with
// a scan launch — the scan kernel, whose front end (raw_scan_waves) parses
// the requests that lie inside their wave's LDS stage, and a second kernel
// that finishes the others from the scan's deferred list.  lists: the
// requests are cg_http_pack header lists instead of HTTP/1 heads.
//
// The host-layout sequence (CILIUM_GPU_RAW_LAYOUT=host).  The scan and rank
// kernels run http_raw_grid(R, lists, n, cus) blocks over the requests in
// the same order.  With http_raw_lds_keys(R) the scan writes
// per-block bucket counts (counts[key * grid + block]) and raw_prefix turns
// them into per-block slot offsets (bbase) and totals (hist); otherwise the
// scan adds into a global histogram (counts = hist) and the rank takes slots
// from global cursors.  sbuf: the request-ordered string buffer
// (records per request, http_raw.cc), cst its per-request stride.  A list
// longer than kFieldsMaxList sets kRawListTooLong in *ovf_bytes.  The
// deferred list is dlist (*dcount, zeroed by the caller; room for n).
constexpr unsigned long long kRawListTooLong = 1ull << 63;
size_t http_raw_grid(const HttpRawDev& R, bool lists, size_t n, int cus);
bool http_raw_lds_keys(const HttpRawDev& R);
int launch_http_raw_scan(const HttpRawDev& R, bool lists, const RawReqs& q, uint32_t* counts, void* rinfo,
                         uint8_t* sbuf, uint32_t cst, unsigned long long* ovf_bytes, uint32_t* dlist,
                         uint32_t* dcount, void* stream, int cus);
int launch_http_raw_prefix(const uint32_t* bcount, uint32_t nkeys, uint32_t nblk, uint32_t* bbase, uint32_t* hist,
                           void* stream);
int launch_http_raw_rank(const HttpRawDev& R, bool lists, size_t n, const void* rinfo, uint32_t* cursor,
                         const uint32_t* bbase, uint32_t* order, void* stream, int cus);
int launch_http_raw_build(const HttpRawDev& R, const HttpRawRun* runs, uint32_t nruns, uint32_t ntiles,
                          HttpTile* ttab, uint8_t* tiles, uint32_t* order, const uint8_t* sbuf, uint8_t* arena,
                          unsigned long long* arena_cursor, void* stream, int cus);

// The device-layout sequence (the default; all on one stream with no host
// round trip): launch_http_raw_dl_scan puts each request into its slot of
// the batch laid out by L (dev_types.h RawLayoutDev) or on L's walk list;
// launch_http_raw_seal pads the last tiles and writes the chunk table and
// header; then launch_http over the batch (order = L.order) and
// launch_http_raw_walk for the walk list.
size_t http_raw_dl_grid(const HttpRawDev& R, bool lists, size_t n, int cus);
int launch_http_raw_dl_scan(const HttpRawDev& R, bool lists, const RawReqs& q, const RawLayoutDev& L, void* stream,
                            int cus);
int launch_http_raw_seal(const HttpRawDev& R, const RawLayoutDev& L, void* batch, uint32_t epoch, uint64_t ttab_off,
                         uint64_t tiles_off, uint64_t total_bytes, void* stream);
int launch_http_raw_walk(const HttpDev& T, const HttpRawDev& R, bool lists, const RawReqs& q, const RawLayoutDev& L,
                         uint8_t* out, void* stream, int cus);

// The persistent verdict ring (ring.cc): nwg one-wave workgroups serving
// the slots of G until its stop word, idle_ticks without a call or
// life_ticks; `state` is http_ring_state_bytes() of zeroed device memory.
// LDS of the ring kernel: `cells` of program block, the list parser's tables
// when `tabs`; ring_tables_small: tables small enough to stage always
size_t ring_lds_bytes(const HttpRawDev& R, uint32_t cells, bool tabs);
bool ring_tables_small(const HttpRawDev& R);
size_t http_ring_state_bytes();
int launch_http_ring(const HttpDev& HT, const HttpRawDev& R, const HttpRingDev& G, void* state, void* stream);
// the device's wall_clock64() into *d_out (ring.cc measures its rate)
int ring_clock(unsigned long long* d_out, void* stream);

// The selector cache (kernels_selcache.hip).  bits[T.n][I.words]: one ballot
// word per (selector, 64-identity group), padding bits zero.  The label
// section's whole words come from selcache_match_kernel; with a prefix section
// (I.nc) the words from I.n / 64 on come from selcache_cidr_match_kernel.
int launch_selcache_match(const ScIdentDev& I, const ScSelDev& T, unsigned long long* bits, void* stream, int cus);
// ing/eg[n][words], flags[n] for the endpoints eps[n] (identity indices; an
// index >= n_ids yields zero rows).  R.M is the rule selectors' match matrix.
int launch_selcache_reach(const ScRuleDev& R, uint32_t n_ids, uint32_t words, const uint32_t* eps, size_t n,
                          unsigned long long* ing, unsigned long long* eg, uint8_t* flags, void* stream);
// Expansion: count per row into row_off[0..R), exclusive scan in place to
// row_off[0..R] (and *total when not NULL), then emit keys[total] / proxy[total]
// unless total > cap.  keys is 8-byte aligned.  R = 0 runs the scan alone.
int launch_selcache_expand(const ScExpDev& X, unsigned long long* row_off, void* keys, uint16_t* proxy,
                           unsigned long long cap, unsigned long long* total, void* stream, int cus);
// Words of a row one emit round of a block covers (one per lane).
uint32_t selcache_expand_span();

}  // namespace cg
