/*
 * cilium_gpu.h — C ABI of libciliumgpu.so, the MI355X (gfx950) batched
 * policy-verdict engine.
 *
 * This is the drop-in boundary for Cilium's data-parallel classification path
 * (SURVEY.md §8).  Every entry point is plain C: integers, pointers and sizes;
 * no C++ or torch types cross it.  Conventions kept from the reference:
 *
 *  - Return codes reuse proxylib's FilterResult numbering for the shared
 *    values (proxylib/proxylib/types.h:38-47); engine-specific codes start at
 *    16.  Nothing throws across the ABI (proxylib/proxylib/connection.go:119-135
 *    recovers panics into PARSER_ERROR; we return codes).
 *  - Buffers are caller-owned; the library never retains a caller pointer
 *    after a call returns (proxylib/proxylib.go:46-51 copies strings on entry).
 *  - Policy updates are all-or-nothing: the new tables are compiled and
 *    uploaded first, then published by a pointer swap, so a failed update
 *    leaves the previous snapshot serving (proxylib/proxylib/instance.go:180-215,
 *    envoy/cilium_network_policy.cc onConfigUpdate).
 *  - "_dev" verdict calls take DEVICE pointers and a hipStream_t (passed as
 *    void*, NULL = the handle's stream) and are asynchronous; the "_host"
 *    variants take host pointers and return when the verdicts are written.
 *
 * Each declaration cites the reference interface it replaces.
 */
#ifndef CILIUM_GPU_H
#define CILIUM_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Result codes                                                              */
/* ------------------------------------------------------------------------ */
typedef enum {
  CG_OK = 0,                  /* FILTER_OK                 types.h:39 */
  CG_POLICY_DROP = 1,         /* FILTER_POLICY_DROP        types.h:40 */
  CG_PARSER_ERROR = 2,        /* FILTER_PARSER_ERROR       types.h:41 */
  CG_UNKNOWN_PARSER = 3,      /* FILTER_UNKNOWN_PARSER     types.h:42 */
  CG_UNKNOWN_CONNECTION = 4,  /* FILTER_UNKNOWN_CONNECTION types.h:43 */
  CG_INVALID_ADDRESS = 5,     /* FILTER_INVALID_ADDRESS    types.h:44 */
  CG_INVALID_INSTANCE = 6,    /* FILTER_INVALID_INSTANCE   types.h:45 */
  CG_UNKNOWN_ERROR = 7,       /* FILTER_UNKNOWN_ERROR      types.h:46 */
  /* engine-specific */
  CG_INVALID_ARGUMENT = 16,
  CG_NO_DEVICE = 17,          /* no usable gfx950 device / HIP error at open */
  CG_DEVICE_ERROR = 18,       /* a HIP call failed */
  CG_POLICY_REJECTED = 19,    /* policy failed to parse/compile; old snapshot kept */
  CG_REVISION_MISMATCH = 20,  /* prefilter.go:131-133 "Latest revision is %d not %d" */
  CG_MAP_FULL = 21,           /* bpf map E2BIG: more keys than max_entries */
  CG_NOT_FOUND = 22,          /* key/CIDR/policy not present (ENOENT) */
  CG_NO_MAP = 23,             /* prefilter.go:137-139 "No map enabled for CIDR" */
  CG_UNSUPPORTED = 24         /* regex construct outside the supported subset */
} cg_result;

typedef struct {
  const char* key;
  const char* value;
} cg_kv;

/* ------------------------------------------------------------------------ */
/* Module lifetime — replaces proxylib OpenModule/CloseModule                */
/* (proxylib/libcilium.h:107-115, proxylib/proxylib.go:118-155).             */
/* params: "device" = HIP device ordinal (default "0").                      */
/* Returns 0 on error (same convention as OpenModule).  Host-only work       */
/* (policy compilation, table builds) works on a handle opened with          */
/* "device" = "-1" (no GPU); verdict calls on such a handle return           */
/* CG_NO_DEVICE — there is no CPU fallback.                                  */
/* ------------------------------------------------------------------------ */
uint64_t cg_open(const cg_kv* params, size_t n_params, uint8_t debug);
void cg_close(uint64_t h);
/* Last error message of the calling thread (static storage, never NULL). */
const char* cg_last_error(void);
/* Library/kernels build string, e.g. "libciliumgpu gfx950 r1". */
const char* cg_version(void);

/* ======================================================================== */
/* L4: policymap verdicts — bpf/lib/policy.h:46-163                          */
/* ======================================================================== */

/* struct policy_key, bpf/lib/common.h:180-186; Go PolicyKey,
 * pkg/maps/policymap/policymap.go:64-69.  dport in NETWORK byte order. */
typedef struct {
  uint32_t sec_label;
  uint16_t dport;     /* network byte order */
  uint8_t protocol;   /* u8proto: TCP=6, UDP=17 (pkg/u8proto/u8proto.go:27-28) */
  uint8_t egress;     /* bit0: TrafficDirection Ingress=0/Egress=1 (trafficdirection.go:20-29) */
} cg_policy_key;

/* struct policy_entry, bpf/lib/common.h:188-193; Go PolicyEntry,
 * policymap.go:73-80.  proxy_port in NETWORK byte order. */
typedef struct {
  uint16_t proxy_port; /* network byte order */
  uint16_t pad[3];
  uint64_t packets;
  uint64_t bytes;
} cg_policy_entry;

/* One packet to classify: the arguments of __policy_can_access
 * (bpf/lib/policy.h:46-49) that reach the verdict, packed to 12 bytes. */
typedef struct {
  uint32_t identity;   /* sec_label of the remote endpoint */
  uint16_t dport;      /* network byte order (tuple.dport) */
  uint8_t proto;       /* tuple.nexthdr */
  uint8_t flags;       /* CG_L4_F_* */
  uint32_t len;        /* skb->len, added to policy_entry.bytes on a hit */
} cg_l4_tuple;

#define CG_L4_F_INGRESS 0x01u   /* dir == CT_INGRESS (common.h:328); else CT_EGRESS */
#define CG_L4_F_FRAGMENT 0x02u  /* is_fragment */
#define CG_L4_F_CB_POLICY 0x04u /* skb->cb[CB_POLICY] set (policy.h:98) */

/* Verdict values written per tuple (int32), identical to the return of
 * __policy_can_access: >0 proxy_port as stored (network order, read as a
 * host u16), 0 = TC_ACT_OK, DROP_POLICY = -133 (common.h:240),
 * DROP_FRAG_NOSUPPORT = -157 (common.h:264). */
#define CG_DROP_POLICY (-133)
#define CG_DROP_FRAG_NOSUPPORT (-157)

/* Policy maps — one per endpoint, like cilium_policy_<epid>.
 * max_entries: 0 = PolicyMap MaxEntries 16384 (policymap.go:37). */
int cg_policymap_create(uint64_t h, uint32_t max_entries, uint32_t* map_id);
int cg_policymap_destroy(uint64_t h, uint32_t map_id);
/* PolicyMap.AllowKey/Allow (policymap.go:162-176): insert or update
 * proxy_port (network order) for each key.  Existing counters are kept.
 * CG_MAP_FULL if a new key would exceed max_entries (nothing applied). */
int cg_policymap_allow(uint64_t h, uint32_t map_id, const cg_policy_key* keys,
                       const uint16_t* proxy_ports_be, size_t n);
/* PolicyMap.DeleteKey/Delete (policymap.go:187-199); CG_NOT_FOUND if any key
 * is absent (nothing applied). */
int cg_policymap_delete(uint64_t h, uint32_t map_id, const cg_policy_key* keys, size_t n);
/* PolicyMap.Exists + LookupElement (policymap.go:181-185). */
int cg_policymap_lookup(uint64_t h, uint32_t map_id, const cg_policy_key* key,
                        cg_policy_entry* entry);
/* PolicyMap.DumpToSlice (policymap.go:224-255).  Writes up to cap entries,
 * sets *n to the number of entries in the map. */
int cg_policymap_dump(uint64_t h, uint32_t map_id, cg_policy_key* keys,
                      cg_policy_entry* entries, size_t cap, size_t* n);
/* PolicyMap.Flush (policymap.go:257-280). */
int cg_policymap_flush(uint64_t h, uint32_t map_id);

/* Batched policy_can_access over tuples (policy.h:46-110).  Counters of the
 * matching entry advance exactly as the BPF code's __sync_fetch_and_add
 * (policy.h:68-69,80-81,92-93).  Device pointers, async on stream. */
int cg_l4_verdicts_dev(uint64_t h, uint32_t map_id, const cg_l4_tuple* d_tuples,
                       size_t n, int32_t* d_verdicts, void* stream);
int cg_l4_verdicts_host(uint64_t h, uint32_t map_id, const cg_l4_tuple* tuples,
                        size_t n, int32_t* verdicts);

/* The verdict wrappers around __policy_can_access (bpf/lib/policy.h:126-163),
 * selected by `mode`:
 *   CG_L4_CAN_ACCESS  __policy_can_access itself: each tuple's CG_L4_F_INGRESS
 *                     and CG_L4_F_FRAGMENT flags (what cg_l4_verdicts_* do);
 *   CG_L4_INGRESS     policy_can_access_ingress (policy.h:126-146, called at
 *                     bpf_lxc.c:814,948): dir = CT_INGRESS for every tuple,
 *                     the tuple's is_fragment; any negative result becomes
 *                     DROP_POLICY (so an unmatched fragment is -133, not -157);
 *   CG_L4_EGRESS      policy_can_egress (policy.h:150-163, via
 *                     policy_can_egress{4,6} at bpf_lxc.c:220,527): dir =
 *                     CT_EGRESS, is_fragment = false; negative → DROP_POLICY.
 * OR CG_L4_IGNORE_DROP to model a datapath built with IGNORE_DROP: the
 * wrappers then return TC_ACT_OK instead of DROP_POLICY.  CG_L4_F_CB_POLICY
 * (skb->cb[CB_POLICY]) is honoured in every mode, as in policy.h:98. */
#define CG_L4_CAN_ACCESS 0u
#define CG_L4_INGRESS 1u
#define CG_L4_EGRESS 2u
#define CG_L4_IGNORE_DROP 0x100u
int cg_l4_policy_verdicts_dev(uint64_t h, uint32_t map_id, uint32_t mode, const cg_l4_tuple* d_tuples,
                              size_t n, int32_t* d_verdicts, void* stream);
int cg_l4_policy_verdicts_host(uint64_t h, uint32_t map_id, uint32_t mode, const cg_l4_tuple* tuples,
                               size_t n, int32_t* verdicts);

/* The policy program array, cilium_policy[lxc_id] (bpf/lib/maps.h:44-62):
 * delivery to a local endpoint tail-calls into that endpoint's own policy
 * program, tail_call(skb, &cilium_policy, ep->lxc_id) (bpf/lib/l3.h:99,130),
 * which runs policy_can_access_ingress on the endpoint's map (bpf_lxc.c:948).
 * Here a slot names a policy map, and the cg_l4_array_verdicts_* entries take
 * each tuple's lxc_id, so one launch judges a batch addressed to many
 * endpoints.
 *  - set and clear are all-or-nothing per call: every argument is checked
 *    before any slot changes.
 *  - A tuple that names an empty slot gets CG_DROP_MISSED_TAIL_CALL in every
 *    mode, CG_L4_IGNORE_DROP included, and moves no counter: the tail call
 *    missed, so nothing of policy.h ran (l3.h:99-100).
 *  - Destroying a policy map empties the slots that name it.  Its tables stay
 *    alive until the launches already enqueued have run.
 *  - A verdict call sees one snapshot of the whole array, taken under the
 *    handle lock: a concurrent cg_policymap_* or cg_policy_array_* update is
 *    seen by that call entirely or not at all. */
#define CG_DROP_MISSED_TAIL_CALL (-140) /* bpf/lib/common.h:247 */
#define CG_POLICY_ARRAY_SLOTS 65536u    /* POLICY_PROG_MAP_SIZE, node_config.h:62 */
int cg_policy_array_create(uint64_t h, uint32_t* arr_id);
int cg_policy_array_destroy(uint64_t h, uint32_t arr_id);
/* slot lxc_ids[i] -> map_ids[i].  CG_NOT_FOUND for an unknown map (nothing
 * applied); an lxc_id >= CG_POLICY_ARRAY_SLOTS would be CG_INVALID_ARGUMENT,
 * which a uint16_t cannot reach.  The same map may sit in several slots. */
int cg_policy_array_set(uint64_t h, uint32_t arr_id, const uint16_t* lxc_ids, const uint32_t* map_ids, size_t n);
int cg_policy_array_clear(uint64_t h, uint32_t arr_id, const uint16_t* lxc_ids, size_t n);
/* *map_id = 0 for an empty slot. */
int cg_policy_array_get(uint64_t h, uint32_t arr_id, uint16_t lxc_id, uint32_t* map_id);

/* Verdicts across endpoints: tuple i is judged by the map in slot lxc_ids[i],
 * with `mode` as cg_l4_policy_verdicts_* take it.  The verdict is bit for bit
 * what cg_l4_policy_verdicts_* return for that tuple on that map, and the
 * matching entry's packets and bytes advance exactly as there.  18 bytes per
 * tuple: 12 of cg_l4_tuple, 2 of lxc_id, 4 of verdict. */
int cg_l4_array_verdicts_dev(uint64_t h, uint32_t arr_id, uint32_t mode, const uint16_t* d_lxc_ids,
                             const cg_l4_tuple* d_tuples, size_t n, int32_t* d_verdicts, void* stream);
int cg_l4_array_verdicts_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint16_t* lxc_ids,
                              const cg_l4_tuple* tuples, size_t n, int32_t* verdicts);
/* The same with each tuple's identity taken from the ipcache resolution of
 * its remote address, as cg_l4_verdicts_ipcache*_ resolve it (family 4: u32
 * addresses in network order; 6: 16 bytes each), then `mode`. */
int cg_l4_array_verdicts_ipcache_dev(uint64_t h, uint32_t arr_id, uint32_t ipc_id, uint32_t mode, int family,
                                     const void* d_remote, const uint16_t* d_lxc_ids, const cg_l4_tuple* d_tuples,
                                     size_t n, int32_t* d_verdicts, void* stream);
int cg_l4_array_verdicts_ipcache_host(uint64_t h, uint32_t arr_id, uint32_t ipc_id, uint32_t mode, int family,
                                      const void* remote, const uint16_t* lxc_ids, const cg_l4_tuple* tuples,
                                      size_t n, int32_t* verdicts);

/* The endpoint map, cilium_lxc (bpf/lib/maps.h, struct endpoint_key /
 * endpoint_info bpf/lib/common.h:147-173, lookup_ip{4,6}_endpoint
 * bpf/lib/eps.h:26-46, pkg/maps/lxcmap/lxcmap.go): a local endpoint's address
 * -> {lxc_id, flags}.  On the device it is an exact-match table, published by
 * swap like every other table.  cg_prefilter_set_endpoints keeps its own
 * membership set. */
typedef struct {
  uint8_t family;   /* 4 or 6 */
  uint8_t pad[3];
  uint8_t addr[16]; /* network byte order; v4 uses addr[0..3] */
} cg_endpoint_key;
typedef struct {
  uint16_t lxc_id;
  uint16_t pad;
  uint32_t flags;   /* CG_ENDPOINT_F_* */
} cg_endpoint_info;
#define CG_ENDPOINT_F_HOST 1u /* EndpointFlagHost, lxcmap.go:91-92 */
/* max_entries 0 = MaxEntries 65535 (lxcmap.go:33). */
int cg_endpoint_map_create(uint64_t h, uint32_t max_entries, uint32_t* ep_id);
int cg_endpoint_map_destroy(uint64_t h, uint32_t ep_id);
/* WriteEndpoint (lxcmap.go:160-180) for each pair; an existing key is
 * overwritten.  All-or-nothing as cg_ipcache_update: CG_INVALID_ADDRESS for a
 * family other than 4 / 6, CG_MAP_FULL when the batch would exceed
 * max_entries, and nothing is applied. */
int cg_endpoint_map_update(uint64_t h, uint32_t ep_id, const cg_endpoint_key* keys, const cg_endpoint_info* values,
                           size_t n);
/* DeleteEntry (lxcmap.go:195-205); CG_NOT_FOUND (nothing deleted) if any key is absent. */
int cg_endpoint_map_delete(uint64_t h, uint32_t ep_id, const cg_endpoint_key* keys, size_t n);
int cg_endpoint_map_lookup(uint64_t h, uint32_t ep_id, const cg_endpoint_key* key, cg_endpoint_info* value);
/* DumpToMap (lxcmap.go:207-216): keys in (family, address) order; *n gets the total. */
int cg_endpoint_map_dump(uint64_t h, uint32_t ep_id, cg_endpoint_key* keys, cg_endpoint_info* values, size_t cap,
                         size_t* n);

/* L4 verdicts from raw frames: the endpoint's ingress policy program,
 * handle_policy (bpf/bpf_lxc.c:1030-1058), from the Ethernet header on.  Frame
 * i is raw[raw_off[i] .. raw_off[i+1]) (n + 1 offsets, as the raw HTTP path);
 * one launch does the header walk of ipv4_policy / ipv6_policy
 * (bpf_lxc.c:890-950, :744-816: ipv6_hdrlen lib/ipv6.h:61-98, the tuple
 * extraction of ct_lookup4/6 lib/conntrack.h:467-556, :310-400 and the CT_NEW
 * reversal :579-584) and then policy_can_access_ingress(src_label, dport,
 * nexthdr, is_fragment) on the map in the endpoint's slot of the policy
 * array, with the entry's packets and bytes advancing as in
 * cg_l4_array_verdicts_*.  The program is the one built with CONNTRACK over an
 * empty conntrack table: every packet is CT_NEW, tc_index and cb[CB_POLICY]
 * are 0.  skb_load_bytes(off, n) and revalidate_data fail when off + n passes
 * the frame's length.
 *
 * mode: CG_L4_INGRESS [| CG_L4_IGNORE_DROP]; anything else is
 * CG_INVALID_ARGUMENT.  Exactly one of each resolver pair is given (both or
 * neither: CG_INVALID_ARGUMENT):
 *  - the endpoint: lxc_ids[i] (the tail call's index), or ep_id != 0: the
 *    endpoint map looked up by the packet's destination address, the lookup
 *    in front of the tail call in from-netdev / from-overlay
 *    (bpf_netdev.c:414-420, :241-247);
 *  - cb[CB_SRC_LABEL]: src_labels[i], or ipc_id != 0: the ipcache resolution
 *    of the packet's source address exactly as cg_l4_array_verdicts_ipcache_*
 *    resolve a remote address (miss or sec_label 0: CG_WORLD_ID).  The
 *    HOST_ID exception and the packet-mark identity of bpf_netdev.c:370-389
 *    belong to the from-host caller and are not modelled.
 * pkt_len[i] is skb->len for the byte counters; NULL: the frame's length.
 *
 * Order with lxc_ids (tail_call + handle_policy):
 *  1. empty slot: CG_DROP_MISSED_TAIL_CALL; nothing is read, no counter moves;
 *  2. frame shorter than 14 bytes: CG_DROP_INVALID (the reference never sees
 *     such an skb; the engine treats the missing ethertype as an invalid
 *     packet);
 *  3. ethertype other than 0x0800 / 0x86DD: CG_DROP_UNKNOWN_L3;
 *  4. the walk: its DROP_* codes are returned as they are (neither the ingress
 *     wrapper nor CG_L4_IGNORE_DROP touches them);
 *  5. the source identity;  6. the policy verdict under `mode`.
 * Order with ep_id:
 *  1. frame shorter than 14 bytes or a non-IP ethertype: CG_FRAME_NOT_LOCAL;
 *  2. IP header short (14 + 20 / 14 + 40 bytes): CG_DROP_INVALID;
 *  3. destination address not in the map: CG_FRAME_NOT_LOCAL;
 *  4. an entry with CG_ENDPOINT_F_HOST: CG_FRAME_TO_HOST;
 *  5. else as above from step 1 with the found lxc_id.
 * CG_FRAME_NOT_LOCAL and CG_FRAME_TO_HOST are the engine's own: they lie
 * outside the DROP_* range and mean "no policy program ran" (from-netdev
 * forwards such packets elsewhere).
 *
 * A frame whose range runs backwards is empty.  The device reads only bytes
 * in [raw + raw_off[0], raw + raw_off[n]); a frame range that leaves that
 * window is cut to it.  The call takes one snapshot of the array, the
 * endpoint map and the ipcache under the handle lock, and the launch holds
 * all three. */
#define CG_DROP_INVALID (-134)          /* bpf/lib/common.h */
#define CG_DROP_CT_INVALID_HDR (-135)
#define CG_DROP_CT_UNKNOWN_PROTO (-137)
#define CG_DROP_UNKNOWN_L3 (-139)
#define CG_DROP_INVALID_EXTHDR (-156)
#define CG_FRAME_NOT_LOCAL (-1)
#define CG_FRAME_TO_HOST (-2)
/* What the walk found, 16 bytes per frame; fields of a stage the frame did
 * not reach are 0.  t.len (the length counted) and family are set once the
 * frame is read, lxc_id once it is known, t.proto with tuple.nexthdr,
 * t.dport (after the reversal; ICMP echo request: the raw u16 8 / 128) and
 * t.flags (CG_L4_F_INGRESS [| CG_L4_F_FRAGMENT]) when the walk completes,
 * t.identity when the source is resolved. */
typedef struct {
  cg_l4_tuple t;
  uint16_t lxc_id;
  uint8_t family; /* 0, 4 or 6 */
  uint8_t pad;
} cg_l4_frame_info;
int cg_l4_frames_verdicts_dev(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* d_raw,
                              const uint64_t* d_raw_off, size_t n, const uint16_t* d_lxc_ids, uint32_t ep_id,
                              const uint32_t* d_src_labels, uint32_t ipc_id, const uint32_t* d_pkt_len,
                              int32_t* d_verdicts, cg_l4_frame_info* d_info /* may be NULL */, void* stream);
int cg_l4_frames_verdicts_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                               const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids, uint32_t ep_id,
                               const uint32_t* src_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                               int32_t* verdicts, cg_l4_frame_info* info /* may be NULL */);

/* The conntrack maps, cilium_ct{4,6}_* and cilium_ct_any{4,6}_* (pkg/maps/ctmap,
 * bpf/lib/conntrack.h): one object holds the TCP and the ANY map of both
 * families, for every scope.  A key is struct ipv4_ct_tuple / ipv6_ct_tuple
 * exactly as the datapath stores it (bpf/lib/common.h:338-378,
 * ctmap/ipv4.go:29-36: ports in network order, flags TUPLE_F_*) together with
 *  - kind: which map.  get_ct_map4/6 (bpf_lxc.c:101-107) picks the TCP map for
 *    nexthdr == TCP and the ANY map otherwise, and ct_create* writes a flow's
 *    ICMP "related" key into the flow's own map (conntrack.h:756-769,
 *    :645-664): a TCP flow's related key lives in the TCP map, where an ICMP
 *    error, looked up in the ANY map, does not find it;
 *  - scope: conntrack maps are per endpoint (cilium_ct4_<id>: scope = the lxc
 *    id) or global.  A map created with CG_CT_MAP_F_GLOBAL holds scope 0 only,
 *    and every frame looks up scope 0.
 * On the device it is an exact-match table of 128-byte buckets sized for HBM
 * (DESIGN.md 2), published by swap like every other table: a verdict call
 * sees one snapshot of the whole map, taken under the handle lock together
 * with the array's, the endpoint map's and the ipcache's, so a concurrent
 * cg_ct_map_* update is seen by that call entirely or not at all.  The device
 * holds rev_nat_index and lb_loopback per key; the rest of the entry stays on
 * the host for lookup and dump. */
#define CG_CT_MAP_TCP 0u
#define CG_CT_MAP_ANY 1u
#define CG_CT_MAP_F_GLOBAL 1u
#define CG_TUPLE_F_OUT 0u /* bpf/lib/conntrack.h:63-66 */
#define CG_TUPLE_F_IN 1u
#define CG_TUPLE_F_RELATED 2u
#define CG_TUPLE_F_SERVICE 4u
typedef struct {
  uint8_t daddr[16]; /* network byte order; v4 uses [0..3], the rest 0 */
  uint8_t saddr[16];
  uint16_t dport;    /* network byte order, as stored */
  uint16_t sport;
  uint8_t nexthdr;
  uint8_t flags;     /* CG_TUPLE_F_*: bits above 0x07 are CG_INVALID_ARGUMENT */
  uint16_t pad;
  uint16_t scope;
  uint8_t family;    /* 4 or 6 */
  uint8_t kind;      /* CG_CT_MAP_TCP / CG_CT_MAP_ANY */
} cg_ct_key;         /* 44 bytes */
/* struct ct_entry (bpf/lib/common.h:380-406), field for field; `flags` is its
 * bit field as one u16. */
#define CG_CT_E_RX_CLOSING 0x01u
#define CG_CT_E_TX_CLOSING 0x02u
#define CG_CT_E_NAT46 0x04u
#define CG_CT_E_LB_LOOPBACK 0x08u
#define CG_CT_E_SEEN_NON_SYN 0x10u
typedef struct {
  uint64_t rx_packets, rx_bytes, tx_packets, tx_bytes;
  uint32_t lifetime;
  uint16_t flags; /* CG_CT_E_* */
  uint16_t rev_nat_index;
  uint16_t slave;
  uint8_t tx_flags_seen, rx_flags_seen;
  uint32_t src_sec_id;
  uint32_t last_tx_report, last_rx_report;
} cg_ct_entry; /* 56 bytes */
/* max_entries bounds the object's keys, all kinds, families and scopes
 * together; 0 = 1 << 20. */
int cg_ct_map_create(uint64_t h, uint32_t max_entries, uint32_t flags, uint32_t* ct_id);
int cg_ct_map_destroy(uint64_t h, uint32_t ct_id);
/* map_update_elem(BPF_ANY) for each pair; a key given twice keeps its last
 * value.  All-or-nothing as cg_endpoint_map_update: CG_INVALID_ADDRESS for a
 * family other than 4 / 6, CG_INVALID_ARGUMENT for an unknown kind, flag bits
 * above 0x07, a v4 key with address bytes past the fourth, or a non-zero
 * scope on a global map; CG_MAP_FULL when the batch would exceed max_entries;
 * and nothing is applied. */
int cg_ct_map_update(uint64_t h, uint32_t ct_id, const cg_ct_key* keys, const cg_ct_entry* values, size_t n);
/* CG_NOT_FOUND (nothing deleted) if any key is absent. */
int cg_ct_map_delete(uint64_t h, uint32_t ct_id, const cg_ct_key* keys, size_t n);
int cg_ct_map_lookup(uint64_t h, uint32_t ct_id, const cg_ct_key* key, cg_ct_entry* value);
/* Keys in the order (scope, kind, family, then the tuple's bytes as the
 * datapath stores them: daddr, saddr, dport, sport, nexthdr, flags, compared
 * byte by byte); *n gets the total. */
int cg_ct_map_dump(uint64_t h, uint32_t ct_id, cg_ct_key* keys, cg_ct_entry* values, size_t cap, size_t* n);

/* cg_l4_frames_verdicts_* with the conntrack lookup in its place:
 * ct_lookup4 / ct_lookup6 (bpf/lib/conntrack.h:467-590, :310-437) in front of
 * the policy, and the tail of ipv4_policy / ipv6_policy that acts on its
 * result (bpf_lxc.c:948-976, :814-840).  Everything cg_l4_frames_verdicts_*
 * state holds, and a frame whose walk returns before the lookup (every code
 * of the two orders above, the walk's DROP_* codes included) gets that code
 * and an all-zero record.  For the others:
 *  - the tuple is the header's saddr / daddr as found (IPv6: before the
 *    rev-NAT bits of the destination are zeroed, bpf_lxc.c:764-766),
 *    TUPLE_F_OUT, nexthdr, and the ports of the head of ct_lookup*: the four
 *    port bytes in {dport, sport}; ICMP dest-unreach / time-exceeded /
 *    parameter-problem (3, 11, 12) and ICMPv6 dest-unreach / packet-too-big /
 *    time-exceeded / parameter-problem (1..4) set TUPLE_F_RELATED, an echo
 *    reply sets dport = 8 / 128, an echo request sport = 8 / 128 (raw u16);
 *  - the map is the TCP one for nexthdr 6, else the ANY one; the scope is the
 *    frame's lxc id, or 0 on a global map;
 *  - the tuple as loaded is looked up first: a hit is CT_RELATED with
 *    TUPLE_F_RELATED, else CT_REPLY.  On a miss the tuple is reversed
 *    (addresses and ports swapped, TUPLE_F_IN flipped) and looked up again:
 *    CT_ESTABLISHED, or CT_NEW.  __ct_lookup never tests an entry's lifetime
 *    or closing bits for its result, so neither does this;
 *  - the policy is evaluated exactly as cg_l4_frames_verdicts_* evaluate it,
 *    whatever the state, and its counters move (the reference's call on a
 *    REPLY / RELATED packet passes the unreversed dport; here the key and its
 *    counters are those of the call without conntrack);
 *  - REPLY / RELATED: verdict 0, never a proxy port.  Policy denies
 *    otherwise: CG_DROP_POLICY, and op DELETE of the matched key if the state
 *    was ESTABLISHED.  NEW and allowed: op CREATE, the policy's verdict (0 or
 *    the proxy port).  ESTABLISHED and allowed: the policy's verdict, no op.
 *    CG_L4_IGNORE_DROP turns the policy's denial into 0 before this, as the
 *    datapath built with IGNORE_DROP does.
 * The map is read, never written: the ops are reported in the records and
 * cg_ct_map_apply carries them out.  Within one call a second packet of a
 * flow that the first would have created still reads CT_NEW; both get CREATE,
 * which apply makes idempotent.  Not modelled: lifetime and flags-seen
 * updates, CONNTRACK_ACCOUNTING, rev-NAT (rev_nat_index / loopback are
 * reported, not acted on), NAT46. */
#define CG_CT_STATE_NONE 0u /* the walk did not reach the lookup */
#define CG_CT_STATE_NEW 1u  /* 1 + CT_NEW .. CT_RELATED (bpf/lib/common.h:331-336) */
#define CG_CT_STATE_ESTABLISHED 2u
#define CG_CT_STATE_REPLY 3u
#define CG_CT_STATE_RELATED 4u
#define CG_CT_OP_NONE 0u
#define CG_CT_OP_CREATE 1u
#define CG_CT_OP_DELETE 2u
#define CG_DROP_CT_CREATE_FAILED (-155) /* bpf/lib/common.h:262 */
/* 64 bytes per frame.  key: the tuple the op applies to, in the form the
 * reference writes or deletes it — after the reversal (what ct_create*
 * receives, what matched as ESTABLISHED); for REPLY / RELATED the tuple as it
 * matched.  key.kind, key.family and key.scope name the map looked up.
 * rev_nat_index / loopback: the matched entry's, 0 for NEW. */
typedef struct {
  uint8_t state; /* CG_CT_STATE_* */
  uint8_t op;    /* CG_CT_OP_* */
  uint8_t loopback;
  uint8_t pad0; /* dir: 0 ingress, 1 egress (cg_l4_frames_egress_verdicts_*), 2 service */
  uint16_t rev_nat_index;
  uint16_t pad1;    /* the slave (cg_l4_frames_egress_svc_verdicts_*) */
  uint32_t pad2[2]; /* [0]: src_sec_id of an egress record (the header's seclabel); [1]: ct_state.addr */
  cg_ct_key key;
  uint32_t pad3; /* ct_state.svc_addr */
} cg_ct_record;
/* ct_id: the conntrack map; d_records / records may be NULL. */
int cg_l4_frames_ct_verdicts_dev(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* d_raw,
                                 const uint64_t* d_raw_off, size_t n, const uint16_t* d_lxc_ids, uint32_t ep_id,
                                 const uint32_t* d_src_labels, uint32_t ipc_id, const uint32_t* d_pkt_len,
                                 uint32_t ct_id, int32_t* d_verdicts, cg_l4_frame_info* d_info,
                                 cg_ct_record* d_records, void* stream);
int cg_l4_frames_ct_verdicts_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                                  const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids, uint32_t ep_id,
                                  const uint32_t* src_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                                  uint32_t ct_id, int32_t* verdicts, cg_l4_frame_info* info, cg_ct_record* records);
/* Carry out the records' ops on the map, in frame order (host side):
 *  - CREATE: ct_create4/6 with a zero ct_state (conntrack.h:691-772, :616-667):
 *    the flow's key, then the ICMP / ICMPv6 related key (same addresses, ports
 *    0, flags | TUPLE_F_RELATED, same kind and scope), each with rx_packets =
 *    1, rx_bytes = pkt_len[i] (NULL: 0), src_sec_id = src_labels[i] (NULL: 0);
 *    the related entry has seen_non_syn set.  Existing keys are overwritten,
 *    so a duplicate CREATE leaves one pair;
 *  - DELETE: the key is removed; a key already gone is not an error
 *    (ct_delete* ignores it).
 *  - the fields cg_l4_frames_egress_svc_verdicts_* fill, all 0 in every other
 *    record: CREATE writes rev_nat_index, loopback (lb_loopback) and pad1
 *    (slave) into both entries.  pad0 == 2 (CT_SERVICE) creates as any dir
 *    that is not CT_INGRESS does: tx counters, src_sec_id 0, the related key
 *    with TUPLE_F_SERVICE | TUPLE_F_RELATED.  A v4 egress CREATE with pad2[1]
 *    (ct_state.addr) != 0 also writes ct_create4's second entry
 *    (conntrack.h:725-753): the key with daddr = addr, and on loopback flags
 *    = TUPLE_F_IN and saddr = pad3 (svc_addr); the three keys fit together or
 *    none is written;
 *  - UPDATE_SLAVE (ct_update{4,6}_slave): sets slave = pad1 on the key; a
 *    missing key is ignored.
 * results[i] (may be NULL): 0, or CG_DROP_CT_CREATE_FAILED when the frame's
 * new keys did not fit under max_entries; neither key is written then. */
int cg_ct_map_apply(uint64_t h, uint32_t ct_id, const cg_ct_record* records, size_t n, const uint32_t* pkt_len,
                    const uint32_t* src_labels, int32_t* results);

/* Endpoint program headers: the compile-time constants of an endpoint's
 * from-container program (pkg/endpoint/bpf.go:154-180 writes them into the
 * program's header file), one 64-byte record per slot of the policy array.
 *  - set_headers / clear_headers are all-or-nothing per call: every argument
 *    is checked before any header changes.  Flag bits outside CG_EPH_F_* are
 *    CG_INVALID_ARGUMENT; pad must be 0.
 *  - A header is independent of the map in the slot: cg_policy_array_set /
 *    clear and cg_policymap_destroy leave it alone.
 *  - Headers are published with the array's snapshot: a verdict call sees a
 *    concurrent set_headers entirely or not at all. */
#define CG_EPH_F_IPV4 0x01u    /* LXC_IPV4 is defined: `ipv4` is valid */
#define CG_EPH_F_NO_SMAC 0x02u /* DISABLE_SMAC_VERIFICATION (lib/lxc.h:31-43) */
#define CG_EPH_F_NO_DMAC 0x04u /* DISABLE_DMAC_VERIFICATION (lib/lxc.h:76-88) */
#define CG_EPH_F_NO_SIP 0x08u  /* DISABLE_SIP_VERIFICATION (lib/lxc.h:45-74) */
typedef struct {
  uint8_t lxc_mac[6], node_mac[6]; /* LXC_MAC, NODE_MAC */
  uint32_t ipv4;                   /* LXC_IPV4, network order; valid with CG_EPH_F_IPV4 */
  uint8_t ipv6[16];                /* LXC_IP */
  uint8_t router_ip6[16];          /* ROUTER_IP (icmp6_handle) */
  uint32_t seclabel;               /* SECLABEL */
  uint32_t flags;                  /* CG_EPH_F_* */
  uint32_t pad[2];
} cg_endpoint_header; /* 64 bytes */
int cg_policy_array_set_headers(uint64_t h, uint32_t arr_id, const uint16_t* lxc_ids,
                                const cg_endpoint_header* headers, size_t n);
int cg_policy_array_clear_headers(uint64_t h, uint32_t arr_id, const uint16_t* lxc_ids, size_t n);
/* CG_NOT_FOUND for a slot without a header. */
int cg_policy_array_get_header(uint64_t h, uint32_t arr_id, uint16_t lxc_id, cg_endpoint_header* out);

/* L4 verdicts from raw frames, egress: the endpoint's from-container program
 * up to its verdict — handle_ingress (bpf/bpf_lxc.c:708-742),
 * handle_ipv4_from_lxc (:432-570), handle_ipv6 + ipv6_l3_from_lxc (:389-416,
 * :114-266) — per frame of a blob, on the map and the header in the
 * endpoint's slot of the policy array.  The program is the one built with
 * CONNTRACK, LB_L3 and LB_L4; these entries run it over an empty services map
 * (lb{4,6}_lookup_service finds nothing, lb*_local and lb*_rev_nat never run,
 * ct_state_new.rev_nat_index stays 0), cg_l4_frames_egress_svc_verdicts_* below
 * over a cg_lb_map.  MAC rewrite, forwarding and local delivery behind the
 * verdict are not modelled.
 *
 * mode: CG_L4_EGRESS [| CG_L4_IGNORE_DROP]; anything else is
 * CG_INVALID_ARGUMENT.  lxc_ids is mandatory (the program hangs on the
 * endpoint's own veth; no lookup names the endpoint).  Exactly one of
 * dst_labels / ipc_id is given (both or neither: CG_INVALID_ARGUMENT).
 * ct_id 0: no conntrack map, every packet is CT_NEW; records then must be NULL
 * (CG_INVALID_ARGUMENT).  The blob window, backwards ranges and pkt_len are
 * those of cg_l4_frames_verdicts_*.  One hold of the handle lock takes one
 * snapshot of the array (headers included), the ipcache and the conntrack
 * map; the launch holds all of them.
 *
 * Order per frame (codes: bpf/lib/common.h:237-264):
 *  1. empty slot: CG_DROP_MISSED_TAIL_CALL; nothing is read, no counter moves;
 *  2. slot without a header: CG_FRAME_NO_HEADER (the engine's own: there is no
 *     such program);
 *  3. frame shorter than 14 bytes: CG_DROP_INVALID (the engine's choice, as on
 *     ingress);
 *  4. ethertype (handle_ingress's switch, :713-737): 0x0806 →
 *     CG_FRAME_ANSWERED (the engine's own: tail_handle_arp replies itself, no
 *     policy runs); any other non-IP ethertype → CG_DROP_UNKNOWN_L3;
 *  5. IPv4 (:450-466): shorter than 34 → CG_DROP_INVALID; nexthdr = protocol;
 *     is_valid_lxc_src_mac fails (bytes 6..11 != lxc_mac) →
 *     CG_DROP_INVALID_SMAC; else is_valid_gw_dst_mac fails (bytes 0..5 !=
 *     node_mac) → CG_DROP_INVALID_DMAC; else is_valid_lxc_src_ipv4 fails
 *     (saddr != ipv4, or the header has no CG_EPH_F_IPV4, lib/lxc.h:55-63) →
 *     CG_DROP_INVALID_SIP.  A CG_EPH_F_NO_* flag skips its test.
 *     l4_off = 14 + ihl * 4, ihl as found;
 *  6. IPv6 (:396-415, :132-146): shorter than 54 → CG_DROP_INVALID.  If the
 *     fixed header's nexthdr is 58 (not after extension headers): shorter than
 *     14 + 40 + 8 → CG_DROP_INVALID; the byte at 54 being 135 →
 *     CG_FRAME_ANSWERED; 128 with daddr == router_ip6 → CG_FRAME_ANSWERED
 *     (icmp6_handle, lib/icmp6.h:390-412).  This comes before the MAC checks.
 *     Then SMAC / DMAC / SIP as above (is_valid_lxc_src_ip: saddr != ipv6),
 *     then ipv6_hdrlen with the codes of the ingress walk
 *     (CG_DROP_INVALID_EXTHDR, CG_DROP_FRAG_NOSUPPORT, CG_DROP_INVALID);
 *  7. lb{4,6}_extract_key → extract_l4_port (lib/lb.h:192-216): TCP / UDP load
 *     2 bytes at l4_off + 2; on failure the reference returns skb_load_bytes's
 *     own error (l4_load_port, lib/l4.h:62-65, passes it on and IS_ERR is
 *     true for it), not a DROP_*: CG_FRAME_EFAULT.  ICMP / ICMPv6 pass.
 *     Anything else is DROP_UNKNOWN_L4, which only skips the service lookup;
 *  8. the head of ct_lookup4/6 with dir = CT_EGRESS (lib/conntrack.h:496-556,
 *     :339-400): the tuple's flags start as TUPLE_F_IN; otherwise as on
 *     ingress: ICMP type byte missing, TCP shorter than l4_off + 14, UDP
 *     shorter than l4_off + 4 → CG_DROP_CT_INVALID_HDR; a protocol other than
 *     TCP / UDP / the family's ICMP → CG_DROP_CT_UNKNOWN_PROTO; the ICMP
 *     related / echo rules and the four port bytes into {dport, sport} as
 *     cg_l4_frames_ct_verdicts_* state them;
 *  9. with a conntrack map, the two lookups of ct_lookup*: the tuple as loaded
 *     first (hit: CT_RELATED with TUPLE_F_RELATED, else CT_REPLY), then the
 *     reversed tuple (CT_ESTABLISHED, else CT_NEW); the TCP map for nexthdr 6,
 *     else the ANY map; the scope is the lxc id, or 0 on a global map.
 *     Without a map every packet is CT_NEW;
 * 10. the destination identity: dst_labels[i], or the ipcache resolution of
 *     the header's destination address (miss or sec_label 0: CG_WORLD_ID;
 *     with no services orig_dip is the header's daddr, :493, :180);
 * 11. policy_can_egress (lib/policy.h:150-177) {identity, dport, nexthdr,
 *     egress = 1}, never a fragment: is_fragment is passed false, so an IPv4
 *     fragment is judged by the bytes where its ports would be.  As on the
 *     ingress route the policy is evaluated on the reversed tuple's dport
 *     whatever the state, and its counters move (the reference's call on a
 *     REPLY / RELATED packet passes the unreversed dport; here the key and its
 *     counters are those of the call without conntrack);
 * 12. the outcome (:528-570, :222-266): REPLY / RELATED → 0, never a proxy
 *     port; denied → CG_DROP_POLICY, op DELETE of the matched key if
 *     ESTABLISHED; NEW and allowed → op CREATE and the policy's verdict (0 or
 *     the proxy port); ESTABLISHED and allowed → the verdict.
 *     CG_L4_IGNORE_DROP turns the denial into 0 before this.
 *
 * Records: cg_ct_record, with two pad fields given meaning (both 0 in every
 * record of the ingress route): pad0 = dir (0 ingress, 1 egress), pad2[0] =
 * src_sec_id, on egress the header's seclabel (:544, :238).  A frame that
 * returned before step 9 gets an all-zero record.  cg_ct_map_apply on a record
 * with dir == 1 does ct_create* as CT_EGRESS (conntrack.h:706-712):
 * tx_packets = 1, tx_bytes = pkt_len[i], rx stays 0, src_sec_id from the
 * record (src_labels[i] is ignored for it); the related key as for ingress.
 *
 * Info: cg_l4_frame_info; t.identity is the destination identity, t.flags is
 * CG_L4_F_WALKED once the walk reached the policy (never CG_L4_F_INGRESS),
 * t.len is set from step 3 on, family from step 5 / 6, t.proto with
 * tuple.nexthdr, t.dport and t.identity with the policy call. */
#define CG_L4_F_WALKED 0x08u /* egress frame info only: the walk reached the policy */
#define CG_DROP_INVALID_SMAC (-130) /* bpf/lib/common.h:237-239 */
#define CG_DROP_INVALID_DMAC (-131)
#define CG_DROP_INVALID_SIP (-132)
#define CG_FRAME_ANSWERED (-3)
#define CG_FRAME_NO_HEADER (-4)
#define CG_FRAME_EFAULT (-14)
int cg_l4_frames_egress_verdicts_dev(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* d_raw,
                                     const uint64_t* d_raw_off, size_t n, const uint16_t* d_lxc_ids,
                                     const uint32_t* d_dst_labels, uint32_t ipc_id, const uint32_t* d_pkt_len,
                                     uint32_t ct_id /* 0: none */, int32_t* d_verdicts, cg_l4_frame_info* d_info,
                                     cg_ct_record* d_records, void* stream);
int cg_l4_frames_egress_verdicts_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                                      const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids,
                                      const uint32_t* dst_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                                      uint32_t ct_id, int32_t* verdicts, cg_l4_frame_info* info,
                                      cg_ct_record* records);

/* Service load-balancing: cilium_lb{4,6}_services and
 * cilium_lb{4,6}_reverse_nat (bpf/lib/lb.h:38-84, pkg/maps/lbmap) of one node
 * in one object, with the node constant IPV4_LOOPBACK (node_config.h; network
 * order, 0 is legal: the loopback case then rewrites no source).
 *  - A service key is struct lb{4,6}_key {address, dport (network order),
 *    slave}: slave 0 is the master, whose value's `count` says how many slaves
 *    follow; slaves 1..count carry the backends.  A value is struct
 *    lb{4,6}_service {target, port (network order), count, rev_nat_index,
 *    weight}.  weight is stored and dumped and never read: the datapath's use
 *    of the _rr_seq maps is compiled out (lb.h:139, :173), so they are not built.
 *  - A reverse-NAT entry is u16 index -> {address, port (network order)}.
 *  - max_entries bounds each of the four maps by itself; 0 = 65536
 *    (CILIUM_LB_MAP_MAX_ENTRIES).  Updates are all-or-nothing per call:
 *    CG_INVALID_ADDRESS for a family other than 4 / 6, CG_INVALID_ARGUMENT for a
 *    v4 key or value with address bytes past the fourth or a non-zero pad,
 *    CG_MAP_FULL when the batch would exceed max_entries; nothing is applied.
 *    A key given twice keeps its last value.  delete: CG_NOT_FOUND (nothing
 *    deleted) if any key is absent.
 *  - Dump order: services by (family, address bytes, dport's two bytes as
 *    stored, slave as a number); reverse NAT by (family, index).
 *  - On the device: an exact-match table per family in HBM and the reverse-NAT
 *    entries as a dense array indexed by the u16, published by
 *    swap; a verdict call takes its snapshot under the same hold of the handle
 *    lock as the array's, the ipcache's and the conntrack map's. */
#define CG_LB_MAP_MAX_ENTRIES 65536u
typedef struct {
  uint8_t address[16]; /* network byte order; v4 uses [0..3], the rest 0 */
  uint16_t dport;      /* network byte order, as stored; 0: the L3 service */
  uint16_t slave;      /* 0: the master */
  uint8_t family;      /* 4 or 6 */
  uint8_t pad[3];
} cg_lb_key; /* 24 bytes */
typedef struct {
  uint8_t target[16];
  uint16_t port; /* network byte order; 0: the port is not rewritten */
  uint16_t count;
  uint16_t rev_nat_index;
  uint16_t weight;
} cg_lb_service; /* 24 bytes */
typedef struct {
  uint16_t index;
  uint8_t family;
  uint8_t pad;
} cg_lb_revnat_key; /* 4 bytes */
typedef struct {
  uint8_t address[16];
  uint16_t port;
  uint16_t pad;
} cg_lb_revnat; /* 20 bytes */
int cg_lb_map_create(uint64_t h, uint32_t max_entries, uint32_t ipv4_loopback, uint32_t* lb_id);
int cg_lb_map_destroy(uint64_t h, uint32_t lb_id);
int cg_lb_map_set_loopback(uint64_t h, uint32_t lb_id, uint32_t ipv4_loopback);
int cg_lb_map_service_update(uint64_t h, uint32_t lb_id, const cg_lb_key* keys, const cg_lb_service* values, size_t n);
int cg_lb_map_service_delete(uint64_t h, uint32_t lb_id, const cg_lb_key* keys, size_t n);
int cg_lb_map_service_lookup(uint64_t h, uint32_t lb_id, const cg_lb_key* key, cg_lb_service* value);
int cg_lb_map_service_dump(uint64_t h, uint32_t lb_id, cg_lb_key* keys, cg_lb_service* values, size_t cap, size_t* n);
int cg_lb_map_revnat_update(uint64_t h, uint32_t lb_id, const cg_lb_revnat_key* keys, const cg_lb_revnat* values,
                            size_t n);
int cg_lb_map_revnat_delete(uint64_t h, uint32_t lb_id, const cg_lb_revnat_key* keys, size_t n);
int cg_lb_map_revnat_lookup(uint64_t h, uint32_t lb_id, const cg_lb_revnat_key* key, cg_lb_revnat* value);
int cg_lb_map_revnat_dump(uint64_t h, uint32_t lb_id, cg_lb_revnat_key* keys, cg_lb_revnat* values, size_t cap,
                          size_t* n);

/* cg_l4_frames_egress_verdicts_* over a services map: the from-container
 * program with lb{4,6}_lookup_service, lb{4,6}_local and lb*_xlate (bpf/lib/lb.h;
 * bpf_lxc.c:468-484, :148-170) in their place between steps 7 and 8 of the
 * order above, one launch.  The arguments are those entries' plus lb_id, the
 * map, and hash; ct_id and ipc_id are mandatory and dst_labels must be NULL
 * (CG_INVALID_ARGUMENT otherwise; an unknown lb_id is CG_NOT_FOUND):
 * lb*_local is conntrack, and the backend's identity exists only after the
 * translation.  The frame blob is read-only: the translation lives in the
 * tuple the later steps take.  Checksums and store errors are not modelled.
 *
 *  7a. the service key {tuple.daddr, dport, slave 0}: dport is the two bytes at
 *      l4_off + 2 for TCP / UDP, 0 for ICMP / ICMPv6.  Any other protocol
 *      (DROP_UNKNOWN_L4) skips 7b-7e, as the reference's goto does;
 *  7b. lb*_lookup_service (lb.h:604-635, :351-380): with dport != 0 the L4
 *      master, which counts only with count != 0; otherwise key.dport is zeroed,
 *      and stays zeroed, and the L3 master is looked up, again only with count
 *      != 0.  A miss leaves the program exactly as it runs without services;
 *  7c. lb*_local: ct_lookup* as CT_SERVICE — the tuple's flags are
 *      TUPLE_F_SERVICE [| RELATED], ports and ICMP rules those of the head of
 *      ct_lookup*, one lookup of the tuple as loaded, no reversal
 *      (conntrack.h:580, :423), map kind and scope those of the egress lookup.
 *      A frame for which the head of ct_lookup* fails (e.g. TCP with l4_off + 4
 *      <= len < l4_off + 14) leaves with CG_DROP_NO_SERVICE, not the head's own
 *      code.  CT_NEW: slave = hash % count + 1, op CREATE.  REPLY / RELATED:
 *      the slave is the matched entry's;
 *  7d. lb*_lookup_slave with key.slave = slave; any entry counts.  On a miss
 *      lb*_lookup_service runs again with the key as it now stands, slave
 *      number included (lb.h:737-744): with key.dport != 0, {daddr, dport,
 *      slave} (which just missed) and then {daddr, 0, slave} with count != 0;
 *      with key.dport == 0 nothing new.  A hit re-selects the slave from that
 *      entry's count (op UPDATE_SLAVE) and that entry is the one translated
 *      to; a miss is CG_DROP_NO_SERVICE.  Over maps the control plane wrote
 *      (count 0 in every slave slot) a flow whose slave slot has gone therefore
 *      leaves with CG_DROP_NO_SERVICE;
 *  7e. rev_nat_index = svc.rev_nat_index; the new destination is svc.target.
 *      v4 with saddr == svc.target (lb.h:761-770): the new source is
 *      IPV4_LOOPBACK, loopback = 1, ct_state.addr = IPV4_LOOPBACK, svc_addr =
 *      saddr, and tuple.daddr stays the VIP; otherwise tuple.daddr = target
 *      (v4: ct_state.addr = target).  TCP / UDP with svc.port != 0 and
 *      key.dport != svc.port (key.dport is 0 after the L3 fallback): dport =
 *      svc.port;
 *  8-12 as above on the translated tuple: the CT_EGRESS lookups use tuple.daddr
 *      after 7e and the rewritten dport, the ipcache resolves tuple.daddr after
 *      7e, policy_can_egress takes that identity and that dport, and an egress
 *      CREATE record carries ct_state_new: rev_nat_index, loopback, pad1 =
 *      slave, pad2[1] = ct_state.addr, pad3 = svc_addr;
 *  reverse NAT: REPLY / RELATED with the matched entry's rev_nat_index != 0
 *      (bpf_lxc.c:554-565, :248-262) reports what lb{4,6}_rev_nat(…, flags 0)
 *      would write: the entry's address as the new source, its port as the new
 *      sport for TCP / UDP when non-zero, on v4 loopback the old source as the
 *      new destination.  A missing entry reports nothing; the verdict does not
 *      change.  The ingress program's lb4_rev_nat stays out.
 *
 * hash[i] (may be NULL) stands for get_hash_recalc(skb), the kernel's flow
 * hash, which the engine cannot reproduce; NULL: cg_diag_ct_hash of the
 * frame's CT_SERVICE key.
 *
 * records: the CT_EGRESS step's, as above.  svc_records (may be NULL): the
 * CT_SERVICE step's cg_ct_record per frame, all-zero when the service steps
 * did not run, missed, or left before the lookup: state, op, the key with
 * TUPLE_F_SERVICE, pad0 = 2 (CT_SERVICE), pad1 = the slave.  A CT_NEW frame whose
 * slave is re-selected in 7d gets one op, CREATE, with the slave it ends with.
 * xlate (may be NULL): a cg_lb_xlate per frame.  cg_ct_map_apply takes
 * svc_records first, then records.  The reference fails closed when the
 * service entry cannot be created; here the create happens in apply, after the
 * verdict, and the failure shows in apply's results — the divergence the
 * egress CREATE already has. */
#define CG_DROP_NO_SERVICE (-158) /* bpf/lib/common.h:265 */
#define CG_CT_OP_UPDATE_SLAVE 3u  /* ct_update{4,6}_slave: sets slave on an existing key */
#define CG_LB_NONE 0u       /* the service steps did not run */
#define CG_LB_MISS 1u       /* no service for the destination */
#define CG_LB_TRANSLATED 2u
#define CG_LB_NO_SERVICE 3u /* the frame left with CG_DROP_NO_SERVICE */
#define CG_LB_F_L3 0x01u       /* the master that matched is the L3 one (key.dport == 0) */
#define CG_LB_F_PORT 0x02u     /* the destination port was rewritten */
#define CG_LB_F_LOOPBACK 0x04u /* the v4 loopback case */
#define CG_LB_F_REVNAT 0x08u   /* a reverse translation is reported */
/* 48 bytes, written as three 16-byte pieces.  The addresses and ports are the
 * packet's after the translation (status TRANSLATED) or after the reverse
 * translation (CG_LB_F_REVNAT); all four are 0 otherwise, as is family. */
typedef struct {
  uint8_t status; /* CG_LB_* */
  uint8_t flags;  /* CG_LB_F_* */
  uint16_t slave;
  uint16_t rev_nat_index;
  uint16_t dport; /* network byte order */
  uint16_t sport;
  uint8_t family;
  uint8_t pad0;
  uint32_t pad1;
  uint8_t daddr[16];
  uint8_t saddr[16];
} cg_lb_xlate;
int cg_l4_frames_egress_svc_verdicts_dev(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* d_raw,
                                         const uint64_t* d_raw_off, size_t n, const uint16_t* d_lxc_ids,
                                         const uint32_t* d_dst_labels, uint32_t ipc_id, const uint32_t* d_pkt_len,
                                         uint32_t ct_id, uint32_t lb_id, const uint32_t* d_hash, int32_t* d_verdicts,
                                         cg_l4_frame_info* d_info, cg_ct_record* d_records,
                                         cg_ct_record* d_svc_records, cg_lb_xlate* d_xlate, void* stream);
int cg_l4_frames_egress_svc_verdicts_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                                          const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids,
                                          const uint32_t* dst_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                                          uint32_t ct_id, uint32_t lb_id, const uint32_t* hash, int32_t* verdicts,
                                          cg_l4_frame_info* info, cg_ct_record* records, cg_ct_record* svc_records,
                                          cg_lb_xlate* xlate);

/* ======================================================================== */
/* LPM: XDP CIDR prefilter — bpf/bpf_xdp.c:88-184,                           */
/* pkg/datapath/prefilter/prefilter.go:57-298                                */
/* ======================================================================== */

/* A CIDR as the agent holds it (net.IPNet; cidrKey cidrmap.go:52-64). */
typedef struct {
  uint8_t family;     /* 4 or 6 */
  uint8_t prefixlen;  /* ones of the mask */
  uint8_t pad[2];
  uint8_t addr[16];   /* network byte order; v4 uses addr[0..3] */
} cg_cidr;

/* preFilterConfig (prefilter.go:49-54); NewPreFilter default is fix4|fix6
 * with dyn maps disabled (prefilter.go:281-298). */
#define CG_PF_DYN4 0x1u
#define CG_PF_DYN6 0x2u
#define CG_PF_FIX4 0x4u
#define CG_PF_FIX6 0x8u

/* XDP verdicts written per address (linux enum xdp_action). */
#define CG_XDP_DROP 1
#define CG_XDP_PASS 2

/* NewPreFilter.  max_lpm/max_hash: 0 = maxLKeys 65536 / maxHKeys 20M
 * (prefilter.go:43-44).  Revision starts at 1 (prefilter.go:291). */
int cg_prefilter_create(uint64_t h, uint32_t config, uint32_t max_lpm, uint32_t max_hash,
                        uint32_t* pf_id);
int cg_prefilter_destroy(uint64_t h, uint32_t pf_id);
/* PreFilter.Insert (prefilter.go:125-159): revision check (0 = any), per-CIDR
 * map selection (selectMap :108-122), undo on failure.  *revision_out gets the
 * new revision on success. */
int cg_prefilter_insert(uint64_t h, uint32_t pf_id, int64_t revision, const cg_cidr* cidrs,
                        size_t n, int64_t* revision_out);
/* PreFilter.Delete (prefilter.go:162-203). */
int cg_prefilter_delete(uint64_t h, uint32_t pf_id, int64_t revision, const cg_cidr* cidrs,
                        size_t n, int64_t* revision_out);
/* PreFilter.Dump (prefilter.go:99-106): entries of dyn4, fix4, dyn6, fix6
 * in that map order; *n gets the total. */
int cg_prefilter_dump(uint64_t h, uint32_t pf_id, cg_cidr* out, size_t cap, size_t* n,
                      int64_t* revision);
/* The local endpoint set cilium_lxc consulted by check_v{4,6}_endpoint
 * (bpf_xdp.c:88-95,123-130 → bpf/lib/eps.h:26-46).  Replaces the set. */
int cg_prefilter_set_endpoints(uint64_t h, uint32_t pf_id, const uint32_t* v4_be, size_t n4,
                               const uint8_t* v6, size_t n6);
/* check_v4 / check_v6 (bpf_xdp.c:97-156) over a batch.
 * v4: n4 records of {saddr, daddr} (u32 each, network order as in iphdr);
 * v6: n6 records of {saddr[16], daddr[16]}.  out: one CG_XDP_* byte each. */
int cg_prefilter_verdicts_dev(uint64_t h, uint32_t pf_id, const uint32_t* d_v4, size_t n4,
                              uint8_t* d_out4, const uint8_t* d_v6, size_t n6, uint8_t* d_out6,
                              void* stream);
int cg_prefilter_verdicts_host(uint64_t h, uint32_t pf_id, const uint32_t* v4, size_t n4,
                               uint8_t* out4, const uint8_t* v6, size_t n6, uint8_t* out6);

/* ======================================================================== */
/* ipcache: IP -> security identity (cilium_ipcache, bpf/lib/maps.h:135-159; */
/* pkg/maps/ipcache/ipcache.go:36-130; lookup bpf/lib/eps.h:48-115)         */
/* ======================================================================== */

/* RemoteEndpointInfo (bpf/lib/common.h:175-178, ipcache.go:127-130). */
typedef struct {
  uint32_t sec_label;
  uint32_t tunnel_endpoint;  /* as stored: the node IPv4 address bytes */
} cg_remote_endpoint_info;

/* identity the callers fall back to (bpf/node_config.h:35) */
#define CG_WORLD_ID 2

/* A cilium_ipcache map.  max_entries 0 = MaxEntries 512000 (ipcache.go:36). */
int cg_ipcache_create(uint64_t h, uint32_t max_entries, uint32_t* ipc_id);
int cg_ipcache_destroy(uint64_t h, uint32_t ipc_id);
/* Map.Update of {Key, RemoteEndpointInfo} pairs (ipcache.go NewKey: prefix
 * from the mask, address masked to it, family 4/6).  BPF_ANY semantics: an
 * existing key is overwritten.  All-or-nothing: CG_MAP_FULL when the batch
 * would exceed max_entries, and nothing is applied. */
int cg_ipcache_update(uint64_t h, uint32_t ipc_id, const cg_cidr* keys,
                      const cg_remote_endpoint_info* values, size_t n);
/* Map.Delete; CG_NOT_FOUND (nothing deleted) if any key is absent. */
int cg_ipcache_delete(uint64_t h, uint32_t ipc_id, const cg_cidr* keys, size_t n);
/* Exact-key lookup (bpf map lookup of a full key); CG_NOT_FOUND if absent. */
int cg_ipcache_lookup(uint64_t h, uint32_t ipc_id, const cg_cidr* key, cg_remote_endpoint_info* value);
/* Map.Dump: keys in (family, prefixlen, address) order; *n gets the total. */
int cg_ipcache_dump(uint64_t h, uint32_t ipc_id, cg_cidr* keys, cg_remote_endpoint_info* values,
                    size_t cap, size_t* n);
/* lookup_ip4_remote_endpoint / lookup_ip6_remote_endpoint over a batch,
 * resolved as bpf_lxc.c:509-518 does: the longest covering prefix's
 * {sec_label, tunnel_endpoint} if it exists and sec_label != 0, else
 * {CG_WORLD_ID, 0}.  v4: n4 u32 addresses (network order, as iphdr.daddr);
 * v6: n6 16-byte addresses.  out: one cg_remote_endpoint_info each. */
int cg_ipcache_resolve_dev(uint64_t h, uint32_t ipc_id, const uint32_t* d_v4, size_t n4,
                           cg_remote_endpoint_info* d_out4, const uint8_t* d_v6, size_t n6,
                           cg_remote_endpoint_info* d_out6, void* stream);
int cg_ipcache_resolve_host(uint64_t h, uint32_t ipc_id, const uint32_t* v4, size_t n4,
                            cg_remote_endpoint_info* out4, const uint8_t* v6, size_t n6,
                            cg_remote_endpoint_info* out6);

/* The egress flow of bpf_lxc.c:509-527 over a batch: each tuple's remote
 * identity is lookup_ip4_remote_endpoint(remote_v4[i]) resolved as the
 * datapath does (WORLD_ID on a miss or sec_label 0), then
 * policy_can_egress4 (policy.h:172-176 → policy_can_egress :150-163):
 * dir = CT_EGRESS and is_fragment = false whatever the tuple's flags say,
 * any negative result → DROP_POLICY.  The tuples' identity fields are
 * ignored.  remote_v4: network-order IPv4 addresses (iphdr.daddr).  Counters
 * advance as in cg_l4_verdicts_*. */
int cg_l4_verdicts_ipcache_dev(uint64_t h, uint32_t map_id, uint32_t ipc_id, const uint32_t* d_remote_v4,
                               const cg_l4_tuple* d_tuples, size_t n, int32_t* d_verdicts, void* stream);
int cg_l4_verdicts_ipcache_host(uint64_t h, uint32_t map_id, uint32_t ipc_id, const uint32_t* remote_v4,
                                const cg_l4_tuple* tuples, size_t n, int32_t* verdicts);
/* The IPv6 twin (bpf_lxc.c:205-220: lookup_ip6_remote_endpoint, then
 * policy_can_egress6 → policy_can_egress): remote_v6 holds n 16-byte
 * addresses in network order. */
int cg_l4_verdicts_ipcache6_dev(uint64_t h, uint32_t map_id, uint32_t ipc_id, const uint8_t* d_remote_v6,
                                const cg_l4_tuple* d_tuples, size_t n, int32_t* d_verdicts, void* stream);
int cg_l4_verdicts_ipcache6_host(uint64_t h, uint32_t map_id, uint32_t ipc_id, const uint8_t* remote_v6,
                                 const cg_l4_tuple* tuples, size_t n, int32_t* verdicts);

/* ======================================================================== */
/* proxylib generic L7 (proxylib/proxylib/policymap.go:118-260)              */
/* ======================================================================== */

/* Install the NetworkPolicy list of a proxylib instance (the id OpenModule
 * returned, include/cilium_proxylib.h) — what the reference receives over
 * NPDS (xds-path).  protobuf-JSON form with generic L7 rules:
 *   [{"name": "cp1", "ingress_per_port_policies": [{"port": 80, "rules": [
 *       {"remote_policies": [1], "l7_proto": "r2d2",
 *        "l7_rules": {"l7_rules": [{"rule": {"cmd": "READ", "file": "s.*"}}]}}]}]}]
 * Rule parsers: r2d2 (r2d2parser.go:91-123) and cassandra
 * (cassandraparser.go:97-131); a rule with another l7_proto drops its port
 * (policymap.go:186-204).  ParseError conditions → CG_POLICY_REJECTED and the
 * previous snapshot stays.  Verdict contract: exact port, port 0, else deny. */
int cg_proxylib_policy_update(uint64_t instance, const char* json, size_t len);

/* The proxylib update from the NPDS wire form (a serialized DiscoveryResponse
 * of cilium.NetworkPolicy resources, as Instance.PolicyUpdate receives it,
 * proxylib/proxylib/instance.go:180-215, with the same Validate() rules as
 * cg_http_policy_update_npds). */
int cg_proxylib_policy_update_npds(uint64_t instance, const uint8_t* discovery_response, size_t len);

/* OnData calls with request frames whose verdicts the instance has decided,
 * and the GPU batches that decided them: concurrent calls of different
 * connections share a batch (flat combining; calls > batches under load). */
int cg_proxylib_stats(uint64_t instance, uint64_t* batches, uint64_t* calls);

/* Batching window of the OnData combiner.  A call that finds no batch in
 * flight becomes the flusher; with min_calls > 1 it waits until min_calls
 * calls are queued or max_wait_us microseconds have passed, then decides
 * everything queued as one GPU batch.  Default (1, 0): decide at once.
 * No reference counterpart (Go proxylib decides each frame in the calling
 * goroutine, proxylib/proxylib/connection.go:176-179); a latency/throughput
 * knob for Envoy worker pools. */
int cg_proxylib_set_batching(uint64_t instance, uint32_t min_calls, uint32_t max_wait_us);

/* ======================================================================== */
/* HTTP L7: Envoy cilium.l7policy — envoy/cilium_network_policy.h:40-237,    */
/* envoy/cilium_l7policy.cc:127-182                                          */
/* ======================================================================== */

/* Install the full set of endpoint NetworkPolicies (the NPDS resource list,
 * envoy/cilium/npds.proto:31-182) given in protobuf-JSON form:
 *   [{"name": "...", "policy": 3,
 *     "ingress_per_port_policies": [{"port": 80, "protocol": "TCP",
 *        "rules": [{"remote_policies": [1],
 *                   "http_rules": {"http_rules": [{"headers": [
 *                       {"name": ":path", "regex_match": "..."} |
 *                       {"name": "...", "exact_match": "..."} |
 *                       {"name": "...", "present_match": true}]}]}}]}],
 *     "egress_per_port_policies": [...]}]
 * Compiles every regex to a minimized union DFA per (policy, direction,
 * port) and swaps the snapshot in; on any error (regex outside the
 * supported ECMAScript subset, duplicate port → EnvoyException
 * "PortNetworkPolicy: Duplicate port number", cilium_network_policy.h:160)
 * the previous snapshot stays and CG_POLICY_REJECTED is returned. */
int cg_http_policy_update(uint64_t h, const char* npds_json, size_t len);
/* The installed HTTP snapshot's compiled tables as a flat image (unions,
 * DFAs, remote tables, program index; a checksum) and its import on another
 * handle — another GPU or process — without recompiling: SURVEY §8(e)
 * "the host compiles once and uploads identical images to each GPU"; also the
 * serialized table cache (§5 checkpoint / resume).  Export with buf = NULL
 * returns the size in *len.  Import is all-or-nothing like an update; an
 * image from another library build is CG_POLICY_REJECTED.  Replaces the
 * per-worker re-translation of NetworkPolicyMap::onConfigUpdate
 * (envoy/cilium_network_policy.cc) with one compile per node. */
int cg_http_policy_export(uint64_t h, void* buf, size_t cap, size_t* len);
int cg_http_policy_import(uint64_t h, const void* buf, size_t len);

/* The same update from the NPDS wire form: a serialized xDS
 * envoy.api.v2.DiscoveryResponse whose resources are google.protobuf.Any
 * of type "type.googleapis.com/cilium.NetworkPolicy" (envoy/cilium/npds.proto:
 * 31-182, the StreamNetworkPolicies payload Envoy's NPDS subscription hands to
 * NetworkPolicyMap::onConfigUpdate, envoy/cilium_network_policy.cc:46-60).
 * The messages are validated as npds.pb.validate.go does (port <= 65535,
 * unique remote_policies, non-empty rule lists, Kafka name patterns); a
 * resource of another type, a malformed message or a failed validation
 * rejects the whole update (CG_POLICY_REJECTED, previous snapshot stays). */
int cg_http_policy_update_npds(uint64_t h, const uint8_t* discovery_response, size_t len);
/* Index of a policy name in the installed snapshot (for the packer);
 * CG_NOT_FOUND → requests naming it are denied (cilium_network_policy.h:232-235). */
int cg_http_policy_index(uint64_t h, const char* name, uint32_t* index);
/* Snapshot statistics: programs, DFA parts, total states, table bytes, fields,
 * rules, policies, remote slots, exceptions, cells, the largest program block,
 * LDS-resident programs, literal tokens and the cells their columns added. */
int cg_http_policy_stats(uint64_t h, uint64_t* out, size_t n);

/* Per-rule hit counters (what = CG_CTR_HTTP_RULES in cg_read_counters): a
 * request Envoy allows through a rule is counted once, on the FIRST rule
 * that allows it in Envoy's evaluation order (PolicyInstance::Allowed →
 * PortNetworkPolicy::Matches: the port's own PortNetworkPolicyRules, then
 * port 0's, each rule's HttpNetworkPolicyRules in order,
 * cilium_network_policy.h:90-192).  Counter i counts the rule described by
 * entry i of cg_http_rule_info_get; a rule of port 0's scope has one counter
 * per exact-port program it is merged into and one in the wildcard-port
 * program.  Requests allowed because no HTTP policy applies (no policy for
 * the port, a port without HTTP rules) are attributed to no rule; denied
 * requests to none (their per-program denied counter counts them). */
typedef struct {
  uint32_t policy;     /* policy index (cg_http_policy_index) */
  uint32_t ingress;    /* 1 ingress, 0 egress */
  uint32_t port;       /* the program's destination port; 0 = the wildcard-port program */
  uint32_t scope;      /* 0: the rule is in this port's PortNetworkPolicy, 1: in port 0's */
  uint32_t rule;       /* PortNetworkPolicyRule index within its scope */
  uint32_t http_rule;  /* HttpNetworkPolicyRule index within it, or one of: */
} cg_http_rule_info;
#define CG_HTTP_RULE_NO_HTTP 0xFFFFFFFFu     /* the PortNetworkPolicyRule has no HTTP rules */
#define CG_HTTP_RULE_SCOPE_ALLOW 0xFFFFFFFEu /* port 0 has no HTTP rules: it allows the rest */
int cg_http_rule_info_get(uint64_t h, cg_http_rule_info* out, size_t cap, size_t* n);

/* Packed request batches.  A record is an 8-byte meta word plus its field
 * string in 16-byte units (at most CG_HTTP_SLOT_BYTES in the record; longer
 * strings go to the overflow arena).  Records are stored tile-transposed in
 * tiles of 64: a tile is its 512-byte meta block then as many string units as
 * its longest string needs (string unit u ≥ 1 of lane l at tile + 512 +
 * (u-1)*1024 + l*16), so a wavefront's 16-byte load of a unit is one
 * contiguous 1 KiB read; when no lane holds more than 8 bytes in the last
 * unit, that unit is stored as a 512-byte half unit (8 bytes per lane; tile
 * table bit 15), in tiles of programs walked from LDS one part at a time.  The
 * packer resolves each request's (policy, direction, port) evaluation
 * program on the host and groups requests by program (padding each group to
 * whole tiles), so a workgroup stages one program's DFA in LDS.  A batch is
 * a 64-byte header (its total_bytes field = the batch's size), a chunk
 * table, a tile table ({offset in 512-B granules, units | half << 15 |
 * last-unit bytes << 16} per tile), then the tiles;
 * slots are in grouped order and order[slot] gives the request index
 * (UINT32_MAX for padding).  Size the buffers with cg_http_batch_bytes /
 * cg_http_batch_slots (upper bounds for n requests under the installed
 * policy; a batch is tied to the snapshot it was packed against — after a
 * policy update it is rejected and every slot is denied).  A program whose
 * strings are packed as byte-class codes spends its free codes on literals of
 * its rules (literal tokens): cg_http_pack writes such a literal as one
 * symbol, the program's table walks it as it walks the literal's bytes, and a
 * string counts as longer than CG_HTTP_SLOT_BYTES by its length before that.
 * CILIUM_GPU_PACK_TOKENS=0, read per call, packs without tokens. */
#define CG_HTTP_TILE 64
#define CG_HTTP_UNITS 9
#define CG_HTTP_SLOT_BYTES 128
#define CG_HTTP_META_BYTES 8
size_t cg_http_batch_bytes(uint64_t h, size_t n);
size_t cg_http_batch_slots(uint64_t h, size_t n);

/* Request flags (meta byte 7).  Meta word: [0..3] remote identity, [4..6]
 * overflow arena offset / 16, [7] flags.  An overflow arena entry is the
 * string's u32 length followed by the string. */
#define CG_HTTP_F_INGRESS 0x01u
#define CG_HTTP_F_OVERFLOW 0x02u  /* fields in the overflow arena */
#define CG_HTTP_F_MALFORMED 0x04u /* field holds a byte Envoy's codec rejects */
#define CG_HTTP_F_PAD 0x08u

/* Worker threads cg_http_pack uses for a large batch (CILIUM_GPU_PACK_THREADS,
 * else the hardware threads, at most 16). */
uint32_t cg_http_pack_threads(void);
/* Pack n requests.  Request i: policy index policy[i] (UINT32_MAX unknown),
 * direction ingress[i], destination port port[i], remote identity
 * remote[i] (source identity on ingress, destination on egress,
 * cilium_l7policy.cc:144-150), and its header list as NUL-separated
 * "name\0value\0" pairs in hdr_blob[hdr_off[i] .. hdr_off[i+1]).  Header
 * names compare case-insensitively and only the first value of a name is
 * seen (Envoy HeaderMap::get).  Records whose slot string exceeds 128 bytes
 * spill into the overflow arena: pass arena/arena_cap (may be NULL/0 to
 * query), *arena_used gets the bytes needed; one batch's arena is at most
 * 256 MiB (CG_INVALID_ARGUMENT beyond: pack such a request set as several
 * batches; cg_http_verdicts_raw_* splits by itself).  *nslots gets the batch's slot
 * count; order must hold cg_http_batch_slots(h, n) entries. */
int cg_http_pack(uint64_t h, size_t n, const uint32_t* policy, const uint8_t* ingress,
                 const uint16_t* port, const uint32_t* remote, const uint8_t* hdr_blob,
                 const uint64_t* hdr_off, void* batch, size_t batch_cap, uint32_t* order,
                 size_t* nslots, uint8_t* arena, size_t arena_cap, size_t* arena_used);

/* HTTP/1.x request heads from raw bytes (the Envoy codec
 * step in front of AccessFilter::decodeHeaders, cilium_l7policy.cc:127-170).
 * Request r is raw[raw_off[r] .. raw_off[r+1]): request-line, header fields,
 * empty line.  Writes the cg_http_pack header lists (:method, :path with the
 * query, :authority from Host, then the other headers as sent) into hdr_blob
 * / hdr_off (n+1 entries) and ok[r] = 0 (ok may be NULL) for a head the
 * codec rejects (bad request-line, non-token name, control byte in a value,
 * no final CRLF).  A rejected head's list is one entry whose value is the
 * byte 0x7F, which cg_http_pack flags CG_HTTP_F_MALFORMED: it is denied
 * under any policy, as Envoy answers 400 before the filter.  hdr_blob NULL
 * = size query (*blob_used). */
int cg_http_parse_heads(const uint8_t* raw, const uint64_t* raw_off, size_t n, uint8_t* hdr_blob,
                        size_t blob_cap, uint64_t* hdr_off, size_t* blob_used, uint8_t* ok);

/* Raw HTTP/1 request heads to verdicts on the device: the codec step of
 * cg_http_parse_heads, the packing of cg_http_pack and the verdicts of
 * cg_http_verdicts_dev in one call, with the request bytes never leaving
 * device memory (the consumer is AccessFilter::
 * decodeHeaders, envoy/cilium_l7policy.cc:127-170).  Request r is
 * d_raw[d_raw_off[r] .. d_raw_off[r+1]) with d_policy/d_ingress/d_port/
 * d_remote as in cg_http_pack; d_out[r] = 1 allow, 0 deny, request order.
 * Heads over 60 KiB are rejected (Envoy's default max_request_headers_kb).
 * Enqueued on `stream` and returns without waiting (NULL: the handle's
 * stream, waited for before the call returns):
 * slots, tiles, chunk table and header are laid out on the device, strings
 * past the 128-byte slot walked one lane each; a later call on another
 * stream waits for this one on the device.  An offset range that runs
 * backwards is an empty (rejected) request — the call has returned before
 * the device reads the offsets.  CILIUM_GPU_RAW_LAYOUT=host selects the
 * round-3 sequence instead (host layout step, synchronizes the stream,
 * CG_INVALID_ARGUMENT for backward offsets).  CG_UNSUPPORTED when the
 * snapshot walks more than 32 header fields or is a proxylib snapshot. */
int cg_http_verdicts_raw_dev(uint64_t h, const uint8_t* d_raw, const uint64_t* d_raw_off, size_t n,
                             const uint32_t* d_policy, const uint8_t* d_ingress, const uint16_t* d_port,
                             const uint32_t* d_remote, uint8_t* d_out, void* stream);

/* cg_http_verdicts_raw_dev from host memory (staged in, verdicts copied out). */
int cg_http_verdicts_raw_host(uint64_t h, const uint8_t* raw, const uint64_t* raw_off, size_t n,
                              const uint32_t* policy, const uint8_t* ingress, const uint16_t* port,
                              const uint32_t* remote, uint8_t* out);

/* Parsed header lists to verdicts on the device: the input of cg_http_pack
 * (request i's "name\0value\0" pairs in d_hdr_blob[d_hdr_off[i] ..
 * d_hdr_off[i+1]), names case-insensitive, first value wins, the codec's
 * value check — the header map AccessFilter::decodeHeaders sees,
 * envoy/cilium_l7policy.cc:127-182) grouped, sorted and packed by the raw
 * path's kernels instead of on the host, then cg_http_verdicts_dev; d_out[i]
 * = 1 allow, 0 deny, request order.  Proxylib snapshots take escaped values
 * as cg_http_pack does.  One request's list holds at most 65535 bytes
 * (Envoy's default header limit is 60 KiB): a longer one is denied here (the
 * host entry and the round-3 sequence refuse the call, CG_INVALID_ARGUMENT).
 * Stream and synchronization as cg_http_verdicts_raw_dev; CG_UNSUPPORTED when
 * the snapshot walks more than 32 header fields. */
int cg_http_verdicts_fields_dev(uint64_t h, const uint8_t* d_hdr_blob, const uint64_t* d_hdr_off, size_t n,
                                const uint32_t* d_policy, const uint8_t* d_ingress, const uint16_t* d_port,
                                const uint32_t* d_remote, uint8_t* d_out, void* stream);

/* cg_http_verdicts_fields_dev from host memory (staged in, verdicts copied
 * out): the drop-in for cg_http_pack + cg_http_verdicts_host.  A call of at
 * most 1024 lists (Envoy-sized: decodeHeaders decides one request,
 * envoy/cilium_l7policy.cc:127-182) is packed on the calling thread and
 * decided with one staged copy in, one launch and one copy out; larger ones
 * are grouped and packed on the GPU.  Any snapshot works at any size: when
 * the device packer does not take it (more than 32 header fields walked),
 * larger calls are packed on the calling thread too, 1M lists at a time. */
int cg_http_verdicts_fields_host(uint64_t h, const uint8_t* hdr_blob, const uint64_t* hdr_off, size_t n,
                                 const uint32_t* policy, const uint8_t* ingress, const uint16_t* port,
                                 const uint32_t* remote, uint8_t* out);

/* The persistent verdict ring: Envoy-sized calls (AccessFilter::decodeHeaders
 * decides one request, envoy/cilium_l7policy.cc:127-182) without a launch,
 * staged copies or a stream synchronization per call.  cg_http_ring_open
 * starts `workgroups` one-wave workgroups (1..256) that poll `slots`
 * (1..64 * workgroups) request slots in pinned host memory; a call of
 * cg_http_ring_verdicts claims a slot, writes its header lists there, rings
 * the slot's doorbell and spins until the kernel has written the verdicts.
 * Same inputs, outputs and verdicts as cg_http_verdicts_fields_host (which
 * decides calls past a slot: more than 256 lists or 32 KiB of list bytes,
 * and snapshots walking more than 32 header fields).  The kernel serves the
 * handle's current policy: a cg_http_policy_update restarts it before the
 * next call; it leaves by itself after 50 ms without a call (the next call
 * starts it again, ~20 us).  cg_http_ring_close (or cg_close) stops it. */
int cg_http_ring_open(uint64_t h, uint32_t workgroups, uint32_t slots);
int cg_http_ring_verdicts(uint64_t h, const uint8_t* hdr_blob, const uint64_t* hdr_off, size_t n,
                          const uint32_t* policy, const uint8_t* ingress, const uint16_t* port,
                          const uint32_t* remote, uint8_t* out);
/* Calls served by the ring's kernels and launches made, cumulative. */
int cg_http_ring_stats(uint64_t h, uint64_t* served, uint64_t* launches);
int cg_http_ring_close(uint64_t h);

/* NetworkPolicyMap::Allowed per slot (cilium_network_policy.h:223-237):
 * d_out[slot] = 1 allow, 0 deny (→ 403), in batch slot order.  d_arena may
 * be NULL when no record overflowed.  Per-(policy,direction,port) allowed/
 * denied counters advance (metrics policy_l7_forwarded/denied_total,
 * pkg/metrics/metrics.go:270-296). */
int cg_http_verdicts_dev(uint64_t h, const void* d_batch, size_t nslots, const uint8_t* d_arena,
                         uint8_t* d_out, void* stream);
/* Host convenience: uploads the batch, runs the kernel and writes out[i]
 * for request i (un-permuting through order). */
int cg_http_verdicts_host(uint64_t h, const void* batch, size_t nslots, const uint32_t* order,
                          size_t n, const uint8_t* arena, size_t arena_len, uint8_t* out);
/* The same verdicts with each request's first matching rule beside it:
 * d_rule[slot] = the per-rule counter index it adds to (cg_http_rule_info_get
 * order: the PortNetworkPolicyRule / HTTP rule that allowed it, Envoy's
 * evaluation order), or UINT32_MAX when no rule allows it (denied, or
 * allowed because no HTTP policy applies).  Replaces the access log's rule
 * attribution (pkg/proxy/accesslog/record.go:36-47) and the policy trace
 * (pkg/policy/policy.go:29-70) for every request of a batch. */
int cg_http_verdicts_rules_dev(uint64_t h, const void* d_batch, size_t nslots, const uint8_t* d_arena,
                               uint8_t* d_out, uint32_t* d_rule, void* stream);
int cg_http_verdicts_rules_host(uint64_t h, const void* batch, size_t nslots, const uint32_t* order,
                                size_t n, const uint8_t* arena, size_t arena_len, uint8_t* out,
                                uint32_t* rule);

/* ======================================================================== */
/* Kafka L7: pkg/kafka/policy.go:144-225 via pkg/proxy/kafka.go:117-153      */
/* ======================================================================== */

/* Install Kafka redirect rule sets, JSON form of L7DataMap per redirect:
 *   [{"name": "...", "selectors": [
 *       {"identities": [1, 2] or null for the wildcard selector,
 *        "rules": [{"role": "...", "apiKey": "...", "apiVersion": "...",
 *                   "clientID": "...", "topic": "..."}]}]}]
 * Each PortRuleKafka is Sanitize()d (pkg/policy/api/rule_validation.go:232-275);
 * a failure rejects the whole update. */
int cg_kafka_policy_update(uint64_t h, const char* json, size_t len);
int cg_kafka_policy_index(uint64_t h, const char* name, uint32_t* index);

/* Packed Kafka request: 64 bytes. */
#define CG_KAFKA_MAX_TOPICS 12
typedef struct {
  int16_t api_key;      /* RequestMessage.kind */
  int16_t api_version;  /* RequestMessage.version */
  uint8_t kind;         /* CG_KAFKA_K_*: which typed request ReadRequest produced */
  uint8_t n_topics;     /* topics in topic_ids (> CG_KAFKA_MAX_TOPICS: in the arena at
                           topic_ids[0]; CG_KAFKA_TOPICS_IN_ARENA: count in topic_ids[1]) */
  uint16_t policy;      /* redirect index (UINT16_MAX unknown → deny) */
  uint32_t remote;      /* source identity (0 = unknown: wildcard rules only) */
  uint32_t client_id;   /* interned ClientID (CG_KAFKA_UNKNOWN_STR if not a rule string) */
  uint32_t topic_ids[CG_KAFKA_MAX_TOPICS]; /* interned topics; overflow: [0] = arena offset */
} cg_kafka_request;

#define CG_KAFKA_TOPICS_IN_ARENA 255  /* n_topics value for 255+ topics */
#define CG_KAFKA_K_NIL 0      /* request == nil (unparsed kinds) */
#define CG_KAFKA_K_TYPED 1    /* Produce/Fetch/Offset/Metadata/OffsetCommit/OffsetFetch */
#define CG_KAFKA_K_CONSUMER_METADATA 2
#define CG_KAFKA_UNKNOWN_STR 0xFFFFFFFFu

/* Intern a string against the installed Kafka snapshot's topic / clientID
 * dictionaries (what=0 topic, 1 clientID). */
int cg_kafka_intern(uint64_t h, uint32_t what, const char* s, size_t len, uint32_t* id);

/* Kafka requests from their wire bytes: ReadRequest (pkg/kafka/request.go:
 * 186-229) with the vendored optiopay/kafka decoders it calls (proto
 * ReadReq and Read{Produce,Fetch,Offset,Metadata,ConsumerMetadata,
 * OffsetCommit,OffsetFetch}Req, messages.go:124-166,504,767,1033,1173,1389,
 * 1591,1810; produce message sets parsed in full with CRC32 checks and
 * gzip / snappy payloads inflated, as pkg/proxy/kafka.go:449-451 configures).
 * Request i is raw[raw_off[i] .. raw_off[i+1]): the connection's bytes from
 * the start of the request (ReadReq reads 4 + size of them).  Writes one
 * cg_kafka_request per request (topics and clientID interned against the
 * installed snapshot, redirect[i] / remote[i] copied) and status[i]:
 * CG_KAFKA_DECODE_OK, or CG_KAFKA_DECODE_ERROR when ReadRequest returns an
 * error — the proxy closes the connection (kafka.go:340-347); such a
 * record is marked to be denied (policy UINT16_MAX).  Topic lists longer
 * than CG_KAFKA_MAX_TOPICS go to `arena` (arena_cap u32 entries); *arena_used
 * gets the entries the batch needs, and the call fails with CG_MAP_FULL
 * when that exceeds arena_cap (arena_cap >= raw bytes / 2 always suffices).
 * raw_off must be non-decreasing; raw holds raw_off[n] bytes.  The decode
 * runs on the GPU (cg_kafka_decode_dev on staged copies). */
#define CG_KAFKA_DECODE_OK 0
#define CG_KAFKA_DECODE_ERROR 1
int cg_kafka_decode_host(uint64_t h, const uint8_t* raw, const uint64_t* raw_off, size_t n,
                         const uint16_t* redirect, const uint32_t* remote, cg_kafka_request* reqs,
                         uint32_t* arena, size_t arena_cap, size_t* arena_used, uint8_t* status);

/* Kafka decode accounting of the handle, cumulative: compressed message
 * payloads (gzip / snappy, optiopay proto/messages.go:460-480) decoded on
 * the GPU, and requests the device handed to the host decoder (a nested
 * compressed set, a second gzip member, a payload past the per-call inflate
 * arena).  Either pointer may be NULL. */
int cg_kafka_decode_stats(uint64_t h, uint64_t* device_inflated, uint64_t* host_deferred);

/* Compressed payloads the device handed to the host decoder without
 * reserving inflate-arena space, cumulative: the per-call arena
 * (kKafkaInflateArena) was full, or the size the payload declares (gzip
 * ISIZE, snappy length) is more than its bytes can decode to (DEFLATE
 * 1032:1, snappy 32:1), so a sender's claim cannot use up the arena.  The
 * host decoder gives these requests their outcome either way. */
int cg_kafka_inflate_stats(uint64_t h, uint64_t* unreserved);

/* The same decode on the GPU (one lane per request, raw bytes in HBM),
 * records and statuses in device memory.  d_raw_off holds n + 1 offsets.
 * Requests carrying gzip / snappy messages are finished by the host
 * decoder (the device reports them, the call decodes them on the CPU and
 * patches their records before returning), so this call synchronizes.
 * d_arena: arena_cap u32 entries of device memory for long topic lists;
 * *arena_used and CG_MAP_FULL as for cg_kafka_decode_host.  A decreasing
 * offset pair is read as an empty request. */
int cg_kafka_decode_dev(uint64_t h, const uint8_t* d_raw, const uint64_t* d_raw_off, size_t n,
                        const uint16_t* d_redirect, const uint32_t* d_remote, cg_kafka_request* d_reqs,
                        uint32_t* d_arena, size_t arena_cap, size_t* arena_used, uint8_t* d_status,
                        void* stream);

/* Raw requests → verdicts in one call (decode on the GPU, then the verdict
 * kernel): out[i] = 1 forward, 0 deny (ErrTopicAuthorizationFailed),
 * 2 = ReadRequest failed (connection closed). */
#define CG_KAFKA_V_DENY 0
#define CG_KAFKA_V_ALLOW 1
#define CG_KAFKA_V_CLOSE 2
int cg_kafka_verdicts_raw_host(uint64_t h, const uint8_t* raw, const uint64_t* raw_off, size_t n,
                               const uint16_t* redirect, const uint32_t* remote, uint8_t* out);

/* kafkaRedirect.canAccess per request: out[i] = 1 allow, 0 deny. */
int cg_kafka_verdicts_dev(uint64_t h, const cg_kafka_request* d_reqs, size_t n,
                          const uint32_t* d_arena, uint8_t* d_out, void* stream);
int cg_kafka_verdicts_host(uint64_t h, const cg_kafka_request* reqs, size_t n,
                           const uint32_t* arena, size_t arena_len, uint8_t* out);
/* The same verdicts over the record split in two arrays: d_heads[i] = the
 * first 16 bytes of cg_kafka_request i, d_topics[12 i .. 12 i + 11] = its
 * topic_ids.  Most requests are settled from the head alone (the decision
 * summaries), so HBM moves 16 bytes per request instead of a 64-byte record
 * line; topic tails are read only for the requests that need their topics. */
typedef struct {
  int16_t api_key;
  int16_t api_version;
  uint8_t kind;
  uint8_t n_topics;
  uint16_t policy;
  uint32_t remote;
  uint32_t client_id;
} cg_kafka_request_head;
int cg_kafka_verdicts_split_dev(uint64_t h, const cg_kafka_request_head* d_heads, const uint32_t* d_topics,
                                size_t n, const uint32_t* d_arena, uint8_t* d_out, void* stream);

/* ======================================================================== */
/* Counters                                                                  */
/* ======================================================================== */
/* what: 0 = HTTP per-program {allowed, denied} u64 pairs,
 *       1 = Kafka per-redirect {allowed, denied} u64 pairs,
 *       2 = prefilter {drop, pass} u64 pair for pf_or_map,
 *       3 = HTTP per-rule first-match hits (cg_http_rule_info_get order),
 *       4 = the HTTP all-reduce vector: the per-program pairs, the stale-
 *           batch count, then the per-rule hits (one contiguous device
 *           buffer, summed across GPUs by RCCL).
 * Writes min(cap, available) u64 values, *n = available. */
#define CG_CTR_HTTP_PROGRAMS 0u
#define CG_CTR_KAFKA 1u
#define CG_CTR_PREFILTER 2u
#define CG_CTR_HTTP_RULES 3u
#define CG_CTR_HTTP_ALLREDUCE 4u
int cg_read_counters(uint64_t h, uint32_t what, uint32_t pf_or_map, uint64_t* out, size_t cap,
                     size_t* n);
/* Same, into a device buffer (for an RCCL all-reduce across GPUs). */
int cg_counters_device_ptr(uint64_t h, uint32_t what, uint32_t pf_or_map, void** d_ptr,
                           size_t* n);
/* Async device-to-device copy of up to n counters into d_dst on stream. */
int cg_counters_copy_dev(uint64_t h, uint32_t what, uint32_t pf_or_map, void* d_dst, size_t n,
                         void* stream);
int cg_reset_counters(uint64_t h);

/* Synchronize the handle's stream. */
int cg_sync(uint64_t h);

/* Regex syntax check, no compilation: flavour CG_REGEX_GO = Go 1.10
 * regexp.Compile's grammar (PortRuleHTTP.Sanitize,
 * pkg/policy/api/http.go:66-84; proxylib's regexp.MustCompile,
 * proxylib/r2d2/r2d2parser.go:103), CG_REGEX_ECMA = std::regex's (what
 * Envoy compiles for regex_match, envoy/cilium_network_policy.h:68-71).
 * Returns CG_OK or CG_POLICY_REJECTED (message in cg_last_error). */
enum { CG_REGEX_ECMA = 0, CG_REGEX_GO = 1 };
int cg_regex_validate(const char* re, size_t re_len, uint32_t flavour);

/* ======================================================================== */
/* Selector cache: label selectors -> identity sets, and L3 reachability    */
/* (getSecurityIdentities, pkg/endpoint/policy.go:93-106;                   */
/* computeDesiredL3PolicyMapEntries, :298-371; EndpointSelector.Matches,    */
/* pkg/policy/api/selector.go:279-310; LabelArray.Get,                      */
/* pkg/labels/array.go:90-131; canReachIngress / canReachEgress,            */
/* pkg/policy/rule.go:352-440; GetRulesMatching, repository.go:624-643)     */
/* ======================================================================== */

/* Requirement operators.  MATCH_LABEL is a matchLabels pair (one value, may
 * be ""); the others are the matchExpressions operators.  Any other value is
 * refused with CG_POLICY_REJECTED. */
enum {
  CG_SEL_MATCH_LABEL = 0,
  CG_SEL_IN = 1,
  CG_SEL_NOT_IN = 2,
  CG_SEL_EXISTS = 3,
  CG_SEL_DOES_NOT_EXIST = 4
};

/* A table of selectors.  Selector s owns the requirements
 * [req_off[s], req_off[s+1]); requirement r has the key string
 * key_blob[key_off[r] .. key_off[r+1]) ("source:key"; without a colon the
 * source is "any"), the operator ops[r], and the value strings
 * [val_off[r], val_off[r+1]), value v being val_blob[val_str_off[v] ..
 * val_str_off[v+1]).  A selector without requirements, or with a MATCH_LABEL
 * key exactly "reserved:all", selects every identity. */
typedef struct {
  size_t n_selectors;
  const uint32_t* req_off;      /* n_selectors + 1 */
  const uint8_t* ops;           /* per requirement: CG_SEL_* */
  const uint8_t* key_blob;
  const uint64_t* key_off;      /* requirements + 1 */
  const uint32_t* val_off;      /* requirements + 1 */
  const uint8_t* val_blob;
  const uint64_t* val_str_off;  /* values + 1 */
} cg_selector_table;

/* A rule set over a selector table, per direction d (0 ingress, 1 egress):
 * rule r's "require" selectors are req_idx[d][req_off[d][r] .. req_off[d][r+1])
 * (FromRequires / ToRequires of all its direction rules) and its "allow"
 * selectors allow_idx[d][...] (the source / destination selectors, entities
 * included, of its direction rules without ToPorts). */
typedef struct {
  size_t n_rules;
  const uint32_t* subject;       /* n_rules: the rule's EndpointSelector */
  const uint8_t* dir_flags;      /* n_rules: bit 0 has ingress rules, bit 1 has egress rules */
  const uint32_t* req_off[2];    /* n_rules + 1 each */
  const uint32_t* req_idx[2];
  const uint32_t* allow_off[2];  /* n_rules + 1 each */
  const uint32_t* allow_idx[2];
} cg_selcache_rules;

int cg_selcache_create(uint64_t h, uint32_t* sc_id);
int cg_selcache_destroy(uint64_t h, uint32_t sc_id);
/* The identity cache, replaced as a whole: identity i (ids[i]) has the labels
 * [label_off[i], label_off[i+1]) in the given order, label l being the key
 * key_blob[key_off[l] .. key_off[l+1]) ("source:key") and the value
 * val_blob[val_off[l] .. val_off[l+1]).  Bit positions of every result
 * follow this order. */
int cg_selcache_set_identities(uint64_t h, uint32_t sc_id, const uint32_t* ids, size_t n,
                               const uint32_t* label_off, const uint8_t* key_blob, const uint64_t* key_off,
                               const uint8_t* val_blob, const uint64_t* val_off);
/* The prefix section, replaced as a whole (all or nothing): identities that
 * are a CIDR prefix (AllocateCIDRs, pkg/ipcache/cidr.go:26-86).  The cache
 * then holds the N label identities of cg_selcache_set_identities followed by
 * these n prefix identities: bits N .. N+n-1 in the given order, no padding
 * between the sections, words = ceil((N + n) / 64), and every result —
 * match, reach, expansion, entries, cg_selcache_info — covers both.  Prefix
 * identity P/m behaves in every selector exactly as a label identity carrying
 * GetCIDRLabels(P/m) (pkg/labels/cidr/cidr.go:32-50) in that order:
 * cidr:<P masked to i>/i for i in 0..m when m > 0, then reserved:world, all
 * with the value "".  Address bits below the prefix are masked (as NewKey
 * does for the ipcache); a family other than 4 or 6 or a prefix length past
 * the family's is CG_INVALID_ARGUMENT and keeps the previous tables.
 * Replacing the label section leaves this one in place and the other way
 * round; n = 0 (the state after create) leaves a label-only cache. */
int cg_selcache_set_cidr_identities(uint64_t h, uint32_t sc_id, const uint32_t* ids, const cg_cidr* prefixes,
                                    size_t n);
/* The rule set and its selectors, replaced as a whole (all or nothing). */
int cg_selcache_set_rules(uint64_t h, uint32_t sc_id, const cg_selector_table* sels,
                          const cg_selcache_rules* rules);
/* sizes of the current tables: identities (both sections), words per row
 * (ceil(n / 64)), selectors of the rule set, rules */
int cg_selcache_info(uint64_t h, uint32_t sc_id, size_t* n_identities, size_t* words, size_t* n_selectors,
                     size_t* n_rules);
/* bits[S][W]: bit i of word w of row s says whether selector s selects
 * identity 64*w + i; the padding bits of the last word are zero.  sels (a
 * HOST table in both variants) may be NULL: the rule set's selectors.
 * cap_words: room in bits (>= S * W). */
int cg_selcache_match_dev(uint64_t h, uint32_t sc_id, const cg_selector_table* sels, uint64_t* d_bits,
                          size_t cap_words, void* stream);
int cg_selcache_match_host(uint64_t h, uint32_t sc_id, const cg_selector_table* sels, uint64_t* bits,
                           size_t cap_words);
/* Per endpoint e (an index into the identity table): the identities it
 * accepts at L3 on ingress ing[e][W] and may reach on egress eg[e][W]
 * (AllowsIngressLabelAccess / AllowsEgressLabelAccess against every
 * identity), and flags[e] (bit 0 ingress, bit 1 egress enforcement:
 * GetRulesMatching). */
int cg_selcache_reach_dev(uint64_t h, uint32_t sc_id, const uint32_t* d_endpoints, size_t n, uint64_t* d_ing,
                          uint64_t* d_eg, uint8_t* d_flags, void* stream);
int cg_selcache_reach_host(uint64_t h, uint32_t sc_id, const uint32_t* endpoints, size_t n, uint64_t* ing,
                           uint64_t* eg, uint8_t* flags);

/* Expansion of bitset rows into policy-map entries: the identity loops of
 * convertL4FilterToPolicyMapKeys (pkg/endpoint/policy.go:111-130),
 * computeDesiredL4PolicyMapEntries (:144-193) and
 * computeDesiredL3PolicyMapEntries (:298-371) over a source matrix
 * src[src_rows][W] in the layout of the match / reach results. */
#define CG_EXP_ALL 0x1u /* the row holds every identity (an unenforced direction, policy.go:311-313,343-345) */
/* One expansion row: the policy-map key every entry of the row shares
 * (policymap.go:64-69) and its value's proxy port (policymap.go:73-80). */
typedef struct {
  uint16_t dport;       /* network byte order */
  uint8_t protocol;
  uint8_t egress;
  uint16_t proxy_port;  /* network byte order */
  uint16_t flags;       /* CG_EXP_* */
} cg_expand_row;
/* Row r's identity set is the OR of the source rows
 * src_idx[src_off[r] .. src_off[r+1]) — every identity with CG_EXP_ALL, none
 * for an empty list without it — restricted to the identities that exist
 * (padding bits of the source matrix are ignored). */
typedef struct {
  size_t n_rows;
  const cg_expand_row* rows;
  const uint32_t* src_off;  /* n_rows + 1 */
  const uint32_t* src_idx;
} cg_expand_table;
/* row_off[n_rows + 1]: row r owns the entries [row_off[r], row_off[r+1]), in
 * ascending bit order; keys[k].sec_label is the identity number of the bit,
 * the rest of the key and proxy[k] are the row's.  *total (may be NULL in
 * the _dev variant) = row_off[n_rows].  When *total > cap_entries, keys and
 * proxy are left untouched and row_off is still valid, so cap_entries = 0
 * sizes the buffers as cg_policymap_dump does.  table is a HOST table in all
 * variants; a source index >= src_rows is CG_INVALID_ARGUMENT.
 * _dev: device pointers (d_keys 8-byte aligned), asynchronous on stream. */
int cg_selcache_expand_dev(uint64_t h, uint32_t sc_id, const cg_expand_table* table, const uint64_t* d_src,
                           size_t src_rows, uint64_t* d_row_off, cg_policy_key* d_keys, uint16_t* d_proxy,
                           size_t cap_entries, uint64_t* d_total, void* stream);
int cg_selcache_expand_host(uint64_t h, uint32_t sc_id, const cg_expand_table* table, const uint64_t* src,
                            size_t src_rows, uint64_t* row_off, cg_policy_key* keys, uint16_t* proxy,
                            size_t cap_entries, uint64_t* total);
/* The fused regeneration step (computeDesiredPolicyMapState's identity
 * loops, policy.go:144-193 and :298-371): match, reach, expansion and one
 * copy back on the handle's stream.  The source matrix is sels' match rows
 * (S of them; sels may be NULL, S = 0), then the endpoints' ingress reach
 * rows (n_endpoints), then their egress reach rows.  flags[n_endpoints] are
 * the enforcement flags of cg_selcache_reach_host. */
int cg_selcache_entries_host(uint64_t h, uint32_t sc_id, const cg_selector_table* sels, const uint32_t* endpoints,
                             size_t n_endpoints, const cg_expand_table* table, uint64_t* row_off,
                             cg_policy_key* keys, uint16_t* proxy, size_t cap_entries, uint64_t* total,
                             uint8_t* flags);

/* syncPolicyMap (pkg/endpoint/endpoint.go:2621-2701) as one update: the map
 * holds exactly the given entries afterwards.  Keys absent from the list are
 * deleted (*deleted); keys that are new or whose proxy port differs are
 * written (*added); surviving keys keep their counters; a key given twice
 * takes its last value.  All or nothing: more distinct keys than max_entries
 * is CG_MAP_FULL and the map is unchanged.  One table rebuild and one
 * publish, at the next verdict call.  added / deleted may be NULL. */
int cg_policymap_sync(uint64_t h, uint32_t map_id, const cg_policy_key* keys, const uint16_t* proxy_ports_be,
                      size_t n, size_t* added, size_t* deleted);

/* ======================================================================== */
/* Diagnostics (CPU test-suite only; no verdict entry point calls these)    */
/* ======================================================================== */
/* Compile `re` with the engine's regex compiler and run the DFA on s
 * (search = 0: std::regex_match, ECMAScript; 1: Go regexp.MatchString). */
int cg_diag_regex_match(const char* re, size_t re_len, const uint8_t* s, size_t len,
                        uint32_t search, uint8_t* result);
/* Walk the compiled HTTP / Kafka tables on the host, exactly as the kernels
 * do, to test the compilers without a GPU. */
int cg_diag_http_eval_host(uint64_t h, const void* batch, size_t nslots, const uint32_t* order,
                           size_t n, const uint8_t* arena, size_t arena_len, uint8_t* out);
/* The literal tokens of program `prog` (its index in the per-program
 * counters): code_map[256] receives the code the packer writes for each
 * string byte (the byte itself for a program without class codes), out the
 * records {token code, length, that many class codes}; *used is their size.
 * cg_http_pack writes a token's code for its class-code sequence unless
 * CILIUM_GPU_PACK_TOKENS=0 is set; the tables walk both to the same state. */
int cg_diag_http_tokens(uint64_t h, uint32_t prog, uint8_t* code_map, uint8_t* out, size_t cap, size_t* used);
/* The same walk, reporting per request the per-rule hit counter it adds to
 * (cg_http_rule_info_get index), or UINT32_MAX when no rule allows it. */
int cg_diag_http_rules_host(uint64_t h, const void* batch, size_t nslots, const uint32_t* order,
                            size_t n, const uint8_t* arena, size_t arena_len, uint32_t* rule);
int cg_diag_kafka_eval_host(uint64_t h, const cg_kafka_request* reqs, size_t n,
                            const uint32_t* arena, size_t arena_len, uint8_t* out);
/* cg_kafka_decode_host's decode on the CPU (the host decoder that also
 * finishes compressed produce requests), for cross-checking the GPU. */
int cg_diag_kafka_decode_host(uint64_t h, const uint8_t* raw, const uint64_t* raw_off, size_t n,
                              const uint16_t* redirect, const uint32_t* remote, cg_kafka_request* reqs,
                              uint32_t* arena, size_t arena_cap, size_t* arena_used, uint8_t* status);
int cg_diag_l4_eval_host(uint64_t h, uint32_t map_id, const cg_l4_tuple* tuples, size_t n,
                         int32_t* verdicts);
/* The array's tables walked on the host exactly as l4_array_kernel walks
 * them, with `mode` applied (no counters). */
int cg_diag_l4_array_eval_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint16_t* lxc_ids,
                               const cg_l4_tuple* tuples, size_t n, int32_t* verdicts);
/* cg_l4_frames_verdicts_* on the host: the kernel's own walk (frame_walk.h,
 * l4_walk.h) over the host copies of the tables.  Needs no device and moves
 * no counters.  l4_off (may be NULL): the L4 offset the walk found per frame,
 * 0 where it did not get that far. */
int cg_diag_l4_frames_eval_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                                const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids, uint32_t ep_id,
                                const uint32_t* src_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                                int32_t* verdicts, cg_l4_frame_info* info, uint32_t* l4_off);
/* cg_l4_frames_ct_verdicts_* on the host: the kernel's own walk and lookup
 * (frame_walk.h, ct_walk.h) over the host copy of the conntrack tables.  No
 * device, no counters. */
int cg_diag_l4_frames_ct_eval_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                                   const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids, uint32_t ep_id,
                                   const uint32_t* src_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                                   uint32_t ct_id, int32_t* verdicts, cg_l4_frame_info* info,
                                   cg_ct_record* records, uint32_t* l4_off);
/* cg_l4_frames_egress_verdicts_* on the host: the kernel's own walk
 * (egress_walk.h) over the host views; no device, no counters. */
int cg_diag_l4_frames_egress_eval_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                                       const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids,
                                       const uint32_t* dst_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                                       uint32_t ct_id, int32_t* verdicts, cg_l4_frame_info* info,
                                       cg_ct_record* records, uint32_t* l4_off);
/* The conntrack tables' own hash of each key (before the bucket mask), and
 * the built tables' shape: buckets and the recorded probe bound per family
 * ([0] v4, [1] v6).  For tests that build probe chains. */
/* cg_l4_frames_egress_svc_verdicts_* on the host: the kernel's own walk
 * (egress_walk.h, lb_walk.h) per frame over the maps' host views. */
int cg_diag_l4_frames_egress_svc_eval_host(uint64_t h, uint32_t arr_id, uint32_t mode, const uint8_t* raw,
                                           const uint64_t* raw_off, size_t n, const uint16_t* lxc_ids,
                                           const uint32_t* dst_labels, uint32_t ipc_id, const uint32_t* pkt_len,
                                           uint32_t ct_id, uint32_t lb_id, const uint32_t* hash, int32_t* verdicts,
                                           cg_l4_frame_info* info, cg_ct_record* records, cg_ct_record* svc_records,
                                           cg_lb_xlate* xlate, uint32_t* l4_off);
int cg_diag_ct_hash(const cg_ct_key* keys, size_t n, uint32_t* hashes);
int cg_diag_ct_map_info(uint64_t h, uint32_t ct_id, uint32_t buckets[2], uint32_t probes[2]);
/* The ipcache tables walked on the host exactly as ipcache_kernel does. */
int cg_diag_ipcache_eval_host(uint64_t h, uint32_t ipc_id, const uint32_t* v4, size_t n4,
                              cg_remote_endpoint_info* out4, const uint8_t* v6, size_t n6,
                              cg_remote_endpoint_info* out6);
int cg_diag_prefilter_eval_host(uint64_t h, uint32_t pf_id, const uint32_t* v4, size_t n4,
                                uint8_t* out4, const uint8_t* v6, size_t n6, uint8_t* out6);
/* The selector cache's compiled tables walked on the host (threads: worker
 * threads, 0 = 1); same arguments and results as cg_selcache_match_host /
 * cg_selcache_reach_host.  They also work on a handle without a GPU. */
int cg_diag_selcache_match_host(uint64_t h, uint32_t sc_id, const cg_selector_table* sels, uint64_t* bits,
                                size_t cap_words, uint32_t threads);
int cg_diag_selcache_reach_host(uint64_t h, uint32_t sc_id, const uint32_t* endpoints, size_t n, uint64_t* ing,
                                uint64_t* eg, uint8_t* flags, uint32_t threads);
/* cg_selcache_expand_host / cg_selcache_entries_host from the host walkers
 * (the identity loops of policy.go:111-130, :144-193, :298-371 over the
 * compiled tables); same arguments and results. */
int cg_diag_selcache_expand_host(uint64_t h, uint32_t sc_id, const cg_expand_table* table, const uint64_t* src,
                                 size_t src_rows, uint64_t* row_off, cg_policy_key* keys, uint16_t* proxy,
                                 size_t cap_entries, uint64_t* total, uint32_t threads);
int cg_diag_selcache_entries_host(uint64_t h, uint32_t sc_id, const cg_selector_table* sels,
                                  const uint32_t* endpoints, size_t n_endpoints, const cg_expand_table* table,
                                  uint64_t* row_off, cg_policy_key* keys, uint16_t* proxy, size_t cap_entries,
                                  uint64_t* total, uint8_t* flags, uint32_t threads);

#ifdef __cplusplus
}
#endif
#endif /* CILIUM_GPU_H */
