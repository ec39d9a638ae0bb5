// kernels_l4_array.hip — L4 verdicts across endpoints: every tuple names its
// endpoint (lxc_id) and is judged by the policy map in that slot of the policy
// program array, as tail_call(skb, &cilium_policy, ep->lxc_id) dispatches into
// the endpoint's own policy program (bpf/lib/l3.h:99,130; bpf_lxc.c:948).
//
// One lane per tuple, grid-stride.  The lane reads its slot word, the member
// map's 32-byte L4Dev record, and then runs l4_walk.h over that map's tables
// with the fingerprints read from global memory (256 maps' fingerprints and
// counters do not fit LDS).  Counters go to the selected map's own array.
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>

#include "../../include/cilium_gpu.h"
#include "dev_types.h"
#include "kernels.h"
#include "l4_walk.h"

namespace cg {

namespace {

constexpr int kArrThreads = 256;

// A member map's record as two 16-byte loads (field order of L4Dev).
__device__ __forceinline__ L4Dev l4_array_rec(const L4ArrDev& A, uint32_t idx) {
  const uint4* p = reinterpret_cast<const uint4*>(A.recs + idx);
  const uint4 a = p[0], b = p[1];
  L4Dev t;
  t.slots = reinterpret_cast<const L4Slot*>(((uint64_t)a.y << 32) | a.x);
  t.fp = reinterpret_cast<const uint32_t*>(((uint64_t)a.w << 32) | a.z);
  t.bucket_mask = b.x;
  t.max_entries = b.y;
  t.counters = reinterpret_cast<unsigned long long*>(((uint64_t)b.w << 32) | b.z);
  return t;
}

// kFam 0: the tuple's own identity; 4 / 6: the ipcache resolution of its
// remote address (addrs: u32 IPv4 / 16-byte IPv6, network order), as
// l4_kernel resolves it.
//
// One code path.  Two additions were built behind a switch, measured and
// taken out again (DESIGN §3.2 has the figures): a wave whose lanes all name
// one slot reading the record through scalar registers (under 1% either way,
// also on runs of one endpoint), and lanes that count on the same entry
// combining before the atomic (15% slower on uniform endpoint ids, 1% slower
// on runs: the rounds cost more than the atomics they save).
template <int kFam>
__global__ __launch_bounds__(kArrThreads) void l4_array_kernel(L4ArrDev A, IpcacheDev ipc,
                                                               const void* __restrict__ addrs,
                                                               const uint16_t* __restrict__ lxc,
                                                               const uint32_t* __restrict__ tuples, size_t n,
                                                               int32_t* __restrict__ out, uint32_t mode) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t sw = A.slot[__builtin_nontemporal_load(lxc + i)];
    if (sw == 0) {  // the tail call missed: no table is read, no counter moves
      __builtin_nontemporal_store((int32_t)CG_DROP_MISSED_TAIL_CALL, out + i);
      continue;
    }
    const L4Dev t = l4_array_rec(A, sw - 1);
    uint32_t w0;
    if (kFam == 4) {
      w0 = (uint32_t)ipc_v4_value(ipc, __builtin_bswap32(reinterpret_cast<const uint32_t*>(addrs)[i]));
    } else if (kFam == 6) {
      const uint4 x = reinterpret_cast<const uint4*>(addrs)[i];
      const uint64_t hi = __builtin_bswap64(((uint64_t)x.y << 32) | x.x);
      const uint64_t lo = __builtin_bswap64(((uint64_t)x.w << 32) | x.z);
      const uint32_t tb = (uint32_t)(hi >> (64 - ipc.v6_bits));
      uint32_t k;
      w0 = (uint32_t)kIpcMiss;
      if (ipc_v6_bucket(ipc.code6[tb >> 5], tb, &k)) {
        const uint4 en = reinterpret_cast<const uint4*>(ipc.ent6)[k];
        const uint4* rec = reinterpret_cast<const uint4*>(ipc.runs6 + 4 * (size_t)en.y);
        w0 = ipc_v6_identity(ipc, hi, lo, en, rec[0], rec[1].x);
      }
    } else {
      w0 = __builtin_nontemporal_load(tuples + i * 3 + 0);
    }
    const uint32_t w1 = l4_mode_word(__builtin_nontemporal_load(tuples + i * 3 + 1), mode);
    const uint32_t len = __builtin_nontemporal_load(tuples + i * 3 + 2);
    uint32_t val = 0;
    const int which = l4_resolve(t, [&](uint32_t b) { return t.fp[b]; }, w0, w1, (w1 >> 24) & CG_L4_F_FRAGMENT, &val);
    __builtin_nontemporal_store(l4_wrap(l4_verdict(which, val, w1 >> 24), mode), out + i);
    if (which) {
      const uint32_t id = val & 0xFFFF;
      atomicAdd(&t.counters[2 * id], 1ULL);
      atomicAdd(&t.counters[2 * id + 1], (unsigned long long)len);
    }
  }
}

int resident_blocks(const void* fn) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, int> cache;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find({fn, dev});
  if (it == cache.end()) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, kArrThreads, 0) != hipSuccess || nb < 1) nb = 1;
    it = cache.emplace(std::make_pair(fn, dev), nb).first;
  }
  return it->second;
}

template <int kFam>
int launch_t(const L4ArrDev& A, const IpcacheDev& ipc, const void* addrs, const uint16_t* lxc, const void* tuples,
             size_t n, int32_t* out, uint32_t mode, void* stream, int cus) {
  // grid-stride over exactly the blocks that are resident at once
  size_t need = (n + kArrThreads - 1) / kArrThreads;
  const size_t cap = (size_t)cus * resident_blocks((const void*)l4_array_kernel<kFam>);
  if (need > cap) need = cap;
  hipLaunchKernelGGL(l4_array_kernel<kFam>, dim3((unsigned)need), dim3(kArrThreads), 0, (hipStream_t)stream, A, ipc,
                     addrs, lxc, (const uint32_t*)tuples, n, out, mode);
  return (int)hipGetLastError();
}

}  // namespace

int launch_l4_array(const L4ArrDev& A, const IpcacheDev& ipc, int family, const void* addrs, const uint16_t* lxc,
                    const void* tuples, size_t n, int32_t* out, uint32_t mode, void* stream, int cus) {
  if (n == 0) return 0;
  if (family == 6) return launch_t<6>(A, ipc, addrs, lxc, tuples, n, out, mode, stream, cus);
  if (family == 4) return launch_t<4>(A, ipc, addrs, lxc, tuples, n, out, mode, stream, cus);
  return launch_t<0>(A, ipc, addrs, lxc, tuples, n, out, mode, stream, cus);
}

}  // namespace cg
