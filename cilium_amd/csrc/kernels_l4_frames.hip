// kernels_l4_frames.hip — L4 verdicts from raw frames: the endpoint's ingress
// policy program from the Ethernet header on (frame_walk.h), per frame of a
// blob, on the policy program array of kernels_l4_array.hip.
//
// One lane per frame, grid-stride.  A lane reads its two offsets (coalesced
// across the wave), then the header fields it needs as aligned 4-byte words
// with the bytes shifted out (frame starts have every alignment), the
// endpoint map and the ipcache as its frame asks, and walks the slot's map as
// l4_array_kernel does.  Counters go to the selected map's own array.
// l4_frames_kernel<P> is that lane for every program of frame_progs.h: the
// ingress program, the same with the conntrack lookup of ct_walk.h between the
// walk and the verdict, and the endpoint's from-container program
// (egress_walk.h), each in its resolver combinations: twelve kernels; and the
// from-container program over a services map (lb_walk.h), the thirteenth.
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>

#include "../../include/cilium_gpu.h"
#include "dev_types.h"
#include "frame_progs.h"
#include "kernels.h"

namespace cg {

namespace {

constexpr int kFrmThreads = 256;

// The four bytes at p, read as the two aligned words that hold them.  [lo, hi)
// is the blob's window: words that lie inside it whole are loaded as words;
// at the window's two edges the bytes are read one by one, and a byte outside
// the window reads as 0 (the walk never uses one: it checks the frame's
// length first, and a frame lies inside the window).
__device__ __forceinline__ uint32_t frame_word(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uint8_t* w = reinterpret_cast<const uint8_t*>(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3) * 8;
  if (w >= lo && w + 8 <= hi) {
    const uint32_t w0 = reinterpret_cast<const uint32_t*>(w)[0];
    if (sh == 0) return w0;
    const uint32_t w1 = reinterpret_cast<const uint32_t*>(w)[1];
    return (w0 >> sh) | (w1 << (32 - sh));
  }
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (p + k >= lo && p + k < hi) v |= (uint32_t)p[k] << (8 * k);
  return v;
}

// P: the program a lane runs (frame_progs.h).  With the conntrack lookup a lane
// also reads its frame's two bucket lines of the conntrack table, both
// requested before either is tested, and a record leaves as four 16-byte
// stores.  The from-container program reads the endpoint's 64-byte header as
// four 16-byte loads (a batch touches few distinct headers: they sit in L2) and
// compares the MACs as the frame's first three words.  A program without
// conntrack ignores C and recs.
template <class P>
__global__ __launch_bounds__(kFrmThreads) void l4_frames_kernel(
    L4ArrDev A, typename P::Tab T, IpcacheDev ipc, CtMapDev C, const uint8_t* __restrict__ raw,
    const uint64_t* __restrict__ off, size_t n, const uint16_t* __restrict__ lxc, const uint32_t* __restrict__ labels,
    const uint32_t* __restrict__ pkt_len, int32_t* __restrict__ out, uint4* __restrict__ info,
    uint4* __restrict__ recs, uint32_t mode) {
  const uint64_t wlo = off[0], whi = off[n];
  const uint8_t* lo = raw + wlo;
  const uint8_t* hi = whi > wlo ? raw + whi : lo;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    uint64_t start;
    const uint32_t len = frame_range(off[i], off[i + 1], wlo, whi, &start);
    const uint8_t* base = raw + start;
    const uint32_t plen = pkt_len ? __builtin_nontemporal_load(pkt_len + i) : len;
    const uint32_t id = P::kLxc ? (uint32_t)__builtin_nontemporal_load(lxc + i) : 0u;
    const uint32_t label = P::kLabel ? __builtin_nontemporal_load(labels + i) : 0u;
    cg_l4_frame_info fi;
    CtRecWords r;
    uint32_t l4_off;
    const auto ld = [&](uint32_t o) { return frame_word(base + o, lo, hi); };
    const auto count = [&](const L4Dev& t, uint32_t entry) {
      atomicAdd(&t.counters[2 * entry], 1ULL);
      atomicAdd(&t.counters[2 * entry + 1], (unsigned long long)plen);
    };
    int32_t v;
    if constexpr (HasExtra<P>::value) {  // the program with services: its own per-frame outputs go out here
      typename P::Extra ex;
      v = P::run(A, T, ipc, C, ld, len, id, label, plen, mode, &fi, &l4_off, &r, count, i, &ex);
      P::store(T, i, ex);
    } else {
      v = P::run(A, T, ipc, C, ld, len, id, label, plen, mode, &fi, &l4_off, &r, count);
    }
    __builtin_nontemporal_store(v, out + i);
    if (info) {
      uint4 q;
      q.x = fi.t.identity;
      q.y = (uint32_t)fi.t.dport | (uint32_t)fi.t.proto << 16 | (uint32_t)fi.t.flags << 24;
      q.z = fi.t.len;
      q.w = (uint32_t)fi.lxc_id | (uint32_t)fi.family << 16;
      info[i] = q;
    }
    if (P::kRecs && recs) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        recs[4 * i + q] = make_uint4(r.w[4 * q], r.w[4 * q + 1], r.w[4 * q + 2], r.w[4 * q + 3]);
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
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, kFrmThreads, 0) != hipSuccess || nb < 1) nb = 1;
    it = cache.emplace(std::make_pair(fn, dev), nb).first;
  }
  return it->second;
}

template <class P>
int launch(const L4ArrDev& A, const typename P::Tab& T, const IpcacheDev* ipc, const CtMapDev* C, const FramesBatch& b,
           void* stream, int cus) {
  if (b.n == 0) return 0;
  // sized as l4_array_kernel: grid-stride over exactly the blocks resident at once
  size_t need = (b.n + kFrmThreads - 1) / kFrmThreads;
  const size_t cap = (size_t)cus * resident_blocks((const void*)l4_frames_kernel<P>);
  if (need > cap) need = cap;
  hipLaunchKernelGGL((l4_frames_kernel<P>), dim3((unsigned)need), dim3(kFrmThreads), 0, (hipStream_t)stream, A, T,
                     ipc ? *ipc : IpcacheDev{}, C ? *C : CtMapDev{}, b.raw, b.off, b.n, b.lxc, b.labels, b.pkt_len,
                     b.out, (uint4*)b.info, (uint4*)b.recs, b.mode);
  return (int)hipGetLastError();
}

}  // namespace

int launch_l4_frames(const L4ArrDev& A, const EpMapDev* E, const IpcacheDev* ipc, const CtMapDev* C,
                     const FramesBatch& b, void* stream, int cus) {
  return with_bools(
      [&](auto kEp, auto kIpc, auto kCt) {
        return launch<IngressProg<kEp, kIpc, kCt>>(A, E ? *E : EpMapDev{}, ipc, C, b, stream, cus);
      },
      E != nullptr, ipc != nullptr, C != nullptr);
}

int launch_l4_frames_egress(const L4ArrDev& A, const EpHdrDev& H, const IpcacheDev* ipc, const CtMapDev* C,
                            const FramesBatch& b, void* stream, int cus) {
  return with_bools([&](auto kIpc, auto kCt) { return launch<EgressProg<kIpc, kCt>>(A, H, ipc, C, b, stream, cus); },
                    ipc != nullptr, C != nullptr);
}

int launch_l4_frames_egress_svc(const L4ArrDev& A, const EpHdrSvcDev& T, const IpcacheDev& ipc, const CtMapDev& C,
                                const FramesBatch& b, void* stream, int cus) {
  return launch<EgressSvcProg>(A, T, &ipc, &C, b, stream, cus);
}

}  // namespace cg
