// frame_progs.h — the programs of the raw-frames route as types: what
// l4_frames_kernel<P> (kernels_l4_frames.hip) runs per lane and the
// cg_diag_l4_frames_*_eval_host evaluators run per frame over host views.
//   Tab     the endpoint table the program takes beside the policy array;
//   kLxc    lxc[i] names the frame's endpoint (else the program finds it);
//   kLabel  labels[i] is the remote identity (else the ipcache resolves it);
//   kRecs   run() fills *rec, a conntrack record per frame;
//   run()   one frame: its verdict, *o and *l4_off as frame_verdict leaves them.
#pragma once

#include <type_traits>

#include "ct_walk.h"
#include "egress_walk.h"
#include "frame_walk.h"

namespace cg {

// The ingress program (frame_walk.h), kCt: with the conntrack lookup (ct_walk.h).
template <bool kEp, bool kIpc, bool kCt>
struct IngressProg {
  using Tab = EpMapDev;
  static constexpr bool kLxc = !kEp, kLabel = !kIpc, kRecs = kCt;
  template <class Ld, class Count>
  static CG_HDI int32_t run(const L4ArrDev& A, const EpMapDev& E, const IpcacheDev& ipc, const CtMapDev& C, Ld ld,
                            uint32_t len, uint32_t lxc, uint32_t label, uint32_t pkt_len, uint32_t mode,
                            cg_l4_frame_info* o, uint32_t* l4_off, CtRecWords* rec, Count count) {
    if constexpr (kCt)
      return frame_ct_verdict<kEp, kIpc>(A, E, ipc, C, ld, len, lxc, label, pkt_len, mode, o, l4_off, rec, count);
    else
      return frame_verdict<kEp, kIpc>(A, E, ipc, ld, len, lxc, label, pkt_len, mode, o, l4_off, count);
  }
};

// The from-container program (egress_walk.h).
template <bool kIpc, bool kCt>
struct EgressProg {
  using Tab = EpHdrDev;
  static constexpr bool kLxc = true, kLabel = !kIpc, kRecs = kCt;
  template <class Ld, class Count>
  static CG_HDI int32_t run(const L4ArrDev& A, const EpHdrDev& H, const IpcacheDev& ipc, const CtMapDev& C, Ld ld,
                            uint32_t len, uint32_t lxc, uint32_t label, uint32_t pkt_len, uint32_t mode,
                            cg_l4_frame_info* o, uint32_t* l4_off, CtRecWords* rec, Count count) {
    return egress_verdict<kIpc, kCt>(A, H, ipc, C, ld, len, lxc, label, pkt_len, mode, o, l4_off, rec, count);
  }
};

// f(std::bool_constant<b>{}...): run-time booleans picked once, on the host, as
// the template arguments of a program.
template <class F>
auto with_bools(F f) {
  return f();
}
template <class F, class... Bs>
auto with_bools(F f, bool b, Bs... rest) {
  return b ? with_bools([&](auto... k) { return f(std::true_type{}, k...); }, rest...)
           : with_bools([&](auto... k) { return f(std::false_type{}, k...); }, rest...);
}

}  // namespace cg
