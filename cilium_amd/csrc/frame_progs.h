// frame_progs.h — the programs of the raw-frames route as types: what
// l4_frames_kernel<P> (kernels_l4_frames.hip) runs per lane and the
// cg_diag_l4_frames_*_eval_host evaluators run per frame over host views.
//   Tab     the endpoint table the program takes beside the policy array;
//   kLxc    lxc[i] names the frame's endpoint (else the program finds it);
//   kLabel  labels[i] is the remote identity (else the ipcache resolves it);
//   kRecs   run() fills *rec, a conntrack record per frame;
//   run()   one frame: its verdict, *o and *l4_off as frame_verdict leaves them;
//   Extra   what a frame reports beside them, and store() that writes it to the
//           table's per-frame arrays (only the program with services has any).
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

// The from-container program over a services map (egress_walk.h, lb_walk.h):
// always with the ipcache and the conntrack map.  Its table carries the
// per-frame arrays the other programs do not have, so run() takes the frame's
// index.
struct EgressSvcProg {
  using Tab = EpHdrSvcDev;
  struct Extra {
    LbXlateWords x;
  };
  static constexpr bool kLxc = true, kLabel = false, kRecs = true;
  // The service record is stored from inside run(), as soon as the service steps are done.
  template <class Ld, class Count>
  static CG_HDI int32_t run(const L4ArrDev& A, const EpHdrSvcDev& T, const IpcacheDev& ipc, const CtMapDev& C, Ld ld,
                            uint32_t len, uint32_t lxc, uint32_t, uint32_t pkt_len, uint32_t mode,
                            cg_l4_frame_info* o, uint32_t* l4_off, CtRecWords* rec, Count count, size_t i,
                            Extra* ex) {
    return egress_svc_verdict(
        A, T.H, T.L, ipc, C, ld, len, lxc, pkt_len, mode, T.hash ? T.hash + i : nullptr, o, l4_off, rec,
        [&](const CtRecWords& r) {
          if (!T.svc_recs) return;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            store16(T.svc_recs + 4 * i + q, make_uint4(r.w[4 * q], r.w[4 * q + 1], r.w[4 * q + 2], r.w[4 * q + 3]));
        },
        &ex->x, count);
  }
  static CG_HDI void store(const EpHdrSvcDev& T, size_t i, const Extra& ex) {
    if (T.xlate) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
        store16(T.xlate + 3 * i + q, make_uint4(ex.x.w[4 * q], ex.x.w[4 * q + 1], ex.x.w[4 * q + 2], ex.x.w[4 * q + 3]));
    }
  }
};
template <class P, class = void>
struct HasExtra : std::false_type {};
template <class P>
struct HasExtra<P, std::void_t<typename P::Extra>> : std::true_type {};

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
