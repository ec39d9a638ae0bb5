package gpuclassifier

// #include "cilium_gpu.h"
import "C"

import "unsafe"

// L4 verdict modes of cg_l4_policy_verdicts_* and cg_l4_array_verdicts_*.
const (
	L4ModeCanAccess  uint32 = 0     // __policy_can_access with the tuple's own flags
	L4ModeIngress    uint32 = 1     // policy_can_access_ingress (policy.h:126-146)
	L4ModeEgress     uint32 = 2     // policy_can_egress (policy.h:150-163)
	L4ModeIgnoreDrop uint32 = 0x100 // a datapath built with IGNORE_DROP
)

// DropMissedTailCall is the verdict of a tuple whose slot is empty
// (DROP_MISSED_TAIL_CALL, bpf/lib/common.h:247).
const DropMissedTailCall int32 = -140

// PolicyArray mirrors the policy program array cilium_policy[lxc_id]
// (bpf/lib/maps.h:44-62): slots that name PolicyMaps, and verdicts for
// tuples that each name their endpoint.
type PolicyArray struct {
	e  *Engine
	id C.uint32_t
}

func (e *Engine) NewPolicyArray() (*PolicyArray, error) {
	var id C.uint32_t
	if err := call(func() C.int { return C.cg_policy_array_create(e.h, &id) }); err != nil {
		return nil, err
	}
	return &PolicyArray{e: e, id: id}, nil
}

func (a *PolicyArray) Destroy() error {
	return call(func() C.int { return C.cg_policy_array_destroy(a.e.h, a.id) })
}

// Set puts pm into slot lxcID (all-or-nothing for the batched C call).
func (a *PolicyArray) Set(lxcID uint16, pm *PolicyMap) error {
	l, m := C.uint16_t(lxcID), pm.id
	return call(func() C.int { return C.cg_policy_array_set(a.e.h, a.id, &l, &m, 1) })
}

// Clear empties slot lxcID: tuples that name it get DropMissedTailCall.
func (a *PolicyArray) Clear(lxcID uint16) error {
	l := C.uint16_t(lxcID)
	return call(func() C.int { return C.cg_policy_array_clear(a.e.h, a.id, &l, 1) })
}

// Get returns the id of the map in slot lxcID, 0 for an empty slot.
func (a *PolicyArray) Get(lxcID uint16) (uint32, error) {
	var m C.uint32_t
	err := call(func() C.int { return C.cg_policy_array_get(a.e.h, a.id, C.uint16_t(lxcID), &m) })
	return uint32(m), err
}

// VerdictsDev judges n device tuples, tuple i by the map in slot lxcIDs[i]
// (device uint16), into device verdicts on a hipStream_t, asynchronously.
func (a *PolicyArray) VerdictsDev(mode uint32, lxcIDs, tuples unsafe.Pointer, n int, verdicts, stream unsafe.Pointer) error {
	return call(func() C.int { return C.cg_l4_array_verdicts_dev(a.e.h, a.id, C.uint32_t(mode), (*C.uint16_t)(lxcIDs),
		(*C.cg_l4_tuple)(tuples), C.size_t(n), (*C.int32_t)(verdicts), stream) })
}

// Verdicts is VerdictsDev from host memory.
func (a *PolicyArray) Verdicts(mode uint32, lxcIDs []uint16, tuples []L4Tuple) ([]int32, error) {
	if len(lxcIDs) != len(tuples) {
		return nil, &Error{Code: InvalidArgument, Msg: "lxc ids and tuples differ in length"}
	}
	out := make([]int32, len(tuples))
	if len(tuples) == 0 {
		return out, nil
	}
	err := call(func() C.int { return C.cg_l4_array_verdicts_host(a.e.h, a.id, C.uint32_t(mode),
		(*C.uint16_t)(unsafe.Pointer(&lxcIDs[0])), (*C.cg_l4_tuple)(unsafe.Pointer(&tuples[0])),
		C.size_t(len(tuples)), (*C.int32_t)(unsafe.Pointer(&out[0]))) })
	return out, err
}
