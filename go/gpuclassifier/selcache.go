package gpuclassifier

// #include "cilium_gpu.h"
import "C"

import (
	"fmt"
	"net"
)

// SelectorCache is a selector cache of the engine (cg_selcache_*): the
// identity cache and a rule set's selectors compiled for the bitset kernels.
type SelectorCache struct {
	e  *Engine
	id C.uint32_t
}

// NewSelectorCache creates an empty selector cache.
func (e *Engine) NewSelectorCache() (*SelectorCache, error) {
	var id C.uint32_t
	if err := call(func() C.int { return C.cg_selcache_create(e.h, &id) }); err != nil {
		return nil, err
	}
	return &SelectorCache{e: e, id: id}, nil
}

// Destroy frees the cache's tables.
func (s *SelectorCache) Destroy() error {
	return call(func() C.int { return C.cg_selcache_destroy(s.e.h, s.id) })
}

// SetCIDRIdentities replaces the prefix section: ids[i] is the identity
// AllocateCIDRs (pkg/ipcache/cidr.go:26-86) gave nets[i].  Each behaves in
// every selector as an identity carrying GetCIDRLabels(nets[i]).  The family
// follows the mask's length, so an IPv4-mapped IPv6 prefix stays IPv6.
func (s *SelectorCache) SetCIDRIdentities(ids []uint32, nets []net.IPNet) error {
	if len(ids) != len(nets) {
		return fmt.Errorf("gpuclassifier: %d identities for %d prefixes", len(ids), len(nets))
	}
	if len(ids) == 0 {
		return call(func() C.int { return C.cg_selcache_set_cidr_identities(s.e.h, s.id, nil, nil, 0) })
	}
	recs := make([]C.cg_cidr, len(nets))
	cids := make([]C.uint32_t, len(ids))
	for i, n := range nets {
		ones, bits := n.Mask.Size()
		if bits == 0 {
			return fmt.Errorf("gpuclassifier: prefix %d has a non-contiguous mask", i)
		}
		ip := n.IP
		if bits == 32 {
			ip = ip.To4()
			recs[i].family = 4
		} else {
			ip = ip.To16()
			recs[i].family = 6
		}
		if ip == nil {
			return fmt.Errorf("gpuclassifier: prefix %d: address and mask differ in family", i)
		}
		recs[i].prefixlen = C.uint8_t(ones)
		for k := range ip {
			recs[i].addr[k] = C.uint8_t(ip[k])
		}
		cids[i] = C.uint32_t(ids[i])
	}
	return call(func() C.int {
		return C.cg_selcache_set_cidr_identities(s.e.h, s.id, &cids[0], &recs[0], C.size_t(len(ids)))
	})
}

// Info returns the cache's sizes: identities of both sections, words per
// bitset row, selectors of the rule set, rules.
func (s *SelectorCache) Info() (identities, words, selectors, rules int, err error) {
	var a, b, c, d C.size_t
	err = call(func() C.int { return C.cg_selcache_info(s.e.h, s.id, &a, &b, &c, &d) })
	return int(a), int(b), int(c), int(d), err
}
