"""SelectorCache: label selectors and L3 reachability resolved on the GPU.

The control-plane step ``resolve.py`` restates from the reference —
``get_security_identities`` (pkg/endpoint/policy.go:93-106) per selector and
``allows_{ingress,egress}_label_access`` per identity and direction
(computeDesiredL3PolicyMapEntries, policy.go:298-371) — as two bitset
kernels over the whole identity cache:

* ``identities_of(selectors)``: the selector × identity match matrix, one
  launch for all selectors (``cg_selcache_match_*``);
* ``reach(endpoint_ids)``: per endpoint the ingress / egress allow-bitsets
  over all identities and the enforcement flags (``cg_selcache_reach_*``);
* ``endpoint_policy_map_states``: the dicts ``resolve.endpoint_policy_map_state``
  returns, for many endpoints at once.

The results are bit-exact with ``resolve.EndpointSelector.matches`` and
``Repository.allows_*_label_access`` / ``get_rules_matching``.  Obtained
through ``Classifier.selector_cache()``.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Mapping, Optional, Sequence

import numpy as np

from . import _native as N
from . import resolve as R
from .policy import PolicyKey, TrafficDirection

_OPS = {"In": N.CG_SEL_IN, "NotIn": N.CG_SEL_NOT_IN, "Exists": N.CG_SEL_EXISTS,
        "DoesNotExist": N.CG_SEL_DOES_NOT_EXIST}
_OP_UNKNOWN = 0xFF  # handed to the library, which refuses it (CG_POLICY_REJECTED)


def _p(a):
    return N.ptr(a)


def _strings(strs: list[str]) -> tuple[np.ndarray, np.ndarray]:
    """blob + (n + 1) u64 offsets of the UTF-8 strings."""
    enc = [s.encode("utf-8", "surrogateescape") for s in strs]
    off = np.zeros(len(enc) + 1, np.uint64)
    if enc:
        off[1:] = np.cumsum(np.fromiter(map(len, enc), np.uint64, len(enc)))
    blob = np.frombuffer(b"".join(enc) or b"\0", np.uint8)
    return blob, off


class _SelectorTable:
    """A cg_selector_table built from EndpointSelectors (its arrays are kept
    alive by this object)."""

    def __init__(self, selectors: Sequence[R.EndpointSelector]):
        req_off, ops, keys, val_off, vals = [0], [], [], [0], []
        for sel in selectors:
            for k, v in sel.match_labels:
                ops.append(N.CG_SEL_MATCH_LABEL)
                keys.append(k)
                vals.append(v)
                val_off.append(len(vals))
            for k, op, vs in sel.match_expressions:
                ops.append(_OPS.get(op, _OP_UNKNOWN))
                keys.append(k)
                vals.extend(vs)
                val_off.append(len(vals))
            req_off.append(len(ops))
        self.n = len(selectors)
        self.req_off = np.asarray(req_off, np.uint32)
        self.ops = np.asarray(ops or [0], np.uint8)
        self.key_blob, self.key_off = _strings(keys)
        self.val_off = np.asarray(val_off, np.uint32)
        self.val_blob, self.val_str_off = _strings(vals)
        self.c = N.SelectorTableC(self.n, _p(self.req_off), _p(self.ops), _p(self.key_blob), _p(self.key_off),
                                  _p(self.val_off), _p(self.val_blob), _p(self.val_str_off))

    def ref(self):
        return C.byref(self.c)


def _csr(lists: list[list[int]]) -> tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(lists) + 1, np.uint32)
    if lists:
        off[1:] = np.cumsum([len(x) for x in lists])
    flat = [i for x in lists for i in x]
    return off, np.asarray(flat or [0], np.uint32)


def unpack_rows(bits: np.ndarray, n: int) -> np.ndarray:
    """bits[rows][W] u64 → bool[rows][n] (bit i of word w = column 64*w + i)."""
    bits = np.ascontiguousarray(bits, "<u8")
    rows = bits.shape[0]
    if rows == 0 or n == 0:
        return np.zeros((rows, n), bool)
    return np.unpackbits(bits.view(np.uint8).reshape(rows, -1), axis=1, bitorder="little")[:, :n].astype(bool)


class SelectorCache:
    """The identity cache and a repository's selectors on the device."""

    def __init__(self, cl):
        self.cl = cl
        v = C.c_uint32()
        N.check(N.lib.cg_selcache_create(cl.h, C.byref(v)))
        self.id = v.value
        self.ids = np.zeros(0, np.uint32)       # identity numbers, in bit order
        self.identity_cache: Mapping[int, Mapping[str, str]] = {}
        self._index: dict[int, int] = {}
        self.repo: Optional[R.Repository] = None
        self.words = 0

    def destroy(self) -> None:
        N.check(N.lib.cg_selcache_destroy(self.cl.h, self.id))

    # ------------------------------------------------------------ tables --
    def set_identities(self, identity_cache: Mapping[int, Mapping[str, str]]) -> None:
        """Replace the identity cache ({numeric identity: {"source:key": value}},
        as resolve.py takes it).  Bit i of every result is the i-th identity
        in the mapping's order."""
        ids = np.fromiter((int(i) for i in identity_cache), np.uint32, len(identity_cache))
        lab_off = np.zeros(len(ids) + 1, np.uint32)
        keys: list[str] = []
        vals: list[str] = []
        for n, lbls in enumerate(identity_cache.values()):
            keys.extend(lbls.keys())
            vals.extend(lbls.values())
            lab_off[n + 1] = len(keys)
        kb, ko = _strings(keys)
        vb, vo = _strings(vals)
        N.check(N.lib.cg_selcache_set_identities(self.cl.h, self.id, _p(ids) if len(ids) else None, len(ids),
                                                 _p(lab_off), _p(kb), _p(ko), _p(vb), _p(vo)))
        self.ids = ids
        self.identity_cache = identity_cache
        self._index = {int(i): n for n, i in enumerate(ids)}
        self.words = (len(ids) + 63) // 64

    @staticmethod
    def compile_repository(repo: R.Repository):
        """The repository as index arrays over its distinct selectors:
        (selectors, subject, dir_flags, [ingress, egress] require lists,
        [ingress, egress] allow lists).  A rule's require list holds the
        FromRequires / ToRequires of all its direction rules; its allow list
        the source / destination selectors (entities included) of the
        direction rules without ToPorts (rule.go:352-440)."""
        index: dict[R.EndpointSelector, int] = {}

        def ix(sel):
            return index.setdefault(sel, len(index))
        subject, flags = [], []
        req: list[list[list[int]]] = [[], []]
        allow: list[list[list[int]]] = [[], []]
        for r in repo.rules:
            subject.append(ix(r.EndpointSelector))
            flags.append((1 if r.Ingress else 0) | (2 if r.Egress else 0))
            for d, dir_rules in enumerate((r.Ingress, r.Egress)):
                rq, al = [], []
                for dr in dir_rules:
                    rq += [ix(s) for s in (dr.FromRequires if d == 0 else dr.ToRequires)]
                    if not dr.ToPorts:
                        al += [ix(s) for s in (dr.source_selectors() if d == 0 else dr.destination_selectors())]
                req[d].append(rq)
                allow[d].append(al)
        return list(index), subject, flags, req, allow

    def set_repository(self, repo: R.Repository) -> None:
        """Replace the rule set with `repo`'s rules (all or nothing)."""
        sels, subject, flags, req, allow = self.compile_repository(repo)
        tab = _SelectorTable(sels)
        subj = np.asarray(subject or [0], np.uint32)
        fl = np.asarray(flags or [0], np.uint8)
        keep = [_csr(req[0]), _csr(req[1]), _csr(allow[0]), _csr(allow[1])]
        two = C.c_void_p * 2
        rules = N.SelcacheRulesC(len(subject), _p(subj), _p(fl),
                                 two(_p(keep[0][0]), _p(keep[1][0])), two(_p(keep[0][1]), _p(keep[1][1])),
                                 two(_p(keep[2][0]), _p(keep[3][0])), two(_p(keep[2][1]), _p(keep[3][1])))
        N.check(N.lib.cg_selcache_set_rules(self.cl.h, self.id, tab.ref(), C.byref(rules)))
        self.repo = repo

    def info(self) -> dict:
        v = [C.c_size_t() for _ in range(4)]
        N.check(N.lib.cg_selcache_info(self.cl.h, self.id, *map(C.byref, v)))
        return dict(zip(("identities", "words", "selectors", "rules"), (x.value for x in v)))

    # ------------------------------------------------------------- match --
    def match(self, selectors: Optional[Sequence[R.EndpointSelector]] = None, diag_cpu: bool = False,
              threads: int = 1) -> np.ndarray:
        """bits[S][W] (u64) of `selectors` (None: the repository's), from one
        kernel launch; diag_cpu: the library's host walker instead."""
        tab = None if selectors is None else _SelectorTable(selectors)
        S = self.info()["selectors"] if tab is None else tab.n
        bits = np.zeros((S, self.words), np.uint64)
        out = np.zeros(max(bits.size, 1), np.uint64)
        ref = None if tab is None else tab.ref()
        if diag_cpu:
            N.check(N.lib.cg_diag_selcache_match_host(self.cl.h, self.id, ref, _p(out), bits.size, threads))
        else:
            N.check(N.lib.cg_selcache_match_host(self.cl.h, self.id, ref, _p(out), bits.size))
        bits[...] = out[:bits.size].reshape(bits.shape)
        return bits

    def match_dev(self, selectors: Optional[Sequence[R.EndpointSelector]], d_bits, stream=None) -> None:
        """match() into a device tensor of S * W int64/uint64 words, on `stream`."""
        tab = None if selectors is None else _SelectorTable(selectors)
        N.check(N.lib.cg_selcache_match_dev(self.cl.h, self.id, None if tab is None else tab.ref(), _p(d_bits),
                                            d_bits.numel(), stream))

    def identities_of(self, selectors: Iterable[R.EndpointSelector], diag_cpu: bool = False) -> list[list[int]]:
        """Per selector the sorted identities it selects — each list equals
        resolve.get_security_identities for that selector."""
        selectors = list(selectors)
        distinct = list(dict.fromkeys(selectors))
        rows = unpack_rows(self.match(distinct, diag_cpu=diag_cpu), len(self.ids))
        by_sel = {s: sorted(int(i) for i in self.ids[row]) for s, row in zip(distinct, rows)}
        return [list(by_sel[s]) for s in selectors]

    # ------------------------------------------------------------- reach --
    def _endpoint_indices(self, endpoint_ids: Iterable[int]) -> np.ndarray:
        try:
            return np.asarray([self._index[int(e)] for e in endpoint_ids], np.uint32)
        except KeyError as ex:
            raise KeyError(f"endpoint identity {ex.args[0]} is not in the identity cache") from None

    def reach_indices(self, eps: np.ndarray, diag_cpu: bool = False, threads: int = 1):
        """reach() for endpoints given as indices into the identity table."""
        eps = np.ascontiguousarray(eps, np.uint32).reshape(-1)
        E, W = len(eps), self.words
        ing = np.zeros(max(E * W, 1), np.uint64)
        eg = np.zeros(max(E * W, 1), np.uint64)
        fl = np.zeros(max(E, 1), np.uint8)
        e_ptr = _p(eps) if E else None
        if diag_cpu:
            N.check(N.lib.cg_diag_selcache_reach_host(self.cl.h, self.id, e_ptr, E, _p(ing), _p(eg), _p(fl), threads))
        else:
            N.check(N.lib.cg_selcache_reach_host(self.cl.h, self.id, e_ptr, E, _p(ing), _p(eg), _p(fl)))
        return ing[:E * W].reshape(E, W), eg[:E * W].reshape(E, W), fl[:E]

    def reach(self, endpoint_ids: Iterable[int], diag_cpu: bool = False):
        """(ing[E][W], eg[E][W], flags[E]) for the endpoints' identities: bit i
        of ing[e] says endpoint e accepts the i-th identity at L3
        (allows_ingress_label_access(peer, endpoint)), of eg[e] that it may
        reach it (allows_egress_label_access(endpoint, peer)); flags bit 0 /
        1: some rule selecting the endpoint has ingress / egress rules."""
        return self.reach_indices(self._endpoint_indices(endpoint_ids), diag_cpu)

    def reach_dev(self, d_endpoints, n: int, d_ing, d_eg, d_flags, stream=None) -> None:
        """reach_indices() on device tensors (u32 indices; n * W words each;
        n bytes of flags), on `stream`."""
        N.check(N.lib.cg_selcache_reach_dev(self.cl.h, self.id, _p(d_endpoints), n, _p(d_ing), _p(d_eg),
                                            _p(d_flags), stream))

    # -------------------------------------------------- endpoint policy --
    def endpoint_policy_map_states(self, endpoint_ids: Iterable[int],
                                   redirect_ports: Optional[Mapping[tuple, int]] = None,
                                   diag_cpu: bool = False) -> list[dict]:
        """resolve.endpoint_policy_map_state for each endpoint identity, with
        the identity expansion of all endpoints' L4 filter selectors done by
        one identities_of call and the L3 entries and enforcement flags taken
        from reach().  L4 resolution and merging stay in resolve.py."""
        repo = self.repo
        if repo is None:
            raise ValueError("set_repository first")
        endpoint_ids = [int(e) for e in endpoint_ids]
        redirect_ports = redirect_ports or {}
        ing_bits, eg_bits, flags = self.reach(endpoint_ids, diag_cpu)
        ing_rows = unpack_rows(ing_bits, len(self.ids))
        eg_rows = unpack_rows(eg_bits, len(self.ids))
        mode = repo.cfg.enforcement
        policies = []
        for e, fl in zip(endpoint_ids, flags):
            labels = self.identity_cache[e]
            # ComputePolicyEnforcement (pkg/endpoint/policy.go:616-639)
            if mode == "always":
                ing_on = eg_on = True
            elif mode == "default":
                if "reserved:init" in labels:
                    ing_on = eg_on = True
                else:
                    ing_on, eg_on = bool(fl & 1), bool(fl & 2)
            else:
                ing_on = eg_on = False
            policies.append((ing_on, eg_on,
                             R.L4Policy(Ingress=repo.resolve_l4_ingress_policy(labels) if ing_on else {},
                                        Egress=repo.resolve_l4_egress_policy(labels) if eg_on else {})))
        wanted = dict.fromkeys(sel for _, _, l4 in policies for fm in (l4.Ingress, l4.Egress)
                               for f in fm.values() for sel in f.Endpoints)
        selected = dict(zip(wanted, self.identities_of(wanted, diag_cpu))) if wanted else {}
        out = []
        ids = [int(i) for i in self.ids]
        for n, (ing_on, eg_on, l4) in enumerate(policies):
            desired: dict[PolicyKey, int] = {}
            # computeDesiredL4PolicyMapEntries (policy.go:144-193)
            for filters, direction in ((l4.Ingress, TrafficDirection.Ingress), (l4.Egress, TrafficDirection.Egress)):
                for f in filters.values():
                    proxy = 0
                    if f.is_redirect():
                        proxy = int(redirect_ports.get((f.Ingress, f.Protocol, f.Port), 0))
                        if proxy == 0:
                            continue
                    for sel in f.Endpoints:
                        for ident in selected[sel]:
                            desired[PolicyKey(ident, f.Port & 0xFFFF, f.U8Proto, int(direction))] = proxy
            R.determine_allow_localhost(desired, l4, repo.cfg.always_allow_localhost)
            R.determine_allow_from_world(desired, repo.cfg.host_allows_world)
            ing_row = ing_rows[n] if ing_on else None
            eg_row = eg_rows[n] if eg_on else None
            for k, ident in enumerate(ids):
                if ing_row is None or ing_row[k]:
                    desired[PolicyKey(ident, 0, 0, int(TrafficDirection.Ingress))] = 0
                if eg_row is None or eg_row[k]:
                    desired[PolicyKey(ident, 0, 0, int(TrafficDirection.Egress))] = 0
            out.append(desired)
        return out
