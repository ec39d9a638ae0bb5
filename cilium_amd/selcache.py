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
* ``expand`` / ``endpoint_policy_map_entries`` / ``sync_policy_maps``: the
  bitsets expanded into raw policy-map entries by three more kernels
  (``cg_selcache_expand_*``, ``cg_selcache_entries_host``) and applied with
  one ``PolicyMap.sync`` per map — no Python object per entry;
* ``endpoint_policy_map_states``: the dicts ``resolve.endpoint_policy_map_state``
  returns, for many endpoints at once;
* ``set_cidr_identities``: CIDR prefixes that are identities (``cidr.py``) as a
  second, native section after the label identities — 24 bytes each instead
  of their ``GetCIDRLabels`` labels — which every result above then covers.

The results are bit-exact with ``resolve.EndpointSelector.matches`` and
``Repository.allows_*_label_access`` / ``get_rules_matching``.  Obtained
through ``Classifier.selector_cache()``.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Mapping, Optional, Sequence

import numpy as np

from . import _native as N
from . import cidr as CIDR
from . import resolve as R
from .classifier import POLICY_KEY_DTYPE
from .policy import PolicyKey, TrafficDirection, htons

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


EXPAND_ROW_DTYPE = np.dtype([("dport", "<u2"), ("protocol", "u1"), ("egress", "u1"), ("proxy_port", "<u2"),
                             ("flags", "<u2")])


class ExpandTable:
    """A cg_expand_table built from rows (dport_be, protocol, egress,
    proxy_port_be, flags, [source row indices]); dport and proxy port in
    network byte order, as the policy map stores them.  Its arrays are kept
    alive by this object."""

    def __init__(self, rows: Sequence[tuple]):
        self.n = len(rows)
        self.rows = np.zeros(max(self.n, 1), EXPAND_ROW_DTYPE)
        for i, r in enumerate(rows):
            self.rows[i] = tuple(r[:5])
        self.src_off, self.src_idx = _csr([list(r[5]) for r in rows])
        self.c = N.ExpandTableC(self.n, _p(self.rows), _p(self.src_off), _p(self.src_idx))

    def ref(self):
        return C.byref(self.c)


class _IdentityView(Mapping):
    """The identity cache of both sections as one read-only mapping: the
    label identities' dicts as given, then each prefix identity's
    cidr_labels(prefix), built when it is asked for (a /128 has 130 labels;
    nothing is materialised for a section that is only iterated by key)."""

    def __init__(self, labels: Mapping[int, Mapping[str, str]], prefixes: Mapping[int, "CIDR.Net"]):
        self._labels, self._prefixes = labels, prefixes

    def __getitem__(self, ident):
        if ident in self._labels:
            return self._labels[ident]
        return CIDR.cidr_labels(self._prefixes[ident])

    def __iter__(self):
        yield from self._labels
        yield from self._prefixes

    def __len__(self):
        return len(self._labels) + len(self._prefixes)

    def __contains__(self, ident):
        return ident in self._labels or ident in self._prefixes


class SelectorCache:
    """The identity cache and a repository's selectors on the device."""

    def __init__(self, cl):
        self.cl = cl
        v = C.c_uint32()
        N.check(N.lib.cg_selcache_create(cl.h, C.byref(v)))
        self.id = v.value
        self.ids = np.zeros(0, np.uint32)       # identity numbers of both sections, in bit order
        self.identity_cache: Mapping[int, Mapping[str, str]] = {}
        self._index: dict[int, int] = {}
        self._label_cache: Mapping[int, Mapping[str, str]] = {}
        self._label_ids = np.zeros(0, np.uint32)
        self._cidr_ids = np.zeros(0, np.uint32)
        self.cidr_identities: dict[int, CIDR.Net] = {}  # the prefix section: {identity: network}
        self.repo: Optional[R.Repository] = None
        self.words = 0
        self._entries_cap = 1 << 16             # entries() starts its buffers here and grows them

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
        self._label_ids, self._label_cache = ids, identity_cache
        self._sections_changed()

    def set_cidr_identities(self, prefixes: Mapping[int, str]) -> None:
        """Replace the prefix section ({numeric identity: "prefix"}, e.g.
        CIDRIdentityAllocator.identities()), all or nothing.  Its bits follow
        the label identities' in the mapping's order; a prefix identity
        behaves in every selector as a label identity carrying
        cidr.cidr_labels(prefix), which is also what identity_cache then
        returns for it."""
        nets = [CIDR.to_net(p) for p in prefixes.values()]
        ids = np.fromiter((int(i) for i in prefixes), np.uint32, len(prefixes))
        recs = CIDR.nets_to_keys(nets)
        N.check(N.lib.cg_selcache_set_cidr_identities(self.cl.h, self.id, _p(ids) if len(ids) else None,
                                                      _p(recs) if len(ids) else None, len(ids)))
        self._cidr_ids = ids
        self.cidr_identities = {int(i): n for i, n in zip(ids, nets)}
        self._sections_changed()

    def _sections_changed(self) -> None:
        self.ids = np.concatenate([self._label_ids, self._cidr_ids])
        self.identity_cache = _IdentityView(self._label_cache, self.cidr_identities) if len(self._cidr_ids) \
            else self._label_cache
        self._index = {int(i): n for n, i in enumerate(self.ids)}
        self.words = (len(self.ids) + 63) // 64

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
        endpoint_ids = [int(e) for e in endpoint_ids]
        for e in endpoint_ids:
            if e in self.cidr_identities and e not in self._label_cache:
                raise ValueError(f"identity {e} is a prefix identity ({self.cidr_identities[e]}), not an endpoint")
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

    # ------------------------------------------------------------ expand --
    def expand_into(self, table: ExpandTable, src: np.ndarray, keys: np.ndarray, proxy_be: np.ndarray,
                    diag_cpu: bool = False, threads: int = 1) -> tuple[np.ndarray, int]:
        """Expand `table`'s rows over the source matrix src[rows][W] (u64, the
        layout of match / reach) into the caller's keys (POLICY_KEY_DTYPE) and
        proxy_be (u16) arrays, whose common length is the capacity.  Returns
        (row_off[R + 1], total); when total exceeds the capacity the arrays
        are left untouched and row_off is still valid.  Row r owns
        [row_off[r], row_off[r+1]), in ascending bit order."""
        src = np.ascontiguousarray(src, np.uint64)
        src_rows = src.shape[0] if src.ndim == 2 else (src.size // self.words if self.words else 0)
        if src.size != src_rows * self.words:
            raise ValueError("src is not rows x W words")
        if keys.dtype != POLICY_KEY_DTYPE or proxy_be.dtype != np.uint16 or len(keys) != len(proxy_be) \
                or not keys.flags.c_contiguous or not proxy_be.flags.c_contiguous:
            raise ValueError("keys / proxy_be: contiguous POLICY_KEY_DTYPE and uint16 arrays of one length")
        row_off = np.zeros(table.n + 1, np.uint64)
        total = C.c_uint64()
        cap = len(keys)
        args = (self.cl.h, self.id, table.ref(), _p(src) if src.size else None, src_rows, _p(row_off),
                _p(keys) if cap else None, _p(proxy_be) if cap else None, cap, C.byref(total))
        if diag_cpu:
            N.check(N.lib.cg_diag_selcache_expand_host(*args, threads))
        else:
            N.check(N.lib.cg_selcache_expand_host(*args))
        return row_off, int(total.value)

    def expand(self, table: ExpandTable, src: np.ndarray, diag_cpu: bool = False, threads: int = 1):
        """(row_off, keys, proxy_be) of expand_into, sized by a first call
        with no capacity."""
        none = (np.zeros(0, POLICY_KEY_DTYPE), np.zeros(0, np.uint16))
        row_off, total = self.expand_into(table, src, *none, diag_cpu=diag_cpu, threads=threads)
        if total == 0:
            return (row_off, *none)
        keys, proxy = np.zeros(total, POLICY_KEY_DTYPE), np.zeros(total, np.uint16)
        row_off, _ = self.expand_into(table, src, keys, proxy, diag_cpu=diag_cpu, threads=threads)
        return row_off, keys, proxy

    def expand_dev(self, table: ExpandTable, d_src, src_rows: int, d_row_off, d_keys, d_proxy, cap_entries: int,
                   d_total=None, stream=None) -> None:
        """expand_into() on device tensors, on `stream`: d_src src_rows * W
        words, d_row_off R + 1 words, d_keys cap_entries 8-byte keys, d_proxy
        cap_entries u16, d_total one word (or None).  The table is a host
        table."""
        N.check(N.lib.cg_selcache_expand_dev(self.cl.h, self.id, table.ref(), _p(d_src), src_rows, _p(d_row_off),
                                             _p(d_keys), _p(d_proxy), cap_entries, _p(d_total), stream))

    def entries(self, selectors: Optional[Sequence[R.EndpointSelector]], eps: np.ndarray, table: ExpandTable,
                diag_cpu: bool = False, threads: int = 1):
        """The fused call (cg_selcache_entries_host): `table`'s rows over the
        source matrix [selectors' match rows | eps' ingress reach rows | eps'
        egress reach rows].  Returns (row_off, keys, proxy_be, flags).  The
        entry buffers start at the last call's size and the call is repeated
        once when the result does not fit."""
        eps = np.ascontiguousarray(eps, np.uint32).reshape(-1)
        tab = _SelectorTable(selectors) if selectors else None
        row_off = np.zeros(table.n + 1, np.uint64)
        flags = np.zeros(max(len(eps), 1), np.uint8)
        total = C.c_uint64()
        cap = self._entries_cap
        while True:
            keys, proxy = np.zeros(max(cap, 1), POLICY_KEY_DTYPE), np.zeros(max(cap, 1), np.uint16)
            args = (self.cl.h, self.id, None if tab is None else tab.ref(), _p(eps) if len(eps) else None, len(eps),
                    table.ref(), _p(row_off), _p(keys), _p(proxy), cap, C.byref(total), _p(flags))
            if diag_cpu:
                N.check(N.lib.cg_diag_selcache_entries_host(*args, threads))
            else:
                N.check(N.lib.cg_selcache_entries_host(*args))
            if total.value <= cap:
                break
            cap = int(total.value)
        self._entries_cap = max(self._entries_cap, cap)
        return row_off, keys[:total.value], proxy[:total.value], flags[:len(eps)]

    # -------------------------------------------------- endpoint policy --
    def endpoint_policy_map_entries(self, endpoint_ids: Iterable[int],
                                    redirect_ports: Optional[Mapping[tuple, int]] = None,
                                    diag_cpu: bool = False, threads: int = 1) -> list[tuple[np.ndarray, np.ndarray]]:
        """Per endpoint identity the raw policy-map entries (keys:
        POLICY_KEY_DTYPE, proxy_be: uint16; network byte order) of
        resolve.endpoint_policy_map_state, without a Python object per entry.
        Each L4 filter is one expansion row over its selectors and each
        direction one L3 row — the endpoint's reach row, or every identity
        when the direction is not enforced (policy.go:144-193, :298-371) — and
        all endpoints' rows go through one fused library call.  L4 resolution
        and ComputePolicyEnforcement stay in resolve.py (per endpoint, they
        do not scale with the identity count); the library's enforcement
        flags are checked against that decision.  The localhost / world keys
        (policy.go:267-296) are appended on the host and may repeat an L3
        key; PolicyMap.sync takes the last."""
        repo = self.repo
        if repo is None:
            raise ValueError("set_repository first")
        endpoint_ids = [int(e) for e in endpoint_ids]
        eps = self._endpoint_indices(endpoint_ids)
        redirect_ports = redirect_ports or {}
        sel_index: dict[R.EndpointSelector, int] = {}
        per_ep = []
        for e in endpoint_ids:
            labels = self.identity_cache[e]
            ing_on, eg_on = R.compute_policy_enforcement(repo, labels)
            l4 = R.L4Policy(Ingress=repo.resolve_l4_ingress_policy(labels) if ing_on else {},
                            Egress=repo.resolve_l4_egress_policy(labels) if eg_on else {})
            l4_rows = []
            # computeDesiredL4PolicyMapEntries (policy.go:144-193)
            for filters, direction in ((l4.Ingress, TrafficDirection.Ingress), (l4.Egress, TrafficDirection.Egress)):
                for f in filters.values():
                    proxy = 0
                    if f.is_redirect():
                        proxy = int(redirect_ports.get((f.Ingress, f.Protocol, f.Port), 0))
                        if proxy == 0:
                            continue
                    l4_rows.append((htons(f.Port & 0xFFFF), f.U8Proto, int(direction), htons(proxy), 0,
                                    [sel_index.setdefault(s, len(sel_index)) for s in f.Endpoints]))
            extra: dict[PolicyKey, int] = {}
            R.determine_allow_localhost(extra, l4, repo.cfg.always_allow_localhost)
            R.determine_allow_from_world(extra, repo.cfg.host_allows_world)
            per_ep.append((ing_on, eg_on, l4_rows, extra))
        S, E = len(sel_index), len(endpoint_ids)
        rows, first = [], [0]
        for n, (ing_on, eg_on, l4_rows, _) in enumerate(per_ep):
            rows += l4_rows
            rows.append((0, 0, int(TrafficDirection.Ingress), 0, 0, [S + n]) if ing_on
                        else (0, 0, int(TrafficDirection.Ingress), 0, N.CG_EXP_ALL, []))
            rows.append((0, 0, int(TrafficDirection.Egress), 0, 0, [S + E + n]) if eg_on
                        else (0, 0, int(TrafficDirection.Egress), 0, N.CG_EXP_ALL, []))
            first.append(len(rows))
        row_off, keys, proxy, flags = self.entries(list(sel_index), eps, ExpandTable(rows), diag_cpu, threads)
        if repo.cfg.enforcement == "default":
            for e, fl, (ing_on, eg_on, _, _) in zip(endpoint_ids, flags, per_ep):
                if "reserved:init" not in self.identity_cache[e] and (bool(fl & 1), bool(fl & 2)) != (ing_on, eg_on):
                    raise RuntimeError(f"endpoint {e}: the library's enforcement flags {int(fl)} disagree with "
                                       "resolve.compute_policy_enforcement")
        out = []
        for n, (_, _, _, extra) in enumerate(per_ep):
            lo, hi = int(row_off[first[n]]), int(row_off[first[n + 1]])
            k, p = keys[lo:hi], proxy[lo:hi]
            if extra:
                xk = np.zeros(len(extra), POLICY_KEY_DTYPE)
                for i, key in enumerate(extra):
                    xk[i] = (key.Identity, htons(key.DestPort), key.Nexthdr, key.TrafficDirection)
                k = np.concatenate([k, xk])
                p = np.concatenate([p, np.asarray([htons(v) for v in extra.values()], np.uint16)])
            out.append((k, p))
        return out

    def sync_policy_maps(self, endpoint_ids: Iterable[int], maps: Sequence,
                         redirect_ports: Optional[Mapping[tuple, int]] = None) -> list[tuple[int, int]]:
        """Bring maps[i] (a PolicyMap) to endpoint i's desired state: one
        fused expansion for all endpoints, then one PolicyMap.sync per map.
        Returns the (added, deleted) counts per map."""
        endpoint_ids = list(endpoint_ids)
        if len(maps) != len(endpoint_ids):
            raise ValueError("one map per endpoint")
        ents = self.endpoint_policy_map_entries(endpoint_ids, redirect_ports)
        return [pm.sync(k, p) for pm, (k, p) in zip(maps, ents)]

    def sync_policy_array(self, endpoint_ids: Iterable[int], lxc_ids: Iterable[int], array,
                          redirect_ports: Optional[Mapping[tuple, int]] = None,
                          diag_cpu: bool = False) -> list[tuple[int, int]]:
        """sync_policy_maps over the maps in slots lxc_ids[i] of `array` (a
        PolicyArray): endpoint i's desired state goes into the map its slot
        names; an empty slot gets a fresh PolicyMap, set into the slot.
        Returns the (added, deleted) counts per endpoint.  diag_cpu: the
        entries come from the host evaluator (diagnostics, no GPU needed)."""
        from .classifier import PolicyMap
        endpoint_ids, lxc_ids = list(endpoint_ids), [int(x) for x in lxc_ids]
        if len(lxc_ids) != len(endpoint_ids):
            raise ValueError("one lxc_id per endpoint")
        maps = []
        for lxc in lxc_ids:
            map_id = array.get(lxc)
            if map_id is None:
                maps.append(PolicyMap(self.cl))
                array.set(lxc, maps[-1])
            else:
                maps.append(PolicyMap.attach(self.cl, map_id))
        if not diag_cpu:
            return self.sync_policy_maps(endpoint_ids, maps, redirect_ports)
        ents = self.endpoint_policy_map_entries(endpoint_ids, redirect_ports, diag_cpu=True)
        return [pm.sync(k, p) for pm, (k, p) in zip(maps, ents)]

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
