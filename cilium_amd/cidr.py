"""CIDR policy on the host: the reference's prefix handling restated.

* ``parse_ip`` / ``parse_cidr_go`` / ``ip_string``: Go's ``net.ParseIP``,
  ``net.ParseCIDR`` and ``net.IP.String`` as the reference's Go had them (an
  IPv4 field may carry leading zeros, which Go refused only from 1.17 on).
* ``cidr_sanitize`` / ``cidr_rule_sanitize``: ``CIDR.sanitize`` and
  ``CIDRRule.sanitize`` (pkg/policy/api/rule_validation.go:360-425);
  ``MAX_CIDR_PREFIX_LENGTHS`` is ``MaxCIDRPrefixLengths``.
* ``remove_cidrs`` / ``compute_resultant_cidr_set``: ``RemoveCIDRs`` with
  ``removeCIDR`` (pkg/ip/ip.go:119-259) and ``ComputeResultantCIDRSet``
  (pkg/policy/api/cidr.go:115-132), output order kept.
* ``get_cidr_prefixes``: ``GetCIDRPrefixes`` (pkg/policy/cidr.go:24-70).
* ``ip_string_to_label`` / ``cidr_labels``: ``IPStringToLabel`` /
  ``maskedIPToLabelString`` (pkg/labels/cidr.go:23-81) and ``GetCIDRLabels``
  (pkg/labels/cidr/cidr.go:32-50).
* ``cidr_slice_selectors`` / ``cidr_rule_slice_selectors``:
  ``CIDRSlice.GetAsEndpointSelectors`` / ``CIDRRuleSlice.GetAsEndpointSelectors``
  (pkg/policy/api/cidr.go:70-104), as (matchLabels dicts).
* ``CIDRIdentityAllocator``: ``AllocateCIDRs`` / ``ReleaseCIDRs``
  (pkg/ipcache/cidr.go:26-86, pkg/identity/cidr/identity.go:39-98).

A network is a ``Net``: the masked address as Go holds it (4 bytes for a
prefix written dotted, 16 otherwise) and the ones of its mask.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Iterable, Mapping, Optional, Sequence

MAX_CIDR_PREFIX_LENGTHS = 40  # api.MaxCIDRPrefixLengths (rule_validation.go:28-32)
CIDR_MATCH_ALL = ("0.0.0.0/0", "::/0")  # api.CIDRMatchAll
LABEL_WORLD = "reserved:world"
RESERVED_WORLD = 2  # identity.ReservedIdentityWorld
_V4_IN_V6 = bytes(10) + b"\xff\xff"


# ---------------------------------------------------------------- net text --
def _dtoi(s: str) -> tuple[int, int, bool]:
    """net.dtoi: (value, digits consumed, ok); ok is False without a digit or
    past 0xFFFFFF."""
    n = i = 0
    while i < len(s) and "0" <= s[i] <= "9":
        n = n * 10 + ord(s[i]) - 48
        if n >= 0xFFFFFF:
            return 0xFFFFFF, i, False
        i += 1
    if i == 0:
        return 0, 0, False
    return n, i, True


def _xtoi(s: str) -> tuple[int, int, bool]:
    n = i = 0
    while i < len(s):
        c = s[i]
        if "0" <= c <= "9":
            d = ord(c) - 48
        elif "a" <= c <= "f":
            d = ord(c) - 87
        elif "A" <= c <= "F":
            d = ord(c) - 55
        else:
            break
        n = n * 16 + d
        if n >= 0xFFFFFF:
            return 0, i, False
        i += 1
    if i == 0:
        return 0, i, False
    return n, i, True


def _parse_ipv4(s: str) -> Optional[bytes]:
    """net.parseIPv4: four decimal fields of at most 255 (4 bytes here; Go
    returns the 16-byte mapped form, which To4 turns back)."""
    out = bytearray(4)
    for i in range(4):
        if not s:
            return None
        if i > 0:
            if s[0] != ".":
                return None
            s = s[1:]
        n, c, ok = _dtoi(s)
        if not ok or n > 0xFF:
            return None
        s = s[c:]
        out[i] = n
    return None if s else bytes(out)


def _parse_ipv6(s: str) -> Optional[bytes]:
    """net.parseIPv6 without a zone."""
    ip = bytearray(16)
    ellipsis = -1
    if len(s) >= 2 and s[0] == ":" and s[1] == ":":
        ellipsis = 0
        s = s[2:]
        if not s:
            return bytes(ip)
    i = 0
    while i < 16:
        n, c, ok = _xtoi(s)
        if not ok or n > 0xFFFF:
            return None
        if c < len(s) and s[c] == ".":
            if ellipsis < 0 and i != 12:
                return None
            if i + 4 > 16:
                return None
            ip4 = _parse_ipv4(s)
            if ip4 is None:
                return None
            ip[i:i + 4] = ip4
            s = ""
            i += 4
            break
        ip[i] = n >> 8
        ip[i + 1] = n & 0xFF
        i += 2
        s = s[c:]
        if not s:
            break
        if s[0] != ":" or len(s) == 1:
            return None
        s = s[1:]
        if s[0] == ":":
            if ellipsis >= 0:
                return None
            ellipsis = i
            s = s[1:]
            if not s:
                break
    if s:
        return None
    if i < 16:
        if ellipsis < 0:
            return None
        n = 16 - i
        for j in range(i - 1, ellipsis - 1, -1):
            ip[j + n] = ip[j]
        for j in range(ellipsis + n - 1, ellipsis - 1, -1):
            ip[j] = 0
    elif ellipsis >= 0:
        return None
    return bytes(ip)


def parse_ip(s: str) -> Optional[bytes]:
    """net.ParseIP: 16 bytes (an IPv4 address in its mapped form), or None."""
    for c in s:
        if c == ".":
            v4 = _parse_ipv4(s)
            return None if v4 is None else _V4_IN_V6 + v4
        if c == ":":
            return _parse_ipv6(s)
    return None


def to4(ip: bytes) -> Optional[bytes]:
    """net.IP.To4."""
    if len(ip) == 4:
        return ip
    if len(ip) == 16 and ip[:12] == _V4_IN_V6:
        return ip[12:]
    return None


def ip_string(ip: bytes) -> str:
    """net.IP.String: an address To4 accepts prints dotted; otherwise
    lower-case hex groups with the first longest run of two or more zero
    groups as "::"."""
    p4 = to4(ip)
    if p4 is not None:
        return ".".join(str(b) for b in p4)
    e0 = e1 = -1
    i = 0
    while i < 16:
        j = i
        while j < 16 and ip[j] == 0 and ip[j + 1] == 0:
            j += 2
        if j > i and j - i > e1 - e0:
            e0, e1 = i, j
            i = j
        i += 2
    if e1 - e0 <= 2:
        e0 = e1 = -1
    out = []
    i = 0
    while i < 16:
        if i == e0:
            out.append("::")
            i = e1
            if i >= 16:
                break
        elif i > 0:
            out.append(":")
        out.append("%x" % ((ip[i] << 8) | ip[i + 1]))
        i += 2
    return "".join(out)


def cidr_mask(ones: int, bits: int) -> bytes:
    """net.CIDRMask."""
    return (((1 << ones) - 1) << (bits - ones)).to_bytes(bits // 8, "big")


def _mask(ip: bytes, mask: bytes) -> bytes:
    return bytes(a & m for a, m in zip(ip, mask))


@dataclass(frozen=True)
class Net:
    """net.IPNet with a contiguous mask: the masked address (4 or 16 bytes)
    and the mask's ones."""
    ip: bytes
    ones: int

    @property
    def bits(self) -> int:
        return 8 * len(self.ip)

    @property
    def family(self) -> int:
        return 4 if len(self.ip) == 4 else 6

    def contains(self, ip: bytes) -> bool:
        """net.IPNet.Contains: a 16-byte address To4 accepts is compared as
        IPv4; lengths must then agree."""
        mask = cidr_mask(self.ones, self.bits)
        nn = to4(self.ip)
        if nn is None:
            nn = self.ip
        elif len(mask) == 16:  # networkNumberAndMask: a mapped network is compared as IPv4
            mask = mask[12:]
        x = to4(ip)
        if x is not None:
            ip = x
        if len(ip) != len(nn):
            return False
        return _mask(ip, mask) == _mask(nn, mask)

    def __str__(self) -> str:
        """net.IPNet.String."""
        return f"{ip_string(self.ip)}/{self.ones}"

    def text(self) -> str:
        """A string net.ParseCIDR reads back as this network: String(),
        except for an IPv4-mapped IPv6 network, which String() prints dotted
        (and ParseCIDR would then take for IPv4)."""
        if len(self.ip) == 16 and to4(self.ip) is not None:
            return f"::ffff:{ip_string(self.ip)}/{self.ones}"
        return str(self)


def parse_cidr_go(s: str) -> tuple[bytes, Net]:
    """net.ParseCIDR: (the address as ParseIP gives it, the network); raises
    ValueError("invalid CIDR address: ...")."""
    err = ValueError(f"invalid CIDR address: {s}")
    i = s.find("/")
    if i < 0:
        raise err
    addr, mask = s[:i], s[i + 1:]
    v4 = _parse_ipv4(addr)
    ip = v4 if v4 is not None else _parse_ipv6(addr)
    if ip is None:
        raise err
    n, c, ok = _dtoi(mask)
    if not ok or c != len(mask) or n > 8 * len(ip):
        raise err
    full = _V4_IN_V6 + ip if len(ip) == 4 else ip
    return full, Net(_mask(ip, cidr_mask(n, 8 * len(ip))), n)


# ---------------------------------------------------------------- sanitize --
def cidr_sanitize(cidr: str) -> int:
    """CIDR.sanitize (rule_validation.go:360-385): the prefix length, 0 for a
    bare IP (the reference returns its zero value there).  net.ParseCIDR only
    builds contiguous masks, so the non-contiguous refusal cannot fire from a
    string; `cidr_mask_size` restates it for masks given as bytes."""
    if cidr == "":
        raise ValueError("IP must be specified")
    try:
        _, net = parse_cidr_go(cidr)
    except ValueError as e:
        if parse_ip(cidr) is None:
            raise ValueError(f"Unable to parse CIDR: {e}") from None
        return 0
    return net.ones


def cidr_mask_size(mask: bytes) -> tuple[int, int]:
    """net.IPMask.Size: (ones, bits), or (0, 0) for a non-contiguous mask —
    what the sanitizers refuse with "CIDR cannot specify non-contiguous
    mask"."""
    v = int.from_bytes(mask, "big")
    bits = 8 * len(mask)
    ones = bin(v).count("1")
    if v != ((1 << ones) - 1) << (bits - ones):
        return 0, 0
    return ones, bits


@dataclass
class CIDRRule:
    """api.CIDRRule."""
    Cidr: str = ""
    ExceptCIDRs: list = field(default_factory=list)

    @staticmethod
    def from_json(d) -> "CIDRRule":
        d = {str(k).lower(): v for k, v in (d or {}).items()}
        return CIDRRule(str(d.get("cidr", "")), [str(x) for x in d.get("except") or []])


def cidr_rule_sanitize(rule: CIDRRule) -> int:
    """CIDRRule.sanitize (rule_validation.go:387-425): only <IP>/<prefix>;
    every exception parses and lies inside the allowed prefix (which also
    makes them one family)."""
    try:
        _, net = parse_cidr_go(rule.Cidr)
    except ValueError as e:
        raise ValueError(f'Unable to parse CIDRRule "{rule.Cidr}": {e}') from None
    for p in rule.ExceptCIDRs:
        addr, _ = parse_cidr_go(p)
        if not net.contains(addr):
            raise ValueError(f"allow CIDR prefix {rule.Cidr} does not contain exclude CIDR prefix {p}")
    return net.ones


def sanitize_direction(members: Mapping[str, int], no_ports: Iterable[str], has_ports: bool, cidrs: Sequence[str],
                       cidr_rules: Sequence[CIDRRule], direction: str) -> None:
    """The CIDR part of IngressRule.sanitize / EgressRule.sanitize
    (rule_validation.go:70-143, :147-223).  Of the member-combination checks
    only those with a CIDR member on one side are restated: "Combining X and
    Y is not supported yet" for two non-empty L3 members, and for ingress
    "Combining FromCIDR / FromCIDRSet and ToPorts".  Then every CIDR and
    CIDRRule sanitizes and the distinct prefix lengths stay within
    MaxCIDRPrefixLengths."""
    cidr_members = [m for m in members if "CIDR" in m]
    for m1 in sorted(members):
        for m2 in sorted(members):
            if m1 != m2 and members[m1] > 0 and members[m2] > 0 and (m1 in cidr_members or m2 in cidr_members):
                raise ValueError(f"Combining {m1} and {m2} is not supported yet")
    for m in no_ports:
        if members.get(m, 0) > 0 and has_ports:
            raise ValueError(f"Combining {m} and ToPorts is not supported yet")
    lengths = {cidr_sanitize(c) for c in cidrs} | {cidr_rule_sanitize(r) for r in cidr_rules}
    if len(lengths) > MAX_CIDR_PREFIX_LENGTHS:
        raise ValueError(f"too many {direction} CIDR prefix lengths {len(lengths)}/{MAX_CIDR_PREFIX_LENGTHS}")


# -------------------------------------------------------------- RemoveCIDRs --
def _remove_cidr(allow: Net, remove: Net) -> list[Net]:
    """removeCIDR (ip.go:184-246): the prefixes of lengths Y+1 .. X that cover
    `allow` (length Y) without `remove` (length X), longest last."""
    allow4, remove4 = to4(allow.ip) is not None, to4(remove.ip) is not None
    if allow4 != remove4:
        raise ValueError("cannot mix IP addresses of different IP protocol versions")
    bitlen = 32 if allow4 else 128
    if allow.ones >= remove.ones:
        raise ValueError("allow CIDR prefix must be a superset of remove CIDR prefix")
    a = int.from_bytes(allow.ip, "big")
    r = int.from_bytes(remove.ip, "big")
    out = []
    for i in range(bitlen - allow.ones - 1, bitlen - remove.ones - 1, -1):
        size = bitlen - i
        ip = (r ^ (1 << i)) | a
        ip &= ((1 << size) - 1) << (bitlen - size)
        out.append(Net(ip.to_bytes(bitlen // 8, "big"), size))
    return out


def remove_cidrs(allow: Sequence[Net], remove: Sequence[Net]) -> list[Net]:
    """RemoveCIDRs (ip.go:119-170): `remove` sorted by mask length then
    address, exceptions inside other exceptions dropped, then each allowed
    prefix that holds an exception is replaced — taken out of its place, its
    remainder appended — so the order of the result is the reference's."""
    allow = list(allow)
    remove = sorted(remove, key=lambda n: (n.ones, n.ip))  # sort.Sort(NetsByMask): not stable, ties are equal nets
    again = True
    while again:
        again = False
        for j, r1 in enumerate(remove):
            for i, r2 in enumerate(remove):
                if i != j and r1.contains(r2.ip):
                    del remove[i]
                    again = True
                    break
            if again:
                break
    for rm in remove:
        again = True
        while again:
            again = False
            for i, al in enumerate(allow):
                if (to4(al.ip) is not None) != (to4(rm.ip) is not None):
                    raise ValueError("cannot mix IP addresses of different IP protocol versions")
                if al.contains(rm.ip):
                    nets = _remove_cidr(al, rm)
                    del allow[i]
                    allow += nets
                    again = True
                    break
                if rm.contains(al.ip):
                    del allow[i]
                    again = True
                    break
    return allow


def compute_resultant_cidr_set(rules: Iterable[CIDRRule]) -> list[str]:
    """ComputeResultantCIDRSet (api/cidr.go:115-132)."""
    out: list[str] = []
    for r in rules:
        _, allow = parse_cidr_go(r.Cidr)
        removes = [parse_cidr_go(t)[1] for t in r.ExceptCIDRs]
        out += [str(n) for n in remove_cidrs([allow], removes)]
    return out


def get_cidr_prefixes(rules: Iterable) -> list[Net]:
    """GetCIDRPrefixes (pkg/policy/cidr.go:24-70) over resolve.Rule objects:
    every CIDR the rules refer to, duplicates kept, in rule order."""
    def parse(cidrs):  # ip.ParseCIDRs: a bare IP is a full-length prefix, what does not parse is left out
        return [n for n in map(_to_net, cidrs) if n is not None]
    res: list[Net] = []
    for r in rules:
        for ir in r.Ingress:
            res += parse(ir.FromCIDR)
            res += parse(compute_resultant_cidr_set(ir.FromCIDRSet))
        for er in r.Egress:
            res += parse(er.ToCIDR)
            res += parse(compute_resultant_cidr_set(er.ToCIDRSet))
    return res


# ------------------------------------------------------------------ labels --
@functools.lru_cache(maxsize=1 << 16)  # the short ancestors of many prefixes are the same few strings
def masked_ip_to_label_string(ip: bytes, prefix: int) -> str:
    """maskedIPToLabelString (pkg/labels/cidr.go:23-45)."""
    s = ip_string(ip).replace(":", "-")
    pre = "0" if s[0] == "-" else ""
    post = "0" if s[-1] == "-" else ""
    return f"cidr:{pre}{s}{post}/{prefix}"


def _to_net(prefix) -> Optional[Net]:
    """IPStringToLabel's parse: a CIDR, or a bare IP as a full-length prefix."""
    if isinstance(prefix, Net):
        return prefix
    try:
        return parse_cidr_go(prefix)[1]
    except ValueError:
        ip = parse_ip(prefix)
        if ip is None:
            return None
        p4 = to4(ip)  # Go keeps the 16 bytes beside a 4-byte mask; they print dotted all the same
        return Net(p4, 32) if p4 is not None else Net(ip, 128)


def ip_string_to_label(ip: str) -> Optional[str]:
    """IPStringToLabel (pkg/labels/cidr.go:58-73): the "cidr:..." label key
    of a CIDR or bare IP, None when it parses as neither."""
    net = _to_net(ip)
    return None if net is None else masked_ip_to_label_string(net.ip, net.ones)


def cidr_labels(prefix) -> dict[str, str]:
    """GetCIDRLabels (pkg/labels/cidr/cidr.go:32-50): cidr:<P masked to i>/i
    for i in 0..m when m > 0, then reserved:world; all values ""."""
    net = _to_net(prefix)
    if net is None:
        raise ValueError(f"invalid CIDR address: {prefix}")
    out: dict[str, str] = {}
    if net.ones > 0:
        bits, nbytes = net.bits, len(net.ip)
        a = int.from_bytes(net.ip, "big")
        for i in range(net.ones + 1):
            sh = bits - i
            out[masked_ip_to_label_string(((a >> sh) << sh).to_bytes(nbytes, "big"), i)] = ""
    out[LABEL_WORLD] = ""
    return out


def cidr_slice_selectors(cidrs: Iterable[str]) -> list[dict[str, str]]:
    """CIDRSlice.GetAsEndpointSelectors (api/cidr.go:70-86) as matchLabels
    dicts: reserved:world once, before the first member that matches all."""
    out: list[dict[str, str]] = []
    world = False
    for c in cidrs:
        if c in CIDR_MATCH_ALL and not world:
            world = True
            out.append({LABEL_WORLD: ""})
        lbl = ip_string_to_label(c)
        if lbl is None:
            raise ValueError(f"Unable to parse CIDR: {c}")
        out.append({lbl: ""})
    return out


def cidr_rule_slice_selectors(rules: Iterable[CIDRRule]) -> list[dict[str, str]]:
    """CIDRRuleSlice.GetAsEndpointSelectors (api/cidr.go:99-104)."""
    return cidr_slice_selectors(compute_resultant_cidr_set(rules))


# --------------------------------------------------------------- allocator --
def nets_to_keys(nets: Sequence[Net]):
    """The networks as a cg_cidr array (classifier.CIDR_DTYPE): what the
    ipcache and SelectorCache.set_cidr_identities take."""
    import numpy as np

    from .classifier import CIDR_DTYPE
    a = np.zeros(len(nets), CIDR_DTYPE)
    for i, n in enumerate(nets):
        a["family"][i] = n.family
        a["prefixlen"][i] = n.ones
        a["addr"][i, :len(n.ip)] = np.frombuffer(n.ip, np.uint8)
    return a


def to_net(prefix) -> Net:
    """A prefix string (or bare IP, or Net) as a Net; ValueError otherwise."""
    n = _to_net(prefix)
    if n is None:
        raise ValueError(f"invalid CIDR address: {prefix}")
    return n


class CIDRIdentityAllocator:
    """AllocateCIDRs / ReleaseCIDRs (pkg/ipcache/cidr.go:26-86) over a local
    allocator: one numeric identity per distinct prefix from `base` up
    (identity.MinimalNumericIdentity is 256), reference-counted, and the
    prefix → identity mapping kept in `ipcache` (an IPCache) so the datapath
    lookup returns the same number.

    A /0 prefix has the label set {reserved:world} alone, for which
    identity.AllocateIdentity returns the reserved identity 2 (world) through
    LookupReservedIdentityByLabels without touching the allocator, and
    Identity.Release ignores it: so a /0 allocates nothing, is never counted
    and never released, and maps to 2 in the ipcache."""

    def __init__(self, base: int = 256, ipcache=None, max_id: int = 0xFFFF):
        if base < 256:
            raise ValueError("CIDR identities start at 256 or above")
        self.base, self.max_id, self.ipcache = base, max_id, ipcache
        self._ids: dict[Net, int] = {}
        self._refs: dict[Net, int] = {}
        self._free: list[int] = []
        self._next = base

    @staticmethod
    def _nets(prefixes) -> list[Net]:
        out = []
        for p in prefixes:
            n = _to_net(p)
            if n is None:
                raise ValueError(f"invalid CIDR address: {p}")
            out.append(n)
        return out

    def allocate(self, prefixes: Iterable) -> list[int]:
        """The identities of `prefixes`, in order; all or nothing."""
        nets = self._nets(prefixes)
        fresh = {n for n in nets if n.ones > 0 and n not in self._ids}
        if self._next + len(fresh) - len(self._free) - 1 > self.max_id:
            raise RuntimeError("no more available IDs in configured space")
        out = []
        for n in nets:
            if n.ones == 0:
                out.append(RESERVED_WORLD)
                continue
            if n not in self._ids:
                if self._free:
                    self._ids[n] = self._free.pop()
                else:
                    self._ids[n] = self._next
                    self._next += 1
            self._refs[n] = self._refs.get(n, 0) + 1
            out.append(self._ids[n])
        if self.ipcache is not None and nets:
            self.ipcache.update(nets_to_keys(nets), [[i, 0] for i in out])
        return out

    def release(self, prefixes: Iterable) -> None:
        """ReleaseCIDRs: one reference of each prefix; the last one frees the
        identity and deletes the ipcache entry."""
        gone = []
        for n in self._nets(prefixes):
            if n.ones == 0 or n not in self._refs:
                continue
            self._refs[n] -= 1
            if self._refs[n] == 0:
                del self._refs[n]
                self._free.append(self._ids.pop(n))
                gone.append(n)
        if self.ipcache is not None and gone:
            self.ipcache.delete(nets_to_keys(gone))

    def lookup(self, prefix) -> Optional[int]:
        n = _to_net(prefix)
        if n is not None and n.ones == 0:
            return RESERVED_WORLD
        return self._ids.get(n)

    def identities(self) -> dict[int, str]:
        """{identity: "prefix"} of the live allocations, in allocation order:
        what SelectorCache.set_cidr_identities takes."""
        return {i: n.text() for n, i in self._ids.items()}
