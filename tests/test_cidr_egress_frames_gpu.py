"""toCIDRSet + except + toPorts on packets: policy JSON → CIDR identity
allocator → ipcache + selector cache → sync_policy_maps → the from-container
program's verdict per raw frame (cg_l4_frames_egress_verdicts_*), every probe
against the brute-force evaluation of the rule text, and the reply of an
allowed flow coming back in through the ingress program."""
import ipaddress

import numpy as np
import pytest

import cidr_util as CU
import egress_util as E
import frames_util as F
from cilium_amd import _native as N
from cilium_amd import cidr as CIDR
from cilium_amd import resolve as R

pytestmark = pytest.mark.gpu

LXC = 42


@pytest.fixture
def world(gpu):
    repo = R.Repository([R.Rule.from_json(r) for r in CU.E2E_POLICY],
                        R.PolicyConfig(always_allow_localhost=False, enforcement="always"))
    ic, sc, pm, arr, ct = gpu.ipcache(), gpu.selector_cache(), gpu.policy_map(), gpu.policy_array(), gpu.conntrack_map()
    alloc = CIDR.CIDRIdentityAllocator(base=1000, ipcache=ic)
    alloc.allocate(CIDR.get_cidr_prefixes(repo.rules))
    sc.set_identities(CU.E2E_LABELS)
    sc.set_cidr_identities(alloc.identities())
    sc.set_repository(repo)
    sc.sync_policy_maps([CU.E2E_APP1], [pm])
    arr.set(LXC, pm)
    arr.set_header(LXC, mac="0a:00:00:00:00:2a", node_mac=E.NODE_MAC, ipv4="10.0.0.42", ipv6="fd00::2a",
                   router_ip6=E.ROUTER_IP6, seclabel=CU.E2E_APP1)
    yield repo, ic, pm, arr, ct, E.header_dict(arr.get_header(LXC))
    for x in (ct, arr, pm, sc, ic):
        x.destroy()


def _frame(hd, family, addr, dport, proto, sport=40000):
    l4 = E.tcp(sport, dport) if proto == 6 else E.udp(sport, dport)
    if family == 4:
        return E.ip4(hd, str(ipaddress.IPv4Address(addr)), proto, l4)
    return E.ip6(hd, str(ipaddress.IPv6Address(addr)), proto, l4)


def test_every_probe_on_frames(gpu, world):
    repo, ic, pm, arr, ct, hd = world
    probes = CU.e2e_probes(repo)
    want = np.array([CU.e2e_oracle(CU.E2E_POLICY, *p) for p in probes])
    assert 0.2 < want.mean() < 0.8
    raw, off = F.join([_frame(hd, *p) for p in probes])
    lxc = np.full(len(probes), LXC)
    v, info = arr.frame_egress_verdicts(raw, off, lxc_ids=lxc, ipcache=ic, info=True)
    assert set(v.tolist()) == {0, N.CG_DROP_POLICY}
    bad = [probes[i] for i in np.flatnonzero((v == 0) != want)]
    assert not bad, bad
    assert (info["t"]["flags"] == N.CG_L4_F_WALKED).all()
    hv, hinfo = arr.frame_egress_eval_host_diag(raw, off, lxc_ids=lxc, ipcache=ic, info=True)
    assert np.array_equal(v, hv) and info.tobytes() == hinfo.tobytes()


def test_named_cases_and_the_reply_coming_back(gpu, world):
    repo, ic, pm, arr, ct, hd = world
    a = lambda s: int(ipaddress.ip_address(s))
    cases = [("an allowed prefix", (4, a("10.1.2.3"), 80, 6), 0),
             ("the excepted sub-prefix", (4, a("10.100.0.1"), 80, 6), N.CG_DROP_POLICY),
             ("a wrong port", (4, a("10.1.2.3"), 81, 6), N.CG_DROP_POLICY),
             ("world", (4, a("8.8.8.8"), 80, 6), N.CG_DROP_POLICY)]
    frames = [_frame(hd, *p) for _, p, _ in cases]
    raw, off = F.join(frames)
    lxc = [LXC] * len(cases)
    v, info, rec = arr.frame_egress_verdicts(raw, off, lxc_ids=lxc, ipcache=ic, info=True, conntrack=ct)
    assert v.tolist() == [w for _, _, w in cases]
    ident = info["t"]["identity"].tolist()
    # the exception is cut out of the prefixes that get identities: its addresses resolve to world
    assert ident[0] == ident[2] >= 1000 and ident[1] == ident[3] == N.CG_WORLD_ID
    assert rec["op"].tolist() == [1, 0, 0, 0] and (rec["pad2"][:, 0] == CU.E2E_APP1).all()
    # the reply to the allowed flow, coming in: new and denied before apply (no ingress rule, enforcement always) ...
    back, boff = F.join([E.reply_of(frames[0], E.mac("0a:00:00:00:99:99"), hd["lxc_mac"])])
    kw = dict(lxc_ids=[LXC], ipcache=ic, info=True, conntrack=ct)
    bv, _, brec = arr.frame_verdicts(back, boff, **kw)
    assert bv.tolist() == [N.CG_DROP_POLICY] and brec["state"].tolist() == [N.CG_CT_STATE_NEW]
    assert ct.apply(rec, [len(f) for f in frames]).tolist() == [0] * 4
    # ... and a reply after it
    bv, _, brec = arr.frame_verdicts(back, boff, **kw)
    assert bv.tolist() == [0] and brec["state"].tolist() == [N.CG_CT_STATE_REPLY]
    # the reply to the denied flow was never created
    back2, boff2 = F.join([E.reply_of(frames[2], E.mac("0a:00:00:00:99:99"), hd["lxc_mac"])])
    assert arr.frame_verdicts(back2, boff2, **kw)[0].tolist() == [N.CG_DROP_POLICY]
