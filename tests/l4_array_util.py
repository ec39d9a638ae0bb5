"""The array, maps and tuples that test_l4_array.py (host evaluator) and
test_l4_array_gpu.py (kernel) share, and the per-map expectation."""
import functools

import numpy as np

from cilium_amd import _native as N
from cilium_amd import synth
from cilium_amd.classifier import L4_TUPLE_DTYPE, POLICY_KEY_DTYPE

EMPTY_SLOT = 2
SLOTS = [0, 1, EMPTY_SLOT, 7, 300, 65535]  # the six endpoint ids of the tuples, slot 2 left empty
BIG_IDS = 512  # identities of the 3,000-entry table
SMALL_IDS = 24
MODES = [m | d for m in (N.CG_L4_CAN_ACCESS, N.CG_L4_INGRESS, N.CG_L4_EGRESS) for d in (0, N.CG_L4_IGNORE_DROP)]
N_TUPLES = 4099


@functools.lru_cache(maxsize=None)
def tables():
    """(keys, ports_be, n_ids) of the four distinct maps, in the order of build_maps."""
    l3 = np.zeros(1, POLICY_KEY_DTYPE)
    l3[0] = (777, 0, 0, 0)  # one L3-only ingress entry
    return [
        (np.zeros(0, POLICY_KEY_DTYPE), np.zeros(0, np.uint16), SMALL_IDS),
        (l3, np.zeros(1, np.uint16), SMALL_IDS),
        synth.l4_table(n_entries=64, n_ids=SMALL_IDS, seed=11) + (SMALL_IDS,),
        synth.l4_table(n_entries=3000, n_ids=BIG_IDS, seed=12) + (BIG_IDS,),  # 2,048 buckets; the others have 4 to 32
    ]


def build_maps(cl):
    """Four maps: empty, one L3-only entry, max_entries=64 filled to 64, a
    default map of ~3,000 entries."""
    maps = []
    for i, (keys, ports, _) in enumerate(tables()):
        pm = cl.policy_map(max_entries=64 if i == 2 else 0)
        if len(keys):
            pm.allow_keys(keys, ports)
        maps.append(pm)
    return maps


# slot -> index into build_maps(): the big map sits in two slots
SLOT_MAP = {0: 0, 1: 1, 7: 2, 300: 3, 65535: 3}


def build_array(cl, maps):
    arr = cl.policy_array()
    arr.set_many(list(SLOT_MAP), [maps[i] for i in SLOT_MAP.values()])
    return arr


@functools.lru_cache(maxsize=None)
def tuples_round_robin():
    """(lxc_ids, tuples): N_TUPLES tuples, endpoint ids round-robin over SLOTS
    (adjacent tuples never share a table).  Each tuple is drawn for its own
    slot's table: config 2's generator over that table's identities and ports
    (unknown identities, 1% fragments, 1% CB_POLICY), and then a third of them
    rewritten to hit an entry of the table — an exact {id, port, proto} key, an
    L3-only key with some port, or a wildcard-identity key with an identity
    the table does not know — with fragments and CB_POLICY raised to 10%."""
    rng = np.random.default_rng(99)
    lxc = np.array(SLOTS, np.uint16)[np.arange(N_TUPLES) % len(SLOTS)]
    t = np.zeros(N_TUPLES, L4_TUPLE_DTYPE)
    for slot in SLOTS:
        idx = np.flatnonzero(lxc == slot)
        keys, _, n_ids = tables()[SLOT_MAP.get(slot, 3)]
        part = synth.l4_tuples(len(idx), keys, n_ids=n_ids, seed=1000 + slot)
        if len(keys):
            hit = np.flatnonzero(rng.random(len(idx)) < 0.34)
            k = keys[rng.integers(0, len(keys), len(hit))]
            l3 = k["dport"] == 0
            part["identity"][hit] = np.where(k["sec_label"] == 0, 900_001, k["sec_label"])
            part["dport"][hit] = np.where(l3, rng.integers(1, 65536, len(hit)), k["dport"])
            part["proto"][hit] = np.where(l3, 6, k["protocol"])
            part["flags"][hit] = (part["flags"][hit] & ~np.uint8(1)) | (k["egress"] ^ 1)
        t[idx] = part
    t["flags"] |= (rng.random(N_TUPLES) < 0.1).astype(np.uint8) << 1
    t["flags"] |= (rng.random(N_TUPLES) < 0.1).astype(np.uint8) << 2
    t["len"][::97] = 70_000  # past the 16 bits a packed counter would hold
    return lxc, t


def apply_mode(tuples, mode):
    """The tuple flags __policy_can_access sees under `mode` (l4_walk.h
    l4_mode_word): the ingress wrapper forces dir = CT_INGRESS, the egress one
    dir = CT_EGRESS and is_fragment = false."""
    t = tuples.copy()
    if mode & 3 == N.CG_L4_INGRESS:
        t["flags"] |= N.CG_L4_F_INGRESS
    elif mode & 3 == N.CG_L4_EGRESS:
        t["flags"] &= ~np.uint8(N.CG_L4_F_INGRESS | N.CG_L4_F_FRAGMENT)
    return t


def wrap(verdicts, mode):
    """l4_walk.h l4_wrap: both wrappers turn any negative result into
    DROP_POLICY, or TC_ACT_OK with IGNORE_DROP."""
    if mode & 3 == N.CG_L4_CAN_ACCESS:
        return verdicts
    return np.where(verdicts < 0, 0 if mode & N.CG_L4_IGNORE_DROP else N.CG_DROP_POLICY, verdicts).astype(np.int32)


def expected_per_map(maps, lxc, tuples, mode, per_map):
    """Tuple i's verdict from per_map(maps[SLOT_MAP[lxc[i]]], tuples of that
    slot), -140 for the empty slot.  per_map(pm, tuples) -> verdicts."""
    out = np.full(len(tuples), N.CG_DROP_MISSED_TAIL_CALL, np.int32)
    for slot, mi in SLOT_MAP.items():
        idx = np.flatnonzero(lxc == slot)
        if len(idx):
            out[idx] = per_map(maps[mi], tuples[idx])
    return out


def expected_host(maps, lxc, tuples, mode):
    """From the per-map host evaluator, which is plain CAN_ACCESS: the mode
    goes into the flags first and round the result afterwards."""
    return expected_per_map(maps, lxc, tuples, mode,
                            lambda pm, t: wrap(pm.eval_host_diag(apply_mode(t, mode)), mode))


def counters(pm):
    return sorted((k.Identity, k.DestPort, k.Nexthdr, k.TrafficDirection, e.ProxyPort, e.Packets, e.Bytes)
                  for k, e in pm.dump_to_slice())
