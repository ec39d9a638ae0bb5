"""The fixtures of test_kafka_decode_edges_gpu.py proven on the CPU: every
corpus of kafka_edges_util through its two references (the host decoder and
oracle/kafka_wire_ref.py) against each other, and the coverage condition each
corpus is built for (the stage boundary on both sides, every CRC head / tail
shape, the LDS / arena split of the inflater, hash-table wrap-around and the
equal-hash pair of the intern tables) checked from first principles."""
import numpy as np
import pytest

import kafka_edges_util as E
from cilium_amd import _native as N
from cilium_amd import kafka_requests as K
from oracle import kafka_wire_ref as R

UNKNOWN = N.CG_KAFKA_UNKNOWN_STR


def _refs(host, key, pols, reqs, ids):
    red, rem = E.red_rem(len(reqs), ids)
    h, o = E.references(host, key, pols, reqs, red, rem)
    assert E.first_difference(h, o) is None
    return h


# --------------------------------------------------------- stage layouts --
@pytest.mark.parametrize("S", E.STAGES)
def test_stage_layouts_reach_both_sides_of_the_boundary(host, S):
    pols, topics, clients, ids = E.base_policy()
    sc = E.stage_layouts(S)
    reqs = sc.reqs
    ref = _refs(host, ("stage", S), pols, reqs, ids)
    st = np.array([r[0] for r in ref])
    key = np.array([r[1] for r in ref])
    lens = np.array([len(r) for r in reqs])
    assert len(reqs) == 640 and 0.6 < (st[:448] == 0).mean() < 0.95  # about 70 % left as built, L1 to L4
    ok_produce = (st == 0) & (key == K.PRODUCE) & (lens > 60)
    leads = E.ALL_LEADS if S == 4096 else E.FEW_LEADS
    model = {lead: E.stage_model(lens, lead, S) for lead in leads}

    def wave(name):
        return slice(sc.first[name], sc.first[name] + 64)
    for lead, (staged, at_hi) in model.items():
        assert staged[wave("L1")].all()
        # L2: k straddles the boundary, k - 1 is staged, k + 1 is not
        k = sc.k["L2"]
        assert ok_produce[k - 1:k + 2].all()
        assert staged[k - 1] and not staged[k] and not staged[k + 1]
        # L4: nothing of the wave is staged, its produce requests read HBM
        assert not staged[wave("L4")].any() and ok_produce[wave("L4")].sum() >= 2
        # L5 / L6: zero-length requests count as staged at the stage's start or not at all; no byte is read
        assert (lens[sc.first["L5"] + 64:sc.first["L5"] + 128] == 0).all()
        assert lens[wave("L6")].sum() < 16 and set(lens[wave("L6")]) == {0, 1}
    for d in (0, 8, 15, 16):
        k = sc.k["L3_%d" % d]
        assert ok_produce[k - 1:k + 2].all()
        got = {lead: bool(model[lead][0][k]) for lead in leads}
        # the group starts on a 16-byte boundary of the requests: the window ends lead bytes before start + S
        assert got == {lead: d >= lead for lead in leads}, (d, got)
        assert all(model[lead][0][k - 1] and not model[lead][0][k + 1] for lead in leads)
    # both outcomes for the request at the boundary, and a request that ends exactly at hi
    for d in (0, 8):
        vals = {bool(model[lead][0][sc.k["L3_%d" % d]]) for lead in leads}
        assert vals == {True, False}, d
    assert any(model[lead][1][sc.k["L3_%d" % d]] for lead in leads for d in (0, 8, 15, 16))
    assert model[0][1][sc.k["L3_0"]] and model[15][1][sc.k["L3_15"]]
    assert not any(model[lead][1][sc.k["L3_16"]] for lead in leads)
    # L7: the cuts end in a lone request, a full group less one, a full group, and a group of one
    assert [n % 64 for n in E.STAGE_CUTS] == [1, 63, 0, 1, 1] and max(E.STAGE_CUTS) <= len(reqs)


# ------------------------------------------------------------ CRC shapes --
def test_crc_shapes_cover_every_head_and_tail(host):
    pols, topics, clients, ids = E.base_policy()
    shapes = E.crc_shapes(topics)
    staged = E.crc_staged(topics)
    assert len(staged) == 600 and not any(staged[1::3]) and not any(staged[2::3])
    ref = _refs(host, "crc-staged", pols, staged, ids)
    assert all(r[0] == 0 for r in ref[::3])  # all well-formed
    # a rejected CRC is a decode error in these requests: one bit of each CRC field flipped
    for (v, c, ver, m), r in zip(shapes, staged[::3]):
        at, n = E.crc_region(r, m)
        assert n == (10 if ver == 0 else 18) + v
        bad = bytearray(r)
        bad[at - 1] ^= 0x10
        assert R.decode(r) is not None and R.decode(bytes(bad)) is None
    # (region start mod 4, region length mod 8): all 32 pairs over the leads
    raw, off = K.concat(staged)
    pairs = set()
    for lead in E.ALL_LEADS:
        for j, ((v, c, ver, m), r) in enumerate(zip(shapes, staged[::3])):
            at, n = E.crc_region(r, m)
            pairs.add(((lead + int(off[3 * j]) + at) % 4, n % 8))
    assert len(pairs) == 32
    # the staged placement is staged, the other is not
    lens = [len(r) for r in staged]
    assert all(E.stage_model(lens, lead, 4096)[0].all() for lead in E.ALL_LEADS)
    unstaged = E.crc_unstaged(topics)
    ref = _refs(host, "crc-unstaged", pols, unstaged, ids)
    assert all(r[0] == 0 for r in ref) and len(unstaged) == 204
    lens = [len(r) for r in unstaged]
    assert not any(E.stage_model(lens, lead, 4096)[0].any() for lead in E.ALL_LEADS)
    raw, off = K.concat(unstaged)
    real = [j for j in range(len(unstaged)) if j % 64]
    assert [unstaged[j] for j in real] == staged[::3]
    pairs = {((lead + int(off[j]) + E.crc_region(unstaged[j], m)[0]) % 4, (len(m) - 16) % 8)
             for lead in E.ALL_LEADS for j, (v, c, ver, m) in zip(real, shapes)}
    assert len(pairs) == 32


def test_crc_inner_sets_tell_a_rejected_crc(host):
    pols, topics, clients, ids = E.base_policy()
    reqs, poisoned = E.crc_inner_all(topics)
    assert len(reqs) == 1600
    ref = _refs(host, "crc-inner", pols, reqs, ids)
    # the poisoned sets are errors exactly because the message before the poison was accepted
    assert [r[0] for r in ref] == [1 if p else 0 for p in poisoned]
    # ... and stop being errors when that message's CRC is rejected
    for ver in (0, 1):
        m = E.crc_message(9, 2, ver)
        bad = bytearray(m)
        bad[12] ^= 1
        ts = None if ver == 0 else 0
        for inner, want in ((m + E.poison_message(ver), None), (bytes(bad) + E.poison_message(ver), "ok")):
            r = E._two_topic_produce(ver, b"c", topics[:2], K.message(None, K.snappy_block(inner), 2, 0, ts) + E.TERMINATOR)
            assert (R.decode(r) is None) == (want is None)


# -------------------------------------------------------- inflate shapes --
def test_inflate_shapes_are_the_devices_to_finish(host):
    pols, topics, clients, ids = E.base_policy()
    reqs, wrappers, decoded = E.inflate_shapes(topics, clients)
    ref = _refs(host, "inflate", pols, reqs, ids)
    assert all(r[0] == 0 for r in ref)
    n_shapes = (3 * len(E.INFLATE_SIZES) + 3) * len(E.ENCODERS)
    assert wrappers == n_shapes + 12 * 3 + sum(range(13, 21)) and len(reqs) == n_shapes + 12 + 8
    # a full inflate arena is never legitimate for this batch
    assert decoded < E.INFLATE_ARENA // 2
    assert {n for n in E.INFLATE_SIZES if n <= E.KINF_LDS} == {26, 255, 256}
    assert max(len(R.decode(r)[4]) for r in reqs) == 20
    deferred = E.inflate_deferred(topics, clients)
    ref = _refs(host, "inflate-deferred", pols, deferred, ids)
    assert all(r[0] == 0 for r in ref) and len(deferred) == 12


# ---------------------------------------------------------------- intern --
@pytest.mark.parametrize("both", [False, True])
def test_intern_fixtures(host, both):
    assert E.fnv1a(E.PAIR[0]) == E.fnv1a(E.PAIR[1]) == E.PAIR_HASH
    assert len(E.PAIR[0]) == len(E.PAIR[1]) > 16 and E.PAIR[0][:16] == E.PAIR[1][:16] and E.PAIR[0] != E.PAIR[1]
    pols, topics, clients = E.intern_policy(both)
    reqs, tc, cc = E.intern_requests(both)
    ids = [1]
    _refs(host, ("intern", both), pols, reqs, ids)
    host.update_kafka_policy(pols)
    for what, strings, cands in (("topic", topics, tc), ("client", clients, cc)):
        assert len(set(strings)) == len(strings) == (14 if both else 13)
        cap = E.dict_capacity(len(strings))
        assert cap == 32
        # three names whose home slot is the table's last: two of them wrap to slot 0 and on
        homes = [E.fnv1a(s) & (cap - 1) for s in strings]
        assert homes.count(cap - 1) >= 3
        assert sorted(len(s) for s in strings[:len(E.INTERN_LENS)]) == list(E.INTERN_LENS)
        got = {s: host.kafka_intern(what, s) for s in cands}
        known = {s: got[s] for s in strings}
        assert UNKNOWN not in known.values() and len(set(known.values())) == len(strings)
        # whatever is not a rule's string is unknown: near misses, the empty string, 300 bytes
        assert all(got[s] == UNKNOWN for s in cands if s not in known)
        assert b"" in cands and got[b""] == UNKNOWN and any(len(s) == 300 for s in cands)
        assert (got[E.PAIR[1]] == UNKNOWN) == (not both) and got[E.PAIR[0]] != got[E.PAIR[1]]
        # every candidate is named by some request
        seen = set()
        for r in reqs:
            d = R.decode(r)
            seen.add(d[3])
            seen.update(d[4])
        assert set(cands) <= seen
    n_topics = [len(R.decode(r)[4]) for r in reqs]
    assert max(n_topics) == len(tc) > 12 and 12 in n_topics
