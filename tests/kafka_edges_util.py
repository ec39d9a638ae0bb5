"""Hand-built Kafka request corpora that aim at the device-only parts of
kafka_decode_kernel and kafka_inflate_kernel (kernels_kafka.hip): the
per-wave LDS stage and its boundary, LdsCrc's head / body / tail paths on
its three kinds of pointer, kw_intern's blob compare and probe wrap-around,
and DevInflate's LDS / arena split and block kinds.

Nothing here states what the device should answer: the expectations are the
host decoder (diag_cpu) and oracle/kafka_wire_ref.py, see references().  The
stage model below restates the kernel's lo / hi / staged arithmetic only to
prove that a fixture reaches the case it is named for.

A bad message CRC is not a decode error: readMessageSet ends the set there
and leaves the rest of it unread (messages.go:352-494), so a one-message set
parses alike whatever its CRC.  The CRC fixtures therefore end every outer
set with TERMINATOR, twelve bytes that read as "offset, size 0" (the set's
end) when the parser reaches them as a message header, and as a topic name
of 32767 bytes (a decode error) when a rejected CRC left them for the next
topic's decoder.  Inside a compressed payload nothing follows the set, so
there a second, poisoned message is what tells the two outcomes apart."""
from __future__ import annotations

import gzip
import struct
import zlib

import numpy as np

from cilium_amd import _native as N
from cilium_amd import kafka_requests as K
from cilium_amd import synth
from cilium_amd.classifier import KAFKA_REQ_DTYPE
from kafka_corpus import mutate, oracle_view, records_view
from oracle import kafka_wire_ref as R
from test_kw_inflate import _gz_raw

ALL_LEADS = tuple(range(16))
FEW_LEADS = (0, 5, 15)
STAGES = (4096, 8192, 16384)
KINF_LDS = 256  # kInfLds: payloads decoding to at most this many bytes stay in LDS
INFLATE_ARENA = 64 << 20  # kKafkaInflateArena
MAX_PARSE_BUF = 100 * 65535
TERMINATOR = struct.pack(">qi", 0x7FFF000000000000, 0)


def fnv1a(b: bytes) -> int:
    h = 2166136261
    for c in b:
        h = ((h ^ c) * 16777619) & 0xFFFFFFFF
    return h


def dict_capacity(n_strings: int) -> int:
    """build_dict (kafka.cc): a power of two >= max(16, 2 * strings)."""
    cap = 16
    while cap < 2 * n_strings:
        cap <<= 1
    return cap


# ------------------------------------------------------------ running ----
def red_rem(n: int, ids):
    return np.zeros(n, np.uint16), np.asarray(ids, np.uint32)[np.arange(n) % len(ids)]


_REFS: dict = {}


def references(host, key, pols, reqs, red, rem):
    """(host decoder records, oracle records) of reqs under pols, computed
    once per key and never changed."""
    if key not in _REFS:
        host.update_kafka_policy(pols)
        raw, off = K.concat(reqs)
        h = records_view(*host.kafka_decode(raw, off, red, rem, diag_cpu=True))
        o = oracle_view([R.decode(r) for r in reqs], red, rem, host.kafka_intern)
        _REFS[key] = (h, o)
    return _REFS[key]


def decode_dev(gpu, reqs, lead, red, rem):
    """cg_kafka_decode_dev on reqs placed `lead` bytes past a 16-byte
    boundary of device memory → records_view tuples."""
    import torch
    raw, off = K.concat(reqs)
    n, tot = len(reqs), int(off[-1])
    dev = torch.device("cuda:0")
    buf = torch.zeros(lead + max(tot, 1), dtype=torch.uint8, device=dev)
    if tot:
        buf[lead:lead + tot] = torch.from_numpy(raw[:tot].copy()).to(dev)
    d_raw = buf[lead:]
    assert d_raw.data_ptr() % 16 == lead
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    d_red = torch.from_numpy(np.ascontiguousarray(red, np.uint16).view(np.int16).copy()).to(dev)
    d_rem = torch.from_numpy(np.ascontiguousarray(rem, np.uint32).view(np.int32).copy()).to(dev)
    d_reqs = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    cap = tot // 2 + 16
    arena = torch.zeros(cap, dtype=torch.int32, device=dev)
    gpu.kafka_decode_dev(d_raw, d_off, n, d_red, d_rem, d_reqs, arena, cap, d_st,
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return records_view(d_reqs.cpu().numpy().view(KAFKA_REQ_DTYPE), arena.cpu().numpy().view(np.uint32),
                        d_st.cpu().numpy())


def decode_stats(gpu):
    """(device_inflated, host_deferred, unreserved) counters of the handle."""
    import ctypes as C
    i, d, u = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert N.lib.cg_kafka_decode_stats(gpu.h, C.byref(i), C.byref(d)) == N.CG_OK
    assert N.lib.cg_kafka_inflate_stats(gpu.h, C.byref(u)) == N.CG_OK
    return i.value, d.value, u.value


def first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return i, g, w
    return None if len(got) == len(want) else (min(len(got), len(want)), None, None)


def base_policy():
    """The rule set of the decoder parity tests: (policies, topics, clients, ids)."""
    pols, info = synth.kafka_policy(n_rules=200, n_topics=60, n_clients=12, seed=5)
    return pols, [t.encode() for t in info["topics"]], [c.encode() for c in info["clients"]], info["ids"]


def _bytes(n: int, salt: int) -> bytes:
    """n bytes that depend on every index (no run a wrong CRC table would survive)."""
    return ((np.arange(n, dtype=np.uint64) * 0x9E3779B1 + salt * 0x85EBCA6B >> 7) & 0xFF).astype(np.uint8).tobytes()


def plain_produce(client: bytes, topic: bytes, vlen: int, version: int = 0) -> bytes:
    """A well-formed produce request: one topic, one partition, one
    uncompressed message with a value of vlen bytes."""
    return K.produce(version, client, [(topic, [(0, [(None, _bytes(vlen, vlen))])])])


def produce_exact(nbytes: int, client: bytes, topic: bytes) -> bytes:
    base = len(plain_produce(client, topic, 0))
    assert nbytes >= base, (nbytes, base)
    r = plain_produce(client, topic, nbytes - base)
    assert len(r) == nbytes
    return r


# ------------------------------------------------- corpus 1: the stage ----
def stage_model(lens, lead: int, S: int):
    """kafka_decode_kernel's stage window per 64-request group for a buffer
    whose address is `lead` mod 16 → (staged[i], ends_at_hi[i])."""
    n = len(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    staged, at_hi = np.zeros(n, bool), np.zeros(n, bool)
    for g in range(0, n, 64):
        last = min(g + 63, n - 1)
        start, end = int(off[g]), int(off[last + 1])
        lo = start - ((lead + start) & 15)
        hi = max(end, start)
        hi = lo + ((hi - lo + 15) & ~15)
        hi = min(hi, lo + S)
        for i in range(g, last + 1):
            a, ln = int(off[i]), int(lens[i])
            staged[i] = a >= lo and a + ln <= hi
            at_hi[i] = a + ln == hi
    return staged, at_hi


class StageCorpus:
    """reqs: the layouts back to back, each whole 64-request groups whose
    bytes total a multiple of 16 (so a group starts `lead` past a 16-byte
    boundary of memory); first[name]: a layout's first request; k[name]: the
    request aimed at the boundary."""

    def __init__(self):
        self.reqs, self.first, self.k = [], {}, {}

    def add(self, name, group, k=None):
        assert len(group) % 64 == 0
        self.first[name] = len(self.reqs)
        if k is not None:
            self.k[name] = len(self.reqs) + k
        self.reqs += group


def _mixed(rng, topics, clients, hint: int) -> bytes:
    """A metadata, fetch or plain produce request of about hint bytes, 30 % mutated."""
    kind = int(rng.integers(0, 3))
    client = clients[int(rng.integers(0, len(clients)))]

    def pick(n):
        return [topics[int(rng.integers(0, len(topics)))] for _ in range(n)]
    if kind == 0:
        r = K.metadata(int(rng.integers(0, 5)), client, pick(max(1, min(hint // 10, 40))))
    elif kind == 1:
        r = K.fetch(int(rng.integers(0, 8)), client, [(t, [0]) for t in pick(max(1, min(hint // 30, 20)))])
    else:
        nm = int(rng.integers(1, 4))
        msgs = [(None if rng.random() < 0.7 else b"k%d" % j,
                 bytes(rng.integers(0, 256, max(0, (hint - 60) // nm), np.uint8))) for j in range(nm)]
        r = K.produce(int(rng.integers(0, 4)), client, [(pick(1)[0], [(0, msgs)])])
    return mutate(rng, r) if rng.random() < 0.3 else r


def _fill(rng, topics, clients, count: int, budget: int, hint: int):
    """count mixed requests of at most budget bytes together."""
    small = K.metadata(0, b"", [topics[0]])
    out, tot = [], 0
    for j in range(count):
        r = _mixed(rng, topics, clients, hint)
        if tot + len(r) + (count - j - 1) * len(small) > budget:
            r = small
        out.append(r)
        tot += len(r)
    assert tot <= budget, (tot, budget)
    return out


def _closing(group, client, topic) -> bytes:
    """A plain produce request that brings the group's bytes to a multiple of 16."""
    tot = sum(len(r) for r in group)
    base = len(plain_produce(client, topic, 0))
    return produce_exact(base + (-(tot + base)) % 16, client, topic)


def stage_layouts(S: int) -> StageCorpus:
    pols, topics, clients, ids = base_policy()
    rng = np.random.default_rng(0x57A6E + S)
    c, t = clients[0], topics[1]
    sc = StageCorpus()
    tail_hint = 60

    def close(group):
        group.append(_closing(group, c, t))
        assert len(group) % 64 == 0 and sum(len(r) for r in group) % 16 == 0
        return group

    def total(group):
        return sum(len(r) for r in group)

    # L1: all 64 inside the stage
    g = _fill(rng, topics, clients, 63, S - 160, (S - 160) // 63 - 16)
    close(g)
    assert total(g) <= S - 16
    sc.add("L1", g)

    def boundary(name, k_end, k_len):
        """Requests k-1, k, k+1 are plain produce requests, k of k_len bytes
        ending k_end bytes after the group's start."""
        g = _fill(rng, topics, clients, 31, S - 900, (S - 900) // 31 - 16)
        g.append(produce_exact(k_end - k_len - total(g), c, t))
        g.append(produce_exact(k_len, clients[1], topics[2]))
        assert total(g) == k_end
        g.append(produce_exact(150, clients[2], topics[3]))
        g += _fill(rng, topics, clients, 29, 29 * 4 * tail_hint, tail_hint)
        sc.add(name, close(g), 32)

    # L2: request 32 straddles start + S
    boundary("L2", S + 200, 300)
    # L3: request 32 ends d bytes before start + S, request 33 starts there
    for d in (0, 8, 15, 16):
        boundary("L3_%d" % d, S - d, 200)
    # L4: the first request alone is longer than the stage
    g = [produce_exact(S + 37, c, t)] + _fill(rng, topics, clients, 62, 62 * 4 * tail_hint, tail_hint)
    sc.add("L4", close(g), 0)
    # L5: zero-length requests at lanes 0, 31 and 63; then a whole wave of them
    body = _fill(rng, topics, clients, 60, 60 * 4 * tail_hint, tail_hint)
    g = [b""] + body[:30] + [b""] + body[30:]
    g.append(_closing(g, c, t))
    g.append(b"")
    assert len(g) == 64 and g[0] == g[31] == g[63] == b"" and total(g) % 16 == 0
    sc.add("L5", g + [b""] * 64)
    # L6: lengths 0 and 1 only, under 16 bytes in the wave (last: it ends the alignment)
    g = [bytes([7 * j & 0xFF]) if j % 7 == 3 else b"" for j in range(64)]
    assert 0 < total(g) < 16
    sc.add("L6", g)
    return sc


STAGE_CUTS = (1, 63, 64, 65, 129)  # L7: ragged ends, the last two a final group of one


# ------------------------------------------------ corpus 2: CRC shapes ----
CRC_VLENS = tuple(range(25))
CRC_CLIENTS = (b"", b"a", b"ab", b"abc")


def crc_message(v: int, c: int, version: int) -> bytes:
    """The message under test: CRC over 10 + v bytes (v0) or 18 + v (v1)."""
    return K.message(None, _bytes(v, 31 * v + 7 * c + version), 0, 0, None if version == 0 else 0)


def crc_region(req: bytes, msg: bytes):
    """(offset, length) of msg's CRC-covered bytes inside req."""
    return req.index(msg) + 16, len(msg) - 16


def _two_topic_produce(version: int, client: bytes, topics, ms: bytes) -> bytes:
    """Produce: topics[0] with one partition holding ms, then topics[1]
    without partitions (what a set that stopped early is misread into)."""
    body = (K.string(b"") if version >= 3 else b"") + K.i16(1) + K.i32(1000) + K.i32(2)
    body += K.string(topics[0]) + K.i32(1) + K.i32(0) + K.i32(len(ms)) + ms + K.string(topics[1]) + K.i32(0)
    return K._request(K.PRODUCE, version, client, body)


def poison_message(version: int) -> bytes:
    """A message with a good CRC whose key length exceeds maxParseBufSize:
    a decode error, if the parser gets as far as reading it."""
    body = K.i8(0 if version == 0 else 1) + K.i8(0) + (K.i64(0) if version >= 1 else b"") + K.i32(MAX_PARSE_BUF + 1)
    m = struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF) + body
    return K.i64(1) + K.i32(len(m)) + m


def crc_shapes(topics):
    """(v, c, version, message) for every shape, in request order."""
    return [(v, c, ver, crc_message(v, c, ver)) for ver in (0, 1) for c in range(len(CRC_CLIENTS)) for v in CRC_VLENS]


def crc_requests(topics):
    return [_two_topic_produce(ver, CRC_CLIENTS[c], topics[:2], m + TERMINATOR) for v, c, ver, m in crc_shapes(topics)]


def crc_staged(topics):
    """Request 3 * j is shape j; two zero-length requests follow each, so
    that a wave's 64 requests fit the 4 KiB stage."""
    return [x for r in crc_requests(topics) for x in (r, b"", b"")]


def crc_unstaged(topics, S: int = 4096):
    """The same requests, every wave led by a request longer than the stage."""
    out = []
    for j, r in enumerate(crc_requests(topics)):
        if j % 63 == 0:
            out.append(produce_exact(S + 64 + j % 5, b"lead", topics[2]))
        out.append(r)
    return out


def crc_inner(topics, codec: int, big: bool, poison: bool):
    """Each shape as the inner set of a gzip / snappy wrapper: alone (decoded
    into LDS), or behind a message of 300 + c value bytes (decoded into the
    arena, and moved by c)."""
    out = []
    for v, c, ver, m in crc_shapes(topics):
        ts = None if ver == 0 else 0
        inner = (K.message(None, _bytes(300 + c, v), 0, 0, ts) if big else b"") + m + (poison_message(ver) if poison else b"")
        assert (len(inner) > KINF_LDS) == big
        val = gzip.compress(inner, mtime=0) if codec == K.CODEC_GZIP else K.snappy_block(inner)
        out.append(_two_topic_produce(ver, CRC_CLIENTS[c], topics[:2], K.message(None, val, codec, 0, ts) + TERMINATOR))
    return out


def crc_inner_all(topics):
    """→ (requests, poisoned[i])."""
    reqs, poisoned = [], []
    for codec in (K.CODEC_GZIP, K.CODEC_SNAPPY):
        for big in (False, True):
            for poison in (False, True):
                part = crc_inner(topics, codec, big, poison)
                reqs += part
                poisoned += [poison] * len(part)
    return reqs, poisoned


# -------------------------------------------- corpus 3: inflate shapes ----
INFLATE_SIZES = (26, 255, 256, 257, 260, 261, 512, 4096, 40_000, 70_000)
_WORDS = [b"topic", b"kafka", b"cilium", b"message", b"\x00\x01", b"value-", b"key"]


def _content(rng, kind: str, n: int) -> bytes:
    text = b"".join(_WORDS[int(i)] for i in rng.integers(0, len(_WORDS), max(1, n // 2 + 1)))[:n]
    noise = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "text":
        return text
    if kind == "noise":
        return noise
    return bytes(a if rng.random() < 0.7 else b for a, b in zip(text, noise)) if n <= 5000 else text[:n // 2] + noise[:n - n // 2]


ENCODERS = [
    ("deflate-0", 1, lambda d: _gz_raw(d, 0)),
    ("deflate-1", 1, lambda d: _gz_raw(d, 1)),
    ("deflate-6", 1, lambda d: _gz_raw(d, 6)),
    ("deflate-9", 1, lambda d: _gz_raw(d, 9)),
    ("fixed", 1, lambda d: _gz_raw(d, 6, zlib.Z_FIXED)),
    ("huffman-only", 1, lambda d: _gz_raw(d, 6, zlib.Z_HUFFMAN_ONLY)),
    ("rle", 1, lambda d: _gz_raw(d, 6, zlib.Z_RLE)),
    ("header-fields", 1, lambda d: _gz_raw(d, 6, extra=b"xy" * 3, name=b"set.bin", comment=b"c", fhcrc=True)),
    ("gzip", 1, lambda d: gzip.compress(d, mtime=0)),
    ("snappy", 2, K.snappy_block),
    ("xerial-8", 2, lambda d: K.snappy_xerial(d, 8)),
    ("xerial-64", 2, lambda d: K.snappy_xerial(d, 64)),
    ("xerial-4096", 2, lambda d: K.snappy_xerial(d, 4096)),
]


def _produce_sets(client: bytes, topic_sets) -> bytes:
    """Produce v0: per topic, one partition per message set."""
    body = K.i16(-1) + K.i32(5000) + K.i32(len(topic_sets))
    for t, sets in topic_sets:
        body += K.string(t) + K.i32(len(sets)) + b"".join(K.i32(p) + K.i32(len(ms)) + ms for p, ms in enumerate(sets))
    return K._request(K.PRODUCE, 0, client, body, 7)


_INFLATE: dict = {}


def inflate_shapes(topics, clients):
    """→ (requests, wrappers, decoded_bytes): every request well-formed, every
    compressed payload one the device must finish alone."""
    if "ok" in _INFLATE:
        return _INFLATE["ok"]
    rng = np.random.default_rng(0x1F1A7E)
    inners = []
    for L in INFLATE_SIZES:
        for kind in ("text", "noise", "mixed"):
            inner = K.message(None, _content(rng, kind, L - 26), 0, 0)
            assert len(inner) == L
            inners.append(inner)
    # sets of several messages
    inners.append(b"".join(K.message(None, _content(rng, "text", 40), 0, o) for o in range(5)))
    inners.append(b"".join(K.message(b"key-%d" % o, _content(rng, "mixed", 7 * o), 0, o) for o in range(40)))
    inners.append(b"".join(K.message(None, _content(rng, "noise", 1000), 0, o) for o in range(9)))
    wrappers = [(len(inner), K.message(None, enc(inner), codec, 0)) for inner in inners for _, codec, enc in ENCODERS]
    order = rng.permutation(len(wrappers))
    reqs = [_produce_sets(clients[int(j) % len(clients)], [(topics[int(j) % len(topics)], [wrappers[int(j)][1]])])
            for j in order]
    count, decoded = len(wrappers), sum(n for n, _ in wrappers)
    small = [(n, w) for n, w in wrappers if n <= 4096]
    # several partitions, each holding a compressed set
    for j in range(12):
        pick = [small[(5 * j + 17 * p) % len(small)] for p in range(3)]
        reqs.append(_produce_sets(clients[j % len(clients)], [(topics[j], [w for _, w in pick])]))
        count, decoded = count + 3, decoded + sum(n for n, _ in pick)
    # 13-20 topics: the ids go to the topic arena in a second pass
    for nt in range(13, 21):
        pick = [small[(nt * 29 + 7 * q) % len(small)] for q in range(nt)]
        reqs.append(_produce_sets(clients[nt % len(clients)],
                                  [(topics[(nt + 3 * q) % len(topics)], [w]) for q, (_, w) in enumerate(pick)]))
        count, decoded = count + nt, decoded + sum(n for n, _ in pick)
    _INFLATE["ok"] = (reqs, count, decoded)
    return _INFLATE["ok"]


def inflate_deferred(topics, clients):
    """Requests the device may not finish: a second gzip member, and a
    compressed set inside a compressed set."""
    reqs = []
    plain = b"".join(K.message(None, b"value-%d" % o * 9, 0, o) for o in range(12))
    for cut in (len(plain) // 2, 26 * 3, len(plain) - 30):
        two = gzip.compress(plain[:cut], mtime=0) + gzip.compress(plain[cut:], mtime=0)
        reqs.append(_produce_sets(clients[0], [(topics[0], [K.message(None, two, K.CODEC_GZIP, 0)])]))
    big = b"".join(K.message(None, _bytes(700, o), 0, o) for o in range(4))
    two = _gz_raw(big[:1452], 6) + _gz_raw(big[1452:], 0)
    reqs.append(_produce_sets(clients[1], [(topics[1], [K.message(None, two, K.CODEC_GZIP, 0)])]))
    for outer in (K.CODEC_GZIP, K.CODEC_SNAPPY):
        for inner in (K.CODEC_GZIP, K.CODEC_SNAPPY):
            for body in (plain[:52], big):
                iv = gzip.compress(body, mtime=0) if inner == K.CODEC_GZIP else K.snappy_block(body)
                im = K.message(None, iv, inner, 0)
                ov = gzip.compress(im, mtime=0) if outer == K.CODEC_GZIP else K.snappy_block(im)
                reqs.append(_produce_sets(clients[2], [(topics[2], [K.message(None, ov, outer, 0)])]))
    return reqs


# ---------------------------------------------------- corpus 4: intern ----
INTERN_LENS = (1, 15, 16, 17, 31, 32, 33, 64, 255)  # 255: the longest topic a rule may name
PAIR = (b"orders.eu-west.1zqdz", b"orders.eu-west.12wlt")  # equal FNV-1a, length and first 16 bytes
PAIR_HASH = 146151182
_ALPHABET = b"abcdefghijklmnopqrstuvwxyz0123456789._-ABCDEFGHIJKLMNOPQRSTUVWXYZ"


def _name(prefix: bytes, n: int) -> bytes:
    return (prefix + _ALPHABET * 5)[:n]


def wrap_names(prefix: bytes, cap: int, count: int = 3):
    """Names whose home slot is the last of a table of cap slots."""
    out, i = [], 0
    while len(out) < count:
        s = prefix + b"wrap.%d" % i
        if fnv1a(s) & (cap - 1) == cap - 1:
            out.append(s)
        i += 1
    return out


def intern_strings(prefix: bytes, both: bool):
    n = len(INTERN_LENS) + 3 + (2 if both else 1)
    return [_name(prefix, k) for k in INTERN_LENS] + wrap_names(prefix, dict_capacity(n)) + list(PAIR[:2 if both else 1])


def intern_policy(both: bool):
    """→ (policies, rule topics, rule clientIDs): `both` names the second
    string of PAIR too."""
    topics, clients = intern_strings(b"t", both), intern_strings(b"c", both)
    rules = [{"topic": t.decode(), "apiKey": "fetch"} for t in topics] + [{"clientID": c.decode()} for c in clients]
    return [{"name": "edges", "selectors": [{"identities": None, "rules": rules}]}], topics, clients


def near_misses(s: bytes):
    out = []
    for i in (0, 15, 16, len(s) - 1):
        if i < len(s):
            out.append(s[:i] + bytes([s[i] ^ 1]) + s[i + 1:])
    return out + [s[:-1], s + b"x"]


def intern_candidates(rule_strings):
    """The rule strings, PAIR, their near misses, the empty string and a
    300-byte one; no duplicates, in a fixed order."""
    out = list(rule_strings) + list(PAIR)
    for s in list(rule_strings) + list(PAIR):
        out += near_misses(s)
    out += [b"", _name(b"long.", 300)]
    return list(dict.fromkeys(out))


def intern_requests(both: bool):
    """→ (requests, topic candidates, client candidates)."""
    _, topics, clients = intern_policy(both)
    tc, cc = intern_candidates(topics), intern_candidates(clients)
    reqs = []
    for j in range(0, len(tc), 12):  # inline topic ids
        chunk = tc[j:j + 12]
        reqs.append(K.metadata(1, cc[j % len(cc)], chunk))
        reqs.append(K.fetch(2, cc[(j + 1) % len(cc)], [(t, [0]) for t in chunk]))
    reqs.append(K.metadata(0, clients[0], tc))  # through the arena
    reqs.append(K.fetch(0, PAIR[1], [(t, [0]) for t in tc]))
    for j, c in enumerate(cc):  # every clientID candidate
        reqs.append(K.metadata(0, c, [tc[j % len(tc)]]))
    return reqs, tc, cc
