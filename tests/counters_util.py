"""What the kernels' counters must hold, worked out without the kernels.

HTTP: http_kernel counts {allowed, denied} per program.  Which program a
request runs under is the packer's decision, recorded in the packed batch
(csrc/dev_types.h: HttpBatchHeader, HttpChunk, HttpTile; the meta block's
flags, include/cilium_gpu.h CG_HTTP_F_*).  program_of_slots reads it back
from the bytes; expected_program_counters joins it with the oracle's
verdicts.  Kafka, L4 and the prefilter need no batch: their counters are
keyed by values the requests carry."""
import numpy as np

NO_REQ = 0xFFFFFFFF
F_MALFORMED, F_PAD = 0x04, 0x08  # CG_HTTP_F_MALFORMED, CG_HTTP_F_PAD
HDR_BYTES, CHUNK_BYTES, TILE_LANES, META_BYTES, GRANULE = 64, 16, 64, 8, 512


def batch_header(b):
    """HttpBatchHeader fields of a packed batch."""
    u32 = b.batch[:16].view(np.uint32)
    u64 = b.batch[16:56].view(np.uint64)
    return dict(magic=int(u32[0]), epoch=int(u32[1]), nchunks=int(u32[2]), ntiles=int(u32[3]),
                tiles_off=int(u64[0]), nslots=int(u64[1]), ttab_off=int(u64[2]), total_bytes=int(u64[3]),
                arena_bytes=int(u64[4]))


def chunk_table(b):
    """(nchunks, 4) u32: {prog, first_tile, ntiles, pad} per chunk."""
    h = batch_header(b)
    return b.batch[HDR_BYTES:HDR_BYTES + CHUNK_BYTES * h["nchunks"]].view(np.uint32).reshape(-1, 4)


def _tile_table(b):
    h = batch_header(b)
    assert h["nslots"] == b.nslots == h["ntiles"] * TILE_LANES
    return h, b.batch[h["ttab_off"]:h["ttab_off"] + 8 * h["ntiles"]].view(np.uint32).reshape(-1, 2)


def flags_of_slots(b):
    """Per slot the CG_HTTP_F_* flags of its record: meta[lane].y >> 24 of the
    tile's meta block at tiles_off + at * 512."""
    h, ttab = _tile_table(b)
    flags = np.zeros((h["ntiles"], TILE_LANES), np.uint32)
    for t in range(h["ntiles"]):
        at = h["tiles_off"] + int(ttab[t, 0]) * GRANULE
        meta = b.batch[at:at + TILE_LANES * META_BYTES].view(np.uint32).reshape(TILE_LANES, 2)
        flags[t] = meta[:, 1] >> 24
    return flags.reshape(-1)


def program_of_slots(b, nprogs):
    """Per slot of the batch: the program index its chunk names (0xFFFFFFFE /
    0xFFFFFFFF: the special programs "no policy for the port" / "unknown
    policy") and whether the kernel counts it: a real request (order[slot] is
    a request), neither padding nor malformed, under a program of the
    snapshot."""
    h, _ = _tile_table(b)
    tile_prog = np.full(h["ntiles"], 0xFFFFFFFF, np.uint32)
    seen = np.zeros(h["ntiles"], bool)
    for prog, first, nt, _ in chunk_table(b):
        assert first + nt <= h["ntiles"] and not seen[first:first + nt].any()  # every tile in one chunk
        seen[first:first + nt] = True
        tile_prog[first:first + nt] = prog
    assert seen.all()
    flags = flags_of_slots(b)
    prog = np.repeat(tile_prog, TILE_LANES)
    order = np.asarray(b.order[:b.nslots])
    pad = (flags & F_PAD) != 0
    assert np.array_equal(pad, order == NO_REQ)  # padding slots, and only they, belong to no request
    counted = ~pad & ((flags & F_MALFORMED) == 0) & (prog < nprogs)
    return prog, counted


def program_of_requests(b, nprogs):
    """program_of_slots in request order: (program, counted) per request."""
    prog, counted = program_of_slots(b, nprogs)
    order = np.asarray(b.order[:b.nslots])
    real = order != NO_REQ
    assert np.array_equal(np.sort(order[real]), np.arange(b.n, dtype=order.dtype))  # each request in one slot
    rprog = np.zeros(b.n, np.uint32)
    rcnt = np.zeros(b.n, bool)
    rprog[order[real]] = prog[real]
    rcnt[order[real]] = counted[real]
    return rprog, rcnt


def program_counters(req_prog, req_counted, verdicts, nprogs):
    """[2p] allowed, [2p + 1] denied over the counted requests of program p."""
    v = np.asarray(verdicts).astype(bool)
    out = np.zeros(2 * nprogs, np.uint64)
    idx = 2 * req_prog[req_counted].astype(np.int64) + (~v[req_counted]).astype(np.int64)
    out += np.bincount(idx, minlength=2 * nprogs).astype(np.uint64)
    return out


def expected_program_counters(b, verdicts, nprogs):
    """The CG_CTR_HTTP_PROGRAMS vector the kernel must hold after one run of
    batch b from zeroed counters, given the requests' verdicts (request order)."""
    return program_counters(*program_of_requests(b, nprogs), verdicts, nprogs)


def rule_groups(info):
    """http_rule_info grouped by (policy, ingress, port): per rule counter the
    index of its group, having checked that every group is one contiguous
    range (so ranges of different programs are disjoint)."""
    key = np.stack([info["policy"], info["ingress"], info["port"]], 1).astype(np.int64)
    start = np.ones(len(key), bool)
    start[1:] = (key[1:] != key[:-1]).any(1)
    group = np.cumsum(start) - 1
    firsts = [tuple(k) for k in key[start]]
    assert len(set(firsts)) == len(firsts), "a program's rule counters are not contiguous"
    return group


def kafka_redirect_counters(redirect, verdicts, nredirects):
    """[2r] allowed, [2r + 1] denied among the requests naming redirect r;
    requests naming a redirect the snapshot does not have count nowhere."""
    red = np.asarray(redirect, np.int64)
    v = np.asarray(verdicts).astype(bool)
    known = red < nredirects
    out = np.zeros(2 * nredirects, np.uint64)
    out += np.bincount(2 * red[known] + (~v[known]).astype(np.int64), minlength=2 * nredirects).astype(np.uint64)
    return out


def l4_entry_counters(pm, keys):
    """(Packets, Bytes) of every key, in keys' order, from one dump_to_slice()."""
    dump = {(k.Identity, k.DestPort, k.Nexthdr, k.TrafficDirection): e for k, e in pm.dump_to_slice()}
    ents = [dump[(int(k["sec_label"]), int(k["dport"]), int(k["protocol"]), int(k["egress"]))] for k in keys]
    return (np.array([e.Packets for e in ents], np.uint64), np.array([e.Bytes for e in ents], np.uint64))
