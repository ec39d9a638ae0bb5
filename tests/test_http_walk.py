"""http_walk.h on the host.  The header is host+device and
cg_diag_http_eval_host is one lane of http_kernel_global built from it, so
these run the kernels' own walk code without a GPU: the functions alone
(tests/native/http_walk_test.cc, built with hipcc's host compiler), a program
of more than four mask words against the oracle, and the kernels' handling of
a batch that cg_http_pack would not produce, on packed batches edited in
place."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from test_cpu_differential import all_matcher_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_HIT = 0xFFFFFFFF


def test_http_walk_functions_on_host(tmp_path):
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("no hipcc")
    exe = str(tmp_path / "http_walk_test")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17",
                    "-I", os.path.join(ROOT, "cilium_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "http_walk_test.cc"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "http_walk ok" in r.stdout


def _prefix_policy(n_rules, word_len, seed=1):
    """One program of n_rules path prefixes "/<word>" for remote 7."""
    r = random.Random(seed)
    al = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
    words = ["".join(r.choice(al) for _ in range(word_len)) for _ in range(n_rules)]
    rules = [{"headers": [{"name": ":path", "regex_match": "/" + w + ".*"}]} for w in words]
    return [{"name": "big", "policy": 1, "ingress_per_port_policies": [{"port": 80, "rules": [
        {"remote_policies": [7], "http_rules": {"http_rules": rules}}]}]}], words


def _requests(paths, remotes):
    lists = [b":method\0GET\0:path\0" + p + b"\0" for p in paths]
    n = len(lists)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return dict(policy=np.zeros(n, np.uint32), ingress=np.ones(n, np.uint8), port=np.full(n, 80, np.uint16),
                remote=np.asarray(remotes, np.uint32), hdr_blob=np.frombuffer(b"".join(lists), np.uint8).copy(),
                hdr_off=off)


def _word_requests(words, n, seed=5):
    """"/<word>/<i>": every word in turn, 30% with its last letter spoiled,
    every ninth from remote 5, which no rule selects."""
    rng = np.random.default_rng(seed)
    paths = []
    for i in range(n):
        w = words[i % len(words)]
        if rng.random() < 0.3:
            w = w[:-1] + "_"
        paths.append(b"/%s/%d" % (w.encode(), i))
    return _requests(paths, np.where(np.arange(n) % 9 == 8, 5, 7))


def _tables(b):
    """Views into a packed batch (dev_types.h HttpBatchHeader): the chunk
    table rows {prog, first_tile, ntiles, pad}, the tile table rows {at,
    units}, and the byte offset of the tile data.  Writes go to the batch."""
    u32, u64 = b.batch[:64].view(np.uint32), b.batch[:64].view(np.uint64)
    nchunks, ntiles, tiles_off, ttab_off = int(u32[2]), int(u32[3]), int(u64[2]), int(u64[4])
    chunks = b.batch[64:64 + 16 * nchunks].view(np.uint32).reshape(-1, 4)
    ttab = b.batch[ttab_off:ttab_off + 8 * ntiles].view(np.uint32).reshape(-1, 2)
    return chunks, ttab, tiles_off


def test_program_of_five_mask_words(host):
    """257 rules: W = 5, first_meet's default branch (the GPU suite reaches it
    with 513 and more rules; no other CPU test has more than 256 rules in a
    program).  Verdicts against the oracle, and some request's first rule is
    rule 256, the only bit of the last word."""
    pols, words = _prefix_policy(257, 3)
    host.update_http_policy(pols)
    assert host.http_policy_stats()["rules"] == 257
    rq = _word_requests(words, 257 * 6)
    b = host.pack_http(**rq)
    want = oracle.HttpOracle(pols).eval(**rq)
    assert np.array_equal(host.http_eval_host_diag(b), want)
    rules = host.http_rules_host_diag(b)
    assert np.array_equal(rules != NO_HIT, want.astype(bool))
    hit = rules[rules != NO_HIT] - rules[rules != NO_HIT].min()
    assert hit.max() == 256 and len(np.unique(hit)) > 200


def test_overflow_entry_past_the_arena(host):
    """Table row 1: an overflow entry reaching past arena_bytes ends in the
    dead state, so no HTTP rule allows the request, but the always mask (a
    PNPR without HTTP rules, remote 8 here) still does."""
    pols = [{"name": "ov", "policy": 1, "ingress_per_port_policies": [{"port": 80, "rules": [
        {"remote_policies": [7], "http_rules": {"http_rules": [
            {"headers": [{"name": ":path", "regex_match": "/ok/.*"}]}]}},
        {"remote_policies": [8]}]}]}]
    host.update_http_policy(pols)
    paths = [(b"/ok/" if i % 2 else b"/no/") + b"q" * (150 + i) for i in range(60)]
    rq = _requests(paths, [(7, 8, 9)[i % 3] for i in range(60)])
    b = host.pack_http(**rq)
    want = oracle.HttpOracle(pols).eval(**rq)
    assert np.array_equal(host.http_eval_host_diag(b), want)
    assert want[rq["remote"] == 7].any() and not want[rq["remote"] == 7].all() and want[rq["remote"] == 8].all()
    _, ttab, tiles_off = _tables(b)
    moved = 0
    for at in ttab[:, 0]:
        meta = b.batch[tiles_off + 512 * int(at):tiles_off + 512 * int(at) + 512].reshape(64, 8)
        ov = (meta[:, 7] & 0x02) != 0  # CG_HTTP_F_OVERFLOW
        meta[ov, 4:7] = 0xFF  # offset / 16 = 0xFFFFFF: 256 MiB, past any arena
        moved += int(ov.sum())
    assert moved == 60
    assert np.array_equal(host.http_eval_host_diag(b), (rq["remote"] == 8).astype(np.uint8))


def _matcher_batch(host):
    pols, rq, _ = all_matcher_case(0, 6000)
    host.update_http_policy(pols)
    b = host.pack_http(**rq)
    base = host.http_eval_host_diag_slots(b)
    chunks, ttab, _ = _tables(b)
    # a chunk of a walked program with both verdicts in it, and kChunkTiles +
    # 1 tiles from its first still inside the tile table
    nprogs = host.http_policy_stats()["programs"]
    for c, (prog, first, nt, _pad) in enumerate(chunks.tolist()):
        sl = slice(64 * first, 64 * (first + nt))
        if prog < nprogs and first + 65 <= len(ttab) and base[sl].any() and not base[sl].all():
            return b, base, chunks, c, sl, nprogs
    raise AssertionError("no such chunk")


@pytest.mark.parametrize("edit", ["ntiles", "first_tile", "prog"])
def test_malformed_chunk(host, edit):
    """Table rows 2 and 3: a chunk of kChunkTiles + 1 tiles, or one reaching
    past the tile table, is skipped: its slots stay 0 and no tile of it is
    read.  A chunk whose program id is nprogs is denied.  The other chunks'
    verdicts stay."""
    b, base, chunks, c, sl, nprogs = _matcher_batch(host)
    if edit == "ntiles":
        chunks[c, 2] = 64 + 1
    elif edit == "first_tile":
        chunks[c, 1] = len(base) // 64 - chunks[c, 2] + 1
    else:
        chunks[c, 0] = nprogs
    want = base.copy()
    want[sl] = 0
    assert np.array_equal(host.http_eval_host_diag_slots(b), want)


def test_half_tile_in_the_generic_walker(host):
    """Table row 6: cg_http_pack gives half last units only to one-part LDS
    programs; http_tiles, which walks every other program, denies a tile
    with kTileHalfLast unwalked.  734 rules: one program too large for LDS
    (and W = 12)."""
    pols, words = _prefix_policy(734, 12)
    host.update_http_policy(pols)
    assert host.http_policy_stats()["lds_programs"] == 0
    rq = _word_requests(words, 734 * 2)
    b = host.pack_http(**rq)
    assert np.array_equal(host.http_eval_host_diag(b), oracle.HttpOracle(pols).eval(**rq))
    base = host.http_eval_host_diag_slots(b)
    _, ttab, _ = _tables(b)
    assert not (ttab[:, 1] & 0x8000).any()
    t = 1
    assert (ttab[t, 1] & 0x7FFF) > 0 and base[64 * t:64 * t + 64].any()
    ttab[t, 1] |= 0x8000  # kTileHalfLast
    want = base.copy()
    want[64 * t:64 * t + 64] = 0
    assert np.array_equal(host.http_eval_host_diag_slots(b), want)
