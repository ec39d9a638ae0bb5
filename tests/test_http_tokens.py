"""Literal tokens (csrc/clsdfa.h pick_tokens, cg_http_pack): a class-mode
program spends its free class codes on literals of its rules, each one more
column of its table with δ(S, token) = δ*(S, the token's classes), and the
packer writes a literal it finds as that one symbol.  Whatever the packer
tokenizes, a string ends in the state its plain class codes end in, so the
verdicts of the tokenized batch, of the CILIUM_GPU_PACK_TOKENS=0 batch and of
the oracle are the same, request for request."""
import numpy as np
import pytest

import oracle
from cilium_amd import synth
from cilium_amd.classifier import Classifier
from cilium_amd.policy import (PortRuleHTTP, get_http_rule, network_policy, port_network_policy,
                               port_network_policy_rule)
from counters_util import GRANULE, META_BYTES, TILE_LANES, batch_header, flags_of_slots

F_OVERFLOW = 0x02  # CG_HTTP_F_OVERFLOW
SLOT_BYTES = 128   # CG_HTTP_SLOT_BYTES
# dev_types.h kTwoWgLdsCells: two workgroups' LDS in one CU's 160 KiB,
# (lds_cells + 64 + kLdsRuleHits + 3) * 4 <= 80 KiB with lds_cells a multiple of 256
TWO_WG_CELLS = (80 * 1024 // 4 - 64 - 512 - 3) & ~255


def pack(cl, rq, monkeypatch, tokens):
    if tokens:
        monkeypatch.delenv("CILIUM_GPU_PACK_TOKENS", raising=False)
    else:
        monkeypatch.setenv("CILIUM_GPU_PACK_TOKENS", "0")
    b = cl.pack_http(**rq)
    monkeypatch.delenv("CILIUM_GPU_PACK_TOKENS", raising=False)
    return b


def tile_table(b):
    h = batch_header(b)
    t = b.batch[h["ttab_off"]:h["ttab_off"] + 8 * h["ntiles"]].view(np.uint32).reshape(-1, 2)
    units = (t[:, 1] & 0x7FFF).astype(np.int64)
    half = ((t[:, 1] >> 15) & 1).astype(np.int64)
    return h, t[:, 0].astype(np.int64), units, half


def tile_bytes_per_slot(b):
    """Σ granules · 512 / slots over the tile table (dev_types.h tile_granules)."""
    h, _, units, half = tile_table(b)
    return float((1 + 2 * units - half).sum()) * GRANULE / h["nslots"]


def strings_of_requests(b):
    """Per request the bytes its slot holds in the tile's string units (the
    coded string, then zero padding up to the tile's last unit)."""
    h, at, units, half = tile_table(b)
    out = {}
    for t in range(h["ntiles"]):
        base = h["tiles_off"] + int(at[t]) * GRANULE + TILE_LANES * META_BYTES
        for lane in range(TILE_LANES):
            req = int(b.order[t * TILE_LANES + lane])
            if req == 0xFFFFFFFF:
                continue
            s = b""
            for u in range(int(units[t])):
                w = 8 if half[t] and u + 1 == units[t] else 16
                o = base + u * TILE_LANES * 16 + lane * w
                s += b.batch[o:o + w].tobytes()
            out[req] = s
    return out


def three_way(cl, pols, rq, monkeypatch):
    """Host walk of the tokenized batch == of the plain batch == the oracle."""
    bt = pack(cl, rq, monkeypatch, True)
    bp = pack(cl, rq, monkeypatch, False)
    want = oracle.HttpOracle(pols).eval(**rq, nthreads=8)
    got_t = cl.http_eval_host_diag_slots(bt)
    got_p = cl.http_eval_host_diag_slots(bp)
    for b, got in ((bt, got_t), (bp, got_p)):
        order = b.order[:b.nslots]
        real = order < b.n
        assert np.array_equal(got[real], want[order[real]])
        assert not got[~real].any()
    return bt, bp, want


# ------------------------------------------------------------ exactness ----
def test_tokens_exact_2000_rules(host, monkeypatch):
    pols, info = synth.http10k_rules(n_rules=2000, n_ports=16)
    host.update_http_policy(pols)
    st = host.http_policy_stats()
    assert st["tokens"] > 0 and st["token_cells"] > 0
    rq = synth.http10k_requests_fast(65536, info, seed=41)
    bt, bp, want = three_way(host, pols, rq, monkeypatch)
    assert bt.used_bytes() < bp.used_bytes()
    assert 0.1 < want.mean() < 0.9


def test_tokens_exact_starwars(host, monkeypatch):
    pols = synth.starwars_policy()
    host.update_http_policy(pols)
    rq = synth.starwars_requests(65536, seed=42)
    bt, bp, want = three_way(host, pols, rq, monkeypatch)
    assert bt.used_bytes() <= bp.used_bytes()
    assert 0.1 < want.mean() < 0.9


# ----------------------------------------------------------- edge strings ----
def edge_policy():
    """One program (ingress, port 80).  Literals shared by many rules
    (/api/v, /svc, /static/, .example.com, the methods), fields: method,
    path, authority and one header, so most strings end with REST."""
    rules = []
    for k in range(6):
        rules.append(PortRuleHTTP(Method="GET|HEAD", Path=f"/api/v[0-9]+/svc{k}/.*",
                                  Host=f"svc{k}\\.example\\.com" if k % 2 == 0 else ""))
    for k in range(6, 12):
        rules.append(PortRuleHTTP(Method="POST", Path=f"/static/{k}/[a-z]+\\.(js|css)", Host="",
                                  Headers=["X-Tenant-1: t1"] if k == 7 else []))
    for k in range(12, 18):
        rules.append(PortRuleHTTP(Method="DELETE", Path=f"/svc{k}/alpha", Host=f"svc{k}\\.example\\.com",
                                  Headers=["X-Tenant-1: t1"] if k == 13 else []))
    hs = [get_http_rule(r)[0] for r in rules]
    return [network_policy("edge", 7, ingress=[port_network_policy(80, [port_network_policy_rule([7], hs)])])]


def edge_requests():
    """(name, method, path, host, header value or None) of every edge string."""
    rs = []
    # exact-match rules: the whole string is literals of the rules
    for k in range(12, 18):
        rs.append((f"exact{k}", b"DELETE", b"/svc%d/alpha" % k, b"svc%d.example.com" % k, b"t1" if k == 13 else None))
    # a run of digits of every length moves the tokens behind it over every
    # byte of a unit: a token ends at byte 8 and at byte 16 for some of them
    for d in range(1, 34):
        rs.append((f"shift{d}", b"GET", b"/api/v" + b"7" * d + b"/svc1/x", b"h.example.com", None))
        rs.append((f"shiftH{d}", b"HEAD", b"/api/v" + b"7" * d + b"/svc2/", b"svc2.example.com", None))
    # a literal broken by one mutated byte stays bytes and dies
    rs.append(("mutated-host", b"DELETE", b"/svc14/alpha", b"svc14.exbmple.com", None))
    rs.append(("mutated-path", b"GET", b"/apj/v1/svc1/x", b"h.example.com", None))
    rs.append(("mutated-method", b"DELETF", b"/svc14/alpha", b"svc14.example.com", None))
    rs.append(("mutated-static", b"POST", b"/statjc/8/abc.js", b"h.example.com", None))
    rs.append(("static-ok", b"POST", b"/static/8/abc.js", b"h.example.com", None))
    # the same literal followed by SEP REST, by SEP and a header, and by more host
    rs.append(("sep-rest", b"DELETE", b"/svc13/alpha", b"svc13.example.com", None))
    rs.append(("sep-header", b"DELETE", b"/svc13/alpha", b"svc13.example.com", b"t1"))
    rs.append(("sep-header-bad", b"DELETE", b"/svc13/alpha", b"svc13.example.com", b"t2"))
    rs.append(("host-goes-on", b"DELETE", b"/svc12/alpha", b"svc12.example.com.example.com", None))
    rs.append(("static-header", b"POST", b"/static/7/abc.css", b"x", b"t1"))
    rs.append(("static-no-header", b"POST", b"/static/7/abc.css", b"x", None))
    # literals of the rules inside fields no rule constrains
    rs.append(("free-host", b"GET", b"/api/v1/svc1/x", b"/api/v/static/DELETE.example.com/svc", None))
    rs.append(("free-tail", b"GET", b"/api/v1/svc3/.example.com/api/v1/svc/static/", b"svc3.example.com", None))
    rs.append(("free-tail-deny", b"GET", b"/api/v1/svc4/.example.com", b"svc3.example.com", None))
    # past the slot untokenized: the overflow arena, whatever the tokens would save
    rs.append(("overflow", b"GET", b"/api/v1/svc1/" + b".example.com" * 12, b"h.example.com", None))
    rs.append(("remote8", b"DELETE", b"/svc12/alpha", b"svc12.example.com", None))  # an identity no rule selects
    rs.append(("overflow-deny", b"GET", b"/api/v1/svc0/" + b".example.com" * 12, b"h.example.com", None))
    return rs


def as_request_arrays(rs):
    lists = []
    for _, m, p, h, t in rs:
        x = b":method\0" + m + b"\0:path\0" + p + b"\0:authority\0" + h + b"\0"
        if t is not None:
            x += b"X-Tenant-1\0" + t + b"\0"
        lists.append(x)
    n = len(lists)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return dict(policy=np.zeros(n, np.uint32), ingress=np.ones(n, np.uint8), port=np.full(n, 80, np.uint16),
                remote=np.array([8 if r[0].startswith("remote8") else 7 for r in rs], np.uint32),
                hdr_blob=np.frombuffer(b"".join(lists), np.uint8).copy(), hdr_off=off)


def test_tokens_edge_strings(host, monkeypatch):
    pols = edge_policy()
    host.update_http_policy(pols)
    st = host.http_policy_stats()
    assert st["programs"] == 1 and st["lds_programs"] == 1 and st["tokens"] >= 4
    code_map, toks = host.http_tokens_diag(0)
    max_class = int(code_map.max())
    tok_codes = {c for c, _ in toks}
    assert len(toks) == st["tokens"] and all(c > max_class and c % 4 == 0 and c < 256 for c in tok_codes)
    assert all(2 <= len(seq) <= 16 and max(seq) <= max_class for _, seq in toks)
    spelled = {c: seq for c, seq in toks}
    firsts = [seq[0] for _, seq in toks]
    assert len(set(firsts)) < len(firsts)  # tokens that share their first code: the packer tries the longest first
    print("tokens:", [(c, bytes(int(np.argmax(code_map == x)) for x in seq)) for c, seq in toks])

    rs = edge_requests()
    names = [r[0] for r in rs]
    rq = as_request_arrays(rs)
    bt, bp, want = three_way(host, pols, rq, monkeypatch)
    verdict = dict(zip(names, want.tolist()))
    # the oracle's verdicts are the ones each string was made for
    assert all(verdict[f"exact{k}"] for k in range(12, 18))
    assert not any(verdict[n] for n in names if n.startswith("mutated") or n.endswith("deny") or n.endswith("bad"))
    assert verdict["sep-header"] and verdict["free-tail"] and verdict["static-header"] and not verdict["sep-rest"]
    assert not verdict["static-no-header"] and not verdict["host-goes-on"] and not verdict["remote8"]

    tok_s, plain_s = strings_of_requests(bt), strings_of_requests(bp)
    idx = {n: i for i, n in enumerate(names)}

    def expand(s):  # a tokenized string back to class codes
        return b"".join(spelled.get(c, bytes([c])) for c in s)

    # every slot string is its plain string with literals replaced, nothing else
    for n, i in idx.items():
        if n.startswith("overflow"):
            continue
        assert expand(tok_s[i]).rstrip(b"\0") == plain_s[i].rstrip(b"\0"), n
    # a string made only of tokens
    only = [n for n, i in idx.items() if n.startswith("exact") and set(tok_s[i].rstrip(b"\0")) <= tok_codes]
    assert only, "no exact-match request is spelled by tokens alone"
    # a token as the 8th and as the 16th symbol of a unit
    ends8 = [n for n, i in idx.items() if any(c in tok_codes for c in tok_s[i][7::16])]
    ends16 = [n for n, i in idx.items() if any(c in tok_codes for c in tok_s[i][15::16])]
    assert ends8 and ends16
    # a broken literal stays bytes: the token of the whole literal is gone, the string longer than its twin's
    for broken, twin in (("mutated-host", "exact14"), ("mutated-method", "exact14"), ("mutated-path", "shift1"),
                         ("mutated-static", "static-ok")):
        assert verdict[twin] and set(tok_s[idx[twin]]) & tok_codes - set(tok_s[idx[broken]]), broken
        assert len(tok_s[idx[broken]].rstrip(b"\0")) > len(tok_s[idx[twin]].rstrip(b"\0")), broken
    # tokens inside unconstrained fields
    assert any(c in tok_codes for c in tok_s[idx["free-host"]]) and any(c in tok_codes for c in tok_s[idx["free-tail"]])
    # over 128 bytes untokenized: the arena, although its tokenized form would fit the slot
    flags = flags_of_slots(bt)
    for n in ("overflow", "overflow-deny"):
        slot = int(np.nonzero(bt.order[:bt.nslots] == idx[n])[0][0])
        assert flags[slot] & F_OVERFLOW
        i = idx[n]
        plain = bytes(rq["hdr_blob"][int(rq["hdr_off"][i]):int(rq["hdr_off"][i + 1])])
        assert len(plain) > SLOT_BYTES
    used = batch_header(bt)["arena_bytes"]
    assert used == batch_header(bp)["arena_bytes"] > 2 * SLOT_BYTES and np.array_equal(bt.arena[:used], bp.arena[:used])
    assert verdict["overflow"] and not verdict["overflow-deny"]


# ------------------------------------------------------ config 5: budget, payoff ----
@pytest.fixture(scope="module")
def config5():
    cl = Classifier(device=-1)
    pols, info = synth.http10k_rules()
    cl.update_http_policy(pols)
    yield cl, info
    cl.close()


def test_tokens_budget_config5(config5):
    """Tokens never cost a program its LDS residency, nor the kernel its two
    workgroups per CU."""
    cl, _ = config5
    st = cl.http_policy_stats()
    print({k: int(v) for k, v in st.items()})
    assert st["programs"] == 64 and st["lds_programs"] == 64  # none walked from global memory
    assert st["max_program_cells"] <= TWO_WG_CELLS
    assert ((st["max_program_cells"] + 255) // 256 * 256 + 64 + 512 + 3) * 4 <= 80 * 1024
    assert st["tokens"] > 0
    for p in range(64):
        code_map, toks = cl.http_tokens_diag(p)
        assert int(code_map.max()) // 4 + 1 + len(toks) <= 64


def test_tokens_payoff_config5(config5, monkeypatch):
    cl, info = config5
    rq = synth.http10k_requests_fast(262144, info, seed=synth.SEED)
    with_t = tile_bytes_per_slot(pack(cl, rq, monkeypatch, True))
    without = tile_bytes_per_slot(pack(cl, rq, monkeypatch, False))
    print(f"tile bytes per slot: {with_t:.2f} with tokens, {without:.2f} without, ratio {with_t / without:.3f}")
    assert with_t <= 0.80 * without


# ------------------------------------------------------------------ image ----
def _fnv64(data):
    h = 1469598103934665603
    for x in data:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _same_batch(a, b):
    """Batches equal in every byte a reader follows, but for the header's
    snapshot epoch: header, chunk table, tile table, tiles, order, arena (the
    tables are laid out for the most tiles the requests could need; the room
    behind their last entry is not written)."""
    ha, hb = batch_header(a), batch_header(b)
    if {**ha, "epoch": 0} != {**hb, "epoch": 0}:
        return False
    spans = [(8, 64), (64, 64 + 16 * ha["nchunks"]), (ha["ttab_off"], ha["ttab_off"] + 8 * ha["ntiles"]),
             (ha["tiles_off"], ha["total_bytes"])]
    used = ha["arena_bytes"]
    return all(np.array_equal(a.batch[lo:hi], b.batch[lo:hi]) for lo, hi in spans) and \
        np.array_equal(a.order[:a.nslots], b.order[:b.nslots]) and np.array_equal(a.arena[:used], b.arena[:used])


def test_tokens_travel_in_the_image(config5, monkeypatch):
    cl, info = config5
    rq = synth.http10k_requests_fast(32768, info, seed=43)
    other = Classifier(device=-1)
    try:
        other.import_http_policy(cl.export_http_policy())
        assert other.http_policy_stats() == cl.http_policy_stats()
        assert other.http_tokens_diag(5)[1] == cl.http_tokens_diag(5)[1]
        a, b = pack(cl, rq, monkeypatch, True), pack(other, rq, monkeypatch, True)
        assert _same_batch(a, b)
        assert a.used_bytes() < pack(cl, rq, monkeypatch, False).used_bytes()
    finally:
        other.close()


def test_image_without_tokens_imports(host, monkeypatch):
    """An image of the version before tokens (no token section) imports with
    none: its tables still walk plain class codes."""
    pols = edge_policy()
    host.update_http_policy(pols)
    img = bytearray(host.export_http_policy())
    # the token section: two totals, the program count, per program a count
    # and {code, length, codes} records; then the checksum
    _, toks = host.http_tokens_diag(0)
    section = 8 + 8 + 8 + 4 + sum(8 + len(seq) for _, seq in toks)
    old = img[:len(img) - 8 - section]
    version = int.from_bytes(old[4:8], "little")
    assert version & 0xFF == 2
    old[4:8] = ((version & ~0xFF) | 1).to_bytes(4, "little")
    old += _fnv64(old).to_bytes(8, "little")
    other = Classifier(device=-1)
    try:
        other.import_http_policy(bytes(old))
        assert other.http_policy_stats()["tokens"] == 0 and other.http_tokens_diag(0)[1] == []
        rq = as_request_arrays(edge_requests())
        a = pack(other, rq, monkeypatch, True)
        assert _same_batch(a, pack(host, rq, monkeypatch, False))
        want = oracle.HttpOracle(pols).eval(**rq)
        assert np.array_equal(other.http_eval_host_diag(a), want)
    finally:
        other.close()
