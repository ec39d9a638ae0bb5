"""Literal tokens on the GPU (test_http_tokens.py has the CPU side): the
tokenized batch through http_kernel equals the oracle, leaves the counters the
untokenized batch leaves, and strings of plain class codes, as the raw-head
path builds them on the device, still walk the widened tables to the oracle's
verdicts."""
import numpy as np
import pytest

import oracle
from cilium_amd import _native as N
from cilium_amd import synth
from test_http_parse import _blob, _raw_requests
from test_http_raw_gpu import _oracle as _raw_oracle
from test_http_tokens import as_request_arrays, edge_policy, edge_requests, pack

pytestmark = pytest.mark.gpu


def _on_device(gpu, b):
    """One http_verdicts_dev launch from zeroed counters: verdicts in request
    order, the per-program and the per-rule counters."""
    import torch
    dev = torch.device("cuda:0")
    d_batch = torch.from_numpy(b.batch[:b.used_bytes()].copy()).to(dev)
    d_arena = torch.from_numpy(np.concatenate([b.arena.view(np.uint8), np.zeros(16, np.uint8)])).to(dev)
    d_out = torch.zeros(b.nslots, dtype=torch.uint8, device=dev)
    gpu.reset_counters()
    gpu.http_verdicts_dev(d_batch, b.nslots, d_arena, d_out, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    order = b.order[:b.nslots]
    real = order < b.n
    v = np.zeros(b.n, np.uint8)
    v[order[real]] = out[real]
    assert not out[~real].any()
    return v, gpu.read_counters(N.CG_CTR_HTTP_PROGRAMS).copy(), gpu.http_rule_hits().copy()


def _tokenized_equals_plain(gpu, pols, rq, monkeypatch):
    gpu.update_http_policy(pols)
    assert gpu.http_policy_stats()["tokens"] > 0
    want = oracle.HttpOracle(pols).eval(**rq, nthreads=8)
    bt, bp = pack(gpu, rq, monkeypatch, True), pack(gpu, rq, monkeypatch, False)
    assert bt.used_bytes() < bp.used_bytes()
    vt, pt, rt = _on_device(gpu, bt)
    vp, pp, rp = _on_device(gpu, bp)
    assert np.array_equal(vt, want) and np.array_equal(vp, want)
    assert np.array_equal(pt, pp) and pt.sum() > 0
    assert np.array_equal(rt, rp) and rt.sum() == want.sum()
    return want


def test_tokens_gpu_2000_rules(gpu, monkeypatch):
    pols, info = synth.http10k_rules(n_rules=2000, n_ports=16)
    rq = synth.http10k_requests_fast(65536, info, seed=41)
    want = _tokenized_equals_plain(gpu, pols, rq, monkeypatch)
    assert 0.1 < want.mean() < 0.9


def test_tokens_gpu_edge_strings(gpu, monkeypatch):
    rs = edge_requests()
    rs = [rs[i % len(rs)] for i in range(4096)]
    want = _tokenized_equals_plain(gpu, edge_policy(), as_request_arrays(rs), monkeypatch)
    assert 0.1 < want.mean() < 0.9


def test_tokens_gpu_raw_heads_keep_plain_codes(gpu):
    import torch
    pols, info = synth.http10k_rules(n_rules=2000, n_ports=16)
    gpu.update_http_policy(pols)
    assert gpu.http_policy_stats()["tokens"] > 0
    n = 4096
    rq = synth.http10k_requests_fast(n, info, seed=44)
    raws = _raw_requests(rq)
    args = (rq["policy"], rq["ingress"], rq["port"], rq["remote"])
    want = _raw_oracle(pols, *args, raws)
    blob, off = _blob(raws)
    dev = torch.device("cuda:0")
    d_raw = torch.from_numpy(blob[:int(off[-1])].copy()).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_pol = torch.from_numpy(np.asarray(args[0]).astype(np.int32)).to(dev)
    d_ing = torch.from_numpy(np.asarray(args[1]).astype(np.uint8)).to(dev)
    d_port = torch.from_numpy(np.asarray(args[2]).astype(np.int16)).to(dev)
    d_rem = torch.from_numpy(np.asarray(args[3]).astype(np.int32)).to(dev)
    d_out = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    gpu.http_verdicts_raw_dev(d_raw, d_off, n, d_pol, d_ing, d_port, d_rem, d_out)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)
    assert 0.1 < want.mean() < 0.9
