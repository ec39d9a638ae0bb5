"""Both raw-path sequences (http_raw.cc: the device layout, the default, and
CILIUM_GPU_RAW_LAYOUT=host) over the same small batches, against an
independent oracle: heads and header lists, two policies whose lookup tables
and bucket counters fit the scan's LDS (star wars, the 10K-rule set) and one
whose tables and bucket counters stay in global memory (3,000 rules on 959
ports, a program each), with requests past the 128-byte slot
(overflow arena / walk list) and past the wave's 6 KiB stage (deferred)
present by construction.  The two sequences share one scan front end
(kernels_http_raw.hip raw_scan_waves), so every case reaches it through
another of its template instances."""
import os

import numpy as np
import pytest

from cilium_amd import synth
from test_http_fields_gpu import _host_path as _fields_host_path
from test_http_fields_gpu import _join, _pairs, _split
from test_http_fields_gpu import _oracle as _fields_oracle
from test_http_fields_gpu import _vary as _fields_vary
from test_http_parse import _blob, _raw_requests
from test_http_raw_gpu import _host_path, _oracle, _vary

pytestmark = [pytest.mark.gpu, pytest.mark.run_last]

N_REQ = 3_000


@pytest.fixture
def layout_env():
    """The environment the sequences read per call, restored afterwards."""
    old = {k: os.environ.get(k) for k in ("CILIUM_GPU_RAW_LAYOUT", "CILIUM_GPU_RAW_SUBBATCH", "CILIUM_GPU_RAW_SPIN")}
    yield os.environ
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _args(rq):
    return rq["policy"], rq["ingress"], rq["port"], rq["remote"]


def _policy(which):
    if which == "starwars":
        pols = synth.starwars_policy()
        return pols, synth.starwars_requests(N_REQ, seed=151)
    if which == "http10k":
        pols, info = synth.http10k_rules()
        return pols, synth.http10k_requests(N_REQ, info, seed=152)
    # 3,000 rules over 959 ports, a program each: the program hash alone
    # (2 x 2,048 words) passes the 8 KiB the scan stages in LDS
    # (lds_tables_fit: the kLdsTabs = false instances), and 961 program groups
    # x 10 bucket keys pass the 32 KiB of LDS bucket counters
    # (http_raw_lds_keys: global counters and cursors)
    pols, info = synth.http10k_rules(n_rules=3000, n_ports=1000)
    scopes = len(pols[0]["ingress_per_port_policies"])  # (policy, direction, port) keys of the program hash
    assert 2 * 4 * 2 * scopes > 8 * 1024  # its keys and values at >= 2 slots per scope: lds_tables_fit is false
    assert (scopes + 2) * 10 * 4 > 32 * 1024  # a program per scope, 10 u32 bucket counters each: http_raw_lds_keys is false
    return pols, synth.http10k_requests(N_REQ, info, seed=153)


def _long_heads(raws, rng):
    """i % 8 == 1: a path 130-400 bytes longer (the walked string passes the
    slot); i % 8 == 2: one more header of 6,200-9,000 bytes (the head passes
    the wave's stage); the rest varied as clients send them."""
    rest = iter(_vary([r for i, r in enumerate(raws) if i % 8 not in (1, 2)], rng))
    out = []
    for i, r in enumerate(raws):
        if i % 8 == 1:
            assert b" HTTP/" in r
            out.append(r.replace(b" HTTP/", b"/" + b"q" * int(rng.integers(130, 401)) + b" HTTP/", 1))
        elif i % 8 == 2:
            assert b"\r\n\r\n" in r
            out.append(r.replace(b"\r\n\r\n", b"\r\nX-Big: " + b"b" * int(rng.integers(6200, 9001)) + b"\r\n\r\n", 1))
        else:
            out.append(next(rest))
    return out


def _long_lists(lists, rng):
    """As _long_heads, on "name\\0value\\0" lists: a longer :path value, one
    more pair of 6,200-9,000 bytes."""
    rest = iter(_fields_vary([l for i, l in enumerate(lists) if i % 8 not in (1, 2)], rng))
    out = []
    for i, lst in enumerate(lists):
        if i % 8 == 1:
            ps = _pairs(lst)
            j = [n for n, _ in ps].index(b":path")
            ps[j] = (ps[j][0], ps[j][1] + b"/" + b"q" * int(rng.integers(130, 401)))
            out.append(b"".join(n + b"\0" + v + b"\0" for n, v in ps))
        elif i % 8 == 2:
            out.append(lst + b"x-big\0" + b"b" * int(rng.integers(6200, 9001)) + b"\0")
        else:
            out.append(next(rest))
    return out


_cases = {}
_SEEDS = {(inp, which): 160 + 3 * a + b for a, inp in enumerate(("heads", "lists"))
          for b, which in enumerate(("starwars", "http10k", "wide"))}


def _case(cl, inp, which):
    """The requests of (input, policy), the oracle's verdicts and the host
    path's: computed once, shared by both layouts, never modified."""
    key = (inp, which)
    if key not in _cases:
        pols, rq = _policy(which)
        cl.update_http_policy(pols)
        rng = np.random.default_rng(_SEEDS[key])  # per case: a selection of cases sees the full run's inputs
        if inp == "heads":
            raws = _long_heads(_raw_requests(rq), rng)
            blob, off = _blob(raws)
            exp = _oracle(pols, *_args(rq), raws)
            host = _host_path(cl, *_args(rq), raws)
        else:
            blob, off = _join(_long_lists(_split(rq["hdr_blob"], rq["hdr_off"]), rng))
            exp = _fields_oracle(pols, *_args(rq), blob, off)
            host = _fields_host_path(cl, *_args(rq), blob, off)
        for a in (exp, host):
            a.setflags(write=False)
        _cases[key] = (pols, rq, blob, off, exp, host)
    return _cases[key]


@pytest.mark.parametrize("which", ["starwars", "http10k", "wide"])
@pytest.mark.parametrize("inp", ["heads", "lists"])
@pytest.mark.parametrize("layout", ["device", "host"])
def test_gpu_raw_layouts(gpu, layout_env, layout, inp, which):
    pols, rq, blob, off, exp, host = _case(gpu, inp, which)
    gpu.update_http_policy(pols)
    layout_env["CILIUM_GPU_RAW_LAYOUT"] = layout
    call = gpu.http_verdicts_raw if inp == "heads" else gpu.http_verdicts_fields
    got = np.asarray(call(*_args(rq), blob, off))
    assert len(got) == N_REQ
    bad = np.nonzero(got != exp)[0]
    assert not len(bad), [(int(i), int(got[i]), int(exp[i])) for i in bad[:8]]
    assert np.array_equal(got, host)
    rest = np.array([i % 8 not in (1, 2) for i in range(N_REQ)])
    print(f"{layout}/{inp}/{which}: mean of the varied remainder {got[rest].mean():.3f}")
    assert 0.1 < got[rest].mean() < 0.9
