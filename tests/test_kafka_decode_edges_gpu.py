"""kafka_decode_kernel and kafka_inflate_kernel (kernels_kafka.hip) on the
corpora of kafka_edges_util, whose fixtures test_kafka_decode_edges.py
proves on the CPU: the per-wave LDS stage at and around its boundary for
the three stage sizes that ship, LdsCrc on every head / tail shape through
the stage, HBM, and the inflater's output in LDS and in the arena,
kw_intern's blob compare and probe wrap-around, and DevInflate on every
block kind and size around the LDS / arena split — with the counters that
show the device finished the payloads itself (the host decoder inside the
same call would otherwise hide a device that gives up).

Every record is compared with the host decoder's (diag_cpu) and with
oracle/kafka_wire_ref.py's."""
import pytest

import kafka_edges_util as E

pytestmark = pytest.mark.gpu


def _expect(host, key, pols, reqs, ids):
    red, rem = E.red_rem(len(reqs), ids)
    h, o = E.references(host, key, pols, reqs, red, rem)
    return red, rem, h, o


def _check(got, h, o, what):
    assert E.first_difference(got, h) is None, (what, "host decoder", E.first_difference(got, h))
    assert E.first_difference(got, o) is None, (what, "oracle", E.first_difference(got, o))


def _stage(gpu, host, S, leads):
    pols, topics, clients, ids = E.base_policy()
    reqs = E.stage_layouts(S).reqs
    red, rem, h, o = _expect(host, ("stage", S), pols, reqs, ids)
    gpu.update_kafka_policy(pols)
    for lead in leads:
        _check(E.decode_dev(gpu, reqs, lead, red, rem), h, o, ("all layouts", lead))
        for n in E.STAGE_CUTS:  # L7
            _check(E.decode_dev(gpu, reqs[:n], lead, red[:n], rem[:n]), h[:n], o[:n], ("cut", n, lead))


def test_gpu_stage_layouts_default_stage(gpu, host):
    """Layouts L1-L7 with the 4 KiB stage at every pointer alignment."""
    _stage(gpu, host, 4096, E.ALL_LEADS)


@pytest.mark.run_last
@pytest.mark.parametrize("kb", [8, 16])
def test_gpu_stage_layouts_larger_stages(gpu, host, monkeypatch, kb):
    """kafka_decode_kernel<8192> and <16384> (CILIUM_GPU_KAFKA_STAGE_KB) on
    layouts sized for them."""
    monkeypatch.setenv("CILIUM_GPU_KAFKA_STAGE_KB", str(kb))
    _stage(gpu, host, kb * 1024, E.FEW_LEADS)


@pytest.mark.parametrize("placement", ["staged", "unstaged"])
def test_gpu_crc_shapes(gpu, host, placement):
    """One-message produce requests of every CRC region length and start
    alignment, read from the LDS stage and from HBM: a message the device
    rejects turns its request into a decode error."""
    pols, topics, clients, ids = E.base_policy()
    reqs = E.crc_staged(topics) if placement == "staged" else E.crc_unstaged(topics)
    red, rem, h, o = _expect(host, "crc-" + placement, pols, reqs, ids)
    gpu.update_kafka_policy(pols)
    for lead in E.ALL_LEADS:
        _check(E.decode_dev(gpu, reqs, lead, red, rem), h, o, (placement, lead))


def test_gpu_crc_shapes_in_inflated_sets(gpu, host):
    """The same messages as inner sets of gzip and snappy wrappers, decoded
    into LDS (alone) and into the arena (behind a 300-byte message): the
    gzip trailer's CRC and the inner messages' CRCs run over the inflater's
    output.  Every payload is the device's to finish."""
    pols, topics, clients, ids = E.base_policy()
    reqs, _ = E.crc_inner_all(topics)
    red, rem, h, o = _expect(host, "crc-inner", pols, reqs, ids)
    gpu.update_kafka_policy(pols)
    for lead in E.ALL_LEADS:
        i0, d0, u0 = E.decode_stats(gpu)
        got = E.decode_dev(gpu, reqs, lead, red, rem)
        i1, d1, u1 = E.decode_stats(gpu)
        print(f"crc inner sets, lead {lead}: requests {len(reqs)}, device_inflated {i1 - i0}, host_deferred {d1 - d0}")
        _check(got, h, o, ("inner", lead))
        assert (i1 - i0, d1 - d0, u1 - u0) == (len(reqs), 0, 0), lead


def test_gpu_inflate_shapes(gpu, host):
    """Inner sets of exact sizes around kInfLds and up to 70 000 bytes under
    every encoder: the device decodes each compressed payload itself — none
    handed to the host, none turned away by the arena."""
    pols, topics, clients, ids = E.base_policy()
    reqs, wrappers, decoded = E.inflate_shapes(topics, clients)
    red, rem, h, o = _expect(host, "inflate", pols, reqs, ids)
    gpu.update_kafka_policy(pols)
    for lead in (0, 7):
        i0, d0, u0 = E.decode_stats(gpu)
        got = E.decode_dev(gpu, reqs, lead, red, rem)
        i1, d1, u1 = E.decode_stats(gpu)
        print(f"inflate shapes, lead {lead}: requests {len(reqs)}, wrappers {wrappers}, decoded bytes {decoded}, "
              f"device_inflated {i1 - i0}, host_deferred {d1 - d0}, unreserved {u1 - u0}")
        _check(got, h, o, ("inflate", lead))
        assert d1 - d0 == 0, "requests handed to the host decoder"
        assert i1 - i0 == wrappers
        assert u1 - u0 == 0


def test_gpu_inflate_deferred_to_the_host(gpu, host):
    """What the device may not finish (a second gzip member, a compressed
    set inside a compressed set): each such request reaches the host
    decoder, once."""
    pols, topics, clients, ids = E.base_policy()
    reqs = E.inflate_deferred(topics, clients)
    red, rem, h, o = _expect(host, "inflate-deferred", pols, reqs, ids)
    gpu.update_kafka_policy(pols)
    i0, d0, u0 = E.decode_stats(gpu)
    got = E.decode_dev(gpu, reqs, 3, red, rem)
    i1, d1, u1 = E.decode_stats(gpu)
    print(f"deferred shapes: requests {len(reqs)}, device_inflated {i1 - i0}, host_deferred {d1 - d0}")
    _check(got, h, o, "deferred")
    assert d1 - d0 == len(reqs)


@pytest.mark.parametrize("both", [False, True])
def test_gpu_intern_edges(gpu, host, both):
    """Rule topics and clientIDs of lengths around the 16-byte prefix and
    the blob, names that wrap from the table's last slot to slot 0, and two
    names of equal hash, length and prefix, of which the policy names one
    (the other must come out unknown) or both (each its own id); with near
    misses of every one of them, inline and through the topic arena."""
    pols, topics, clients = E.intern_policy(both)
    reqs, tc, cc = E.intern_requests(both)
    red, rem, h, o = _expect(host, ("intern", both), pols, reqs, [1])
    gpu.update_kafka_policy(pols)
    for lead in (0, 7):
        _check(E.decode_dev(gpu, reqs, lead, red, rem), h, o, ("intern", both, lead))
