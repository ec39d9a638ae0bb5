"""ASan + UBSan run of the host code of service load-balancing on the egress
frames route, as a stand-alone program (no Python process loads anything
sanitized, nothing is preloaded).

Builds every translation unit of cilium_amd/build.py with the sanitizers on
the host side (build_asan.py's objects), links them with
service_standalone.cc into tools/sanitize/_build/service_standalone, writes two
worlds with the batches and the results the Python oracle (tests/service_util.py)
expects — the shared service batch with a given hash and with NULL, with and
without IGNORE_DROP, and the hand-written cases of
tests/golden/l4_service_kat.json — and runs the program over them.  CPU only.

    python tools/sanitize/service_standalone.py
"""
from __future__ import annotations

import concurrent.futures as cf
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(HERE)]
import build_asan as A  # noqa: E402
import egress_standalone as ES  # noqa: E402
from cilium_amd import build as B  # noqa: E402

EXE = A.OUT / "service_standalone"


def build() -> Path:
    A.OUT.mkdir(exist_ok=True)
    with cf.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(A.compile_one, B.SOURCES))
    main_o = A.OUT / "service_standalone.o"
    cmds = [[B.HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", *ES.HOST_SAN, "-I", str(ROOT / "include"), "-c",
             str(HERE / "service_standalone.cc"), "-o", str(main_o)],
            [B.HIPCC, f"--offload-arch={B.ARCH}", str(main_o), *map(str, objs), "-o", str(EXE), "-lpthread", "-lz",
             "-lhsa-runtime64", "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined"]]
    for cmd in cmds:
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError(f"failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    return EXE


def _service_sections(world) -> dict:
    from cilium_amd.classifier import LB_KEY_DTYPE, LB_REVNAT_DTYPE, LB_REVNAT_KEY_DTYPE, LB_SERVICE_DTYPE
    k, v = np.zeros(len(world["services"]), LB_KEY_DTYPE), np.zeros(len(world["services"]), LB_SERVICE_DTYPE)
    for i, ((fam, addr, dport, slave), s) in enumerate(world["services"].items()):
        k["address"][i, :len(addr)] = np.frombuffer(addr, np.uint8)
        k["family"][i], k["dport"][i], k["slave"][i] = fam, dport, slave
        v["target"][i, :len(s["target"])] = np.frombuffer(s["target"], np.uint8)
        v["port"][i], v["count"][i], v["rev_nat_index"][i], v["weight"][i] = s["port"], s["count"], s["rev_nat"], s["weight"]
    rk, rv = np.zeros(len(world["revnat"]), LB_REVNAT_KEY_DTYPE), np.zeros(len(world["revnat"]), LB_REVNAT_DTYPE)
    for i, ((fam, idx), (addr, port)) in enumerate(world["revnat"].items()):
        rk["index"][i], rk["family"][i] = idx, fam
        rv["address"][i, :len(addr)] = np.frombuffer(addr, np.uint8)
        rv["port"][i] = port
    return {"svc_keys": k, "svc_vals": v, "rn_keys": rk, "rn_vals": rv,
            "loopback": np.frombuffer(world["loopback"], np.uint32)}


def worlds():
    import ct_util as T
    import egress_util as E
    import frames_util as F
    import l4_array_util as U
    import service_util as S
    from cilium_amd.classifier import POLICY_KEY_DTYPE, PolicyArray
    from cilium_amd.policy import htons
    ipc_k, ipc_v = ES._cidrs(F.IPCACHE)
    # the shared service batch
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    items, values = S.shared_table()
    s = {"n_maps": np.uint32(len(U.tables())), "ipc_keys": ipc_k, "ipc_vals": ipc_v,
         "slots": np.array(list(E.SLOT_MAP), np.uint16), "slot_maps": np.array(list(E.SLOT_MAP.values()), np.uint32),
         "hdr_slots": np.array(list(E.HEADER_SPECS), np.uint16),
         "hdrs": np.concatenate([E.header_record(x) for x in E.HEADER_SPECS.values()]),
         "ct_keys": T.keys_array(items), "ct_vals": S.values_array(values),
         "raw": raw, "off": off, "lxc": lxc, "hash": S.shared_hash(), "plen": pkt_len}
    s.update(_service_sections(S.shared_world()))
    for m, (keys, ports, _) in enumerate(U.tables()):
        s[f"map{m}_keys"], s[f"map{m}_ports"], s[f"map{m}_max"] = keys, ports, np.uint32(64 if m == 2 else 0)
    for with_hash in (True, False):
        for ign in (False, True):
            tag = ("hash" if with_hash else "null") + ("_ign" if ign else "")
            e = S.shared_expected(with_hash, ign)
            s["v_" + tag], s["info_" + tag], s["rec_" + tag], s["srec_" + tag], s["xl_" + tag] = e[:5]
    yield "service_shared.bin", s
    # the hand-written cases
    g = S.load_kat()
    h = g["header"]
    keys = np.zeros(len(g["policy"]), POLICY_KEY_DTYPE)
    for i, p in enumerate(g["policy"]):
        keys[i] = (p["identity"], htons(p["dport"]), p["proto"], 1)
    kc_k, kc_v = ES._cidrs([tuple(x) for x in g["ipcache"]])
    ct_items, ct_values = S.kat_ct_items(g)
    raw, off = F.join([bytes.fromhex(c["hex"]) for c in g["frames"]])
    k = {"n_maps": np.uint32(1), "map0_keys": keys, "map0_max": np.uint32(0),
         "map0_ports": np.array([htons(p["proxy_port"]) for p in g["policy"]], np.uint16),
         "ipc_keys": kc_k, "ipc_vals": kc_v, "slots": np.array([h["slot"]], np.uint16),
         "slot_maps": np.zeros(1, np.uint32), "hdr_slots": np.array([h["slot"]], np.uint16),
         "hdrs": PolicyArray.header(**{x: h[x] for x in h if x != "slot"}),
         "ct_keys": T.keys_array(ct_items), "ct_vals": S.values_array(ct_values),
         "raw": raw, "off": off, "lxc": np.full(len(g["frames"]), h["slot"], np.uint16),
         "hash": np.array([c["hash"] for c in g["frames"]], np.uint32), "plen": np.zeros(0, np.uint32)}
    k.update(_service_sections(S.kat_world(g)))
    e = S.kat_oracle(g)
    k["v_hash"], k["info_hash"], k["rec_hash"], k["srec_hash"], k["xl_hash"] = e[:5]
    yield "service_kat.bin", k


def main() -> int:
    exe = build()
    paths = []
    for name, sections in worlds():
        ES.write_world(A.OUT / name, sections)
        paths.append(str(A.OUT / name))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=1:detect_odr_violation=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([str(exe), *paths], env=env).returncode


if __name__ == "__main__":
    sys.exit(main())
