"""ASan + UBSan run of the egress frames route's host code, as a stand-alone
program (no Python process loads anything sanitized, nothing is preloaded).

Builds every translation unit of cilium_amd/build.py with the sanitizers on
the host side (build_asan.py's objects), links them with
egress_standalone.cc into tools/sanitize/_build/egress_standalone, writes two
worlds with the batches and the results the Python oracle (tests/egress_util.py)
expects — the shared egress batch over every resolver combination, with and
without conntrack and IGNORE_DROP, and the hand-written cases of
tests/golden/l4_egress_kat.json — and runs the program over them.  CPU only.

    python tools/sanitize/egress_standalone.py
"""
from __future__ import annotations

import concurrent.futures as cf
import ipaddress
import os
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(HERE)]
import build_asan as A  # noqa: E402
from cilium_amd import build as B  # noqa: E402

EXE = A.OUT / "egress_standalone"
HOST_SAN = ["-fsanitize=address", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def build() -> Path:
    A.OUT.mkdir(exist_ok=True)
    with cf.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(A.compile_one, B.SOURCES))
    main_o = A.OUT / "egress_standalone.o"
    cmds = [[B.HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", *HOST_SAN, "-I", str(ROOT / "include"), "-c",
             str(HERE / "egress_standalone.cc"), "-o", str(main_o)],
            [B.HIPCC, f"--offload-arch={B.ARCH}", str(main_o), *map(str, objs), "-o", str(EXE), "-lpthread", "-lz",
             "-lhsa-runtime64", "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined"]]
    for cmd in cmds:
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError(f"failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    return EXE


def write_world(path: Path, sections: dict) -> None:
    with open(path, "wb") as f:
        for name, data in sections.items():
            b = np.ascontiguousarray(data).tobytes()
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<Q", len(b)) + b)


def _cidrs(entries):
    from cilium_amd.classifier import CIDR_DTYPE
    k = np.zeros(len(entries), CIDR_DTYPE)
    v = np.zeros((len(entries), 2), np.uint32)
    for i, (cidr, ident) in enumerate(entries):
        net = ipaddress.ip_network(cidr)
        k["family"][i], k["prefixlen"][i] = net.version, net.prefixlen
        k["addr"][i, :len(net.network_address.packed)] = np.frombuffer(net.network_address.packed, np.uint8)
        v[i, 0] = ident
    return k, v


def worlds():
    import ct_util as T
    import egress_util as E
    import frames_util as F
    import l4_array_util as U
    from cilium_amd.classifier import POLICY_KEY_DTYPE
    from cilium_amd.policy import htons
    ipc_k, ipc_v = _cidrs(F.IPCACHE)
    # the shared batch
    raw, off, pkt_len, labels, lxc = E.shared_frames()
    items, values = E.shared_table()
    s = {"n_maps": np.uint32(len(U.tables())), "ipc_keys": ipc_k, "ipc_vals": ipc_v,
         "slots": np.array(list(E.SLOT_MAP), np.uint16), "slot_maps": np.array(list(E.SLOT_MAP.values()), np.uint32),
         "hdr_slots": np.array(list(E.HEADER_SPECS), np.uint16),
         "hdrs": np.concatenate([E.header_record(x) for x in E.HEADER_SPECS.values()]),
         "ct_keys": T.keys_array(items), "ct_vals": T.values_array(values),
         "raw": raw, "off": off, "lxc": lxc, "labels": labels, "plen": pkt_len}
    for m, (keys, ports, _) in enumerate(U.tables()):
        s[f"map{m}_keys"], s[f"map{m}_ports"], s[f"map{m}_max"] = keys, ports, np.uint32(64 if m == 2 else 0)
    for ci, name in enumerate(("lab", "ipc")):
        for with_ct in (False, True):
            for ign in (False, True):
                tag = name + ("_ct" if with_ct else "_noct") + ("_ign" if ign else "")
                ev, einfo, erec, _, _ = E.shared_expected(ci, ign, with_ct)
                s["v_" + tag], s["info_" + tag], s["rec_" + tag] = ev, einfo, erec
    yield "egress_shared.bin", s
    # the hand-written cases
    g = E.load_kat()
    st, hd, ctmap = E.kat_oracle_world(g)
    keys = np.zeros(len(g["policy"]), POLICY_KEY_DTYPE)
    for i, p in enumerate(g["policy"]):
        keys[i] = (p["identity"], htons(p["dport"]), p["proto"], p["egress"])
    with_map = [h["slot"] for h in g["headers"].values() if h.get("map", True)]
    with_hdr = [h for h in g["headers"].values() if h.get("header", True)]
    from cilium_amd.classifier import PolicyArray
    frames = [bytes.fromhex(c["hex"]) for c in g["frames"]]
    raw, off = F.join(frames)
    lxc = np.array([g["headers"][c["header"]]["slot"] for c in g["frames"]], np.uint16)
    labels = np.array([c.get("dst_label", g["dst_label"]) for c in g["frames"]], np.uint32)
    ct_items = [T.golden_item(e) for c in g["frames"] for e in c.get("entries", [])]
    k = {"n_maps": np.uint32(1), "map0_keys": keys, "map0_max": np.uint32(0),
         "map0_ports": np.array([htons(p["proxy_port"]) for p in g["policy"]], np.uint16),
         "ipc_keys": ipc_k, "ipc_vals": ipc_v, "slots": np.array(with_map, np.uint16),
         "slot_maps": np.zeros(len(with_map), np.uint32), "hdr_slots": np.array([h["slot"] for h in with_hdr], np.uint16),
         "hdrs": np.concatenate([PolicyArray.header(**E.kat_header_spec(h)) for h in with_hdr]),
         "ct_keys": T.keys_array(ct_items), "ct_vals": T.values_array([{}] * len(ct_items)),
         "raw": raw, "off": off, "lxc": lxc, "labels": labels, "plen": np.zeros(0, np.uint32)}
    for ign in (False, True):
        ev, einfo, erec, _, _ = E.evaluate(frames, st, hd, lxc_ids=lxc, dst_labels=labels, ctmap=ctmap, ignore_drop=ign)
        tag = "lab_ct" + ("_ign" if ign else "")
        k["v_" + tag], k["info_" + tag], k["rec_" + tag] = ev, einfo, erec
    yield "egress_kat.bin", k


def main() -> int:
    exe = build()
    paths = []
    for name, sections in worlds():
        write_world(A.OUT / name, sections)
        paths.append(str(A.OUT / name))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=1:detect_odr_violation=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([str(exe), *paths], env=env).returncode


if __name__ == "__main__":
    sys.exit(main())
