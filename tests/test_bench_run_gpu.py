"""A plain `bench.py --gpus 1` run on the GPU, at a small batch: it times
exactly --steps steps, runs none of --full's legs, and --dump-outputs leaves
the last step's verdicts, which equal the oracle's on the same seeded
requests."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(120)
def test_plain_run_times_the_steps_and_dumps_the_verdicts(tmp_path):
    import oracle
    from cilium_amd import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    D, per_gpu, steps = 65_536, 200_000, 3
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--prewarm-seconds", "0", "--distinct", str(D), "--requests-per-gpu",
                        str(per_gpu), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=110, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    reps = -(-per_gpu // D)
    assert d["steps"] == steps and d["n_gpus"] == 1 and d["unit"] == "verdicts/s" and d["dtype"] == "u8"
    assert d["higher_is_better"] is True and d["config"]["requests_per_gpu"] == reps * D
    # the headline is the timed steps' own rate, and the kernel's events cover every one of them
    assert d["ms_per_step"] > 0 and abs(d["value"] - reps * D / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert 0 < d["roofline"]["kernel_ms"] <= d["ms_per_step"]
    for leg in ("parity_check", "sustained", "distinct_262k", "end_to_end", "host_entry", "cpu_baseline"):
        assert d[leg] is None, leg
    pols, info = synth.http10k_rules()
    exp = oracle.HttpOracle(pols).eval(**synth.http10k_requests_fast(D, info, seed=synth.SEED), nthreads=8)
    v, c = np.load(tmp_path / "verdicts.npy"), np.load(tmp_path / "allowed_copies.npy")
    assert v.dtype == c.dtype == np.float32
    assert np.array_equal(v, exp) and np.array_equal(c, reps * exp.astype(np.float32))
