#!/bin/bash
# GPU box: the whole -m gpu suite, smoke(), the default bench line, the raw
# path lines (device layout, the default) under a kernel trace, the
# Envoy-batch latency driver.  A failing test does not stop the
# measurements; a timeout, abort or crash ends the call.
cd "$GRAFT_REPO_ROOT" || exit 1
tag=${1:-r05i}; out=gpurun_out/$tag
mkdir -p $out
export TMPDIR=/tmp
fatal() { case $1 in 124|134|137|139) echo "fatal $1" >> $out/rc.txt; exit $1;; esac; }
: > $out/rc.txt
timeout -k 10 900 python3 -u -m pytest tests -m gpu -v --timeout 200 --timeout-method thread > $out/pytest.log 2>&1
rc=$?; echo "pytest rc=$rc" >> $out/rc.txt; fatal $rc
timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke()" > $out/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc" >> $out/rc.txt; fatal $rc
timeout -k 10 500 python3 bench.py --full > $out/bench.log 2>&1
rc=$?; echo "bench rc=$rc" >> $out/rc.txt; fatal $rc
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $out/raw -o run --output-format csv -- python3 tools/bench_paths.py --paths httpraw,httpfields --steps 3 --cpu-seconds 0 > $out/raw.log 2>&1
rc=$?; echo "raw rc=$rc" >> $out/rc.txt; fatal $rc
timeout -k 10 400 python3 tools/http_latency.py --seconds 0.5 > $out/latency.jsonl 2> $out/latency.err
rc=$?; echo "latency rc=$rc" >> $out/rc.txt; fatal $rc
