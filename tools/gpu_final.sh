#!/bin/bash
OUT=${OUT:-out}; export OUT   # where the logs and profiles go
# Round-end set on one box: GPU tests, smoke(), the default bench line (its
# roofline from the newest profiles/rNN/pmc.json), then the N=2 exchange rehearsal
# (two ranks on cuda:0 over gloo).  TAG names the outputs.
export TMPDIR=/tmp
cd "$(dirname "$0")/.." || exit 1
mkdir -p $OUT
T=${TAG:-fin}
timeout -k 10 900 python -u -m pytest tests -m gpu -v --timeout 300 --timeout-method thread > $OUT/${T}_pytest.log 2>&1
rc=$?; tail -2 $OUT/${T}_pytest.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${T}_smoke.log 2>&1 || exit $?
tail -1 $OUT/${T}_smoke.log
timeout -k 10 600 python -u bench.py --full > $OUT/${T}_bench_full.log 2>&1 || exit $?
tail -1 $OUT/${T}_bench_full.log | cut -c1-300
bash tools/gpu_rehearse_multi.sh
