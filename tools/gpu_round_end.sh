#!/bin/bash
OUT=${OUT:-out}; export OUT   # where the logs and profiles go
# What the driver runs at round end: GPU tests, smoke(), the default bench.
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -x -q -m gpu --timeout 300 > $OUT/re_pytest.log 2>&1; rc=$?; tail -3 $OUT/re_pytest.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/re_smoke.log 2>&1; rc=$?; tail -2 $OUT/re_smoke.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 600 python bench.py --full > $OUT/re_bench.log 2>&1; rc=$?; tail -1 $OUT/re_bench.log | cut -c1-300; exit $rc
