#!/bin/bash
# whole GPU suite + default bench line (with its secondary figures) -> $OUT (default results/)
set -o pipefail
OUT=${OUT:-results}
mkdir -p "$OUT"
timeout -k 10 1000 python -m pytest tests -x -q -m gpu -s > "$OUT/full_tests.log" 2>&1
rc=$?
grep -E "passed|failed|FAILED|Error|e_ref|g4:|cfg3|full28" "$OUT/full_tests.log" | tail -30
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 600 python bench.py --full > "$OUT/bench_full.json" 2> "$OUT/bench_full.err"
rc=$?
tail -3 "$OUT/bench_full.err"
cat "$OUT/bench_full.json"
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 400 python bench.py --full --config cfg1 > "$OUT/bench_cfg1.json" 2> "$OUT/bench_cfg1.err"
rc=$?
tail -3 "$OUT/bench_cfg1.err"
cat "$OUT/bench_cfg1.json"
exit $rc
