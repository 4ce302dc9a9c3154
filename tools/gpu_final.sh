set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-results}/final
mkdir -p "$OUT"
( while sleep 45; do echo "[tick] $(date +%T)"; done ) &
TICK=$!
trap "kill $TICK" EXIT
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/tok" -o tok -- python3 tools/tokbench.py > "$OUT/tok.out" 2> "$OUT/tok.err" || { tail -5 "$OUT/tok.err"; exit 3; }
grep round "$OUT/tok.out"
find "$OUT/tok" -name "*kernel_trace.csv" -delete
timeout -k 10 500 python bench.py --full 2>"$OUT/bench_default.err" | tail -1 > "$OUT/bench_default.json" || exit 4
cut -c1-200 "$OUT/bench_default.json"
timeout -k 10 300 python bench.py --full --config cfg1 2>"$OUT/bench_cfg1.err" | tail -1 > "$OUT/bench_cfg1.json" || exit 5
cut -c1-200 "$OUT/bench_cfg1.json"
