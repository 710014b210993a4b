#!/bin/bash
# Round evidence of the tree as it is (on the GPU box): the GPU test suite,
# smoke(), the --full bench line, then a kernel trace of the bench's primary
# leg checked against its ms_per_step (scripts/trace_fit.py).  Everything is
# written under $OUT_DIR (default bench_out/ in the repository).
set -o pipefail
cd "$(dirname "$0")/.."
OUT="${OUT_DIR:-bench_out}"; mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread \
    > "$OUT/pytest_gpu.log" 2>&1 || { echo "pytest failed"; tail -40 "$OUT/pytest_gpu.log"; exit 1; }
tail -2 "$OUT/pytest_gpu.log"
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" \
    > "$OUT/smoke.log" 2>&1 || { echo "smoke failed"; tail -20 "$OUT/smoke.log"; exit 1; }
tail -1 "$OUT/smoke.log"
t0=$SECONDS
timeout -k 10 600 python bench.py --full > "$OUT/bench_default.json" 2> "$OUT/bench_default.err" \
    || { echo "bench rc=$?"; tail -20 "$OUT/bench_default.err"; cat "$OUT/bench_default.json"; exit 1; }
echo "bench wall seconds: $((SECONDS - t0))" | tee "$OUT/bench_wall.txt"
cat "$OUT/bench_default.json"
[ "$1" = "--trace" ] || exit 0
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/bench_trace" -o run --output-format csv -- \
    python3 bench.py --full --no-secondary --no-w3 --no-8k --no-single --no-e2e --no-stream --no-cpu-baseline --no-bands --no-host-api \
    > "$OUT/bench_trace.json" 2> "$OUT/bench_trace.err" || { echo "trace failed"; exit 1; }
python3 scripts/trace_fit.py "$OUT/bench_trace" "$OUT/bench_trace.json"
