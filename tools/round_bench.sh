# Record of HEAD on one MI355X: GPU tests, smoke, the plain bench (--steps 20 --warmup 5) and the
# default bench (100 timed transitions per chain) with everything --full adds.
# Run from anywhere; writes into $OUT (default build/round_bench under the repository root).
set -e
cd "$(dirname "$0")/.."; OUT=${OUT:-build/round_bench}; mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -v > "$OUT/gpu_tests.log" 2>&1 || { tail -40 "$OUT/gpu_tests.log"; exit 1; }
tail -1 "$OUT/gpu_tests.log"
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
timeout -k 10 400 python -u bench.py --gpus 1 --steps 20 --warmup 5 > "$OUT/bench20.json" 2> "$OUT/bench20.err"
timeout -k 10 600 python -u bench.py --full > "$OUT/bench100.json" 2> "$OUT/bench100.err"
