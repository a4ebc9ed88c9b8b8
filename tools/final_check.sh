# round-end rehearsal on a GPU box: smoke, the GPU suite, a plain and a --full bench run, and the rocprofv3 kernel stats of the --full bench command
# usage: bash tools/final_check.sh [OUT_DIR]   (default: bench_out/ in the repository root); stops at the first step that fails
set -eo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$ROOT/bench_out}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
cd "$ROOT"
timeout -k 10 600 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
timeout -k 10 1000 python -m pytest tests -x -q -m gpu > "$OUT/final_gpu_tests.log" 2>&1 || { tail -5 "$OUT/final_gpu_tests.log"; exit 1; }
tail -2 "$OUT/final_gpu_tests.log"
timeout -k 10 300 python bench.py > "$OUT/bench_final.json" 2> "$OUT/bench_final.err"; echo "bench rc=$?"
timeout -k 10 600 python bench.py --full > "$OUT/bench_final_full.json" 2> "$OUT/bench_final_full.err"; echo "bench --full rc=$?"
PROF=$(mktemp -d)
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$PROF" -- python3 "$ROOT/bench.py" --full --no-cpu > "$PROF/prof.log" 2>&1; echo "rocprof rc=$?"
f=$(find "$PROF" -name "*kernel_stats.csv" | head -1); cp "$f" "$OUT/final_bench_kernel_stats.csv"; head -3 "$OUT/final_bench_kernel_stats.csv" | cut -c1-120
rm -rf "$PROF"
