OUT=${1:-$(mktemp -d)}  # where the two bench lines go (argument 1, else a fresh temporary directory)
mkdir -p "$OUT"
echo "output: $OUT"
stat() { grep -E "nr_throttled|throttled_usec" /sys/fs/cgroup/cpu.stat | tr '\n' ' '; }
echo "before: $(stat)"
python3 bench.py --full --no-cpu-baseline --no-scaling-probe --no-compare --no-spmv --steps 20 --warmup 5 > "$OUT/quiet.json" 2>/dev/null
echo "after quiet run: $(stat)"
python3 tools/read_bench_line.py "$OUT/quiet.json" | grep -E "iterations/s|direction_update_us  |stage direction"
# 40 busy loops: far beyond the container's 16-CPU quota -> CFS throttles the whole cgroup, the solver's host thread included
for i in $(seq 40); do ( timeout 45 python3 -c "while True: pass" & ) ; done
sleep 2
python3 bench.py --full --no-cpu-baseline --no-scaling-probe --no-compare --no-spmv --steps 20 --warmup 5 > "$OUT/hogged.json" 2>/dev/null
echo "after hogged run: $(stat)"
python3 tools/read_bench_line.py "$OUT/hogged.json" | grep -E "iterations/s|direction_update_us  |stage direction"
sleep 40
