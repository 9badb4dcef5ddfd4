#!/bin/bash
# A/B of bench.py lines between builds of the library, alternated (profiles/store_path/ab.txt):
#   tools/store_path_ab.sh ROUNDS "BENCH ARGS" name=path/to/librsmi.so [name=path ...]
# Each run is its own process under its own time limit (RSMI_LIB selects the build); a run that
# fails ends the script.  Prints value (GiB/s), the kernels' event-timed GB/s and launch times
# (us: bench.py's HIP events around every 5th step, the encode's average and median), then
# median / min / max / range of value per build.
set -o pipefail
cd "$(dirname "$0")/.."
ROUNDS=$1
ARGS=$2
shift 2
echo "build    rep       value  enc GB/s  rec GB/s  enc us  enc med us  rec us"
T=$(mktemp)
for rep in $(seq 1 "$ROUNDS"); do
  for nv in "$@"; do
    name=${nv%%=*}
    lib=${nv#*=}
    out=$(RSMI_LIB=$(pwd)/$lib timeout -k 10 200 python bench.py $ARGS --steps 50 2>/dev/null) || { echo "$name $rep failed"; exit 1; }
    echo "$out" | python3 -c "
import json, sys
d = json.loads(sys.stdin.read().strip().splitlines()[-1]); r = d.get('reconstruct', {}); f = d['roofline']
rec = r.get('avg_launch_ms')
print('%-8s %-3s %11.2f %9.1f %9s %7.1f %11.1f %7s' % ('$name', '$rep', d['value'], f['achieved'], r.get('achieved_GBs'),
      f['avg_launch_ms'] * 1e3, f['median_launch_ms'] * 1e3, '%.1f' % (rec * 1e3) if rec else None))" | tee -a "$T"
  done
done
python3 - "$T" <<'EOF'
import statistics, sys
runs = {}
for ln in open(sys.argv[1]):
    p = ln.split()
    runs.setdefault(p[0], []).append(float(p[2]))
base = statistics.median(next(iter(runs.values())))
for k, v in runs.items():
    print("  %-7s median %8.2f  min %8.2f  max %8.2f  range %5.2f  vs %s %+.2f %%" % (
        k, statistics.median(v), min(v), max(v), max(v) - min(v), next(iter(runs)), (statistics.median(v) / base - 1) * 100))
EOF
rm -f "$T"
