#!/bin/bash
# Every BASELINE config as a bench side line, with the copy-inclusive leg (host-resident
# data through page-locked buffers) and the CPU baseline.  One JSON line per config, kept as
# OUTDIR/cfg_<config>.json.   tools/bench_all_configs.sh OUTDIR
set -o pipefail
cd "$(dirname "$0")/.."
D=${1:?usage: bench_all_configs.sh OUTDIR}
mkdir -p "$D"
for c in rs10_4_256k rs4_2_256k rs10_4_1m rs16_4_4m rs2_1_256k; do
  timeout -k 10 300 python bench.py --config $c --copy-inclusive --full --cpu-seconds 5 > $D/cfg_$c.json 2> $D/cfg_$c.err || { tail -20 $D/cfg_$c.err; exit 1; }
  tail -1 $D/cfg_$c.json
done
