#!/usr/bin/env bash
# Kernel trace of one bench workload (c5 / c2 / c3): rocprof summary + per-step timeline.
# Usage (via gpurun): bash tools/wl_trace.sh TAG WORKLOAD [extra bench args]
set -o pipefail
O=${U2GNN_OUT:-bench_out}   # output directory, relative to the repository root
TAG=${1:-wl}; W=${2:-c2}; shift 2
R=${U2GNN_ROOT:-$(pwd)}; cd "$R"; mkdir -p $O; export TMPDIR=/tmp
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d "$R/$O/${TAG}_p" -o run -- python bench.py --full --workload $W --steps 20 --warmup 3 --cpu-baseline 0 "$@" > $O/${TAG}.json 2> $O/${TAG}.err || { tail -20 $O/${TAG}.err; exit 1; }
DB=$(find "$R/$O/${TAG}_p" -name '*.db' | head -1)
python tools/kstats.py "$DB" $O/${TAG}_kstats.txt "$TAG $W" $O/${TAG}_ktrace.csv > /dev/null && python tools/timeline.py $O/${TAG}_ktrace.csv 5 > $O/${TAG}_timeline.txt
rm -rf "$R/$O/${TAG}_p"
