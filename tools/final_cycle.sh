#!/usr/bin/env bash
# Full measurement of the current build: gpu tests -> bench (CPU baseline) -> rocprof kernel trace
# -> PMC HBM traffic table (separate FETCH_SIZE / WRITE_SIZE passes).  Usage: bash tools/final_cycle.sh TAG
set -o pipefail
O=${U2GNN_OUT:-bench_out}   # output directory, relative to the repository root
TAG=${1:-final}
R=${U2GNN_ROOT:-$(pwd)}; cd "$R"; mkdir -p $O; export TMPDIR=/tmp
bash tools/gpu_cycle.sh $TAG || exit 1
bash tools/gpu_pmc.sh $TAG || exit 1
F=$(find "$R/$O/${TAG}_FETCH_SIZE" -name '*.db' | head -1)
W=$(find "$R/$O/${TAG}_WRITE_SIZE" -name '*.db' | head -1)
python tools/pmc_traffic.py "$F" "$W" $O/${TAG}_pmc_traffic.json > $O/${TAG}_pmc.log 2>&1 || { tail $O/${TAG}_pmc.log; exit 1; }
rm -rf "$R/$O/${TAG}_FETCH_SIZE" "$R/$O/${TAG}_WRITE_SIZE"
echo "pmc table written"
