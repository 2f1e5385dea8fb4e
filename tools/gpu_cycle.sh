#!/usr/bin/env bash
# One GPU iteration: gpu tests -> bench (with CPU baseline unless NOCPU=1) -> rocprofv3 kernel trace of
# the SAME bench command (its dS average must agree with the bench line's live roofline timing).
# GPU_MAX_HW_QUEUES=8 is set in front of rocprofv3 itself: u2gnn_hip.ensure_hw_queues sets it at import,
# which is too late under rocprofv3 (its preloaded library initialises HIP before the program runs).
# Usage (via gpurun): bash tools/gpu_cycle.sh TAG
set -o pipefail
O=${U2GNN_OUT:-bench_out}   # output directory, relative to the repository root
TAG=${1:-run}
R=${U2GNN_ROOT:-$(pwd)}
cd "$R"
mkdir -p $O
export TMPDIR=/tmp
if [ "${NOTESTS:-0}" != "1" ]; then
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $O/${TAG}_tests.log 2>&1
rc=$?; echo "tests rc=$rc" >> $O/${TAG}_tests.log; tail -3 $O/${TAG}_tests.log
[ $rc -eq 0 ] || exit 1
fi
CPU=1; [ "${NOCPU:-0}" = "1" ] && CPU=0
CMD="python bench.py --full --steps 30 --warmup 5 --cpu-baseline $CPU"
timeout -k 10 600 $CMD > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err || { echo "bench failed"; tail -20 $O/${TAG}_bench.err; exit 1; }
cat $O/${TAG}_bench.json
# the profiled run: the same timed region, without the CPU baseline and the extra lines after it (fp32, on-the-fly
# pipeline), so the trace holds the timed steps' launches (and their averages match the bench line's probe)
PCMD="python bench.py --full --steps 30 --warmup 5 --cpu-baseline 0 --fp32-steps 0 --pipeline-steps 0 --configs 0"
GPU_MAX_HW_QUEUES=8 timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$R/$O/${TAG}_prof" -o run -- $PCMD > $O/${TAG}_prof.log 2>&1
echo "prof rc=$?"
DB=$(find "$R/$O/${TAG}_prof" -name '*.db' | head -1)
[ -n "$DB" ] && python tools/kstats.py "$DB" $O/${TAG}_kstats.txt "$TAG $PCMD (rocprofv3 --kernel-trace --stats)" $O/${TAG}_ktrace.csv > /dev/null && python tools/timeline.py $O/${TAG}_ktrace.csv 5 > $O/${TAG}_timeline.txt
find "$R/$O/${TAG}_prof" -name '*kernel_stats.csv' -exec cp {} $O/${TAG}_kernel_stats.csv \;
rm -rf "$R/$O/${TAG}_prof"
