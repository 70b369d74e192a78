#!/bin/bash
# Round evidence in one GPU session: parity tests, smoke, PMC traffic passes, the bench line (reading
# the fresh traffic json) and the rocprofv3 kernel-trace stats of the C2 bench leg alone (its per-kernel
# averages must agree with the bench line's live HIP-event launch times), then of the secondary legs.
# Every GPU step has its own time limit; the chain stops at the first failure.  Outputs land in
# $OUT/profiles_<tag>/ ($OUT: the session's output folder, given by the caller) and are copied into
# profiles/ afterwards.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
TAG=${1:-r02}
OUT=${OUT:?set OUT to the folder for logs and profiles}
export OUT
mkdir -p $OUT
if [ -z "$SKIP_TESTS" ]; then
timeout -k 10 600 python -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 120 --timeout-method thread -ra \
  > $OUT/pytest_gpu.log 2>&1 || { tail -30 $OUT/pytest_gpu.log; exit 2; }
tail -2 $OUT/pytest_gpu.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -20 $OUT/smoke.log; exit 3; }
tail -1 $OUT/smoke.log
fi
bash tools/gpu_traffic.sh $TAG || exit 4
mkdir -p $OUT/profiles_$TAG
cp $OUT/traffic_$TAG/${TAG}_traffic.json $OUT/profiles_$TAG/${TAG}_traffic.json
cp $OUT/traffic_$TAG/${TAG}_traffic.json profiles/${TAG}_traffic.json
timeout -k 10 600 python bench.py --full --steps 20 --warmup 3 > $OUT/bench_$TAG.log 2>&1 || { tail -30 $OUT/bench_$TAG.log; exit 5; }
grep '^{' $OUT/bench_$TAG.log > $OUT/profiles_$TAG/${TAG}_bench.json
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- \
    python3 bench.py --steps 20 --warmup 3 \
    > $OUT/prof_${TAG}_bench.log 2>&1 || { tail -20 $OUT/prof_${TAG}_bench.log; exit 6; }
grep '^{' $OUT/prof_${TAG}_bench.log > $OUT/profiles_$TAG/${TAG}_bench_under_rocprof.json
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_legs -o run -- \
    python3 bench.py --full --steps 3 --warmup 1 --frames 1024 --no-cpu-baseline > $OUT/prof_${TAG}_legs.log 2>&1 || { tail -20 $OUT/prof_${TAG}_legs.log; exit 7; }
cp $(find $OUT/prof_$TAG -name "*kernel_stats.csv" | head -1) $OUT/profiles_$TAG/${TAG}_kernel_stats.csv
cp $(find $OUT/prof_${TAG}_legs -name "*kernel_stats.csv" | head -1) $OUT/profiles_$TAG/${TAG}_kernel_stats_legs.csv
ls $OUT/profiles_$TAG
echo refresh done
