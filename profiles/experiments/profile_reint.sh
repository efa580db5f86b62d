# per-kernel times of the three forms of the re-integration batch (bench.py --reint), rocprofv3 kernel trace
export TMPDIR=/tmp
R=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${PROFILE_RAW:-$R/profiles/raw}
mkdir -p $OUT
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r3_reint_stats -- python3 $R/bench.py --full --steps 60 --warmup 10 --no-cpu-baseline --no-stress --no-extra-rates --mode device > $OUT/r3_reint_stats.log 2>&1; echo rc=$?
