export TMPDIR=/tmp
R=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${PROFILE_RAW:-$R/profiles/raw}
mkdir -p $OUT
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r3_stats_device -- python3 $R/bench.py --steps 100 --warmup 10 --no-cpu-baseline --no-stress --no-extra-rates --reint 0 --mode device > $OUT/r3_stats_device.log 2>&1; echo stats_device rc=$?
cd $R
python bench.py --full --no-cpu-baseline --reint 0 > $OUT/r3_bench_quick.json 2> $OUT/r3_bench_quick.err; echo rc=$?
tail -c 1500 $OUT/r3_bench_quick.json
