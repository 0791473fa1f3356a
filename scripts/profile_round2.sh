# round 2: the driver's own bench command under rocprofv3 (kernel trace + stats), plus the un-profiled line beside it
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p $OUT      # where the results go
export TMPDIR=/tmp
TAG=${1:-r02c}
python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/${TAG}_bench_driver.json 2> $OUT/${TAG}_bench_driver.err
rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_kt -o kt --output-format csv -- python3 bench.py --gpus 1 --steps 20 --warmup 5 --no-side-legs --cpu-seconds 0 > $OUT/${TAG}_kt.json 2>/dev/null
python3 bench.py --full > $OUT/${TAG}_bench_default.json 2> $OUT/${TAG}_bench_default.err
tail -1 $OUT/${TAG}_bench_driver.json | cut -c1-300
tail -1 $OUT/${TAG}_bench_default.json | cut -c1-300
ls $OUT/${TAG}_kt
