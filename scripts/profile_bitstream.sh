# the frames-out leg (with_bitstream) under rocprofv3 --kernel-trace --stats: which of the entropy stage's kernels the device time goes
# to, and how many kernels run at once during the leg (the trace holds the headline leg first: the second half of the window is the leg)
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p $OUT      # where the results go
export TMPDIR=/tmp
TAG=${1:-r03e}
rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_bs -o bs --output-format csv -- python3 bench.py --full --gpus 1 --steps 40 --warmup 5 --only-bitstream --cpu-seconds 0 > $OUT/${TAG}_bs.json 2>/dev/null
cp $OUT/${TAG}_bs/bs_kernel_stats.csv $OUT/${TAG}_bitstream_kernel_stats.csv
python3 scripts/concurrency_of_trace.py $OUT/${TAG}_bs/bs_kernel_trace.csv 60 > $OUT/${TAG}_bitstream_concurrency.txt 2>&1 || true
find $OUT/${TAG}_bs -name "*kernel_trace.csv" -size +30M -delete
cut -c1-170 $OUT/${TAG}_bitstream_kernel_stats.csv | head -24
cat $OUT/${TAG}_bitstream_concurrency.txt | head -40
