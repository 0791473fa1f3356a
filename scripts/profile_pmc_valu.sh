cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p $OUT      # where the results go
export TMPDIR=/tmp
rocprofv3 --pmc SQ_INSTS_VALU -d $OUT/r01g_pmc_valu -o valu --output-format csv -- python3 bench.py --full --steps 32 --warmup 8 --gops-per-gpu 1 --cpu-seconds 0 > $OUT/r01g_pmc_valu.json 2>/dev/null
rocprofv3 --pmc SQ_WAVES SQ_INSTS_SALU -d $OUT/r01g_pmc_waves -o waves --output-format csv -- python3 bench.py --full --steps 32 --warmup 8 --gops-per-gpu 1 --cpu-seconds 0 > $OUT/r01g_pmc_waves.json 2>/dev/null
rocprofv3 --kernel-trace --stats -d $OUT/r01g_intra -o intra --output-format csv -- python3 scripts/intra_bench.py > $OUT/r01g_intra.txt 2>/dev/null
ls $OUT/r01g_pmc_valu $OUT/r01g_pmc_waves $OUT/r01g_intra
