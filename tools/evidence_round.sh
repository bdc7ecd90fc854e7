set -o pipefail
O=${1:?usage: tools/evidence_round.sh OUTDIR}
mkdir -p $O
python3 -m pytest tests -q -m gpu -p no:cacheprovider > $O/r6_suite_final.log 2>&1; echo "suite rc $?"; tail -3 $O/r6_suite_final.log
python3 bench.py --full > $O/r6_bench_default.json 2> $O/r6_bench_default.err; echo "bench rc $?"; wc -c $O/r6_bench_default.json
python3 bench.py --gpus 1 --steps 20 --warmup 5 > $O/r6_bench_driver_shape.json 2> $O/r6_bench_driver_shape.err; echo "bench(driver shape) rc $?"
python3 bench.py --full --extras-verbose > $O/r6_bench_verbose.json 2> $O/r6_bench_verbose.err; echo "bench(verbose) rc $?"
bash tools/profile_round.sh r6 all > $O/r6_profile_round.log 2>&1; echo "profile rc $?"
ls gpurun_out/prof_r6 | head -60
