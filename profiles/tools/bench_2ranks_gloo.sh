export MPP_DIST_BACKEND=gloo
OUT=${OUT:-bench_out}; mkdir -p $OUT
python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --full --gpus 2 --steps 2 --warmup 1 > $OUT/r02_bench_2rank.json 2> $OUT/r02_bench_2rank.err
tail -c 600 $OUT/r02_bench_2rank.json; tail -3 $OUT/r02_bench_2rank.err
