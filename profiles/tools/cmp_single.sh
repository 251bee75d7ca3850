OUT=${OUT:-bench_out}; mkdir -p $OUT
for v in main ldsp; do
  unset MPP_LIB_PATH; [ $v != main ] && export MPP_LIB_PATH=$PWD/mpp_cnn_rs_object_detection_amd/libmppgpu_$v.so
  python bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-convergence --batched-tiles 0 > $OUT/cmp_$v.json 2> $OUT/cmp_$v.err
  python -c "
import json; d=json.load(open('$OUT/cmp_$v.json')); print('$v single', round(d['value']), 'kernel_ms', round(d['roofline']['kernel_ms'],2), 'matched', d['config']['gt_matched_within_2px'])"
done
