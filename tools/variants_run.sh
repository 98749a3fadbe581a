# A/B of prebuilt library variants (build_variants/lib_*.so, built here by hand from -D flags): each takes the library's
# place in turn and runs the named workloads; one line per variant and workload.  Usage: bash tools/variants_run.sh "c4store c5" v0 v1 ...
set -e
OUT=${OUT:-tool_out}; mkdir -p $OUT
KEEP=$OUT/lib_keep.so
W="$1"; shift
cp znippy_amd/libznippy_hip.so $KEEP
for v in "$@"; do
  cp build_variants/lib_$v.so znippy_amd/libznippy_hip.so
  for w in $W; do
    timeout -k 10 300 python bench.py --workload $w --steps 20 --warmup 3 --full --no-cpu-baseline > $OUT/var_${v}_$w.log 2>&1 || { echo "FAILED $v $w"; tail -5 $OUT/var_${v}_$w.log; cp $KEEP znippy_amd/libznippy_hip.so; exit 1; }
    tail -1 $OUT/var_${v}_$w.log | python -c "
import json,sys
d=json.loads(sys.stdin.read())
print('$v', '$w', 'read ms', d['ms_per_step'], 'write ms', d['compress_ms_per_step'], d['roofline']['kernel_ms'], d['compress_kernel_ms'])
"
  done
done
cp $KEEP znippy_amd/libznippy_hip.so
