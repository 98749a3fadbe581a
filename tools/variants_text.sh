# A/B of prebuilt library variants on the default bench's text leg (see tools/variants_run.sh).  Usage: bash tools/variants_text.sh v1 v2 ...
set -e
OUT=${OUT:-tool_out}; mkdir -p $OUT
KEEP=$OUT/lib_keep.so
cp znippy_amd/libznippy_hip.so $KEEP
for v in "$@"; do
  cp build_variants/lib_$v.so znippy_amd/libznippy_hip.so
  timeout -k 10 300 python bench.py --steps 10 --warmup 2 --full --no-cpu-baseline > $OUT/vart_${v}.log 2>&1 || { echo "FAILED $v"; tail -5 $OUT/vart_${v}.log; cp $KEEP znippy_amd/libznippy_hip.so; exit 1; }
  tail -1 $OUT/vart_${v}.log | python -c "
import json,sys
d=json.loads(sys.stdin.read())
t=d['read_text_archive']
print('$v', 'c2 read', d['ms_per_step'], 'write', d['compress_ms_per_step'], 'text ms', t['ms_per_step'], {k:v for k,v in t['kernel_ms'].items() if v>0.05})
"
done
cp $KEEP znippy_amd/libznippy_hip.so
