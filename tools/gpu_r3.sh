#!/bin/bash
# Round-3 GPU sessions.  usage: bash tools/gpu_r3.sh [tests] [newtests] [bench] [benchq] [prof] [pmc] [pmcgstep] [probe] [saveexp] [wgradexp] [soak] [gtimeline] [gstep]
REPO=$(cd "$(dirname "$0")/.." && pwd)
export OUT=${OUT:-$REPO/logs}        # every log and profile of this script goes here
cd "$REPO"
set -u
mkdir -p $OUT
export TMPDIR=/tmp
Q="--full --no-cpu-baseline --no-gstep --no-f32 --no-sweep64"
for what in "$@"; do
case $what in
tests)
  timeout 1500 python -m pytest tests -m gpu -q -s --maxfail=10 > $OUT/tests_full.log 2>&1; grep -h 'parity\]\|dist\]' $OUT/tests_full.log | grep -v 'print(' > $OUT/tests_parity.log; tail -300 $OUT/tests_full.log > $OUT/tests.log
  echo "pytest exit: $?" >> $OUT/tests.log
  timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
  echo "smoke exit: $?" >> $OUT/smoke.log
  tail -n 5 $OUT/tests.log; tail -n 4 $OUT/smoke.log ;;
newtests)   # the tests added this round, without -x, verbose: what they measure decides their asserts
  timeout 1200 python -m pytest tests/test_gpu_parity.py -m gpu -q -s -k "${NEWTESTS:-all_rays or config5 or at_scale or rccl or ddp or repacked or chunked_backward or single_latent_generator or reference_checkpoint}" > $OUT/newtests_full.log 2>&1; grep -h 'parity\]\|dist\]' $OUT/newtests_full.log | grep -v 'print(' > $OUT/newtests_parity.log; tail -150 $OUT/newtests_full.log > $OUT/newtests.log
  cat $OUT/newtests_parity.log | cut -c1-400; grep -E "passed|failed|^E  |FAILED" $OUT/newtests.log | tail -40 ;;
bench)
  timeout 900 python bench.py --full --gpus 1 --steps 20 --warmup 3 > $OUT/bench.log 2>&1
  echo "bench exit: $?" >> $OUT/bench.log
  tail -2 $OUT/bench.log | cut -c1-6000 ;;
benchq)
  timeout 600 python bench.py --full --gpus 1 --steps 20 --warmup 3 --no-cpu-baseline --no-f32 --no-sweep64 --no-gstep-b6 > $OUT/benchq.log 2>&1
  echo "benchq exit: $?" >> $OUT/benchq.log
  tail -2 $OUT/benchq.log | cut -c1-6000 ;;
prof)
  rm -rf $OUT/prof
  (cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o bench -- python $REPO/bench.py --full --gpus 1 --steps 20 --warmup 3) > $OUT/prof.log 2>&1
  echo "prof exit: $?" >> $OUT/prof.log
  find $OUT/prof -type f ! -name "*stats*" -size +2M -delete
  find $OUT/prof -name "*kernel_stats*" | head -1 | xargs head -12 | cut -c1-200 ;;
pmc)
  rm -rf $OUT/pmc; mkdir -p $OUT/pmc
  i=0
  for set in "FETCH_SIZE" "WRITE_SIZE" "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAVES GRBM_GUI_ACTIVE" "SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_INSTS_MFMA SQ_INSTS_VALU SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY" "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS TCC_HIT_sum TCC_MISS_sum"; do
    i=$((i+1))
    (cd /tmp && timeout 300 rocprofv3 --kernel-trace --pmc $set --output-format csv -d $OUT/pmc/p$i -o pmc -- python $REPO/bench.py --gpus 1 --steps 3 --warmup 1 $Q) > $OUT/pmc/p$i.log 2>&1
    echo "pass $i ($set) exit $?" >> $OUT/pmc/summary.txt
  done
  find $OUT/pmc -type f -size +4M -delete
  python tools/pmc_summary.py $OUT/pmc > $OUT/pmc/siren_pmc_summary.txt 2>&1
  cat $OUT/pmc/siren_pmc_summary.txt ;;
pmcgstep)   # HBM bytes of the generator-step kernels (default and AMP weight-gradient operands) and of the SPATIALSIRENGRID launch
  for gp in f32 amp; do
    GSTEP_ARGS="--B 1 --size 128 --grad-precision $gp" bash tools/pmc_gstep.sh > /dev/null 2>&1
    cp $OUT/pmc_gstep/gstep_pmc_summary.txt $OUT/pmc_gstep_$gp.txt
  done
  rm -rf $OUT/pmc_local; mkdir -p $OUT/pmc_local
  for set in FETCH_SIZE WRITE_SIZE; do
    (cd /tmp && timeout 300 rocprofv3 --kernel-trace --pmc $set --output-format csv -d $OUT/pmc_local/$set -o pmc -- python $REPO/tools/bench_local.py --iters 2 --explicit) > $OUT/pmc_local/$set.log 2>&1
  done
  python - <<'PY' > $OUT/pmc_local.txt 2>&1
import csv, glob, os
from collections import defaultdict
agg = defaultdict(lambda: defaultdict(list))
for f in sorted(glob.glob(os.environ["OUT"] + "/pmc_local/*/**/*counter_collection.csv", recursive=True)):
    for row in csv.DictReader(open(f)):
        n = row["Kernel_Name"]
        if "siren_local_kernel" in n or "siren_kernel" in n or "film_prep" in n:
            agg[n.split("(")[0][-60:]][row["Counter_Name"]].append(float(row["Counter_Value"]))
print("kernel,counter,avg_KiB_per_dispatch,bytes_per_point_at_196608_points,n")
for k in sorted(agg):
    for c, v in sorted(agg[k].items()):
        a = sum(v) / len(v)
        print(f"{k},{c},{a:.6g},{a * 1024 / 196608:.1f},{len(v)}")
PY
  find $OUT/pmc_local -type f -size +2M -delete
  head -20 $OUT/pmc_gstep_f32.txt; grep -E "wgrad|bwd16w" $OUT/pmc_gstep_amp.txt; cat $OUT/pmc_local.txt; tail -3 $OUT/pmc_local/FETCH_SIZE.log ;;
probe)
  ./tools/probe/tr_probe > $OUT/tr_probe.log 2>&1; head -40 $OUT/tr_probe.log ;;
saveexp)   # tools/exp/save_store_variants.sh: forward-save with the tape stores removed / redirected / re-hinted
  for v in "" S_L2 S_NOSTORE S_TEMPORAL S_WAIT2 ""; do
    lib=fenerf_amd/libfenerf_hip.so; [ -n "$v" ] && lib=fenerf_amd/libexp_$v.so
    [ -f $lib ] || continue
    echo -n "variant ${v:-shipped}: "
    FENERF_LIB=$PWD/$lib timeout 200 python tools/time_bwd.py 196608 2>&1 | grep -E "forward|chain" | tr '\n' ' '; echo
  done > $OUT/saveexp.log 2>&1
  cat $OUT/saveexp.log ;;
soak)      # determinism / race soak of the fused render and of the generator step (default and AMP-class)
  timeout 900 python tools/soak_render.py --iters ${SOAK_ITERS:-100} > $OUT/soak_render.log 2>&1; tail -12 $OUT/soak_render.log
  timeout 600 python tools/soak_gstep.py ${SOAK_STEPS:-300} > $OUT/soak_gstep.log 2>&1; tail -3 $OUT/soak_gstep.log ;;
gtimeline)   # per-launch timeline of one generator step (kernel trace only, no counters)
  rm -rf $OUT/gtl; mkdir -p $OUT/gtl
  (cd /tmp && timeout 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/gtl -o gtl -- python $REPO/tools/bench_gstep.py --B 1 --size 128 --skip-eager --iters 4 ${GTL_ARGS:-}) > $OUT/gtl/run.log 2>&1
  python tools/gstep_timeline.py $OUT/gtl ${GTL_STEP:-4} > $OUT/gstep_timeline.txt 2>&1
  find $OUT/gtl -type f -size +2M -delete
  tail -45 $OUT/gstep_timeline.txt ;;
wgradexp)   # tools/exp/wgrad_sq_variants.sh built the libexp_Q_*.so here; time them on one backward chunk
  for v in "" Q_NOSTORE Q_NOSIN Q_NOMFMA Q_NOFRAG ""; do
    if [ -z "$v" ]; then lib=$PWD/fenerf_amd/libfenerf_hip.so; else lib=$PWD/fenerf_amd/libexp_$v.so; fi
    [ -f "$lib" ] || continue
    echo -n "variant ${v:-shipped}: "; FENERF_LIB=$lib timeout 200 python tools/time_wgrad.py 2>&1 | tail -1
  done > $OUT/wgradexp.log 2>&1
  cat $OUT/wgradexp.log ;;
gstep)
  timeout 600 python tools/chunk_sweep.py > $OUT/chunk_sweep.log 2>&1; cat $OUT/chunk_sweep.log ;;
esac
done
exit 0
