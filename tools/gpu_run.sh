#!/bin/bash
# One GPU session: parity tests, smoke, bench, rocprofv3 kernel trace.  Each GPU step has its own
# time limit; a crash/abort/timeout (exit >= 124 or 134/139) stops the script, a plain test failure
# (exit 1) does not.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export OUT_DIR="${OUT_DIR:-bench_out}"   # where logs and results go
mkdir -p "$OUT_DIR"
export TMPDIR=/tmp
STEPS="${STEPS:-tests smoke bench prof}"
fatal() { local rc=$1; [ "$rc" -ge 124 ] || [ "$rc" -eq 134 ] || [ "$rc" -eq 139 ]; }
for s in $STEPS; do
  case "$s" in
    tests)
      timeout -k 10 ${T_TESTS:-420} python -u -m pytest tests -m gpu -q -x --timeout 120 --timeout-method thread ${PYTEST_K:+-k "$PYTEST_K"} > $OUT_DIR/pytest_gpu.log 2>&1; rc=$?
      tail -5 $OUT_DIR/pytest_gpu.log; echo "tests rc=$rc" ;;
    smoke)
      timeout -k 10 180 python -c "import __graft_entry__ as g; g.smoke()" > $OUT_DIR/smoke.log 2>&1; rc=$?
      tail -3 $OUT_DIR/smoke.log; echo "smoke rc=$rc" ;;
    bench)
      timeout -k 10 300 python bench.py --full ${BENCH_ARGS:-} > $OUT_DIR/bench.log 2>&1; rc=$?
      tail -3 $OUT_DIR/bench.log; echo "bench rc=$rc" ;;
    ab)  # quick env variants (no CPU baseline, headline mode only; FMA=--exact selects exact accumulation)
      : > $OUT_DIR/ab.log
      IFS=';' read -ra VARS <<< "${AB:-X=1;FMA=--exact}"
      for v in "${VARS[@]}"; do
        env $v bash -c 'timeout -k 10 120 python bench.py --full --no-cpu-baseline --no-alt --steps 300 $FMA' >> $OUT_DIR/ab.log 2>&1; rc=$?
        echo "$v rc=$rc" >> $OUT_DIR/ab.log
        fatal $rc && break
      done
      grep -o '"value": [0-9.]*\|"kernels_ms": {[^}]*}\|VW_NV.*' $OUT_DIR/ab.log ;;
    configs)  # the other BASELINE configs, one bench line each (no CPU baseline)
      : > $OUT_DIR/configs.log
      for c in ${CONFIGS:-sym8-denoise db8-stream coif5-f32}; do
        timeout -k 10 240 python bench.py --full --config $c --no-cpu-baseline --steps ${CFG_STEPS:-10} --warmup 3 >> $OUT_DIR/configs.log 2>&1; rc=$?
        echo "$c rc=$rc" >> $OUT_DIR/configs.log
        fatal $rc && break
      done
      grep -o '"value": [0-9.]*\|"kernels_ms": {[^}]*}\|^[a-z0-9-]* rc=.*' $OUT_DIR/configs.log ;;
    prof)
      timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT_DIR/prof -o run -- python3 bench.py --full --no-cpu-baseline ${BENCH_ARGS:-} > $OUT_DIR/prof.log 2>&1; rc=$?
      tail -3 $OUT_DIR/prof.log; echo "prof rc=$rc" ;;
    traffic)  # HBM bytes per launch (PMC FETCH_SIZE / WRITE_SIZE, separate passes) -> $OUT_DIR/hbm_traffic_<cfg>.json
      rm -rf $OUT_DIR/pmc
      PMC_GROUPS="FETCH_SIZE
WRITE_SIZE" BENCH_ARGS="${BENCH_ARGS:-}" bash tools/pmc.sh; rc=$?
      if [ $rc -eq 0 ]; then
        python3 tools/hbm_traffic.py $OUT_DIR/pmc > $OUT_DIR/hbm_traffic_${CFG:-db4}.json
        python3 tools/pmc_summary.py $OUT_DIR/pmc > $OUT_DIR/pmc_traffic_${CFG:-db4}.txt
        cat $OUT_DIR/hbm_traffic_${CFG:-db4}.json
      fi
      echo "traffic rc=$rc" ;;
    *) echo "unknown step $s"; rc=0 ;;
  esac
  if fatal $rc; then echo "fatal rc=$rc at step $s, stopping"; exit $rc; fi
done
exit 0
