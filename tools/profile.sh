#!/usr/bin/env bash
# Runs on the GPU box (through gpurun): rocprofv3 kernel-trace stats and separate PMC passes over a bench
# command, written under gpurun_out/prof_$TAG/ .  Counter passes are kept apart from --kernel-trace/--stats and
# from each other (TCC slot limits; see MI355X_MICROARCH.md).  The program after `--` is python3 itself.
#   tools/profile.sh TAG [default|headline|nmc|nmc_all|nmc_eu] [PASS ...]
# headline: the timed steps of the default workload alone (no side legs).  PASS: trace, pmc_sq, pmc_sq2, pmc_wait,
# pmc_wr, pmc_rd — all of them when none is named.  The library profiled is the one MCAMD_LIB names, if set.
set -uo pipefail
TAG="${1:-r02}"
MODE="${2:-default}"
shift $(( $# < 2 ? $# : 2 ))
PASSES=("$@")
[ ${#PASSES[@]} -eq 0 ] && PASSES=(trace pmc_sq pmc_sq2 pmc_wait pmc_wr pmc_rd)
R="${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}"
OUT="$R/gpurun_out/prof_$TAG"
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
python3 -c "import sys; sys.path.insert(0, '$R'); import importlib; print(importlib.import_module('monte-carlo-project-cuda_amd').capi.build_id())" > "$OUT/build_id.txt"
case "$MODE" in
  default) BENCH=(python3 "$R/bench.py" --steps 40 --warmup 5 --full --no-cpu-baseline --no-accuracy --no-sweep --no-nmc) ;;
  headline) BENCH=(python3 "$R/bench.py" --steps 40 --warmup 5) ;;
  nmc)     BENCH=(python3 "$R/bench.py" --workload nmc --steps 1 --warmup 1 --no-cpu-baseline) ;;
  nmc_all) BENCH=(python3 "$R/tools/nmc_strategies.py") ;;
  nmc_eu)  BENCH=(python3 "$R/bench.py" --workload nmc --nmc-window european --steps 1 --warmup 0 --no-cpu-baseline) ;;
  *) echo "unknown mode $MODE"; exit 2 ;;
esac
SQ1="SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_WAIT_ANY GRBM_GUI_ACTIVE"
SQ2="SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_LDS SQ_INSTS_SALU SQ_INSTS_VMEM_WR SQ_ACTIVE_INST_VMEM SQ_BUSY_CU_CYCLES"
# where a wavefront's cycles go when it does not issue: SQ_WAIT_ANY parked on s_waitcnt or a barrier, SQ_WAIT_INST_ANY
# stalled at issue, SQ_WAIT_INST_LDS the part of that stalled at the LDS queue; SQ_WAVE_CYCLES again as this pass's own base
SQ3="SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_LDS"
rc=0
for p in "${PASSES[@]}"; do
  case "$p" in
    trace)    ARGS=(--kernel-trace --stats) ;;
    pmc_sq)   ARGS=(--pmc $SQ1) ;;
    pmc_sq2)  ARGS=(--pmc $SQ2) ;;
    pmc_wait) ARGS=(--pmc $SQ3) ;;
    pmc_wr)   ARGS=(--pmc WRITE_SIZE) ;;
    pmc_rd)   ARGS=(--pmc FETCH_SIZE) ;;
    *) echo "unknown pass $p"; exit 2 ;;
  esac
  timeout -k 10 400 rocprofv3 "${ARGS[@]}" --output-format csv -d "$OUT/$p" -- "${BENCH[@]}" > "$OUT/$p.log" 2>&1
  rc=$?
  [ $rc -eq 0 ] || break      # a pass that failed or ran out of time: start nothing more on the GPU
done
# keep the merge small: drop everything but csv + logs
find "$OUT" -type f ! -name '*.csv' ! -name '*.log' ! -name 'build_id.txt' -delete 2>/dev/null
echo "profile $TAG/$MODE rc=$rc"
exit $rc
