#!/bin/bash
export FW_ENABLE_KNOBS=1   # the library honours its A/B switches only with this set
# PMC passes for the bench (run on the GPU box): tools/pmc.sh <outdir> [lib.so] [groups: insts waits fetch write -- default all four]
# Counters are collected in their own runs (kernel-trace only), one rocprofv3 pass per counter group.  Each pass runs under its own
# time limit and the script ends with the first pass that fails: nothing more is started on a device that has just faulted.
OUT=$1; LIB=${2:-}; GROUPS_=${3:-insts waits fetch write}
R=$PWD; export TMPDIR=/tmp; mkdir -p $OUT; cd /tmp
[ -n "$LIB" ] && export FW_LIB_PATH=$R/$LIB
run() {
  name=$1; shift
  timeout -k 10 600 rocprofv3 --kernel-trace --pmc "$@" -d $R/$OUT -o $name --output-format csv -- python $R/bench.py --steps 100 --warmup 20 --no-cpu --no-events > $R/$OUT/$name.log 2>&1
  rc=$?; [ $rc -ne 0 ] && { echo "tools/pmc.sh: pass $name ended with status $rc -- stopping"; exit $rc; }
}
for g in $GROUPS_; do
  case $g in
    insts) run insts SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVES SQ_WAVE_CYCLES ;;
    waits) run waits SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_INST_CYCLES_VMEM SQ_WAIT_INST_LDS GRBM_GUI_ACTIVE ;;
    fetch) run fetch FETCH_SIZE ;;
    write) run write WRITE_SIZE ;;
    *) echo "tools/pmc.sh: unknown group $g"; exit 2 ;;
  esac
done
cd $R; ls $OUT
