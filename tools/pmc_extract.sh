#!/bin/bash
# PMC counters of the extraction kernels alone (192 images of the bench's corridor scene): tools/pmc_extract.sh [tree] [tag] [passes]
#   tree    a checkout whose tools/extract_rate.py and built library are measured (default: this one) - e.g. the parent commit
#   tag     suffix of the output directory's name (default: none)
#   passes  how many of the counter passes below to take (default: all four)
# Every pass is a run of its own under its own time limit, counters only (kernel names, no API tracing); the FIRST failing pass
# ends the script - nothing more is started on the GPU after it.
HERE=$(cd "$(dirname "$0")/.." && pwd)
REPO=$GRAFT_REPO_ROOT
[ -n "$REPO" ] || REPO=$HERE
TREE=${1:-$REPO}
OUT=$REPO/gpurun_out/pmc_extract
OUT=$OUT${2:-}
NPASS=${3:-4}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
PASSES=("SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_SMEM"
        "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT"
        "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_SCA SQ_INST_LEVEL_LDS SQ_INST_LEVEL_VMEM"
        "GRBM_GUI_ACTIVE SQ_INSTS_VMEM_WR SQ_BUSY_CU_CYCLES SQ_THREAD_CYCLES_VALU SQ_INSTS_WAVE32_LDS SQ_INSTS_FLAT")
i=0
for C in "${PASSES[@]}"; do
  i=$((i+1))
  [ $i -gt $NPASS ] && break
  timeout -k 10 200 rocprofv3 --kernel-trace --pmc $C --output-format csv -d $OUT/p$i -o p -- python3 $TREE/tools/extract_rate.py 192 4 corridor > $OUT/out$i.txt 2> $OUT/err$i.txt
  rc=$?
  if [ $rc -ne 0 ]; then
    echo "pass $i failed (exit $rc): stopping"; tail -3 $OUT/err$i.txt
    exit $rc
  fi
done
python3 - <<PY
import csv,glob,collections
agg=collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob("$OUT/p*/*counter_collection.csv"):
    for r in csv.DictReader(open(f)):
        k=r['Kernel_Name'].replace('vslam::','').split('(')[0].replace('void ','')
        agg[k][r['Counter_Name']].append(float(r['Counter_Value']))
for k in sorted(agg):
    if not k.startswith('k_'): continue
    print(k, {c: round(sum(v)/len(v)) for c,v in sorted(agg[k].items())})
PY
cat $OUT/out1.txt | tail -1
rm -rf $OUT/p*
