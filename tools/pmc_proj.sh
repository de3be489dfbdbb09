#!/bin/bash
# PMC counters of the projection-matching kernels alone (tools/proj_rate.py: one primed 128-lane group on the corridor sequence):
#   tools/pmc_proj.sh [lib] [tag] [outdir]
#   lib     the library to measure (default: the tree's) - e.g. the parent commit's build
#   tag     suffix of the output directory's name (default: none)
#   outdir  where the run's output and error logs are kept (default: /tmp/pmc_proj<tag>)
# One run under its own time limit, counters only (no API or kernel tracing beside them); VSLAM_PROJ_SELECT passes through.
# Prints the per-launch average of every counter for the k_proj_* kernels over the whole run (priming included: the counters
# cannot be switched on mid-run).
HERE=$(cd "$(dirname "$0")/.." && pwd)
LIB=${1:-$HERE/gtsam-vslam_amd/libvslam_hip.so}
OUT=${3:-/tmp/pmc_proj${2:-}}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 280 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_SMEM --output-format csv -d $OUT/p -o p -- \
    python3 $HERE/tools/proj_rate.py --lib $LIB --prime 60 --steps 10 --reps 1 > $OUT/out.txt 2> $OUT/err.txt
rc=$?
if [ $rc -ne 0 ]; then
  echo "counter pass failed (exit $rc): stopping"; tail -5 $OUT/err.txt
  exit $rc
fi
python3 - <<PY
import csv,glob,collections
agg=collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob("$OUT/p/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        k=r['Kernel_Name'].replace('vslam::','').split('(')[0].replace('void ','')
        agg[k][r['Counter_Name']].append(float(r['Counter_Value']))
for k in sorted(agg):
    if not k.startswith('k_proj'): continue
    print(k, "launches", len(next(iter(agg[k].values()))), {c: round(sum(v)/len(v)) for c,v in sorted(agg[k].items())})
PY
tail -1 $OUT/out.txt
rm -rf $OUT/p
