#!/bin/bash
# SQ counters of pd_attn_d8's DMA-staged kernel at the headline's shape (scripts/attn_d8_launch.py), one rocprofv3 pass per counter group
# with the kernel trace as the only tracing; summed per launch into $OUT/<tag>.txt (default build_ab/attn_d8_counters, git-ignored).  PD_LIB selects the build.
#   bash scripts/attn_d8_counters.sh <tag>
set -e
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
TAG=${1:-tree}
OUT=${OUT:-build_ab/attn_d8_counters}
mkdir -p $OUT
: > $OUT/$TAG.txt
i=0
for grp in "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAVES GRBM_GUI_ACTIVE" \
           "SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INST_CYCLES_VALU SQ_INSTS_VALU_TRANS_F32" \
           "SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY" \
           "SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE" \
           "SQ_IFETCH SQ_IFETCH_LEVEL SQ_INSTS_SALU SQ_ACTIVE_INST_SCA" \
           "SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_MFMA SQ_ACTIVE_INST_MISC SQ_INSTS_VMEM"; do
  i=$((i + 1))
  d=/tmp/attn_d8_pmc_${TAG}_$i
  rm -rf $d
  rc=0
  timeout -k 10 150 rocprofv3 --kernel-trace --pmc $grp --output-format csv -d $d -- python3 scripts/attn_d8_launch.py --launches 3 > $OUT/${TAG}_pass$i.log 2>&1 || rc=$?
  # a counter this profiler version does not offer fails its pass only; a time limit or a crash ends the collection
  if [ $rc -ne 0 ]; then
    echo "pass $i ($grp): exit $rc" >> $OUT/$TAG.txt
    if [ $rc -ge 124 ]; then cat $OUT/$TAG.txt; exit $rc; fi
    continue
  fi
  python3 - "$(ls $d/*/*_counter_collection.csv | head -1)" >> $OUT/$TAG.txt <<'PY'
import collections, csv, sys
per, disp = collections.defaultdict(float), set()
for r in csv.DictReader(open(sys.argv[1])):
    if "attn_glds_kernel" in r["Kernel_Name"]:
        per[r["Counter_Name"]] += float(r["Counter_Value"]); disp.add(r["Dispatch_Id"])
for k, v in per.items():
    print(f"{k:28s} {v / max(len(disp), 1):16.1f} per launch ({len(disp)} launches)")
PY
done
cat $OUT/$TAG.txt
