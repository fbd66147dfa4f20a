#!/bin/bash
# PMC passes (counters only, no trace domains), one rocprofv3 run per group: the SQ groups, then the memory side —
# FETCH_SIZE, WRITE_SIZE (a pass each) and the L2's hits / misses / requests.
# usage (on the GPU box): bash tools/pmc_variants.sh <outdir> [env assignments...]
#   PMC_CMD    the command to profile (default: tools/profile_variants.py metric; the records of the bench workload use
#              "python3 bench.py --no-cpu-baseline --no-also --steps 300 --warmup 20")
#   PMC_GROUPS the groups, separated by ';' (default: all six)
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
out=$(mkdir -p "$1" && cd "$1" && pwd); shift
for kv in "$@"; do export "$kv"; done
cmd=${PMC_CMD:-python3 $root/tools/profile_variants.py metric}
groups=${PMC_GROUPS:-SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_BUSY_CYCLES SQ_WAVE_CYCLES;SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_LDS SQ_INST_CYCLES_SALU;SQ_THREAD_CYCLES_VALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SMEM SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS;FETCH_SIZE;WRITE_SIZE;TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum}
cd "$root" && export TMPDIR=/tmp
i=0
IFS=';' read -ra list <<< "$groups"
for grp in "${list[@]}"; do
  i=$((i+1))
  timeout -k 10 240 rocprofv3 --pmc $grp --output-format csv -d $out/p$i -o p -- $cmd > $out/p$i.log 2>&1
done
python3 $root/profiles/summarize_pmc.py $out/p*/*counter_collection.csv > $out/pmc.json
