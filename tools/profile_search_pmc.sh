#!/bin/bash
# The two SQ counter passes of the bench kernel, each in a run of its own (issue rate vs LDS cycles vs dependency waits):
#   pass 1: SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_LDS_BANK_CONFLICT
#   pass 2: SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_INSTS_VMEM
# Usage (repository root, on the GPU): tools/profile_search_pmc.sh OUTDIR  -> OUTDIR/{pass1,pass2}_summary.txt
set -u
if [ $# -ne 1 ]; then echo "usage: $0 OUTDIR" >&2; exit 2; fi
REPO=$(pwd); mkdir -p "$1"; OUT=$(cd "$1" && pwd)
PB="python $REPO/bench.py --gpus 1 --steps 4 --warmup 1"
timeout -k 10 300 rocprofv3 --pmc SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_LDS_BANK_CONFLICT \
    -d "$OUT/pass1" -o bench -- $PB > "$OUT/pass1.txt" 2> "$OUT/pass1.err" &&
timeout -k 10 300 rocprofv3 --pmc SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_INSTS_VMEM \
    -d "$OUT/pass2" -o bench -- $PB > "$OUT/pass2.txt" 2> "$OUT/pass2.err"
rc=$?
for p in pass1 pass2; do python tools/summarize_search_pmc.py "$OUT/$p" > "$OUT/${p}_summary.txt" 2>&1; cat "$OUT/${p}_summary.txt"; done
exit $rc
