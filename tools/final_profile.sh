#!/bin/bash
# Round record: the full bench line (--full), rocprofv3 kernel trace of a plain bench run, and the two PMC passes for HBM-side
# traffic of the GEMM launches. usage: tools/final_profile.sh <tag> [outdir]     (outputs under outdir, default build/profile; copy into profiles/)
TAG=$1
O=${2:-build/profile}
export TMPDIR=${TMPDIR:-/tmp}; cd "$(dirname "$0")/.." && mkdir -p $O
python3 bench.py --full > $O/${TAG}_bench_default.json 2> $O/${TAG}_bench.log
# (a plain run: only the setup, warm-up and timed steps of the headline configuration are in the trace, so that the per-kernel
# averages can be compared with the bench line's roofline object)
timeout 600 rocprofv3 --kernel-trace --stats -d $O/prof_t -o t -- python3 bench.py > $O/${TAG}_bench_under_rocprof.json 2>/dev/null
python3 tools/rocprof_summary.py $O/prof_t/t_results.db $O/${TAG}_kernel_trace.md "rocprofv3 --kernel-trace --stats -- python3 bench.py  (3 one-slice setup calls + 2 warm-up + 6 timed steps of 32 slices)"
rm -rf $O/prof_t
timeout 900 rocprofv3 --pmc FETCH_SIZE -d $O/pmc_f -o f -- python3 bench.py --full --no-cpu-baseline --steps 2 --warmup 1 > /dev/null 2>&1
timeout 900 rocprofv3 --pmc WRITE_SIZE -d $O/pmc_w -o w -- python3 bench.py --full --no-cpu-baseline --steps 2 --warmup 1 > /dev/null 2>&1
F=$(ls $O/pmc_f/*.db $O/pmc_f/*/*.db 2>/dev/null | head -1); W=$(ls $O/pmc_w/*.db $O/pmc_w/*/*.db 2>/dev/null | head -1)
python3 tools/pmc_traffic.py $F $W $O/${TAG}_gemm_pmc_traffic.json "rocprofv3 --pmc FETCH_SIZE | WRITE_SIZE -- python3 bench.py --full --no-cpu-baseline --steps 2 --warmup 1"
rm -rf $O/pmc_f $O/pmc_w
cat $O/${TAG}_bench_default.json
