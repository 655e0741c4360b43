#!/bin/bash
# Runs on the GPU box (via gpurun): rocprofv3 kernel trace + separate PMC passes of bench.py.
# Usage: scripts/profile_bench.sh <tag>   -> gpurun_out/prof_<tag>/
TAG=${1:-r1}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$GRAFT_REPO_ROOT/gpurun_out/prof_$TAG
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
# Every pass profiles THE DRIVER'S COMMAND (--steps 20 --warmup 5) without its side measurements (--full for the view counts of the
# roofline object, which scripts/collect_profiles.py reads from the SQ pass's line): the windows of bench.py are replicas
# of the same 20 steps of the same training run, so the kernels of every pass are the kernels of the headline (VERDICT r4 weak #5/#6:
# a 200-step trace of a scene that trains while it is timed was a different workload from the 20 steps the driver times).
CMD="python $ROOT/bench.py --steps 20 --warmup 5 --full --no-cpu-baseline --no-extra --no-pmc --no-stages"
LONG="$CMD"
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o trace -- $LONG > $OUT/bench_trace.json 2> $OUT/trace.err
echo "trace exit $?"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -o fetch -- $CMD > $OUT/bench_fetch.json 2> $OUT/fetch.err
echo "fetch exit $?"
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -o write -- $CMD > $OUT/bench_write.json 2> $OUT/write.err
echo "write exit $?"
# instruction counters of the blend kernels (for the VALU roofline: wave-instructions per blended intersection)
rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY --output-format csv -d $OUT/pmc_sq -o sq -- $CMD > $OUT/bench_sq.json 2> $OUT/sq.err
echo "sq exit $?"
find $OUT -name "*.csv" | head -20
# keep only the small summaries (the raw kernel trace can be large)
find $OUT -name "*kernel_trace.csv" -size +20M -delete
du -sh $OUT
