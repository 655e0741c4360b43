# Side runs of the benchmark with everything it measures: 6 M / 4K / SH 3, the loader feed, SH 3.
#   scripts/run_extra_benches.sh <output dir>   -> <output dir>/*.json, .err
O=$(realpath -m "${1:?usage: scripts/run_extra_benches.sh <output dir>}"); mkdir -p "$O"
cd "$(dirname "$0")/.."
timeout 300 python bench.py --full --workload 6m_4k --sh-degree 3 --steps 3 --warmup 1 --no-cpu-baseline > $O/6m4k.json 2> $O/6m4k.err; echo "6m4k rc $?"
timeout 200 python bench.py --full --feed loader --no-cpu-baseline > $O/feed.json 2> $O/feed.err; echo "feed rc $?"
timeout 200 python bench.py --full --sh-degree 3 --no-cpu-baseline > $O/sh3.json 2> $O/sh3.err; echo "sh3 rc $?"
