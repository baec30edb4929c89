#!/bin/bash
# $MEASURE_OUT/<round>_* (tools/final_measure.sh; default measure_out/) -> profiles/: the committed summaries, then profiles/pmc.json
cd "$(dirname "$0")/.."
RND=${RND:-r06}
OUT=${MEASURE_OUT:-measure_out}
for d in $OUT/${RND}_*/; do
  n=$(basename $d)
  mkdir -p profiles/$n
  for f in kernel_stats.csv bench_line.json pmc_table.txt pmc_summary.json fwd_gantt.txt; do [ -f $d/$f ] && cp $d/$f profiles/$n/; done
done
for f in $OUT/${RND}_bench_*.json $OUT/${RND}_batch_sweep.txt; do [ -f $f ] && cp $f profiles/; done
python profiles/make_pmc_json.py $RND
