#!/bin/bash
# Produces the per-round evidence under gpurun_out/$R (copy what is to be judged into profiles/):
#   PMC passes of the step's dominant kernel (-> profiles/$R_pmc_dominant_kernel.json, read by bench.py for roofline.traffic),
#   the bench lines (fine-tune + meta), rocprofv3 --kernel-trace --stats of the same bench command, per-layer reports.
# usage: tools/round_artifacts.sh r03
R=${1:-r06}
O=$PWD/gpurun_out/$R; mkdir -p $O
export TMPDIR=/tmp
python3 bench.py --full --steps 20 --no-cpu-baseline --no-meta --no-ab > $O/bench_quick.json 2> $O/bench_quick.err
K=$(python3 -c "import json;print(json.load(open('$O/bench_quick.json'))['roofline']['kernel'])")
echo "dominant kernel: $K"
tools/pmc_dominant.sh $R "$K" 3
cp $O/pmc_dominant_kernel.json profiles/${R}_pmc_dominant_kernel.json
python3 bench.py --full > $O/bench_b3.json 2> $O/bench.err; tail -c 400 $O/bench_b3.json
python3 bench.py --full --metric meta > $O/bench_meta_b1.json 2> $O/bench_meta.err; tail -c 300 $O/bench_meta_b1.json
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -- python3 bench.py --full --no-cpu-baseline --no-meta --no-ab > $O/prof_bench.json 2> $O/prof.err
find $O/prof -name '*kernel_stats.csv' | head -1 | xargs -I{} cp {} $O/bench_b3_kernel_stats.csv
head -6 $O/bench_b3_kernel_stats.csv
rm -rf $O/prof
tools/layer_prof.sh $R 3 > /dev/null 2>&1
tools/layer_prof.sh $R 1 > /dev/null 2>&1
python3 tools/parity_margins.py > $O/parity_margins.txt 2>&1
python3 tools/two_engines.py 1 > $O/two_engines_b1.txt 2>&1
python3 tools/two_engines.py 3 > $O/two_engines_b3.txt 2>&1
python3 tools/steptime_gn.py > $O/gn_steptime.txt 2>&1
tools/gn_profile.sh $R/gn 3 > /dev/null 2>&1; cp $O/gn/gn_b3_kernel_stats.csv $O/gn_b3_kernel_stats.csv 2>/dev/null
python3 tools/eval_sequence_time.py > $O/eval_sequence_time.txt 2>&1
