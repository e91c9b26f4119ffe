#!/bin/bash
# usage: [OUT=dir] round_artifacts.sh <tag>   -- everything profiles/README.md cites for one round, written to $OUT/<tag>_*
#   (default ./artifacts; prof_round.sh keeps its own output folder):
#   prof_round.sh (kernel-trace stats, FETCH / WRITE and MFMA-busy PMC passes, flow-op rooflines), the default bench line with
#   its flow / fp32 / parity sub-records (bench.py --full), the R101 384x288 lines, the parity reports and the 300-frame clip log
tag=${1:-r03}
R=${GRAFT_REPO_ROOT:-/root/repo}
cd $R
OUT=${OUT:-artifacts}
mkdir -p $OUT
timeout 1500 tools/dev/prof_round.sh $tag > $OUT/${tag}_prof_round.log 2>&1
export FT_TILE_CACHE=$(cd $OUT && pwd)/tile_cache_$tag.json
timeout 1200 python bench.py --full > $OUT/${tag}_pose_bench_line.json 2> $OUT/${tag}_pose_bench_line.err
timeout 300 python bench.py --full --workload flow --no-extras > $OUT/${tag}_flow_bench_line.json 2>/dev/null
for b in 16 64; do
  timeout 300 python bench.py --full --backbone resnet101 --res 384x288 --batch $b --no-extras --no-cpu-baseline --steps 200 > $OUT/${tag}_pose_r101_384x288_b${b}_bench.json 2>/dev/null
done
timeout 300 python bench.py --full --batch 128 --no-extras --no-cpu-baseline --steps 200 > $OUT/${tag}_pose_r50_b128_bench.json 2>/dev/null
timeout 600 python tests/parity_report.py > $OUT/${tag}_pose_parity_report.json 2>/dev/null
timeout 600 python tests/parity_report.py --workload flow > $OUT/${tag}_flow_parity_report.json 2>/dev/null
timeout 600 python tools/tracking/demo.py --frames 300 --fp16 > $OUT/${tag}_clip_300frames.log 2>&1
cp $FT_TILE_CACHE $OUT/${tag}_tile_benchmark_picks.json
for m in FlowNet2C FlowNet2CS FlowNet2CSS FlowNet2SD FlowNet2; do
  timeout 300 python bench.py --workload flow --flow-model $m --no-extras --no-cpu-baseline --no-roofline --steps 100 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('$m', d['value'], d['ms_per_step'])"
done > $OUT/${tag}_flow_models.txt 2>&1
tail -c 1500 $OUT/${tag}_pose_bench_line.json; tail -5 $OUT/${tag}_clip_300frames.log; cat $OUT/${tag}_flow_models.txt
