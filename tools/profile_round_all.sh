#!/bin/bash
# A whole profile round on the GPU box, from the repository root:  bash tools/profile_round_all.sh <tag> <dir>
# <dir>: the folder tools/profile_round.sh writes <tag>/ under; the figures below go to <dir>/<tag>/ beside its own.
# tools/profile_round.sh, BASELINE configs 3 / 4 / 5 as stated, their kernel statistics, the full bench line at K = 20, the GPU suite.
TAG=${1:-r06}
REPO=$(pwd)
DIR=$(realpath -m "${2:?the folder tools/profile_round.sh writes <tag>/ under}")
OUT=$DIR/$TAG
bash tools/profile_round.sh $TAG > $DIR/${TAG}_profile_round.log 2>&1
tail -2 $DIR/${TAG}_profile_round.log
timeout 300 python bench.py --config 3 > $OUT/config3_full.json 2>/dev/null
timeout 300 python bench.py --config 5 > $OUT/config5_full.json 2>/dev/null
timeout 600 python bench.py --config 4 > $OUT/config4.json 2>/dev/null
cd /tmp && export TMPDIR=/tmp && timeout 300 rocprofv3 --kernel-trace --stats -d /tmp/prof_c3 -o c3 --output-format csv -- python $REPO/tools/config3_batch_profile.py device > /tmp/c3.log 2>&1
cp $(find /tmp/prof_c3 -name "*kernel_stats.csv" | head -1) $OUT/config3_batch_kernel_stats.csv
timeout 300 rocprofv3 --kernel-trace --stats -d /tmp/prof_c5 -o c5 --output-format csv -- python $REPO/bench.py --config 5 --no-cpu-baseline > /tmp/c5.log 2>&1
cp $(find /tmp/prof_c5 -name "*kernel_stats.csv" | head -1) $OUT/config5_kernel_stats.csv
cd $REPO
timeout 300 python bench.py --full --steps 20 --warmup 5 --no-large-bam > $OUT/bench_n1_k20.json 2>/dev/null
timeout 900 python -m pytest tests -m gpu -q > $OUT/gpu_suite_full.log 2>&1
grep -E "passed|failed|FAILED" $OUT/gpu_suite_full.log | tail -4
python - $OUT <<'PY'
import json, sys
out = sys.argv[1]
for f in ('config3_full', 'config5_full', 'config4'):
    d = json.loads(open('%s/%s.json' % (out, f)).read().strip().splitlines()[-1]); print(f, d['value'], d['ms_per_step'], d['host_fed']['value'], d.get('handles_in_parallel', {}).get('value'))
d = json.loads(open('%s/bench_n1.json' % out).read().strip().splitlines()[-1]); print(d['value'], d['roofline']['frac'], d['roofline_streaming']['frac'], d['roofline_streaming']['kernel_ms'])
PY
