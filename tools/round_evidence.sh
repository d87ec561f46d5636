#!/bin/bash
# Round evidence on the GPU box: rocprofv3 kernel trace + FETCH/WRITE passes of the bench
# (seed stage), kernel trace of the C3 FindMatches, full bench line.
set -o pipefail
TAG=${1:-r01}
bash tools/profile_round.sh $TAG || exit $?
bash tools/prof_c3_mums.sh ${TAG}_c3 > /dev/null || exit 21
# the bench line goes next to the kernel trace that tools/profile_round.sh just wrote
OUT=$(dirname "$(ls -t */"$TAG"/kt.log | head -1)")
timeout -k 10 600 python3 -u bench.py --full > $OUT/bench.json 2> $OUT/bench.err || { tail -5 $OUT/bench.err; exit 22; }
cat $OUT/bench.json
