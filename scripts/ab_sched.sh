#!/bin/bash
# Autotune a schedule for the bench config, then A/B it against the committed one (same box),
# ROUNDS times: the committed file in radiancecascade2dglobalillumination_amd/tuning/ vs $OUT/tuning_new.json
# (OUT: where the logs and the new schedule go, default bench_out).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 1
OUT=${OUT:-bench_out}
mkdir -p $OUT; export TMPDIR=/tmp
timeout -k 10 300 python bench.py --autotune --steps 5 --save-tuning $OUT/tuning_new.json \
  > $OUT/tune_new.log 2>&1 || exit $?
cat $OUT/tuning_new.json; echo
for i in $(seq ${ROUNDS:-3}); do
  for s in "" "--load-tuning $OUT/tuning_new.json"; do
    timeout -k 10 120 python bench.py --full --no-cpu-baseline --steps 20 $s > $OUT/ab.log 2>&1 || exit $?
    python3 -c "import json; d=json.loads(open('$OUT/ab.log').read().strip().splitlines()[-1]); print('${s:-committed}'[-20:], d['value'], d['rc_ms_per_frame'], d['rc_level_ms'])"
  done
done
