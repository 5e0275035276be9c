#!/bin/bash
# GPU box: VBR -V2 / -V5 bench lines for several libraries, alternating
cd $GRAFT_REPO_ROOT
X="--full --no-cpu-baseline --no-extras --no-end-to-end --streams 1024 --seconds 5 --steps 2 --warmup 1"
for i in 1 2; do for L in "$@"; do
  for A in "--vbr 2" "--vbr 5"; do
    LAMEHIP_LIB=$PWD/deprecated-lame-mirror_amd/lamehip/$L python bench.py $X $A 2>/dev/null | grep '^{"metric"' | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$L', '$A', d['value'], d['pipeline'].get('kernels_ms_avg'), d['checked_against_oracle']['result'])"
  done
done; done
