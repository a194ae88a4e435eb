#!/bin/bash
# Round 4, last validation of the final build: the GPU suite, smoke(), the default bench line
R=${GRAFT_REPO_ROOT:-/root/repo}
mkdir -p $R/gpurun_out
cd $R
timeout -k 10 900 python3 -m pytest tests -x -q -m gpu > gpurun_out/r4_gputests_final.txt 2>&1; rc=$?
tail -4 gpurun_out/r4_gputests_final.txt
[ $rc = 0 ] || exit $rc
timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke()" > gpurun_out/r4_smoke.txt 2>&1 || { tail -5 gpurun_out/r4_smoke.txt; exit 1; }
tail -3 gpurun_out/r4_smoke.txt
timeout -k 10 600 python3 bench.py --full | python3 -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1])
r=d['roofline']
print('bench: value %.1f Gpoint/s ms_per_step %.3f frac %.3f frac_kernel %.3f traffic_over_algorithmic %s secondary %s cpu %s' % (d['value'], d['ms_per_step'], r['frac'], r['frac_kernel'], r['traffic_over_algorithmic'], d['secondary_fp64']['value'], d['cpu_baseline']['value']))" || exit 1
