#!/bin/bash
# rocprofv3 profile set of the bench at its default size (dev tool, runs on an MI355X):
#   tools/profile_round.sh <tag> [<out>]   -> <out>/<tag>_{conc,ser,fetch,write,mfma}/<host>/<pid>_*.csv  (<out> default: profile_runs/)
# then on the CPU side:  python tools/prof_digest.py <tag> <out>/<tag>_conc <out>/<tag>_ser <out>/<tag>_fetch \
#                                                    <out>/<tag>_write <out>/<tag>_mfma
# The two kernel-trace passes run bench.py --full (their step counts include the roofline's instrumented steps); the PMC passes
# are plain runs of 1 warm-up + 1 timed step.
# PMC counters are collected in their own passes, with --kernel-trace only (MI355X_MICROARCH.md: FETCH_SIZE and WRITE_SIZE do not
# fit one pass; gpurun refuses --pmc together with the system traces).
set -e
T=${1:-r02}
R=$(cd "$(dirname "$0")/.." && pwd)
O=${2:-$R/profile_runs}
mkdir -p "$O"
O=$(cd "$O" && pwd)  # the passes run from /tmp
cd /tmp
export TMPDIR=/tmp
rm -rf $O/${T}_conc $O/${T}_ser $O/${T}_fetch $O/${T}_write $O/${T}_mfma  # one <pid>_*.csv set per directory
rocprofv3 --kernel-trace --stats --output-format csv -d $O/${T}_conc -- python3 $R/bench.py --full --no-cpu-baseline --no-live-traffic --no-secondary > $O/${T}_conc.json 2> $O/${T}_conc.log
rocprofv3 --kernel-trace --stats --output-format csv -d $O/${T}_ser -- python3 $R/bench.py --full --no-cpu-baseline --no-secondary --serialize-streams > $O/${T}_ser.json 2> $O/${T}_ser.log
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/${T}_fetch -- python3 $R/bench.py --no-cpu-baseline --no-roofline --steps 1 --warmup 1 > /dev/null 2> $O/${T}_fetch.log
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/${T}_write -- python3 $R/bench.py --no-cpu-baseline --no-roofline --steps 1 --warmup 1 > /dev/null 2> $O/${T}_write.log
rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/${T}_mfma -- python3 $R/bench.py --no-cpu-baseline --no-roofline --serialize-streams --steps 1 --warmup 1 > /dev/null 2> $O/${T}_mfma.log
echo "profiles done: $T"
