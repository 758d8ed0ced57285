#!/bin/bash
# the -m gpu suite + the full bench line (the headline and every leg beside it): bash tools/gpu_tests.sh <tag>
tag=${1:-tests}
export TMPDIR=/tmp; cd "$(dirname "$0")/.."
out=gpurun_out/$tag; rm -rf $out; mkdir -p $out
timeout 2400 python -m pytest tests -m gpu -x -q > $out/pytest_gpu.log 2>&1; echo "pytest rc $?" >> $out/pytest_gpu.log
timeout 900 python bench.py --full > $out/bench.json 2> $out/bench.err
tail -3 $out/pytest_gpu.log
