#!/bin/bash
# Timing experiments on k_cfconv_fused (the filter-MLP CFConv: what runs when the polynomials are refused or off): phases of the
# kernel taken out one by one.  Builds the diagnostic variant of edge.hip, the only one that reads AGDIFF_ABLATE from the
# environment (tools/build_variant.sh edge.hip ablate -DAG_CONV_ABLATE), and runs bench.py on it through AGDIFF_LIB
# (with --radius-poly off, to reach the kernel).   bash tools/ablate_conv.sh
root=$(cd "$(dirname "$0")/.." && pwd)
bash "$root/tools/build_variant.sh" edge.hip ablate -DAG_CONV_ABLATE || exit 1
export AGDIFF_LIB=$root/_ab/lib_ablate.so
for a in 0 1 2 4 8 16 31 30 29; do AGDIFF_ABLATE=$a python bench.py --workload drugs --radius-poly off --steps 20 --warmup 5 --no-cpu-baseline --no-extra --no-traj 2>/dev/null | python -c "
import json,sys; d=json.loads(sys.stdin.read()); print('ablate',$a,'conv_ms',round(d['roofline']['avg_launch_ms'],4))"; done
