#!/bin/bash
# SQ instruction counters of the BoxScene kernels: tools/box_pmc.sh <outdir> [band_proxy args]
out=$(realpath -m ${1:-gpurun_out/box_pmc})
shift
root=$(pwd)
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVES SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $out/pmc -- python3 $root/tools/band_proxy.py --steps 3 --warmup 1 "$@" > $out/pmc.log 2>&1
echo "== $@"
python3 $root/tools/pmc_sum.py $(ls $out/pmc/*/*counter_collection.csv | head -1) 4
