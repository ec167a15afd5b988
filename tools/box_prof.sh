#!/bin/bash
# rocprofv3 kernel stats of the BoxScene kernels: tools/box_prof.sh <outdir>
out=$(realpath ${1:-gpurun_out/box_prof})
root=$(pwd)
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
for w in 1 8; do
  rocprofv3 --kernel-trace --stats --output-format csv -d $out/w${w} -- python3 $root/tools/band_proxy.py --world $w > $out/w${w}.log 2>&1
done
rocprofv3 --kernel-trace --stats --output-format csv -d $out/f32 -- python3 $root/tools/band_proxy.py --world 1 --f32 --frames 32 --steps 20 > $out/f32.log 2>&1
cd $out
for d in w* f32; do [ -d $d ] && { echo "== $d"; grep "^{" $d.log; cat $d/*/*_kernel_stats.csv | cut -d, -f1-4,6,7 | sed 's/void (anonymous namespace):://; s/(NtCameraFixed.*)"/"/' ; }; done
