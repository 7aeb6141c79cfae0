#!/bin/bash
# Register / scratch / occupancy of every kernel of the device layer: the units of the Makefile's
# DEV_SRC, one after the other (runs anywhere hipcc does).
# SRC=turtle_amd/csrc/rays.hip: that unit alone; SRC=tests/c/device_loops.hip or
# SRC=examples/own_kernel.hip: the kernels written on the device API (include/turtle_amd_device.h),
# e.g.  SRC=tests/c/device_loops.hip scripts/kernel_resources.sh traverse_trip
cd "$(dirname "$0")/.."
SRC=${SRC:-$(sed -n 's/^DEV_SRC *:= *//p' turtle_amd/csrc/Makefile | tr ' ' '\n' | sed 's|^|turtle_amd/csrc/|')}
for src in $SRC; do
hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fPIC -std=c++17 -Iinclude -Iturtle_amd/csrc \
  -c "$src" -o /tmp/device_res.o -Rpass-analysis=kernel-resource-usage 2>&1
done | python3 -c "
import re, sys
name = None; row = {}
for line in sys.stdin:
    m = re.search(r'remark: (.*?)\s*\[-Rpass', line)
    if not m: continue
    t = m.group(1).strip()
    if t.startswith('Function Name:'):
        if name: print(name[:70].ljust(70), row)
        name = t.split(':', 1)[1].strip(); row = {}
    else:
        k, _, val = t.partition(':')
        if k.strip() in ('VGPRs', 'AGPRs', 'SGPRs', 'ScratchSize [bytes/lane]', 'Occupancy [waves/SIMD]', 'LDS Size [bytes/block]'):
            row[k.strip().split(' ')[0]] = val.strip()
if name: print(name[:70].ljust(70), row)
" | grep ${1:-k_}
