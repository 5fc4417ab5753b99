#!/bin/bash
# compile ONE kernel source for gfx950 with the build's flags and print the compiler's per-kernel resource usage (registers, scratch, spills)
#   tools/cc1.sh mlp_fused.hip [-S]     (-S: also write /tmp/<name>.s)
root=$(cd "$(dirname "$0")/.." && pwd)
src=$root/motionbert_amd/csrc/$1
name=$(basename "$1" .hip)
FLAGS=$(python3 -c "import runpy, sys; print(' '.join(runpy.run_path(sys.argv[1])['FLAGS']))" "$root/motionbert_amd/build.py") || exit 1
/opt/rocm/bin/hipcc $FLAGS -Rpass-analysis=kernel-resource-usage -c "$src" -o /tmp/$name.o 2>&1 | grep -v "^$" | grep -E "error|warning: |Function Name|VGPRs|AGPRs|Scratch|Spill|Occupancy" | sed -e 's/\[-Rpass-analysis=kernel-resource-usage\]//' -e 's/^.*remark: //'
if [ "$2" = "-S" ]; then /opt/rocm/bin/hipcc $FLAGS -S --cuda-device-only "$src" -o /tmp/$name.s 2>/dev/null; fi
