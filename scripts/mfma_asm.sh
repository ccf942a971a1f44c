#!/bin/bash
# Compile a matrix-core Kalman kernel file (default kf_scan_mfma.hip; or kf_scan_bf32.hip, mfma_multi.hip) to assembly and
# print register / spill usage and the loop instruction mix.  Further arguments go to hipcc.
here="$(cd "$(dirname "$0")" && pwd)"
src="${1:-kf_scan_mfma.hip}"
[ $# -gt 0 ] && shift
cd "$here/../bayesianfiltering_amd/csrc"
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -I. -I../../include -S --cuda-device-only "$src" -o /tmp/m.s -Rpass-analysis=kernel-resource-usage "$@" 2>&1 | grep -E "error|VGPRs|Scratch|Spill"
python3 "$here/asm_loops.py" /tmp/m.s | head -1
