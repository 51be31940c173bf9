#!/bin/bash
# Device assembly of one translation unit, for checking that a host-side change left the kernels alone:
#   tools/device_asm.sh adt_wide.hip /tmp/wide.s      # at the parent commit and at the change, then cmp the two files
# The lines naming __hip_cuid_ (a random id per compilation) are dropped; everything else is reproducible.
set -o pipefail
[ $# -eq 2 ] || { echo "usage: $0 <file.hip> <out.s>" >&2; exit 2; }
out="$(realpath -m "$2")"
cd "$(dirname "$0")/../adt_amd/csrc" || exit 1
"${HIPCC:-/opt/rocm/bin/hipcc}" --offload-arch=gfx950 -O3 -std=c++17 -fPIC --offload-device-only -S "$1" -o - | grep -v __hip_cuid_ > "$out"
