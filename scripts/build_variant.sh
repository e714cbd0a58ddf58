#!/bin/bash
# A/B builds of the same ABI: scripts/build_variant.sh <name> "<-D flags>" [file=conv.hip] -> nerf_downstream_amd/variants/libmink_hip_<name>.so
# (select at run time with MINK_HIP_LIB=<path>; the other objects are the in-tree ones of the Makefile's SRCS, so run `make` in csrc first)
# The -D switches and the file each belongs to:
#   conv.hip       MINK_CSWZ, MINK_CLDA, MINK_CPF, MINK_CCIN, MINK_CPRIO   (compact_gemm_kernel)
#   conv_wgrad.hip MINK_WPIPE                                              (wgrad_kernel)
set -e
name=$1; flags=$2; file=${3:-conv.hip}
root=$(cd "$(dirname "$0")/.." && pwd)
csrc=$root/nerf_downstream_amd/csrc
out=$root/nerf_downstream_amd/variants
mkdir -p $out
obj=$out/${file%.hip}_$name.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -I$root/include -Wall -Wno-unused-function $flags -c $csrc/$file -o $obj
srcs=$(sed -n 's/^SRCS *:= *//p' $csrc/Makefile)
echo " $srcs " | grep -q " $file " || { echo "$file is not in the Makefile's SRCS" >&2; exit 1; }
others=$(for f in $srcs; do [ "$f" = "$file" ] || echo $csrc/${f%.hip}.o; done)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $out/libmink_hip_$name.so $obj $others
rm -f $obj
echo "built $out/libmink_hip_$name.so"
