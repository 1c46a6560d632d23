#!/bin/bash
# och_build_voxels' host path under AddressSanitizer + UndefinedBehaviorSanitizer
# (CPU only): compiles csrc/och_builder.cpp's host code with both (the device code
# is compiled as usual and never runs here), links it and the normal build's other
# objects with tools/voxel_builder_host_check.c into one program, and runs that.
# Exit status: the program's; any sanitizer report is printed and fails the run.
# Usage: bash tools/voxel_builder_sanitize.sh [scratch_dir]
set -o pipefail
cd "$(dirname "$0")/.."
S=${1:-/tmp/och_voxel_sanitize}
mkdir -p "$S"
make -s -C octree_ray_tracing_amd/csrc || exit 1
H=/opt/rocm/bin/hipcc
C=octree_ray_tracing_amd/csrc
X="-Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined"
$H -std=c++17 -O1 -g -fPIC -ffp-contract=off -fno-fast-math -fno-omit-frame-pointer --offload-arch=gfx950 \
    -fno-gpu-flush-denormals-to-zero -munsafe-fp-atomics $X -c $C/och_builder.cpp -o "$S/och_builder.o" &&
/opt/rocm/lib/llvm/bin/clang -std=c11 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -Iinclude \
    -c tools/voxel_builder_host_check.c -o "$S/host_check.o" &&
$H --offload-arch=gfx950 $X -o "$S/voxel_builder_host_check" "$S/host_check.o" "$S/och_builder.o" \
    $(ls $C/build/*.o | grep -v '/och_builder\.o$') -pthread -ldl || exit 1
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
    timeout 600 "$S/voxel_builder_host_check" 2>&1 | tee "$S/host_check.log"
rc=$?
grep -hE "runtime error|ERROR: (Address|Leak)Sanitizer" "$S/host_check.log" && exit 1
exit $rc
