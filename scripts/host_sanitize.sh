#!/bin/bash
# Host memory of the library's device-free paths under AddressSanitizer and UndefinedBehaviorSanitizer, on a machine WITHOUT a GPU:
#   scripts/host_sanitize.sh [work dir]
# Compiles the host sources of the library (the C-ABI, the plan, the solver's and the preconditioner's host side) with
# -fsanitize=address,undefined, takes the kernel families from the regular build (make -C tfqmrgpu_amd/csrc first), links them with
# tests/c_caller/host_walk.c into ONE stand-alone program and runs it.  Host code only: never run this on a GPU machine or through Python.
set -eu
root=$(cd "$(dirname "$0")/.." && pwd)
csrc=$root/tfqmrgpu_amd/csrc
work=${1:-$(mktemp -d)}
hipcc=${HIPCC:-/opt/rocm/bin/hipcc}
san="-fsanitize=address,undefined -g"
inc="-std=c++17 -fPIC -I$root/include -I$csrc -Wall -Wno-unused-function"
mkdir -p "$work"
objs=""
for f in $(make -s -C "$csrc" print-HIPSRC print-CXXSRC); do
    case $f in
        tfq_api.hip) $hipcc -O1 $inc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -g -c "$csrc/$f" -o "$work/${f%.*}.o"; objs="$objs $work/${f%.*}.o";;
        *.cpp)       $hipcc -O1 $inc -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include $san -c "$csrc/$f" -o "$work/${f%.*}.o"; objs="$objs $work/${f%.*}.o";;
        *)           objs="$objs $root/tfqmrgpu_amd/lib/obj/${f%.*}.o";;     # kernels and their launchers: the regular objects
    esac
done
clang=$(dirname "$($hipcc --version | sed -n 's/^InstalledDir: //p')")/bin/clang
[ -x "$clang" ] || clang=/opt/rocm/llvm/bin/clang
$clang -O1 $san -I"$root/include" -c "$root/tests/c_caller/host_walk.c" -o "$work/host_walk.o"
$hipcc --offload-arch=gfx950 $san -o "$work/host_walk" "$work/host_walk.o" $objs "$root/tfqmrgpu_amd/lib/obj/tfq_fortran.o" -ldl
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$work/host_walk"
