#!/bin/bash
# The block map of tfqmrgpuExt_carry (tfqmrgpu_amd/csrc/tfq_carry_host.cpp: carry_map_ok, carry_compose) under AddressSanitizer and
# UndefinedBehaviorSanitizer, on a machine WITHOUT a GPU:   scripts/carry_map_sanitize.sh [work dir]
# Plain C++: compiled with scripts/carry_map_check.cpp (and tfq_leak_host.cpp, which grows the destination patterns) into ONE stand-alone
# program and run on the patterns that scripts/leak_listing_inputs.py writes.  Host code only: never run this on a GPU machine or through Python.
set -eu
root=$(cd "$(dirname "$0")/.." && pwd)
work=${1:-$(mktemp -d)}
rocm=${ROCM:-/opt/rocm}
cxx=${CXX:-$rocm/llvm/bin/clang++}
[ -x "$cxx" ] || cxx=g++
mkdir -p "$work"
$cxx -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -D__HIP_PLATFORM_AMD__ -I"$rocm/include" \
    -I"$root/include" -I"$root/tfqmrgpu_amd/csrc" "$root/scripts/carry_map_check.cpp" "$root/tfqmrgpu_amd/csrc/tfq_carry_host.cpp" \
    "$root/tfqmrgpu_amd/csrc/tfq_leak_host.cpp" -o "$work/carry_map_check"
files=$(python3 "$root/scripts/leak_listing_inputs.py" "$work/inputs")
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$work/carry_map_check" $files
