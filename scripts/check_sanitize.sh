#!/bin/bash
# The device-free index builders of the library under AddressSanitizer and UndefinedBehaviorSanitizer, on a machine WITHOUT a GPU:
#   scripts/check_sanitize.sh <leak_listing|grow_pattern|shrink_pattern|carry_map> [work dir]
#     leak_listing     the leak listing builder (tfqmrgpu_amd/csrc/tfq_leak_host.cpp)
#     grow_pattern     the grown pattern (tfq_leak_host.cpp: grow_pattern)
#     shrink_pattern   the listing of the drop cost and the shrunk pattern (tfq_leak_host.cpp: drop_listing, shrink_pattern)
#     carry_map        the block map of tfqmrgpuExt_carry (tfq_carry_host.cpp: carry_map_ok, carry_compose; tfq_leak_host.cpp grows the
#                      destination patterns)
# Plain C++: compiled with scripts/<name>_check.cpp into ONE stand-alone program and run on the patterns that
# scripts/leak_listing_inputs.py writes.  Host code only: never run this on a GPU machine or through Python.
set -eu
name=${1:?usage: check_sanitize.sh <leak_listing|grow_pattern|shrink_pattern|carry_map> [work dir]}
root=$(cd "$(dirname "$0")/.." && pwd)
csrc=$root/tfqmrgpu_amd/csrc
case $name in
    leak_listing|grow_pattern|shrink_pattern) srcs="$csrc/tfq_leak_host.cpp";;
    carry_map) srcs="$csrc/tfq_carry_host.cpp $csrc/tfq_leak_host.cpp";;
    *) echo "check_sanitize.sh: unknown check '$name'" >&2; exit 2;;
esac
work=${2:-$(mktemp -d)}
rocm=${ROCM:-/opt/rocm}
cxx=${CXX:-$rocm/llvm/bin/clang++}
[ -x "$cxx" ] || cxx=g++
mkdir -p "$work"
$cxx -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -D__HIP_PLATFORM_AMD__ -I"$rocm/include" \
    -I"$root/include" -I"$csrc" "$root/scripts/${name}_check.cpp" $srcs -o "$work/${name}_check"
files=$(python3 "$root/scripts/leak_listing_inputs.py" "$work/inputs")
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$work/${name}_check" $files
