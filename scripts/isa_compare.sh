#!/bin/bash
# Are the kernels that exist in another checkout (the parent commit) unchanged in this tree?
#   scripts/isa_compare.sh <other checkout> [work dir]
# Compiles every .hip file of the OTHER tree's tfqmrgpu_amd/csrc, there and here, to device-only gfx950 assembly with the
# Makefile's flags and compares the two line by line, leaving out the `__hip_cuid_<hash>` symbol (a hash per compilation).
# A file that differs as a whole is compared function by function (scripts/isa_compare_kernels.py): new kernels beside unchanged ones pass.
# Needs hipcc only, no GPU.  Exit status 1 if a kernel of the other tree differs or is missing here.
set -u
OTHER=${1:?usage: isa_compare.sh <other checkout> [work dir]}
HERE=$(cd "$(dirname "$0")/.." && pwd)
WORK=${2:-$(mktemp -d)}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -mllvm -amdgpu-mfma-vgpr-form=1 --cuda-device-only -S"
mkdir -p "$WORK/other" "$WORK/this"
for src in "$OTHER"/tfqmrgpu_amd/csrc/*.hip; do
    f=$(basename "$src" .hip)
    echo "$HIPCC $FLAGS -I$OTHER/include -I$OTHER/tfqmrgpu_amd/csrc $src -o $WORK/other/$f.s"
    echo "$HIPCC $FLAGS -I$HERE/include -I$HERE/tfqmrgpu_amd/csrc $HERE/tfqmrgpu_amd/csrc/$f.hip -o $WORK/this/$f.s"
done | xargs -P "${JOBS:-8}" -I{} bash -c "{} 2>/dev/null"
rc=0; total=0
for a in "$WORK"/other/*.s; do
    f=$(basename "$a"); b="$WORK/this/$f"
    [ -f "$b" ] || { echo "$f: missing in this tree"; rc=1; continue; }
    n=$(diff <(grep -v '__hip_cuid_' "$a") <(grep -v '__hip_cuid_' "$b") | wc -l)
    k=$(grep -c '\.amdhsa_kernel ' "$a"); total=$((total + k))
    if [ "$n" -eq 0 ]; then echo "$f: identical ($k kernels)"
    # the file as a whole differs: kernels may have been ADDED to it -- then every function of the other tree must still be unchanged
    elif python3 "$HERE/scripts/isa_compare_kernels.py" "$a" "$b"; then echo "$f: every kernel of the other tree identical ($k kernels), new kernels beside them"
    else echo "$f: $n differing lines ($k kernels)"; rc=1; fi
done
echo "kernels compared: $total"
exit $rc
