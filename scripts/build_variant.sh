#!/bin/bash
# A/B builds of the library: scripts/build_variant.sh <name> [extra hipcc flags...] -> scripts/bin/libtfQMRgpu_<name>.so
# (the multiply's translation units -- tfq_spmm*.hip -- are compiled with the extra flags, all other objects are taken from the regular build -- from its
#  lab objects when -DTFQ_LAB is among the flags; TFQMRGPU_LIB=<path> makes the Python binding load a variant;
#  SPMM_SRC=<file> compiles ONE source file with the whole multiply in place of all of them, e.g. an earlier revision from `git show`)
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
csrc=$root/tfqmrgpu_amd/csrc
# the source lists are the Makefile's: tfq_spmm*.hip is the multiply, everything else is linked from the regular (or lab) objects
srcs=""; others=""
for f in $(make -s -C $csrc print-HIPSRC print-CXXSRC); do
    case $f in tfq_spmm*.hip) srcs="$srcs $csrc/$f";; *) others="$others ${f%.*}";; esac
done
[ -n "$SPMM_SRC" ] && srcs=$SPMM_SRC
# timing-only variants (-DTFQ_PROBE=..., -DTFQ_LAB_CLOCK, -DTFQ_LAB_STAMPS, -DTFQ_B8_DEPTH=...) exist only in the lab copy of the multiply, one monolithic
# source (r04: the product sources carry none of them)
case " $* " in *TFQ_PROBE*|*TFQ_LAB_CLOCK*|*TFQ_LAB_STAMPS*|*TFQ_B8_DEPTH*) srcs=${SPMM_SRC:-$root/scripts/lab/tfq_spmm_probes.hip};; esac
# a variant with -DTFQ_LAB is linked against the LAB objects of the other files: one definition of tfq::lab_switch per library
objdir=$root/tfqmrgpu_amd/lib/obj
case " $* " in *"-DTFQ_LAB "*|*"-DTFQ_LAB") objdir=$root/tfqmrgpu_amd/lib/obj/lab;; esac
vdir=$root/scripts/bin/obj_$name
mkdir -p $vdir
make -s -C $csrc >/dev/null
pids=""
for src in $srcs; do
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -I$root/include -I$csrc -Wall -Wno-unused-function --offload-arch=gfx950 \
       -mllvm -amdgpu-mfma-vgpr-form=1 "$@" -x hip -c $src -o $vdir/$(basename $src .hip).o &
    pids="$pids $!"
done
for p in $pids; do wait $p; done
objs=""
for o in $others; do objs="$objs $objdir/$o.o"; done
objs="$objs $root/tfqmrgpu_amd/lib/obj/tfq_fortran.o"
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o $root/scripts/bin/libtfQMRgpu_$name.so $vdir/*.o $objs -Wl,-soname,libtfQMRgpu.so.1 -ldl
rm -rf $vdir
echo built scripts/bin/libtfQMRgpu_$name.so
