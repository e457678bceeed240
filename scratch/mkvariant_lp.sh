#!/bin/bash
# A measurement variant that differs from the tree's build only in the -D switches of the register-resident matrix-core kernels
# (aidax_mfmalp.hip, aidax_tick.hip, aidax_mfmals.hip, aidax_mfmals2.hip): the other objects are copied from build/obj_hooks, these four recompiled.   scratch/mkvariant_lp.sh NAME "-DFOO=1 -DBAR"  ->  scratch/prev_lib/libaidax_NAME.so
set -e
name=$1; shift
make -s -j8 all > /dev/null
rm -rf build/obj_$name; cp -a build/obj_hooks build/obj_$name
for k in aidax_mfmalp aidax_tick aidax_mfmals aidax_mfmals2; do rm -f build/obj_$name/$k.o build/obj_$name/$k.remarks; done
rm -f build/obj_$name/scratch.ok
make -j8 OBJDIR=build/obj_$name LIBDIR=build/lib_$name EXTRA="-DAIDAX_TEST_HOOKS $*" build/lib_$name/libaidax_hip.so 2>&1 | grep -E "error|warning: v|spill|scratch" || true
mkdir -p scratch/prev_lib
cp build/lib_$name/libaidax_hip.so scratch/prev_lib/libaidax_$name.so
ls -la scratch/prev_lib/libaidax_$name.so
