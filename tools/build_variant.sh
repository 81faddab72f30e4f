#!/bin/bash
# Developer tool (build container): tools/build_variant.sh NAME "-DSEG_UNIT=2 ..." -> tools/ablate_build/libpngloss_hip_NAME.so
# (the product library with extra -D flags, built by the product's Makefile into an object directory of its own: EVERY source gets the flags, so that no two
#  files of the library disagree about a layout the flags change -- SegParams is read by pl_seg.hip and by every host file)
set -e
cd "$(dirname "$0")/.."
NAME=$1; DEFS=${2:-}
B=../../tools/ablate_build
make -C pngloss_amd/csrc -s -j"${JOBS:-8}" DEFS="$DEFS" OBJDIR=$B/obj_$NAME HIP_LIB=$B/libpngloss_hip_$NAME.so $B/libpngloss_hip_$NAME.so
echo built tools/ablate_build/libpngloss_hip_$NAME.so
