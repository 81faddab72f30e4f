#!/bin/bash
# Developer tool (build container): the product library with pl_lead_asm.h regenerated under other generator settings and/or extra defines for pl_engine.hip and its parts (pl_wg_*.h):
#   tools/build_wg_variant.sh NAME "PL_LEAD_BURST=2 ..." "-DPL_LEAD_BURST0_CLEAN=2 ..."   -> tools/ablate_build/libpngloss_hip_NAME.so
# (a copy of the sources with the regenerated header, built by the product's Makefile there; the copy lies two directories below one that holds include/,
#  like the sources themselves)
set -e
cd "$(dirname "$0")/.."
NAME=$1; GENENV=${2:-}; DEFS=${3:-}
T=tools/ablate_build/src_$NAME/csrc
rm -rf tools/ablate_build/src_$NAME; mkdir -p $T tools/ablate_build/include
cp pngloss_amd/csrc/*.hip pngloss_amd/csrc/*.h pngloss_amd/csrc/*.c pngloss_amd/csrc/Makefile $T/
cp include/*.h tools/ablate_build/include/
env $GENENV python tools/gen_lead_asm.py > $T/pl_lead_asm.h
make -C $T -s -j"${JOBS:-8}" DEFS="$DEFS" HIP_LIB=../../libpngloss_hip_$NAME.so ../../libpngloss_hip_$NAME.so
echo built tools/ablate_build/libpngloss_hip_$NAME.so
