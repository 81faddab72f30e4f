#!/bin/bash
# Developer tool (build container): tools/build_inflate_variant.sh NAME "-DPLI_LOOP=1 ..." -> tools/ablate_build/libpngloss_hip_NAME.so
# (the product library with extra -D flags meant for pl_inflate.hip: the same build as tools/build_variant.sh -- every source gets the flags, which only
#  pl_inflate.hip and the headers it includes look at)
exec "$(dirname "$0")/build_variant.sh" "$@"
