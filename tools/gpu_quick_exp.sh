#!/bin/bash
# like gpu_quick.sh, for the experiment library (an experiment build of the library named libpngloss_hip_exp.so): usage bash tools/gpu_quick_exp.sh <tag>
export PNGLOSS_HIP_LIBNAME=libpngloss_hip_exp.so
exec bash $(dirname $0)/gpu_quick.sh "$@"
