#!/bin/bash
# Builds the wave-timestamped library variant (-DDLRM_WTRACE) and runs tools/wave_trace.py with it.
#   usage: [DLRM_WT_D=16] [DLRM_WT_DIR=dir] [DLRM_WT_FLAGS="-DDLRM_FWD_WIN=8"] [DLRM_WT_BUILD=0|1|only]
#          tools/wave_trace.sh [modes of wave_trace.py: ops step metric]
# DLRM_WT_DIR (default /tmp/dlrm_wt) holds the library; DLRM_WT_BUILD=only builds and stops (on a
# build host), =0 runs a library built before.
set -e
D=dlrm.jl_amd/csrc
O=${DLRM_WT_DIR:-/tmp/dlrm_wt}
if [ "${DLRM_WT_BUILD:-1}" != 0 ]; then
  SRCS=$(sed -n 's/^SRCS := //p' $D/Makefile)
  mkdir -p "$O"
  for f in $SRCS; do
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=fast -DDLRM_WTRACE $DLRM_WT_FLAGS -x hip -c $D/$f -o "$O/$f.o" &
  done
  wait
  /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o "$O/libdlrm_hip.so" "$O"/*.o \
    -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
  [ "${DLRM_WT_BUILD:-1}" = only ] && exit 0
fi
DLRM_HIP_LIB="$O/libdlrm_hip.so" python3 tools/wave_trace.py "$@"
