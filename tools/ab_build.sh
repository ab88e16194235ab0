#!/bin/bash
# Builds libdlrm_hip.so from a git revision's sources into DIR, for A/B timing against the working
# tree (DLRM_HIP_LIB=DIR/libdlrm_hip.so python tools/bench_update.py).  usage: tools/ab_build.sh REV DIR
# The revision's whole csrc and include are taken and built with its own Makefile, so the file list
# and the flags are the revision's.
set -e -o pipefail
REV=${1:?rev}; DIR=${2:?dir}
rm -rf "$DIR"; mkdir -p "$DIR/r"
DIR=$(cd "$DIR" && pwd)  # (relative to the caller's directory)
cd "$(git rev-parse --show-toplevel)"
git archive "$REV" -- dlrm.jl_amd/csrc include | tar -x -C "$DIR/r"
make -C "$DIR/r/dlrm.jl_amd/csrc" -j16 ../lib/libdlrm_hip.so
cp "$DIR/r/dlrm.jl_amd/lib/libdlrm_hip.so" "$DIR/libdlrm_hip.so"
rm -rf "$DIR/r"
