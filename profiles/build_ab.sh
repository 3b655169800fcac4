#!/bin/bash
# Builds a named variant of the library for an A/B run without touching libmi3pt.so:  _ab/lib<NAME>.so from the working tree's
# sources with extra compiler flags, through csrc/Makefile (its source list and flags are the only ones).
# usage: bash profiles/build_ab.sh NAME [-DPT_X_...=... ...]     (then profiles/ab_quick.py)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
mkdir -p $ROOT/_ab
# -B: always rebuilt, as make does not see that the flags changed
make -B -C $ROOT/webgpu-pathtracer_amd/csrc OUT=$ROOT/_ab/lib$NAME.so EXTRA="$*" && echo "built _ab/lib$NAME.so ($*)"
