#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over csrc/pt_host_reproject.cpp (mi3pt_host_view_frame), beside tests/tools/sanitize_cpu.sh
# for the other host files: a stand-alone program with its own main (sanitize_view_frame.cpp), no Python, nothing preloaded.
#   usage: bash tests/tools/sanitize_view_frame.sh        (seconds; prints one "ok" line)
set -eu
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
W=$(mktemp -d /tmp/mi3pt_san.XXXXXX)
trap 'rm -rf "$W"' EXIT
g++ -O1 -g -std=c++17 -w -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I"$ROOT/include" -I/opt/rocm/include \
    -D__HIP_PLATFORM_AMD__ "$ROOT/webgpu-pathtracer_amd/csrc/pt_host_reproject.cpp" "$ROOT/tests/tools/sanitize_view_frame.cpp" -o "$W/view_frame"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1 "$W/view_frame" 2>"$W/err.txt" || { cat "$W/err.txt"; exit 1; }
