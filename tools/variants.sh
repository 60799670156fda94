#!/bin/bash
# Build A/B variants of libretake_hip.so:  [RTK_SRC=dir] tools/variants.sh name "extra hipcc flags" [name2 "flags2" ...]
# A variant is a modified copy of csrc/ (RTK_SRC, default: the in-tree sources) and/or extra compiler flags; the sources
# themselves hold no build-time knobs.  The source list and the base flags are the Makefile's (csrc/Makefile).
# Output: video-retake_amd/retake/_lib/variants/libretake_hip_<name>.so   (select with RETAKE_HIP_LIB=...)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=${RTK_SRC:-$ROOT/video-retake_amd/csrc}
OUT=$ROOT/video-retake_amd/retake/_lib/variants
mkdir -p $OUT
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  tmp=$(mktemp -d)
  make -s -C "$SRC" -f "$ROOT/video-retake_amd/csrc/Makefile" -j4 BUILD=$tmp OUT=$OUT/libretake_hip_$name.so EXTRA="$flags"
  rm -rf $tmp
  echo built $name
done
