#!/bin/bash
# Build a variant of the library into tools/ab/lib<name>.so with extra compiler flags (diagnostic / A-B builds only):
#   tools/ab/build_variant.sh stamps -DLOCO_GEMM_STAMPS
set -e
name=$1; shift
here=$(cd "$(dirname "$0")" && pwd)
src=$here/../../loco-asr_amd/csrc
out=$here/_build_$name
mkdir -p $out
flags="$(sed -n 's/^CXXFLAGS ?= //p' $src/Makefile | sed 's/$(ARCH)/gfx950/') $(sed -n 's/^override CXXFLAGS += //p' $src/Makefile)"
for f in $(sed -n 's/^SRCS := //p' $src/Makefile); do  # the Makefile's own list: every translation unit of the library
  hipcc $flags "$@" -c $src/$f -o $out/${f%.hip}.o &
done
wait
hipcc --offload-arch=gfx950 -shared -fPIC -o $here/lib$name.so $out/*.o
echo built $here/lib$name.so
