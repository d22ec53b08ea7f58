#!/bin/bash
# Build A/B variants of the library: tools/build_variants.sh name "-DFLAG ..." [name flags]...
# Every source is recompiled with the flags added to the Makefile's own: the Makefile runs on a copy of csrc/ (under
# build/variants/<name>/), so the source list and the link line are always the library's.  ARCH is passed through.
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
arch=${ARCH:-gfx950}
base=$(sed -n 's/^CXXFLAGS := //p' "$root/reactranker_amd/csrc/Makefile" | sed "s/\$(ARCH)/$arch/")
while [ $# -gt 0 ]; do
  name=$1; flags=$2; shift 2
  v="$root/build/variants"
  d="$v/$name/reactranker_amd/csrc"
  rm -rf "$v/$name" && mkdir -p "$d" "$v/$name/include"
  cp "$root"/reactranker_amd/csrc/*.hip "$root"/reactranker_amd/csrc/*.h "$root"/reactranker_amd/csrc/*.cpp "$root/reactranker_amd/csrc/Makefile" "$d/"
  cp "$root"/include/*.h "$v/$name/include/"
  make -C "$d" -j4 ARCH="$arch" CXXFLAGS="$base $flags" > "$v/$name.log" 2>&1 || { tail -20 "$v/$name.log"; exit 1; }
  cp "$d/libreactranker_hip.so" "$v/lib_$name.so"
  rm -rf "$v/$name"
  echo "built $name"
done
