#!/bin/bash
# Product build of a git revision (or the working tree with rev "WT") as
# spatial-intention-maps_amd/simaps/libsimaps_prod_<NAME>.so, for tools/ab_bench.sh: every unit of the
# revision's own csrc/Makefile, from an export of the revision.  The revision's source hash goes to
# libsimaps_prod_<NAME>.hash beside it (SIMAPS_AB_SOURCE_HASH: simaps._lib refuses a library built from
# other sources than the tree's unless it is told which to expect).
#   tools/prod_build.sh <rev|WT> <name> [stamp]      (stamp: the phase-stamp build, `make prof`)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
rev=$1; name=$2; kind=${3:-}
out="$ROOT/spatial-intention-maps_amd/simaps/libsimaps_prod_$name"
tmp=$(mktemp -d)
if [ "$rev" = WT ]; then
  mkdir -p "$tmp/spatial-intention-maps_amd"
  cp -r "$ROOT/include" "$tmp/include"
  cp -r "$ROOT/spatial-intention-maps_amd/csrc" "$tmp/spatial-intention-maps_amd/csrc"
  mkdir -p "$tmp/spatial-intention-maps_amd/simaps"
  cp "$ROOT/spatial-intention-maps_amd/simaps/_srchash.py" "$tmp/spatial-intention-maps_amd/simaps/"
else
  git -C "$ROOT" archive "$rev" include spatial-intention-maps_amd/csrc spatial-intention-maps_amd/simaps/_srchash.py | tar -x -C "$tmp"
fi
python3 "$tmp/spatial-intention-maps_amd/simaps/_srchash.py" > "$out.hash"
if [ "$kind" = stamp ]; then
  make -s -C "$tmp/spatial-intention-maps_amd/csrc" prof PROF="$out.so"
else
  make -s -C "$tmp/spatial-intention-maps_amd/csrc" OUT="$out.so"
fi
rm -rf "$tmp"
