#!/bin/bash
# Developer tool: fast build of the two analytic-scene variants only (tally + history) into build/dev/<name>.so
# usage: tools/dev_build.sh name [extra hipcc flags]      (DEVV=2: the mesh variants instead)
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
flags=$(cd "$root" && python3 -c 'import __graft_entry__ as g; print(" ".join(g.HIPCC_FLAGS))') || exit 1   # build()'s own flags
mkdir -p "$root"/build/dev
cd "$root"/pvtrace_amd/csrc
hipcc $flags -DPVT_DEV_VARIANTS=${DEVV:-1} "$@" pvt_trace.hip -o "$root"/build/dev/$name.so
