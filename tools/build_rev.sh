#!/bin/bash
# Build the library of another git revision as an A/B variant (CPU side): csrc/, include/ and the Makefile of REV are
# materialised in a temporary directory and that revision's own `make` builds its own source list, with OUT redirected
# to car-trailer-mpc_amd/ttmpc/variants/libttmpc_NAME.so (TTMPC_LIB=... selects it in the tools).
# usage: bash tools/build_rev.sh REV NAME [extra hipcc flags]
set -eo pipefail
REV=$1; NAME=$2; shift 2
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
mkdir -p "$T/include" "$T/pkg/csrc"
git show "$REV:include/ttmpc.h" > "$T/include/ttmpc.h"
git show "$REV:car-trailer-mpc_amd/Makefile" > "$T/pkg/Makefile"
for f in $(git ls-tree --name-only "$REV" car-trailer-mpc_amd/csrc/); do git show "$REV:$f" > "$T/pkg/csrc/$(basename "$f")"; done
mkdir -p car-trailer-mpc_amd/ttmpc/variants
OUT="$PWD/car-trailer-mpc_amd/ttmpc/variants/libttmpc_$NAME.so"
# the extra flags ride on the compiler name: the revision's Makefile keeps its own FLAGS
make -C "$T/pkg" -j"${MAX_JOBS:-8}" HIPCC="${HIPCC:-/opt/rocm/bin/hipcc} $*" OUT="$OUT" "$OUT"
echo "built variants/libttmpc_$NAME.so from $REV"
