#!/bin/bash
# Bitwise comparison only (no phase stamps): tools/obca_dump.py of every build, each compared with the first.
# Exit status 1 when a dump fails or any array of any build differs from the first build's.
# usage (GPU box): bash tools/ab_dump.sh OUTDIR NAME=SO [NAME=SO ...]   (SO "" = the in-tree library)
set -o pipefail
OUT=$1; shift
mkdir -p "$OUT"
first=""
rc=0
for spec in "$@"; do
  name=${spec%%=*}; so=${spec#*=}
  TTMPC_LIB=$so timeout -k 10 300 python -u tools/obca_dump.py "$OUT/$name.npz" 64 1000 > "$OUT/dump_$name.txt" 2>&1 || { echo "DUMP_FAILED $name"; tail -5 "$OUT/dump_$name.txt"; exit 1; }
  echo "done $name"
  if [ -z "$first" ]; then first=$name; continue; fi
  python tools/obca_dump.py --compare "$OUT/$first.npz" "$OUT/$name.npz" > "$OUT/compare_$name.txt" 2>&1 || rc=1
  tail -1 "$OUT/compare_$name.txt"
done
exit $rc
