#!/bin/bash
# Per-layer outputs of the VideoMAE classifier: the encode measurements of DESIGN.md "Per-layer outputs", one GPU, one session.
#   tools/introspect_encode_ab.sh <built checkout of the parent commit> [output directory, default profiles]
# Writes <out>/introspect_encode.jsonl - every JSON line tools/bench_encode.py printed, with a "run" field naming the run put in
# front by this script - and <out>/introspect_kernel_counts.txt: launch count and name of every kernel of a flags-off encode of
# 2 clips (rocprofv3 --kernel-trace --stats, a run of its own) for the parent and for this tree, and whether they are identical.
# Runs alternate between the two trees; each has its own time limit and the script stops at the first one that fails.
set -u
PARENT=${1:?path of a built checkout of the parent commit}
HERE=$(cd "$(dirname "$0")/.." && pwd)
OUTDIR=$(mkdir -p "${2:-$HERE/profiles}" && cd "${2:-$HERE/profiles}" && pwd)
OUT=$OUTDIR/introspect_encode.jsonl
TMP=$(mktemp -d)
: > "$OUT"
step() {   # step <directory> <run name> <command...>
  local dir=$1 tag=$2; shift 2
  echo "=== [$tag] $*" >&2
  ( cd "$dir" && timeout -k 10 200 "$@" ) > "$TMP/last" || { echo "=== [$tag] failed: stopping" >&2; exit 1; }
  grep '^{' "$TMP/last" | sed "s/^{/{\"run\": \"$tag\", /" | tee -a "$OUT"
}
B="python tools/bench_encode.py --steps 30 --warmup 5"
step "$HERE" "this probs"         $B --arch base --batch 2,8 --probs
step "$HERE" "this flags-off 1"   $B --arch base --batch 2,8
step "$HERE" "this attentions"    $B --arch base --batch 2,8 --attentions
step "$HERE" "this hidden-states" $B --arch base --batch 2,8 --hidden-states
for round in 1 2; do
  for b in 2 8; do step "$PARENT" "parent flags-off $round" $B --batch $b; done
  step "$HERE" "this flags-off $((round + 1))" $B --arch base --batch 2,8
done
for which in parent this; do
  dir=$HERE; [ $which = parent ] && dir=$PARENT
  ( cd "$dir" && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$TMP/$which" -o t --output-format csv -- \
      python tools/bench_encode.py --batch 2 --steps 2 --warmup 1 ) > "$TMP/$which.log" 2>&1 || { tail -n 5 "$TMP/$which.log" >&2; exit 1; }
  python -c "
import csv, sys
for r in sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: r['Name']):
    print(r['Calls'], r['Name'])" "$(find "$TMP/$which" -name '*kernel_stats.csv' | head -1)" > "$TMP/$which.counts"
done
{
  if diff -q "$TMP/parent.counts" "$TMP/this.counts" > /dev/null; then
    echo "# flags-off encode, 2 clips, 1 warm-up + 2 timed calls: parent and this tree launch the same kernels the same number of times"
  else
    echo "# flags-off encode, 2 clips: kernel names or launch counts DIFFER between the parent and this tree"
    echo "# --- parent"; cat "$TMP/parent.counts"; echo "# --- this tree"
  fi
  cat "$TMP/this.counts"
} > "$OUTDIR/introspect_kernel_counts.txt"
head -n 1 "$OUTDIR/introspect_kernel_counts.txt"
