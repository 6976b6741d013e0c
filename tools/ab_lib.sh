#!/bin/bash
# A/B two builds of the library on ONE box (box-to-box spread is ~1.5 ms per step): tools/probes/bin/lib_prev.so vs the in-tree one.
# usage (on the GPU box): bash tools/ab_lib.sh [bench args]
#   ROUNDS=3             pairs to run (default 2)
#   AB_CMD="python tools/epilogue_bench.py"   run this instead of bench.py under each library; its output is printed, prefixed
#   DUMP_DIR=dir         bench.py only: --dump-outputs into dir/<which>_<round>/, and `cmp` of each pair's latents.npy
set -e
cd "$(dirname "$0")/.."
cp instantir_amd/libinstantir_hip.so /tmp/lib_new.so
trap 'cp /tmp/lib_new.so instantir_amd/libinstantir_hip.so' EXIT
for round in $(seq 1 ${ROUNDS:-2}); do
  for which in prev new; do
    if [ $which = prev ]; then cp tools/probes/bin/lib_prev.so instantir_amd/libinstantir_hip.so; else cp /tmp/lib_new.so instantir_amd/libinstantir_hip.so; fi
    if [ -n "$AB_CMD" ]; then
      timeout -k 10 ${AB_TIMEOUT:-300} $AB_CMD 2>/dev/null | sed "s/^/$which $round | /"
      [ ${PIPESTATUS[0]} -eq 0 ] || { echo "$which $round: the command failed"; exit 1; }
    else
      dump=()
      if [ -n "$DUMP_DIR" ]; then dump=(--dump-outputs "$DUMP_DIR/${which}_$round"); fi
      timeout -k 10 ${AB_TIMEOUT:-300} python bench.py --no-cpu-baseline --no-vae --steps 20 "${dump[@]}" "$@" 2>/dev/null | tail -1 > /tmp/ab.json
      [ ${PIPESTATUS[0]} -eq 0 ] || { echo "$which $round: bench.py failed"; exit 1; }
      python -c "import json; d=json.load(open('/tmp/ab.json')); print('$which', d['ms_per_step'], d['value'], "")"
    fi
  done
  if [ -z "$AB_CMD" ] && [ -n "$DUMP_DIR" ]; then
    if cmp -s "$DUMP_DIR/prev_$round/latents.npy" "$DUMP_DIR/new_$round/latents.npy"; then echo "pair $round: dumped outputs byte-identical"; else echo "pair $round: dumped outputs DIFFER"; fi
  fi
done
