#!/bin/bash
# Developer tool (GPU box): the bench's loop (median window + sustained) on several configs, one line each
# usage: tools/gpu_configs_quick.sh tag cfg...
OUT=${OUT:-out}; mkdir -p "$OUT"   # where the bench lines of this script go
tag=$1; shift
for c in "$@"; do
  python bench.py --full --config $c --repeats 4 --steps 10 --sustained-s 1.5 --total-photons 0 --no-cpu-baseline --extra-configs none --spinup-s 0.2 > "$OUT"/${tag}_$c.json 2>"$OUT"/${tag}_$c.err
  python - <<PY
import json
d = json.load(open("$OUT/${tag}_$c.json"))
print("$c", "median %.3e" % d["value"], "sustained %.3e" % d["sustained"]["value"], "kernel_ms %.3f" % d["roofline"]["kernel_ms_mean"], d["launch"])
PY
done
