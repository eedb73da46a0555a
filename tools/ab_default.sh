#!/bin/bash
# dev: the full invocation twice on a fresh box: headline, value_unchanged with its two readings (right behind the
# headline leg / at the end of the run), host figures, wall time of the whole command.  OUT=<dir> bash tools/ab_default.sh
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:?set OUT to the directory for the lines and the full records}
mkdir -p "$OUT"
for r in 1 2; do
  t0=$(date +%s.%N)
  CODA_BENCH_FULL="$OUT/bench_full.json" python bench.py --full 2>/dev/null > "$OUT/ab_default_line$r.json"
  t1=$(date +%s.%N)
  python - "$r" "$t0" "$t1" "$OUT" <<'PY'
import json, sys, os
r, t0, t1, out = sys.argv[1], float(sys.argv[2]), float(sys.argv[3]), sys.argv[4]
line = os.path.join(out, f"ab_default_line{r}.json")
d = json.loads(open(line).read().strip().splitlines()[-1])
full = None
f = os.path.join(out, "bench_full.json")
if os.path.exists(f):
    full = json.loads(open(f).read().strip().splitlines()[-1])
print(f"run {r}: {t1 - t0:.1f} s wall; value", d["value"], "ms", d["ms_per_step"], "value_unchanged", d.get("value_unchanged"),
      "readings", (full or {}).get("value_unchanged_caller", {}).get("readings"), "host", d["host"], "line bytes",
      os.path.getsize(line))
PY
done
