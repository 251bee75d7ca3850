#!/bin/bash
# A/B of the host-API split on one MI355X (profiles/api_refactor.md): bench.py of a built copy of the parent commit
# (PARENT, e.g. a `git archive` tree with its libmppgpu.so) and of this tree, alternately, N times each with the default
# arguments; the first pair also with --dump-outputs, whose tileNNN_*.npy files must be bit-identical.
# The default line has `value` (one-tile proposals/s) only; the batched rate and kernel_ms come with
#   BENCH_ARGS="--full --no-cpu-baseline --no-convergence --scene 0 --mosaic 0 --dataset-images 0"
# usage: bash profiles/tools/api_refactor_ab.sh PARENT [N] [OUT]     (from the repository root; every step under its own timeout)
set -o pipefail
PARENT=$(realpath "$1"); N=${2:-5}; OUT=$(realpath -m "${3:-bench_out/api_refactor}")
mkdir -p "$OUT/dump_parent" "$OUT/dump_new"
for i in $(seq 1 "$N"); do
  dump_p=""; dump_n=""
  if [ "$i" = 1 ]; then dump_p="--dump-outputs $OUT/dump_parent"; dump_n="--dump-outputs $OUT/dump_new"; fi
  ( cd "$PARENT" && timeout -k 10 400 python bench.py --gpus 1 --steps 5 --warmup 1 $BENCH_ARGS $dump_p > "$OUT/parent_$i.json" 2> "$OUT/parent_$i.err" ) || { echo "parent run $i failed"; exit 1; }
  timeout -k 10 400 python bench.py --gpus 1 --steps 5 --warmup 1 $BENCH_ARGS $dump_n > "$OUT/new_$i.json" 2> "$OUT/new_$i.err" || { echo "run $i of this tree failed"; exit 1; }
done
python - "$OUT" "$N" <<'PY'
import glob, hashlib, json, os, statistics, sys
out, n = sys.argv[1], int(sys.argv[2])
def sha(p): return hashlib.sha256(open(p, "rb").read()).hexdigest()
a = sorted(os.path.basename(p) for p in glob.glob(os.path.join(out, "dump_parent", "tile*_*.npy")))
b = sorted(os.path.basename(p) for p in glob.glob(os.path.join(out, "dump_new", "tile*_*.npy")))
same = bool(a) and a == b and all(sha(os.path.join(out, "dump_parent", f)) == sha(os.path.join(out, "dump_new", f)) for f in a)
print("outputs:", len(a), "files,", "bit-identical" if same else "MISMATCH")
def figures(tag):
    rows = []
    for i in range(1, n + 1):
        r = json.loads(open(os.path.join(out, f"{tag}_{i}.json")).read().strip().splitlines()[-1])
        rows.append((r["value"], (r.get("batched") or {}).get("proposals_per_s"), (r.get("roofline") or {}).get("kernel_ms")))
    return rows
P, Q = figures("parent"), figures("new")
ok = same
for k, name in enumerate(("one-tile proposals/s", "batched proposals/s", "kernel_ms")):
    p, q = [r[k] for r in P], [r[k] for r in Q]
    if None in p or None in q:
        print(f"{name}: not in the bench line (needs --full, see the header)")
        continue
    inside = min(p) <= statistics.median(q) <= max(p)
    ok &= inside
    print(f"{name}: parent {p} (min {min(p):.6g}, max {max(p):.6g}); this tree {q}, median {statistics.median(q):.6g}: "
          f"{'inside' if inside else 'OUTSIDE'} the parent's range")
sys.exit(0 if ok else 1)
PY
