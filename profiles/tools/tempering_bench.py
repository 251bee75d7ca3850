#!/usr/bin/env python3
"""What parallel tempering costs and finds (profiles/tempering.md): the scene of profiles/restarts.md -- 1024 x 1024, 16 tiles
of 256 px -- through ``MPPModel.infer_image`` with ``inference.restarts`` = R in {2, 4, 8} and ``inference.tempering`` over
ratio in {1.25, 1.5, 2, 3} x every in {1024, 4096, 8192}, next to ``restarts`` = R without tempering on a built copy of the
parent commit; and ``restarts`` = R without the key, this tree against the parent, the two alternating in one call.

    python profiles/tools/tempering_bench.py OUT.json [--parent DIR] [--reps N] [--md OUT.md]

Profiler off.  Every setting is warmed up before it is timed.  Wall times are a host clock around ``infer_image``, which ends
in the copy of the merged detections to the host; ``kernel_ms`` is the chain kernels' device time, ``tempering_ms`` that of
the energy and exchange launches.  ``--parent DIR``: a ``git archive`` copy of the parent commit with ``libmppgpu.so`` built
in it.  The A/B runs one worker process per tree and R (``--worker``), each warmed up, and asks them for one repetition in
turn."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SEED = 5
RS, RATIOS, EVERYS = (2, 4, 8), (1.25, 1.5, 2.0, 3.0), (1024, 4096, 8192)


def scene_and_model(root, restarts):
    sys.path.insert(0, root)
    from mpp_cnn_rs_object_detection_amd import mappings, synth
    from mpp_cnn_rs_object_detection_amd.custom_types import ImageWMaps
    from mpp_cnn_rs_object_detection_amd.mpp_model import MPPModel
    from mpp_cnn_rs_object_detection_amd.shapes import Rectangle
    det, marks, gt_xy, _ = synth.make_mosaic(n_side=4, tile=256, n_objects=50, first_tile_id=300, noise=0.2)
    data = ImageWMaps(name="0000", shape=det.shape, image=None, detection_map=det, param_dist_maps=marks,
                      mappings=mappings.default_mappings(), param_names=Rectangle.PARAMETERS, gt_config=[])
    with open(os.path.join(root, "model_configs", "mpp", "config_mpp_log.json")) as f:
        cfg = json.load(f)
    cfg["inference"]["restarts"] = restarts
    cwd = os.getcwd()
    os.chdir(root)                           # (paths_config.json and the stored model are resolved from here)
    try:
        model = MPPModel(cfg, phase="val", load=True)
    finally:
        os.chdir(cwd)
    return data, model


def digest(detections, scores):
    import numpy as np
    h = hashlib.sha256()
    h.update(np.asarray([(p.x, p.y, p.size, p.ratio, p.angle) for p in detections], dtype=np.float64).tobytes())
    h.update(np.asarray(scores, dtype=np.float64).tobytes())
    return h.hexdigest()[:16]


def one_run(data, model):
    import numpy as np
    t0 = time.perf_counter()
    det, scores = model.infer_image(data, seed=SEED)
    wall = (time.perf_counter() - t0) * 1e3
    run = model.last_run
    e, w = run["replica_energy"], run["replica_winner"]
    return {"wall_ms": wall, "kernel_ms": float(run["kernel_ms"]), "n": len(det), "digest": digest(det, scores),
            "winner_energy": float(np.mean(e[w, np.arange(len(w))])), "not_replica0": float(np.mean(w != 0)),
            "tempering": run.get("tempering")}


def worker(root, restarts):
    """``restarts`` = R, no tempering key: one repetition per line read, answered with a JSON line"""
    import logging
    data, model = scene_and_model(root, restarts)
    logging.getLogger().setLevel(logging.WARNING)
    for _ in range(2):
        one_run(data, model)
    print(json.dumps({"ready": root}), flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        r = one_run(data, model)
        r.pop("tempering")
        print(json.dumps(r), flush=True)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def sweep(reps):
    import logging
    out = []
    for R in RS:
        data, model = scene_and_model(REPO, R)
        logging.getLogger().setLevel(logging.WARNING)
        settings = [None] + [{"ratio": ratio, "every": every} for every in EVERYS for ratio in RATIOS]
        for t in settings:
            model.config["inference"].pop("tempering", None)
            if t is not None:
                model.config["inference"]["tempering"] = t
            one_run(data, model)                              # warm-up of this setting
            runs = [one_run(data, model) for _ in range(reps)]
            row = {"restarts": R, "tempering": t, "wall_ms": spread([r["wall_ms"] for r in runs]),
                   "kernel_ms": spread([r["kernel_ms"] for r in runs]), "winner_energy": runs[-1]["winner_energy"],
                   "not_replica0": runs[-1]["not_replica0"], "detections": runs[-1]["n"], "digest": runs[-1]["digest"],
                   "same_every_repetition": len({r["digest"] for r in runs}) == 1}
            if t is not None:
                s = runs[-1]["tempering"]
                row.update(tempering_ms=spread([r["tempering"]["tempering_ms"] for r in runs]), exchanges=s["exchanges"],
                           exchange_rate=[None if v != v else float(v) for v in s["exchange_rate"]],
                           winners_on_rung0=float((s["winner_rung"] == 0).mean()))
            print(json.dumps(row), flush=True)
            out.append(row)
    return out


def ab(parent, restarts, reps):
    procs = {}
    for name, root in (("parent", parent), ("this", REPO)):
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root, "--restarts", str(restarts)],
                                       stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        for p in procs.values():
            assert "ready" in json.loads(p.stdout.readline())
        rows = {"parent": [], "this": []}
        for _ in range(reps):
            for name in ("parent", "this"):
                procs[name].stdin.write("go\n"); procs[name].stdin.flush()
                rows[name].append(json.loads(procs[name].stdout.readline()))
    finally:
        for p in procs.values():
            p.stdin.close()
            p.wait(timeout=60)
    res = {"restarts": restarts}
    for name, r in rows.items():
        res[name] = {"wall_ms": spread([x["wall_ms"] for x in r]), "kernel_ms": spread([x["kernel_ms"] for x in r]),
                     "digests": sorted({x["digest"] for x in r}), "detections": r[0]["n"], "winner_energy": r[0]["winner_energy"]}
    res["same_bytes"] = res["parent"]["digests"] == res["this"]["digests"] and len(res["this"]["digests"]) == 1
    lo, hi = res["parent"]["wall_ms"]["min"], res["parent"]["wall_ms"]["max"]
    res["this_median_within_parent_range"] = res["this"]["wall_ms"]["median"] <= hi
    res["this_median_below_parent_min"] = res["this"]["wall_ms"]["median"] < lo
    print(json.dumps(res), flush=True)
    return res


def fmt(s, digits=1):
    return f"{s['median']:.{digits}f} ({s['min']:.{digits}f} - {s['max']:.{digits}f})"


def markdown(res):
    lines = []
    base = {r["restarts"]: r for r in res.get("restarts_against_parent", [])}
    for R in RS:
        rows = [r for r in res["sweep"] if r["restarts"] == R]
        lines += [f"### R = {R}", "",
                  "| ratio | every | wall ms | chain `kernel_ms` | `tempering_ms` | exchanges | accepted per pair of rungs | "
                  "mean winner energy per tile | winners on rung 0 | detections |", "|---|---|---|---|---|---|---|---|---|---|"]
        if R in base:
            p = base[R]["parent"]
            lines.append(f"| parent, restarts only | - | {fmt(p['wall_ms'])} | {fmt(p['kernel_ms'])} | - | - | - | "
                         f"{p['winner_energy']:.3f} | - | {p['detections']} |")
        for r in rows:
            t = r["tempering"]
            if t is None:
                lines.append(f"| this tree, restarts only | - | {fmt(r['wall_ms'])} | {fmt(r['kernel_ms'])} | - | - | - | "
                             f"{r['winner_energy']:.3f} | - | {r['detections']} |")
                continue
            rate = ", ".join("-" if v is None else f"{v:.2f}" for v in r["exchange_rate"])
            lines.append(f"| {t['ratio']:g} | {t['every']} | {fmt(r['wall_ms'])} | {fmt(r['kernel_ms'])} | {fmt(r['tempering_ms'], 2)} | "
                         f"{r['exchanges']} | {rate} | {r['winner_energy']:.3f} | {100 * r['winners_on_rung0']:.0f} % | {r['detections']} |")
        lines.append("")
    if base:
        lines += ["### `restarts` = R without the key, against the parent commit", "",
                  "| R | tree | wall ms, median (min - max) | chain `kernel_ms` | detections | sha256 of detections + scores |",
                  "|---|---|---|---|---|---|"]
        for R, b in base.items():
            for name in ("parent", "this"):
                x = b[name]
                lines.append(f"| {R} | {name} | {fmt(x['wall_ms'], 2)} | {fmt(x['kernel_ms'], 2)} | {x['detections']} | {', '.join(x['digests'])} |")
        lines.append("")
        for R, b in base.items():
            lines.append(f"R = {R}: same bytes: {b['same_bytes']}; this tree's median no higher than the parent's maximum: "
                         f"{b['this_median_within_parent_range']} (below the parent's minimum: {b['this_median_below_parent_min']}).")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--parent")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md")
    ap.add_argument("--worker")
    ap.add_argument("--restarts", type=int, default=2)
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.restarts)
        return
    res = {"sweep": sweep(args.reps)}
    if args.parent:
        res["restarts_against_parent"] = [ab(os.path.abspath(args.parent), R, 10) for R in RS]
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(res))


if __name__ == "__main__":
    main()
