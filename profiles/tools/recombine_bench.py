#!/usr/bin/env python3
"""What recombining the restarts costs and finds (profiles/recombine.md): the scene of profiles/restarts.md -- 1024 x 1024, 16
tiles of 256 px -- through ``MPPModel.infer_image`` with ``inference.restarts`` = R in {2, 4, 8, 16}, with and without
``inference.recombine``; and ``restarts`` = R without the key, this tree against a built copy of the parent commit, the two
alternating in one call.

    python profiles/tools/recombine_bench.py OUT.json [--parent DIR] [--reps N] [--md OUT.md]

Profiler off.  Every setting is warmed up before it is timed.  Wall times are a host clock around ``infer_image``, which ends
in the copy of the merged detections to the host.  The time of ``mpp_recombine`` and of ``mpp_total_energy_all`` is taken
inside the same ``infer_image`` calls, on the same state: for the duration of the call the context runs on a torch stream and
two events on it bracket the launches and the copy back (``device_ms``); a host clock around the call gives ``host_ms``.
``--parent DIR``: a ``git archive`` copy of the parent commit with ``libmppgpu.so`` built in it.  The A/B runs one worker
process per tree and R (``--worker``), each warmed up, and asks them for one repetition in turn."""
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
RS = (2, 4, 8, 16)
TIMES = {}                      # name of a timed MppContext method -> [(device ms, host ms)] of the calls since it was cleared


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


def time_context_calls(names=("total_energy_all", "recombine")):
    """wrap the named ``MppContext`` methods: each call runs on a torch stream between two events and is clocked on the host"""
    import torch
    from mpp_cnn_rs_object_detection_amd.hip_api import MppContext
    for name in names:
        plain = getattr(MppContext, name)

        def timed(self, *a, _plain=plain, _name=name, **kw):
            dev = torch.device("cuda", self.device)
            stream = torch.cuda.Stream(dev)
            self.synchronize()
            self.set_stream(stream.cuda_stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            out = _plain(self, *a, **kw)
            e1.record(stream)
            e1.synchronize()
            host = (time.perf_counter() - t0) * 1e3
            self.set_stream(None)
            TIMES.setdefault(_name, []).append((e0.elapsed_time(e1), host))
            return out
        setattr(MppContext, name, timed)


def digest(detections, scores):
    import numpy as np
    h = hashlib.sha256()
    h.update(np.asarray([(p.x, p.y, p.size, p.ratio, p.angle) for p in detections], dtype=np.float64).tobytes())
    h.update(np.asarray(scores, dtype=np.float64).tobytes())
    return h.hexdigest()[:16]


def one_run(data, model):
    import numpy as np
    TIMES.clear()
    t0 = time.perf_counter()
    det, scores = model.infer_image(data, seed=SEED)
    wall = (time.perf_counter() - t0) * 1e3
    run = model.last_run
    e, w = run["replica_energy"], run["replica_winner"]
    out = {"wall_ms": wall, "kernel_ms": float(run["kernel_ms"]), "n": len(det), "digest": digest(det, scores),
           "winner_energy": float(np.mean(e[w, np.arange(len(w))])), "calls": {k: list(v) for k, v in TIMES.items()}}
    s = run.get("recombine")
    if s is not None:
        out["recombine"] = {"E_winner": float(np.mean(s["E_winner"])), "E_after": float(np.mean(s["E_after"])),
                            "status1": float(np.mean(s["status"] == 1)), "status2": int(np.count_nonzero(s["status"] == 2)),
                            "clusters": float(np.mean(s["n_clusters"])), "taken": float(np.mean(s["n_taken"])),
                            "worst_tile": float(np.max(s["E_after"] - s["E_winner"]))}
    return out


def worker(root, restarts):
    """``restarts`` = R, no recombine key: one repetition per line read, answered with a JSON line"""
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
        r.pop("calls")
        print(json.dumps(r), flush=True)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def sweep(reps):
    import logging
    out = []
    for R in RS:
        data, model = scene_and_model(REPO, R)
        logging.getLogger().setLevel(logging.WARNING)
        if R == RS[0]:
            time_context_calls()
            for _ in range(3):                                # (the process's first timed calls also pay for torch's streams and events)
                one_run(data, model)
        for on in (False, True):
            model.config["inference"]["recombine"] = on
            one_run(data, model)                              # warm-up of this setting
            runs = [one_run(data, model) for _ in range(reps)]
            row = {"restarts": R, "recombine": on, "wall_ms": spread([r["wall_ms"] for r in runs]),
                   "kernel_ms": spread([r["kernel_ms"] for r in runs]), "winner_energy": runs[-1]["winner_energy"],
                   "detections": runs[-1]["n"], "digest": runs[-1]["digest"],
                   "same_every_repetition": len({r["digest"] for r in runs}) == 1,
                   "total_energy_all_ms": spread([r["calls"]["total_energy_all"][0][0] for r in runs]),
                   "total_energy_all_host_ms": spread([r["calls"]["total_energy_all"][0][1] for r in runs])}
            if on:
                row.update(recombine=runs[-1]["recombine"], recombine_ms=spread([r["calls"]["recombine"][0][0] for r in runs]),
                           recombine_host_ms=spread([r["calls"]["recombine"][0][1] for r in runs]))
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
    res["this_median_within_parent_range"] = lo <= res["this"]["wall_ms"]["median"] <= hi
    res["this_median_no_higher_than_parent_max"] = res["this"]["wall_ms"]["median"] <= hi
    print(json.dumps(res), flush=True)
    return res


def fmt(s, digits=1):
    return f"{s['median']:.{digits}f} ({s['min']:.{digits}f} - {s['max']:.{digits}f})"


def markdown(res):
    lines = ["| R | mean tile energy, restarts winner | recombined | gain per tile | tiles with status 1 | status 2 | clusters per tile | "
             "taken per tile | `mpp_recombine` ms (events) | `mpp_total_energy_all` ms (events) | wall ms, restarts only | "
             "wall ms, with recombine | detections (restarts / recombined) |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for R in RS:
        off = next(r for r in res["sweep"] if r["restarts"] == R and not r["recombine"])
        on = next(r for r in res["sweep"] if r["restarts"] == R and r["recombine"])
        s = on["recombine"]
        lines.append(f"| {R} | {s['E_winner']:.3f} | {s['E_after']:.3f} | {s['E_winner'] - s['E_after']:.3f} | {100 * s['status1']:.0f} % | "
                     f"{s['status2']} | {s['clusters']:.1f} | {s['taken']:.1f} | {fmt(on['recombine_ms'], 3)} | "
                     f"{fmt(on['total_energy_all_ms'], 3)} | {fmt(off['wall_ms'])} | {fmt(on['wall_ms'])} | {off['detections']} / {on['detections']} |")
    lines += ["", "Host clock around the two calls (launches, copy back, synchronise), ms:", "",
              "| R | `mpp_recombine` | `mpp_total_energy_all` | highest E_after - E_winner of a tile |", "|---|---|---|---|"]
    for R in RS:
        on = next(r for r in res["sweep"] if r["restarts"] == R and r["recombine"])
        lines.append(f"| {R} | {fmt(on['recombine_host_ms'], 3)} | {fmt(on['total_energy_all_host_ms'], 3)} | {on['recombine']['worst_tile']:.3g} |")
    lines.append("")
    base = {r["restarts"]: r for r in res.get("restarts_against_parent", [])}
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
            lines.append(f"R = {R}: same bytes: {b['same_bytes']}; this tree's median within the parent's min - max span: "
                         f"{b['this_median_within_parent_range']} (no higher than the parent's maximum: {b['this_median_no_higher_than_parent_max']}).")
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
