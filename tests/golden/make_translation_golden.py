"""Records tests/golden/dota_translation.npz from the reference's shipped sample dataset ``data_sample/DOTA_gsd50``.

Run only in the build container (the reference is mounted read-only at /root/reference and never travels):

    python tests/golden/make_translation_golden.py [reference root]

For images 2800, 2804 (train) and 2781, 2789, 2794 (val) it stores what the reference's own ``translate_dota`` wrote: the raw
annotation text it copied, the metadata (scale, shape, n_objects, original_gsd, source, date) and the annotation pickle
(centers, parameters, categories, difficult).  Only data files are read and only arrays are written; no reference source is
copied.
"""
import json
import os
import pickle
import sys

import numpy as np

IMAGES = [("train", 2800), ("train", 2804), ("val", 2781), ("val", 2789), ("val", 2794)]


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    base = os.path.join(root, "data_sample", "DOTA_gsd50")
    with open(os.path.join(base, "config.json")) as f:
        cfg = json.load(f)
    out = {"ids": np.array([i for _, i in IMAGES], dtype=np.int64), "subsets": np.array([s for s, _ in IMAGES]),
           "categories_config": np.array(cfg["categories"]), "banned_sources": np.array(cfg["banned_sources"]),
           "target_gsd": np.float64(cfg["target_gsd"])}
    n = 0
    for subset, i in IMAGES:
        d = os.path.join(base, subset)
        with open(os.path.join(d, "raw_annotations", f"{i:04}.txt")) as f:
            out[f"text_{i}"] = np.array(f.read())
        with open(os.path.join(d, "metadata", f"{i:04}.json")) as f:
            meta = json.load(f)
        out[f"shape_{i}"] = np.array(meta["shape"], dtype=np.int64)
        out[f"n_objects_{i}"] = np.int64(meta["n_objects"])
        out[f"scale_{i}"] = np.float64(meta["scale"])
        out[f"original_gsd_{i}"] = np.float64(meta["original_gsd"])
        out[f"source_{i}"] = np.array(meta["source"])
        out[f"date_{i}"] = np.array(meta["date"])
        with open(os.path.join(d, "annotations", f"{i:04}.pkl"), "rb") as f:
            lab = pickle.load(f)
        out[f"centers_{i}"] = np.asarray(lab["centers"], dtype=np.int64)
        out[f"parameters_{i}"] = np.asarray(lab["parameters"], dtype=np.float64)
        out[f"categories_{i}"] = np.asarray(lab["categories"]).astype(str)
        out[f"difficult_{i}"] = np.asarray(lab["difficult"], dtype=np.int64)
        n += len(lab["centers"])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dota_translation.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(IMAGES)} images, {n} objects, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
