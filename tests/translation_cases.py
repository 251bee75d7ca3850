"""Shared inputs of the dataset-translation tests (host and GPU): the kernel cases, the test picture, the recorded reference
outputs (tests/golden/dota_translation.npz) and a DOTA-shaped tree fabricated from them."""
import json
import os

import numpy as np

from helpers import GOLDEN

#: (H, W, scale): DOTA image 2781 at its recorded scale (T = 16 taps), a scale near one half, and one just outside the
#: pass-through interval (sigma 0.015: radius 0, T = 2)
KERNEL_CASES = [(2213, 3553, 0.21193735055), (301, 257, 0.5021658679), (640, 480, 0.97)]


def make_image(H, W, seed=0):
    """random uint8 with a flat white and a flat black block: in flat regions 255 v sits on an integer, where truncation bites"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[H // 8:H // 2, W // 10:W // 2] = 255
    img[H // 2 + 5:H - H // 8, W // 3:W - W // 10] = 0
    return img


class Golden:
    def __init__(self):
        z = np.load(os.path.join(GOLDEN, "dota_translation.npz"), allow_pickle=False)
        self.ids = [int(i) for i in z["ids"]]
        self.subset = {int(i): str(s) for i, s in zip(z["ids"], z["subsets"])}
        self.categories = [str(c) for c in z["categories_config"]]
        self.banned_sources = [str(c) for c in z["banned_sources"]]
        self.target_gsd = float(z["target_gsd"])
        self.z = z

    def get(self, key, i):
        v = self.z[f"{key}_{i}"]
        return v.item() if v.ndim == 0 else v


def assert_annotations_equal(lab, gold: Golden, i: int, tol: float = 1e-12):
    assert np.array_equal(np.asarray(lab["centers"]), gold.get("centers", i))
    assert np.asarray(lab["centers"]).dtype.kind == "i"
    assert [str(c) for c in lab["categories"]] == [str(c) for c in gold.get("categories", i)]
    assert np.array_equal(np.asarray(lab["difficult"]), gold.get("difficult", i))
    err = float(np.abs(np.asarray(lab["parameters"]) - gold.get("parameters", i)).max())
    print(f"image {i}: {len(lab['centers'])} objects, max |parameters - reference| = {err:.3g}")
    assert err <= tol


def raw_shape_for(shape, scale):
    """a raw (H, W) whose rounded rescale is ``shape``"""
    from mpp_cnn_rs_object_detection_amd.dataset_translation import rescale_output_shape
    H, W = (int(round(shape[0] / scale)), int(round(shape[1] / scale)))
    for dh in (0, -1, 1):
        for dw in (0, -1, 1):
            if rescale_output_shape(H + dh, W + dw, scale) == (int(shape[0]), int(shape[1])):
                return H + dh, W + dw
    raise AssertionError((shape, scale))


def write_png(path, a, compress_level=1):
    from PIL import Image
    Image.fromarray(a).save(path, format="PNG", compress_level=compress_level)


def meta_text(date, source, gsd):
    return f"acquisition dates:{date}\nimagesource:{source}\ngsd:{gsd}\n"


def build_dota_tree(root, gold: Golden, with_images=True):
    """<root>/<subset>/{images,DOTA-v2.0_<subset>,meta}/P<id>.*: the fixture's annotation texts and meta, random pictures of a
    raw shape that rescales to the recorded shape; plus P9001 (gsd above the target) and P9002 (a banned source) in 'val'."""
    for ss in ("train", "val"):
        for d in ("images", f"DOTA-v2.0_{ss}", "meta"):
            os.makedirs(os.path.join(root, ss, d), exist_ok=True)

    def put(ss, i, text, meta, image):
        with open(os.path.join(root, ss, f"DOTA-v2.0_{ss}", f"P{i:04}.txt"), "w") as f:
            f.write(text)
        with open(os.path.join(root, ss, "meta", f"P{i:04}.txt"), "w") as f:
            f.write(meta)
        if image is None:
            open(os.path.join(root, ss, "images", f"P{i:04}.png"), "w").close()
        else:
            write_png(os.path.join(root, ss, "images", f"P{i:04}.png"), image)

    for i in gold.ids:
        date = gold.get("date", i)
        H, W = raw_shape_for(gold.get("shape", i), gold.get("scale", i))
        put(gold.subset[i], i, gold.get("text", i), meta_text("" if date == "NaT" else date.split(" ")[0], gold.get("source", i),
                                                               repr(gold.get("original_gsd", i))),
            make_image(H, W, seed=i) if with_images else None)
    small = make_image(40, 40, seed=1) if with_images else None
    line = "10.0 10.0 20.0 10.0 20.0 14.0 10.0 14.0 small-vehicle 0\n"
    put("val", 9001, line, meta_text("2016-01-02", "GoogleEarth", 0.8), small)
    put("val", 9002, line, meta_text("2016-01-02", gold.banned_sources[0], 0.2), small)


def dota_config(root, gold: Golden, name="DOTA_test"):
    return {"name": name, "dota_base_path": ["/nonexistent/DOTA/", str(root)], "subsets": ["train", "val"],
            "categories": gold.categories, "banned_sources": gold.banned_sources, "target_gsd": gold.target_gsd, "prune_empty": True}


def write_paths_config(root):
    os.makedirs(os.path.join(root, "data"), exist_ok=True)
    os.makedirs(os.path.join(root, "models_storage"), exist_ok=True)
    with open(os.path.join(root, "paths_config.json"), "w") as f:
        json.dump({"dataset_path": ["data/"], "model_path": ["models_storage/"]}, f)
