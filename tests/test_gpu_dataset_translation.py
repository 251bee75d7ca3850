"""Dataset translation on the GPU: the rescale kernels against the scipy restatement of skimage 0.18.1 (``rescale_ref.py``),
band and pitch invariance, and ``translate_dota`` / ``translate_cowc`` end to end on fabricated trees whose annotations are the
reference's own (tests/golden/dota_translation.npz)."""
import json
import os
import pickle

import numpy as np
import pytest

from mpp_cnn_rs_object_detection_amd import dataset_translation as dt
from rescale_ref import rescale_ref, to_uint8
from translation_cases import (KERNEL_CASES, Golden, assert_annotations_equal, build_dota_tree, dota_config, make_image,
                               write_paths_config, write_png)

pytestmark = pytest.mark.gpu


def device_rescale(ctx, img, scale, **kw):
    """(uint8, float64) of MppContext.rescale for a host picture"""
    import torch
    _, tables = dt.rescale_image_tables(img.shape[0], img.shape[1], scale)
    src = img if hasattr(img, "is_cuda") else torch.from_numpy(np.ascontiguousarray(img)).cuda()
    u8, f64 = ctx.rescale(src, tables, out_f64=True, **kw)
    ctx.synchronize()
    return u8.cpu().numpy(), f64.cpu().numpy()


@pytest.mark.parametrize("H,W,scale", KERNEL_CASES)
def test_kernel_against_the_scipy_restatement(H, W, scale):
    """float64 within 1e-12 (at most (2 * 18 + 2)^2 ~ 1.4 k terms of size <= 1 at eps 1.1e-16: 1.6e-13); the 8-bit output is
    the truncation of the kernel's own float64 output, and equals the restatement's wherever the restatement's 255 v is
    farther than 1e-9 (255 x 1e-12, rounded up) from an integer; elsewhere it differs by at most one level."""
    from mpp_cnn_rs_object_detection_amd import hip_api
    img = make_image(H, W)
    ref = rescale_ref(img, scale)
    ctx = hip_api.MppContext(0)
    u8, f64 = device_rescale(ctx, img, scale)
    assert u8.shape == ref.shape == f64.shape and u8.dtype == np.uint8
    err = float(np.abs(f64 - ref).max())
    ref_u8 = to_uint8(ref)
    frac = np.abs(255 * ref - np.round(255 * ref))
    differ = u8 != ref_u8
    worst = float(frac[differ].max()) if differ.any() else 0.0
    print(f"{H} x {W} @ {scale}: max |device - restatement| = {err:.3g}; {int(differ.sum())} of {differ.size} 8-bit values "
          f"differ, all within {worst:.3g} of an integer; bands {ctx.get_option('rescale_bands')}")
    assert err <= 1e-12
    assert np.array_equal(u8, np.floor(255 * np.clip(f64, 0, 1)).astype(np.uint8))
    assert np.array_equal(u8[frac > 1e-9], ref_u8[frac > 1e-9])
    assert int(np.abs(u8.astype(int) - ref_u8.astype(int)).max()) <= 1


def test_bands_do_not_change_the_result():
    from mpp_cnn_rs_object_detection_amd import hip_api
    H, W, scale = KERNEL_CASES[0]
    img = make_image(H, W, seed=3)
    ctx = hip_api.MppContext(0)
    u8, f64 = device_rescale(ctx, img, scale)
    assert ctx.get_option("rescale_bands") == 1
    whole = ctx.get_option("rescale_bytes")
    limit = whole // 6
    u8b, f64b = device_rescale(ctx, img, scale, workspace_limit=limit)
    bands = ctx.get_option("rescale_bands")
    print(f"workspace {whole} bytes in one band; limit {limit}: {bands} bands")
    assert bands >= 4
    assert np.array_equal(u8, u8b) and np.array_equal(f64, f64b)
    small = hip_api.MppContext(0)                       # a context that starts with the small workspace stays within the limit
    u8c, f64c = device_rescale(small, img, scale, workspace_limit=limit)
    assert small.get_option("rescale_bytes") <= limit and np.array_equal(u8, u8c) and np.array_equal(f64, f64c)
    with pytest.raises(hip_api.MppError, match="workspace"):
        device_rescale(small, img, scale, workspace_limit=4096)


def test_source_pitch():
    import torch
    from mpp_cnn_rs_object_detection_amd import hip_api
    H, W, scale = KERNEL_CASES[1]
    img = make_image(H, W, seed=5)
    ctx = hip_api.MppContext(0)
    u8, f64 = device_rescale(ctx, img, scale)
    wide = torch.from_numpy(make_image(H + 7, W + 37, seed=6)).cuda()
    wide[3:3 + H, 11:11 + W] = torch.from_numpy(img).cuda()
    view = wide[3:3 + H, 11:11 + W]                       # pitch 3 (W + 37), first pixel 33 bytes off a 16-byte boundary
    assert view.stride(0) == 3 * (W + 37)
    u8p, f64p = device_rescale(ctx, view, scale)
    assert np.array_equal(u8, u8p) and np.array_equal(f64, f64p)
    with pytest.raises(ValueError):
        ctx.rescale(wide[:, :, :2], dt.rescale_image_tables(H, W, scale)[1])
    bad = list(dt.rescale_image_tables(H, W, scale)[1])
    bad[2] = bad[2] + 1                                   # a column index W: outside the image, refused before any launch
    with pytest.raises(hip_api.MppError, match="outside"):
        ctx.rescale(torch.from_numpy(img).cuda(), bad)


def test_translate_dota_end_to_end(tmp_path, monkeypatch):
    import torch
    from mpp_cnn_rs_object_detection_amd import hip_api, paths, unet_training
    gold = Golden()
    raw_root = tmp_path / "raw"
    build_dota_tree(str(raw_root), gold)
    write_paths_config(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    timings = dt.translate_dota(dota_config(raw_root, gold))
    base = tmp_path / "data" / "DOTA_test"
    assert json.load(open(base / "config.json"))["name"] == "DOTA_test"
    ctx = hip_api.MppContext(0)
    for ss in ("train", "val"):
        ids = [i for i in gold.ids if gold.subset[i] == ss]
        for d in dt.SUB_FOLDERS:
            assert (base / ss / d).is_dir()
        assert os.listdir(base / ss / "images_w_annotations") == []
        for d, ext in (("raw_images", "png"), ("images", "png"), ("raw_annotations", "txt"), ("annotations", "pkl"), ("metadata", "json")):
            assert sorted(os.listdir(base / ss / d)) == [f"{i:04}.{ext}" for i in sorted(ids)]      # 9001, 9002 absent
        assert [r["id"] for r in json.load(open(base / ss / "paths_and_meta.json"))] == sorted(ids)
        for i in ids:
            with open(base / ss / "annotations" / f"{i:04}.pkl", "rb") as f:
                assert_annotations_equal(pickle.load(f), gold, i, tol=1e-12)
            meta = json.load(open(base / ss / "metadata" / f"{i:04}.json"))
            assert meta["shape"] == list(gold.get("shape", i)) and meta["n_objects"] == gold.get("n_objects", i)
            assert meta["scale"] == gold.get("scale", i) and meta["original_gsd"] == gold.get("original_gsd", i)
            assert meta["source"] == gold.get("source", i) and meta["date"] == gold.get("date", i)
            assert open(base / ss / "raw_annotations" / f"{i:04}.txt").read() == gold.get("text", i)
            raw = dt.read_rgb(str(base / ss / "raw_images" / f"{i:04}.png"))
            assert np.array_equal(raw, dt.read_rgb(str(raw_root / ss / "images" / f"P{i:04}.png")))
            want = ctx.rescale(torch.from_numpy(raw).cuda(), dt.rescale_image_tables(raw.shape[0], raw.shape[1], meta["scale"])[1])
            from PIL import Image
            with Image.open(base / ss / "images" / f"{i:04}.png") as im:
                assert im.mode == "RGB"
                assert np.array_equal(np.asarray(im), want.cpu().numpy())
        listed = paths.fetch_data_paths("DOTA_test", ss)
        assert [os.path.basename(p) for p in listed["images"]] == [f"{i:04}.png" for i in sorted(ids)]
        assert len(listed["annotations"]) == len(listed["metadata"]) == len(ids)
    data = unet_training.ResidentSubset("DOTA_test", "train", 0)          # what train_unet loads its subsets with
    assert data.n_images == 2 and list(data.n_objects) == [gold.get("n_objects", i) for i in (2800, 2804)]
    assert [tuple(s) for s in data.shapes] == [tuple(gold.get("shape", i)[:2]) for i in (2800, 2804)]
    assert sorted(t["id"] for t in timings) == sorted(gold.ids)
    for t in sorted(timings, key=lambda t: t["id"]):
        print("image {id}: decode {decode:.3f} s, upload {upload:.4f} s, kernel {kernel:.5f} s, download {download:.4f} s, "
              "encode {encode:.3f} s".format(**t))


def test_translate_dota_copies_an_image_at_the_target_gsd_through(tmp_path, monkeypatch):
    gold = Golden()
    raw_root = tmp_path / "raw"
    for d in ("images", "DOTA-v2.0_val", "meta"):
        os.makedirs(raw_root / "val" / d)
    img = make_image(70, 90, seed=2)
    write_png(str(raw_root / "val" / "images" / "P0007.png"), np.dstack([img, np.full((70, 90), 255, np.uint8)]))   # RGBA
    write_png(str(raw_root / "val" / "images" / "P0008.png"), img[:, :, 0])                                        # one channel
    for i in (7, 8):
        with open(raw_root / "val" / "DOTA-v2.0_val" / f"P{i:04}.txt", "w") as f:
            f.write("10.0 20.0 30.0 20.0 30.0 28.0 10.0 28.0 small-vehicle 0\n")
        with open(raw_root / "val" / "meta" / f"P{i:04}.txt", "w") as f:
            f.write("acquisition dates:\nimagesource:GoogleEarth\ngsd:0.497\n")
    write_paths_config(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    cfg = dict(dota_config(raw_root, gold, name="THROUGH"), subsets=["val"])
    with pytest.raises(ValueError, match="3 channels"):
        dt.translate_dota(cfg)
    os.remove(raw_root / "val" / "images" / "P0008.png")
    dt.translate_dota(cfg)
    out = tmp_path / "data" / "THROUGH" / "val"
    assert np.array_equal(dt.read_rgb(str(out / "images" / "0007.png")), img)
    meta = json.load(open(out / "metadata" / "0007.json"))
    assert meta["shape"] == [70, 90, 3] and meta["scale"] == 0.497 / 0.5 and meta["date"] == "NaT"
    with open(out / "annotations" / "0007.pkl", "rb") as f:
        assert np.array_equal(pickle.load(f)["centers"], [[24, 20]])     # unscaled


def test_translate_cowc(tmp_path, monkeypatch):
    import torch
    from mpp_cnn_rs_object_detection_amd import hip_api
    raw_root = tmp_path / "cowc"
    os.makedirs(raw_root / "Toronto")
    os.makedirs(raw_root / "Utah")
    pictures = {}
    for k, (town, stem, cars) in enumerate([("Toronto", "a_01", [(3, 7), (100, 50), (199, 299)]), ("Utah", "b_02", []),
                                            ("Utah", "b_03", [(10, 10)])]):
        img = make_image(200, 300, seed=k)
        pictures[stem] = img
        write_png(str(raw_root / town / f"{stem}.png"), np.dstack([img, np.full(img.shape[:2], 255, np.uint8)]))
        ann = np.zeros((200, 300, 4), np.uint8)
        for r, c in cars:
            ann[r, c] = (255, 0, 0, 255)
        write_png(str(raw_root / town / f"{stem}_Annotated_Cars.png"), ann)
        write_png(str(raw_root / town / f"{stem}_Annotated_Negatives.png"), np.zeros((200, 300, 4), np.uint8))
    write_paths_config(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    cfg = {"name": "COWC_test", "cowc_base_path": [str(raw_root)], "target_gsd": 0.5, "prune_empty": True, "drop_rate": 0.0}
    dt.translate_cowc(cfg)
    out = tmp_path / "data" / "COWC_test" / "val"
    assert sorted(os.listdir(out / "images")) == ["0000.png", "0002.png"]              # 0001 has no cars: pruned
    assert sorted(os.listdir(out / "raw_images")) == ["0000.png", "0002.png"] and os.listdir(out / "raw_annotations") == []
    scale = 0.15 / 0.5
    with open(out / "annotations" / "0000.pkl", "rb") as f:
        lab = pickle.load(f)
    assert np.array_equal(lab["centers"], [[int(r * scale), int(c * scale)] for r, c in [(3, 7), (100, 50), (199, 299)]])
    assert np.array_equal(lab["parameters"], [[4.0, 4.0, 0.0]] * 3) and list(lab["categories"]) == ["vehicle"] * 3
    assert np.array_equal(lab["difficult"], np.zeros(3))
    meta = json.load(open(out / "metadata" / "0002.json"))
    assert meta == {"shape": [60, 90, 3], "n_objects": 1, "scale": scale, "original_gsd": 0.15}
    ctx = hip_api.MppContext(0)
    want = ctx.rescale(torch.from_numpy(pictures["b_03"]).cuda(), dt.rescale_image_tables(200, 300, scale)[1])
    assert np.array_equal(dt.read_rgb(str(out / "images" / "0002.png")), want.cpu().numpy())

