"""The CNN-only baseline on the GPU: device threshold + distance NMS (mpp_detect_centers) and mark classes (mpp_mark_classes)
against the reference's recorded output, the tapes' naive init and the host greedy; the output-overflow contract; the
``main.py -m posnet|shapenet -p infereval`` paths; AP on clean synthetic maps and the hbb evaluation."""
import ctypes
import glob
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLDEN, REPO, Tape
from test_cnn_detection_host import CASES, host_greedy, mark_maps
from test_gpu_pipeline import synthetic_dataset, write_image  # noqa: F401  (fixture)
from mpp_cnn_rs_object_detection_amd import cnn_detection as cd
from mpp_cnn_rs_object_detection_amd import dota_eval, hip_api, mappings, shapes, synth
from mpp_cnn_rs_object_detection_amd.dota_results import DOTAResultsTranslator

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "cnn_baseline_golden.npz"))


@pytest.fixture(scope="module")
def golden_marks(golden):
    import torch
    m = mark_maps(golden["mark_cls"], golden["tie_rc"], golden["tie_k"], golden["tie_j"])
    return [torch.from_numpy(x).cuda() for x in m]


def device_equals_host(det, thr, strict, nms=6.0):
    c, s, n = cd.detect_centers(det, thr, strict, nms)
    det_np = det.cpu().numpy() if hasattr(det, "cpu") else det
    hc, hs, hn = host_greedy(det_np, thr, strict, nms)
    assert n == hn
    np.testing.assert_array_equal(c, hc)
    assert s.dtype == np.float32 and np.array_equal(s, hs)
    return c, s, n


@pytest.mark.parametrize("rule,thr", CASES)
def test_device_matches_the_reference_fixture_bit_for_bit(golden, golden_marks, rule, thr):
    key = f"{rule}_{int(round(thr * 10))}"
    centers, scores, n = cd.detect_centers(golden["det"], thr, strict=rule == "gt")
    assert n == int(golden[f"{key}_n_cand"])
    np.testing.assert_array_equal(centers, golden[f"{key}_centers"])
    assert scores.dtype == np.float32 and np.array_equal(scores, golden[f"{key}_scores"])
    np.testing.assert_array_equal(cd.mark_classes(golden_marks, centers), golden[f"{key}_classes"])
    params = cd.mark_params(golden_marks, centers, mappings.default_mappings())
    np.testing.assert_allclose(params, golden[f"{key}_params"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(cd.shapenet_polygons(centers, params), golden[f"{key}_polys"], rtol=0, atol=1e-9)
    np.testing.assert_array_equal(cd.posnet_boxes(centers), golden[f"{key}_boxes"])
    # the float32(thr) boundary pixels: in for >=, out for >, their neighbours on the right side
    t = np.float32(thr)
    kept = {tuple(c) for c in centers}
    for r, c in golden["spots"]:
        v = golden["det"][r, c]
        if abs(float(v) - thr) < 1e-6:
            assert ((r, c) in kept) == (v > t or (rule == "ge" and v == t))


def test_mark_classes_take_the_first_of_tied_maxima(golden, golden_marks):
    cls = cd.mark_classes(golden_marks, golden["tie_rc"])
    rc, k = golden["tie_rc"], golden["tie_k"]
    np.testing.assert_array_equal(cls[np.arange(len(k)), k], golden["mark_cls"][k, rc[:, 0], rc[:, 1]])
    m = [x.cpu().numpy() for x in golden_marks]
    np.testing.assert_array_equal(cls, np.stack([np.argmax(x[rc[:, 0], rc[:, 1]], axis=1) for x in m], axis=1))
    with pytest.raises(ValueError):
        cd.mark_classes(golden_marks, [[0, 320]])


TAPES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "tape_*.npz"))
               if not p.endswith(("_gt.npz", "_empty.npz")))


@pytest.mark.parametrize("name", TAPES)
def test_tapes_naive_init(name):
    """>= at the tape's threshold gives the tape's recorded init: the same centres with the same marks; the order is the key
    order (the recorded one comes from an unstable argsort over tied 1.0 peaks, so only the set is the reference's)"""
    t = Tape(name)
    centers, scores, _ = cd.detect_centers(t.det, t.setup.detection_threshold, strict=False)
    hc, _, _ = host_greedy(t.det, t.setup.detection_threshold, False)
    np.testing.assert_array_equal(centers, hc)
    vals = cd.mark_values(t.marks, centers, mappings.default_mappings())
    got = np.concatenate([centers.astype(float), vals], axis=1)
    rows = lambda a: a[np.lexsort(a[:, :2].T[::-1])]
    np.testing.assert_allclose(rows(got), rows(t.init), rtol=0, atol=1e-12)


def _ramp(H, W):
    return (np.arange(H * W, dtype=np.float64).reshape(H, W) / (H * W)).astype(np.float32)


def test_host_greedy_equivalence_on_hard_maps():
    import torch
    ctx = cd.context(0)
    # plateau: saturated 1.0 blobs, every tie goes to the larger index
    det = np.zeros((200, 260), np.float32)
    for r, c in [(20, 20), (25, 24), (100, 130), (60, 63), (63, 64), (190, 250)]:
        det[max(0, r - 5):r + 6, max(0, c - 5):c + 6] = 1.0
    device_equals_host(det, 0.5, False)
    # strictly monotone ramp: every decision waits on the one before it
    device_equals_host(_ramp(300, 300), 0.0, True)
    assert ctx.get_option("detect_launches") > 1
    # pitched view cut from a larger tensor, H / W not multiples of the tile
    tile = synth.make_tile(512, 300, tile_id=5, noise=0.0)
    big = torch.from_numpy(np.pad(tile.det, ((3, 5), (7, 9)))).cuda()
    device_equals_host(big[3:3 + 333, 7:7 + 451], 0.2, False)
    device_equals_host(tile.det[:97, :130], 0.2, True, 4.5)
    device_equals_host(tile.det, 0.2, True, 0.0)
    # negative values and -0.0 rank like numbers
    rng = np.random.default_rng(3)
    neg = (rng.standard_normal((70, 90)) * 0.3).astype(np.float32)
    neg[5, 5], neg[5, 7] = -0.0, 0.0
    device_equals_host(neg, -0.5, False, 2.5)
    # empty and 1 x 1
    c, s, n = device_equals_host(np.zeros((64, 64), np.float32), 0.2, False)
    assert n == 0 and len(c) == 0 and ctx.get_option("detect_launches") == 0
    device_equals_host(np.full((1, 1), 0.9, np.float32), 0.2, True)
    c, _, n = device_equals_host(np.zeros((0, 5), np.float32), 0.2, True)
    assert n == 0
    with pytest.raises(hip_api.MppError):
        cd.detect_centers(tile.det, 0.2, True, 40.0)


def test_dota_density_4096():
    xy, marks = synth.make_gt(4096, 100000, tile_id=9)
    det = np.full((4096, 4096), 0.02, np.float32)
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[-5:6, -5:6]
    bump = np.exp(-(yy ** 2 + xx ** 2) / (2 * 1.2 ** 2)).astype(np.float32)
    for x, y in xy:
        x0, y0 = max(0, x - 5), max(0, y - 5)
        x1, y1 = min(4096, x + 6), min(4096, y + 6)
        sub = bump[x0 - x + 5:x1 - x + 5, y0 - y + 5:y1 - y + 5]
        det[x0:x1, y0:y1] = np.maximum(det[x0:x1, y0:y1], sub)
    det += (rng.random(det.shape, dtype=np.float32) * 0.05).astype(np.float32)
    c, _, n = device_equals_host(det, 0.1, True)
    assert len(c) >= len(xy) * 0.9 and n > 10 * len(c)


def test_output_overflow_reports_the_needed_count():
    import torch
    tile = synth.make_tile(256, 60, tile_id=3)
    want, _, _ = cd.detect_centers(tile.det, 0.2, True)
    K = len(want)
    assert K > 10
    ctx = cd.context(0)
    det = torch.from_numpy(tile.det).cuda()
    cap = K - 3
    xy = torch.full((K + 8, 2), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((K + 8,), -7.0, dtype=torch.float32, device="cuda")
    n_cand, n_kept = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = ctx._L.mpp_detect_centers(ctx._h, 256, 256, 256, hip_api._ptr(det), 0.2, 1, 6.0, cap, hip_api._ptr(xy), hip_api._ptr(sc),
                                   ctypes.byref(n_cand), ctypes.byref(n_kept))
    torch.cuda.synchronize()
    assert rc == cd.E_OUTPUT_FULL and n_kept.value == K
    assert (xy == -7).all() and (sc == -7.0).all()
    with pytest.raises(hip_api.MppError) as e:
        cd.detect_centers(tile.det, 0.2, True, cap=cap)
    assert e.value.code == cd.E_OUTPUT_FULL


def _write_models(root, pos_name="posvec_dota", shp_name="shape_dota"):
    import torch
    from mpp_cnn_rs_object_detection_amd import unet
    torch.manual_seed(0)
    for kind, name, net in (("posnet", pos_name, unet.PosNet()), ("shapenet", shp_name, unet.ShapeNet())):
        d = root / "models_storage" / kind / name
        os.makedirs(d, exist_ok=True)
        torch.save(net.state_dict(), d / "model.pt")


def _run_main(root, kind, cfg):
    path = root / f"cfg_{kind}_{len(cfg)}.json"
    with open(path, "w") as f:
        json.dump(cfg, f)
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "-p", "infereval", "-m", kind, "-c", str(path), "-d", "SYNTH",
                        "-o"], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = root / "data" / "inference" / "SYNTH" / "val" / cfg["model_name"]
    for t in dota_eval.IOU_THRESHOLDS:
        m = json.load(open(out / "dota" / f"metrics{t:.2f}.json"))
        assert 0.0 <= m["vehicle"]["ap"] <= 1.0
    return out


def test_main_posnet_and_shapenet_infereval(synthetic_dataset):  # noqa: F811
    root, _ = synthetic_dataset
    write_image(root, "val", 8, 23)
    _write_models(root)
    out = _run_main(root, "posnet", {"model_name": "posvec_dota", "data_loader": {"dataset": "SYNTH"}})
    for k in (7, 8):
        res = pickle.load(open(out / f"{k:04}_results.pkl", "rb"))
        assert set(res) == {"detection", "detection_score", "detection_type", "detection_map"}
        assert res["detection_type"] == "map" and res["detection_map"].dtype == np.float32
        cand = np.array(np.where(res["detection_map"] > 0.2)).T
        np.testing.assert_array_equal(res["detection"], cand)
        np.testing.assert_array_equal(res["detection_score"], res["detection_map"][cand[:, 0], cand[:, 1]])
    lines = [l.split() for l in open(out / "dota" / "det" / "vehicle.txt").read().splitlines() if l]
    assert all(len(l) == 6 for l in lines)
    gt = dota_eval.parse_gt(str(out / "dota" / "gt" / "0007.txt"))
    assert len(gt) > 0 and all(len(o["bbox"]) == 8 for o in gt)
    keys = {"output", "mappings", "detection", "detection_type", "detection_center", "detection_score", "detection_params", "pos_model"}
    for cfg in ({"model_name": "shape_dota", "data_loader": {"dataset": "SYNTH"}},
                {"model_name": "shape_dota", "data_loader": {"dataset": "SYNTH"}, "inference": {"pos_model": "posvec_dota"}}):
        out = _run_main(root, "shapenet", cfg)
        for k in (7, 8):
            res = pickle.load(open(out / f"{k:04}_results.pkl", "rb"))
            assert set(res) == keys and res["detection_type"] == "poly"
            assert res["pos_model"] == cfg.get("inference", {}).get("pos_model")
            n = len(res["detection_score"])
            assert res["detection"].shape == (n, 4, 2) and len(res["detection_params"]) == n == len(res["detection_center"])
            assert len(res["output"]) == 3 and res["output"][0].shape[:2] == (1, 32)
            if "inference" not in cfg:
                labels = pickle.load(open(root / "data" / "SYNTH" / "val" / "annotations" / f"{k:04}.pkl", "rb"))
                np.testing.assert_array_equal(res["detection_center"], labels["centers"])
                assert np.all(res["detection_score"] == 1.0)
        lines = [l.split() for l in open(out / "dota" / "det" / "vehicle.txt").read().splitlines() if l]
        assert all(len(l) == 10 for l in lines)


def test_clean_maps_reach_high_ap_and_hbb_equals_obb_of_the_same_boxes(tmp_path):
    H, W = 384, 448
    xy, marks = synth.make_gt(384, 400, tile_id=31)
    xy = xy[(xy[:, 1] < W - 10)]
    marks = marks[: len(xy)]
    d = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)) + np.eye(len(xy)) * 1e9
    assert d.min() > 6
    det, mk = synth.render_maps((H, W), xy, marks)
    centers, scores, _ = cd.detect_centers(det, 0.2, strict=False)
    params = cd.mark_params(mk, centers, mappings.default_mappings())
    polys = cd.shapenet_polygons(centers, params)
    gt_params = np.stack(shapes.sra_to_wla(marks[:, 0], marks[:, 1], marks[:, 2]), axis=1)
    gt_poly = np.array([shapes.rect_to_poly(c, short=p[0], long=p[1], angle=p[2]) for c, p in zip(xy, gt_params)])

    def evaluate(name, det_type, add):
        tr = DOTAResultsTranslator("SYNTH", "val", str(tmp_path / name), det_type, all_classes=["vehicle"])
        tr.add_gt(1, difficulty=np.zeros(len(gt_poly)), polygons=gt_poly, categories=["vehicle"] * len(gt_poly))
        add(tr)
        tr.save()
        base = tmp_path / name / "dota"
        return dota_eval.voc_eval(str(base / "det" / "{:s}.txt"), str(base / "gt" / "{:s}.txt"), str(base / "imageSet.txt"),
                                  "vehicle", ovthresh=0.5, det_type=det_type)[2]

    ap = evaluate("shape", "obb", lambda tr: tr.add_detections(1, scores, ["vehicle"] * len(scores), polygons=polys, flip_coor=True))
    assert ap >= 0.9, ap
    boxes = cd.posnet_boxes(centers)
    ap_hbb = evaluate("hbb", "hbb", lambda tr: tr.add_detections(1, scores, ["vehicle"] * len(scores), bbox=boxes, flip_coor=False))
    quads = cd.box_polygons(boxes)
    tr_q = DOTAResultsTranslator("SYNTH", "val", str(tmp_path / "quads2"), "hbb", all_classes=["vehicle"])
    tr_q.add_gt(1, difficulty=np.zeros(len(gt_poly)), polygons=gt_poly, categories=["vehicle"] * len(gt_poly))
    tr_q.add_detections(1, scores, ["vehicle"] * len(scores), polygons=quads, flip_coor=False)
    tr_q.save()
    base = tmp_path / "quads2" / "dota"
    ap_q = dota_eval.voc_eval(str(base / "det" / "{:s}.txt"), str(base / "gt" / "{:s}.txt"), str(base / "imageSet.txt"), "vehicle",
                              ovthresh=0.5, det_type="obb")[2]
    assert ap_hbb == ap_q and ap_hbb > 0.0
