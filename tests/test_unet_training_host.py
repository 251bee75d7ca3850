"""U-Net training, host side: patch-plan densities and object anchors, the D4 angle convention, unsupported options."""
import copy
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN, REPO
from unet_train_cases import density_images
from mpp_cnn_rs_object_detection_amd import shapes
from mpp_cnn_rs_object_detection_amd import unet_training as ut


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "unet_train_golden.npz"))


def shipped(kind):
    name = "posnet/config_pos.json" if kind == "posnet" else "shapenet/config_shape.json"
    with open(os.path.join(REPO, "model_configs", name)) as f:
        return json.load(f)


@pytest.mark.parametrize("n_patches", [16384, 300])
def test_patch_plan_densities_equal_the_reference(golden, n_patches):
    shp, n_obj = density_images()
    d = ut.sample_density_per_image(shp, n_obj, n_patches, 0.33, 0.66)
    np.testing.assert_allclose(d, golden[f"density_{n_patches}"], rtol=1e-14, atol=0)


class _Subset:
    def __init__(self, shapes_, centers):
        self.shapes = np.asarray(shapes_, dtype=np.int64)
        self.centers = [np.asarray(c, dtype=np.int64).reshape(-1, 2) for c in centers]
        self.n_objects = np.array([len(c) for c in self.centers])


def test_object_anchors_follow_centre_plus_gaussian():
    sub = _Subset([[2000, 2000]], [[[1000, 700]]])
    pm = {"n_patches": 20000, "unf_sampler_weight": 0.0, "obj_sampler_weight": 1.0, "obj_sampler_sigma": 10}
    plan = ut.make_plan(np.random.default_rng(42), sub, 20000, pm)
    assert plan.shape == (20000, 3) and np.all(plan[:, 0] == 0)
    a = plan[:, 1:].astype(np.float64)
    # normal(centre, 10).astype(int) truncates toward zero: mean centre - ~0.5, spread ~10
    n = len(a)
    np.testing.assert_allclose(a.mean(0), [999.5, 699.5], atol=4 * 10 / np.sqrt(n) + 0.02)
    np.testing.assert_allclose(a.std(0), [10.0, 10.0], rtol=0.03)


def test_uniform_anchors_stay_in_the_image_and_empty_images_fall_back_to_uniform():
    sub = _Subset([[50, 80], [64, 64]], [np.zeros((0, 2)), [[3, 4]]])
    pm = {"n_patches": 500, "unf_sampler_weight": 0.5, "obj_sampler_weight": 0.5, "obj_sampler_sigma": 30}
    plan = ut.make_plan(np.random.default_rng(1), sub, 500, pm)
    assert len(plan) == 500
    for i in (0, 1):
        sel = plan[plan[:, 0] == i]
        assert len(sel) > 0
        assert np.all(sel[:, 1:] >= 0) and np.all(sel[:, 1] <= sub.shapes[i, 0]) and np.all(sel[:, 2] <= sub.shapes[i, 1])


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("flip", range(4))
def test_d4_moves_the_polygon_with_the_object(k, flip):
    rng = np.random.default_rng(10 * k + flip)
    P = 128
    for _ in range(50):
        c = rng.integers(0, P, size=2)
        a, b = rng.uniform(2, 8), rng.uniform(8, 20)
        ang = rng.uniform(0, np.pi)
        poly = shapes.rect_to_poly(c, short=a, long=b, angle=ang)
        want = ut.d4_points(poly, k, flip, P)
        c2 = ut.d4_points(c, k, flip, P)
        ang2 = float(ut.d4_angle(ang, k, flip))
        assert 0.0 <= ang2 < np.pi
        got = shapes.rect_to_poly(c2, short=a, long=b, angle=ang2)
        # the same four corners, possibly in another order
        d = np.abs(got[:, None, :] - want[None, :, :]).sum(-1)
        assert np.all(d.min(axis=1) < 1e-9) and np.all(d.min(axis=0) < 1e-9)


def test_d4_image_matches_the_point_map():
    P = 6
    img = np.arange(P * P).reshape(P, P)
    for k in range(4):
        for flip in range(4):
            t = ut.d4_image(img, k, flip)
            for r in range(P):
                for c in range(P):
                    r2, c2 = ut.d4_points(np.array([r, c]), k, flip, P).astype(int)
                    assert t[r2, c2] == img[r, c]


@pytest.mark.parametrize("kind,path,value", [
    ("posnet", ("loss", "target_mode"), "dist"),
    ("posnet", ("loss", "max_distance"), "auto"),
    ("posnet", ("loss", "focal_loss"), True),
    ("posnet", ("loss", "vec_loss_on_prod"), False),
    ("shapenet", ("loss", "mask_mode"), "gaussian"),
    ("shapenet", ("loss", "focal_loss"), True),
])
def test_unsupported_options_raise_naming_the_key(kind, path, value):
    cfg = copy.deepcopy(shipped(kind))
    ut.check_config(cfg, kind)
    cfg[path[0]][path[1]] = value
    with pytest.raises(NotImplementedError, match=path[1]):
        ut.check_config(cfg, kind)
    with pytest.raises(NotImplementedError, match=path[1]):
        ut.train_unet(cfg, kind, dataset="NONE")


def test_shipped_configs_map_to_the_kernel_options():
    pos, shp = shipped("posnet"), shipped("shapenet")
    lab = ut.labels_struct(pos, "posnet")
    assert lab.kind == 0 and lab.uvec == 1 and lab.max_distance == 8.0 and lab.sigma_dil == 0.6
    lab = ut.labels_struct(shp, "shapenet")
    assert lab.kind == 1 and lab.n_classes == 32 and list(lab.cyclic) == [0, 0, 1]
    assert lab.edges[2][1] == np.pi / 32 and lab.edges[0][31] == 31.0
    assert ut.aug_flags(pos, "posnet") == ut.hip_api.AUG_GEOMETRIC | ut.hip_api.AUG_STRONG
    assert ut.aug_flags(shp, "shapenet") == ut.hip_api.AUG_GEOMETRIC | ut.hip_api.AUG_STRONG | ut.hip_api.AUG_PERTURB


def test_existing_model_directory_needs_overwrite(tmp_path):
    cfg = {"model_name": "m"}
    d = ut.startup(cfg, "posnet", overwrite=False, resume=False, model_base=str(tmp_path))
    assert os.path.exists(os.path.join(d, "config.json"))
    with pytest.raises(FileExistsError):
        ut.startup(cfg, "posnet", overwrite=False, resume=False, model_base=str(tmp_path))
    open(os.path.join(d, "stale.txt"), "w").close()
    ut.startup(cfg, "posnet", overwrite=True, resume=False, model_base=str(tmp_path))
    assert not os.path.exists(os.path.join(d, "stale.txt"))


def test_more_than_one_rank_is_refused(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one GPU"):
        ut.train_unet(shipped("posnet"), "posnet", dataset="NONE")
