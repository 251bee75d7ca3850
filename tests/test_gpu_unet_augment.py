"""The spatial ops of the augmentation recipe on the GPU (MPP_AUG_SPATIAL: shadow, fog, CLAHE, downscale, median / box
blur): mpp_train_aug_params against the record restated from the Philox words, mpp_train_batch against the float64 NumPy
restatement of the whole image pipeline (tests/unet_augment_ref.py, pinned by test_unet_augment_host.py) and against
properties that do not lean on it, and train_unet with the shipped strong recipe.

Tolerance of the comparison with the restatement, on the [0, 1] patch: measured on one MI355X over every compared pixel of
the pools below (1 152 patches, P = 128 and 64, strong and medium), the largest |device - restatement| is 2.93e-7
(per op alone: shadow 1.33e-7, fog 2.55e-7, CLAHE 1.24e-7, downscale 1.02e-7, median 9.68e-8, blur 1.82e-7).  That is the
float32 roundings between the ops and of the final value / 255 (half an ulp of a value below 1 is 6e-8, a handful of
them); the kernel forms the colour-space round trips in float64 and rounds once.  TOL = 4 x that maximum, for inputs
that are not in the test.  Of 108 CLAHE-only patches 11 are left out by the bin-flip cap (the random-byte image's, and
posterized ones whose few colours happen to sit on a bin edge).  The median takes no exemption here: a median of nine is
1-Lipschitz in its inputs, so a float32 rounding upstream moves it by no more than that rounding, near ties included."""
import json
import os

import numpy as np
import pytest

from mpp_cnn_rs_object_detection_amd import hip_api
from mpp_cnn_rs_object_detection_amd import unet_training as ut
from test_gpu_unet_training import POS_CFG, SHP_CFG, run_main, tiny_config, write_dataset
import unet_augment_ref as R

pytestmark = pytest.mark.gpu
SPATIAL = hip_api.AUG_SPATIAL
MEASURED_MAX = 2.93e-7           # see the module docstring
TOL = 4 * MEASURED_MAX
OPS = ("shadow", "fog", "clahe", "downscale", "median", "blur")


@pytest.fixture(scope="module")
def mctx():
    import torch
    c = hip_api.MppContext(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def npy(t):
    return t.cpu().numpy()


def desc_of(rows):
    import torch
    return torch.tensor(np.asarray(rows, dtype=np.int32).reshape(-1, 3), device="cuda")


def resident(imgs):
    n = len(imgs)
    return ut.ResidentSubset.from_arrays(imgs, [np.zeros((0, 2))] * n, [np.zeros((0, 3))] * n, 0)


@pytest.fixture(scope="module")
def pools(mctx):
    """per pool of R.POOLS: the device's records, its patches with the flag set and clear, and the restatement"""
    imgs = R.test_images()
    data = resident(imgs)
    out = {}
    for level, P, batches in R.POOLS:
        builder = ut.BatchBuilder(mctx, ut.labels_struct(POS_CFG, "posnet"), P, 0)
        flags = R.pool_flags(level)
        recs, got, plain = [], [], []
        for batch in range(batches):
            desc = desc_of(R.pool_rows(level, P, batch, imgs))
            recs.append(ut.aug_params(mctx, flags, R.SEED, R.EPOCH, batch, R.B, P, len(imgs)))
            got.append(npy(builder.build(data, desc, flags, R.SEED, R.EPOCH, batch, fresh=True)["patch"]))
            plain.append(npy(builder.build(data, desc, flags & ~SPATIAL, R.SEED, R.EPOCH, batch, fresh=True)["patch"]))
        builder.check()
        out[(level, P)] = {"recs": recs, "got": got, "plain": plain, "ref": R.restate_pool(level, P, batches, imgs)}
    return out


# ---- the record ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", ["strong", "medium"])
def test_aug_params_equal_the_host_restatement(mctx, level):
    for P, n_images in ((128, 4), (64, 7), (512, 3)):
        flags = R.pool_flags(level)
        for batch in (0, 5):
            got = ut.aug_params(mctx, flags, R.SEED, R.EPOCH, batch, R.B, P, n_images)
            want = R.aug_params_host(flags, R.SEED, R.EPOCH, batch, R.B, P, n_images)
            assert got.dtype == hip_api.AUG_RECORD_DTYPE and got.shape == (R.B,)
            for name in hip_api.AUG_RECORD_DTYPE.names:
                assert np.array_equal(got[name], want[name]), (P, batch, name)
    # without the flag the same call gives the same other draws and none of the six
    a = ut.aug_params(mctx, R.pool_flags(level, spatial=False), R.SEED, R.EPOCH, 0, R.B, 128, 4)
    b = R.aug_params_host(R.pool_flags(level, spatial=False), R.SEED, R.EPOCH, 0, R.B, 128, 4)
    for name in hip_api.AUG_RECORD_DTYPE.names:
        assert np.array_equal(a[name], b[name]), name
    assert not any(R.selects(r) for r in a)


def test_pool_records_equal_the_hosts(pools):
    for (level, P), pool in pools.items():
        host = {(batch, b): rec for batch, b, rec, _, _, _ in pool["ref"]}
        for batch, recs in enumerate(pool["recs"]):
            for b in range(R.B):
                assert recs[b].tobytes() == host[(batch, b)].tobytes(), (level, P, batch, b)


# ---- flag set, nothing drawn -----------------------------------------------------------------------------------------------
def test_patches_that_draw_none_of_the_six_are_the_flag_clear_patches(pools):
    n = 0
    for (level, P), pool in pools.items():
        for batch, recs in enumerate(pool["recs"]):
            for b in range(R.B):
                if not R.selects(recs[b]):
                    n += 1
    assert n >= 5
    for (level, P), pool in pools.items():
        changed = 0
        for batch, recs in enumerate(pool["recs"]):
            for b in range(R.B):
                same = np.array_equal(pool["got"][batch][b], pool["plain"][batch][b])
                if not R.selects(recs[b]):
                    assert same, (level, P, batch, b)
                changed += not same
        assert changed > R.B // 4, (level, P, changed)                   # ... and the flag does something


# ---- against the restatement -----------------------------------------------------------------------------------------------
def compare(pool, want_ops=None):
    """[(ops, error over the compared pixels or None if the patch is left out, exempted share)] of a pool's patches"""
    res = []
    for batch, b, rec, want, exempt, n_flip in pool["ref"]:
        ops = R.selects(rec)
        if want_ops is not None and ops != want_ops:
            continue
        if n_flip > R.CLAHE_FLIP_CAP:
            res.append((ops, None, 1.0))
            continue
        err = np.abs(pool["got"][batch][b].astype(np.float64) - want).max(0)
        res.append((ops, float(err[~exempt].max()) if (~exempt).any() else 0.0, float(exempt.mean())))
    return res


@pytest.mark.parametrize("op", OPS)
def test_each_op_alone_equals_the_restatement(pools, op):
    res = []
    for pool in pools.values():
        res += compare(pool, (op,))
    kept = [e for _, e, _ in res if e is not None]
    print(f"{op} alone: {len(res)} patches, {len(res) - len(kept)} left out, max error {max(kept):.3g}, "
          f"largest exempted share of a compared patch {max(s for _, e, s in res if e is not None):.3f}")
    assert len(res) >= 8
    assert len(res) - len(kept) <= R.LEFT_OUT_SHARE * len(res)
    assert max(kept) <= TOL


def test_every_patch_equals_the_restatement(pools):
    worst = 0.0
    for (level, P), pool in pools.items():
        res = compare(pool)
        kept = [e for _, e, _ in res if e is not None]
        combos = len({ops for ops, _, _ in res})
        print(f"{level} P={P}: {len(res)} patches, {combos} combinations of ops, {len(res) - len(kept)} left out, "
              f"max error {max(kept):.3g}")
        worst = max(worst, max(kept))
        assert len(res) == len(pool["recs"]) * R.B
        assert len(res) - len(kept) <= R.LEFT_OUT_SHARE * len(res), (level, P)
        bad = [(ops, e) for ops, e, _ in res if e is not None and e > TOL]
        assert not bad, (level, P, bad[:5])
    print(f"measured maximum over all pools: {worst:.3g} (MEASURED_MAX {MEASURED_MAX:.3g}, TOL {TOL:.3g})")
    assert worst <= 1e-4                                                  # anything above is a bug, not a tolerance


# ---- structure that does not lean on the restatement -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(mctx):
    """40 strong batches at P = 128 and 64 from the scenes (no restatement): records, flag-set and flag-clear patches of the
    patches that draw exactly one of the six ops"""
    imgs = R.test_images()
    data = resident(imgs)
    out = []
    for P in (128, 64):
        builder = ut.BatchBuilder(mctx, ut.labels_struct(POS_CFG, "posnet"), P, 0)
        flags = R.pool_flags("strong")
        for batch in range(100, 140):
            rec = ut.aug_params(mctx, flags, R.SEED, R.EPOCH, batch, R.B, P, len(imgs))
            pick = [b for b in range(R.B) if len(R.selects(rec[b])) == 1]
            desc = desc_of(R.pool_rows("strong", P, batch, imgs))
            got = npy(builder.build(data, desc, flags, R.SEED, R.EPOCH, batch, fresh=True)["patch"])
            plain = npy(builder.build(data, desc, flags & ~SPATIAL, R.SEED, R.EPOCH, batch, fresh=True)["patch"])
            for b in pick:
                out.append((P, rec[b].copy(), got[b].astype(np.float64) * 255, plain[b].astype(np.float64) * 255))
    return out


def pointwise_free(rec):
    """no op after the spatial ones changes a value: no channel op, brightness / contrast, colour op or noise"""
    return not (rec["chan_op"] or rec["bc"] or rec["color"] or rec["clahe"] or rec["noise"])


def test_downscale_alone_is_an_exact_gather(many):
    n = 0
    for P, rec, got, plain in many:
        if R.selects(rec) == ("downscale",) and not rec["noise"]:         # (the noise is drawn per output pixel)
            m = R.down_map(P)
            assert np.array_equal(got, plain[:, m][:, :, m])
            n += 1
    assert n >= 8


def test_shadow_alone_halves_the_lightness_below_the_middle(many):
    n = changed = 0
    for P, rec, got, plain in many:
        if R.selects(rec) != ("shadow",):
            continue
        assert np.array_equal(got[:, :P // 2], plain[:, :P // 2])
        if pointwise_free(rec):
            diff = (got != plain).any(0)
            light = lambda x: x.max(0) + x.min(0)                          # noqa: E731
            assert np.abs(light(got)[diff] - light(plain)[diff] / 2).max(initial=0) <= 1e-4 * 255
            n += 1
            changed += int(diff.sum())
    assert n >= 4 and changed > 1000


def test_fog_alone_brightens_by_an_integer_number_of_discs(many):
    n = exact = covered = 0
    for P, rec, got, plain in many:
        if R.selects(rec) != ("fog",) or max(int(P // 3 * rec["fog_coef"]), 10) // 10 > 1:
            continue
        n += 1
        if rec["chan_op"] != 2:                                            # (a dropped channel is 0 with and without fog)
            assert (got >= plain).all()                                    # every later op is monotone
        if pointwise_free(rec):
            keep = 1.0 - 0.08 * float(rec["fog_coef"])
            k = np.arange(int(rec["n_haze"]) + 1)
            want = 255.0 - (255.0 - plain[..., None]) * keep ** k         # [3, P, P, n_haze + 1]
            err = np.abs(want - got[..., None])
            best = err.max(0).argmin(-1)                                   # one k per pixel for its three channels
            assert np.take_along_axis(err.max(0), best[..., None], -1).max() <= 1e-4 * 255
            covered += int(best.max() >= 1)
            exact += 1
    assert n >= 8 and exact >= 2 and covered >= 1


@pytest.fixture(scope="module")
def special(mctx):
    """medium batches from an image of single-pixel impulses on a flat ground and from a constant image, anchors such that
    the crops lie inside"""
    rng = np.random.default_rng(5)
    ground = np.empty((256, 256, 3), np.uint8)
    ground[:] = (90, 140, 60)
    imp = ground.copy()
    for r in range(3, 256, 5):
        for c in range(2 + r % 3, 256, 4):                                 # isolated: at least 3 apart in both directions
            imp[r, c] = rng.choice([0, 255], size=3)
    data = resident([imp, ground])
    P = 64
    builder = ut.BatchBuilder(mctx, ut.labels_struct(POS_CFG, "posnet"), P, 0)
    flags = R.pool_flags("medium")
    out = []
    for batch in range(200, 212):
        rows = [(b % 2, int(rng.integers(P // 2, 256 - P // 2)), int(rng.integers(P // 2, 256 - P // 2))) for b in range(R.B)]
        rec = ut.aug_params(mctx, flags, R.SEED, R.EPOCH, batch, R.B, P, 2)
        got = npy(builder.build(data, desc_of(rows), flags, R.SEED, R.EPOCH, batch, fresh=True)["patch"])
        plain = npy(builder.build(data, desc_of(rows), flags & ~SPATIAL, R.SEED, R.EPOCH, batch, fresh=True)["patch"])
        out += [(rows[b][0], rec[b].copy(), got[b], plain[b]) for b in range(R.B)]
    return out


def test_median_alone_removes_isolated_impulses(special):
    n = 0
    for img, rec, got, plain in special:
        if img == 0 and R.selects(rec) == ("median",) and not rec["noise"]:
            assert len(np.unique(plain.reshape(3, -1), axis=1).T) > 1      # the impulses are in the flag-clear patch
            for ch in range(3):
                assert len(np.unique(got[ch])) == 1
                values, counts = np.unique(plain[ch], return_counts=True)
                assert got[ch, 0, 0] == values[counts.argmax()]            # ... and the ground is what is left
            n += 1
    assert n >= 4


def test_blur_alone_leaves_a_constant_image_alone(special):
    n = 0
    for img, rec, got, plain in special:
        if img == 1 and R.selects(rec) == ("blur",) and not rec["noise"]:
            # nine equal float32 values summed and divided by 9: a few roundings of a value <= 255
            assert np.abs(got.astype(np.float64) - plain).max() <= 1e-6
            n += 1
    assert n >= 4


# ---- frequencies -----------------------------------------------------------------------------------------------------------
def test_frequencies_of_the_draws(mctx):
    def within(x, p, n):
        return abs(x - p) <= 4 * np.sqrt(p * (1 - p) / n)
    for level, want in (("strong", {"shadow": 0.5, "fog": 0.5, "clahe": 0.5 * 0.5 / 1.1, "downscale": 0.5, "median": 0.1, "blur": 0.1}),
                        ("medium", {"shadow": 0.0, "fog": 0.0, "clahe": 0.25, "downscale": 0.0, "median": 0.1, "blur": 0.1})):
        rec = np.concatenate([ut.aug_params(mctx, R.pool_flags(level), R.SEED, R.EPOCH, batch, 1024, 128, 4) for batch in range(8)])
        n = len(rec)
        assert n >= 8192
        freq = {"shadow": rec["shadow"].mean(), "fog": rec["fog"].mean(), "clahe": rec["clahe"].mean(),
                "downscale": rec["downscale"].mean(), "median": (rec["blur"] == 1).mean(), "blur": (rec["blur"] == 2).mean()}
        print(level, {k: round(float(v), 4) for k, v in freq.items()})
        for k, p in want.items():
            assert within(freq[k], p, n), (level, k, freq[k], p)
        assert abs(rec["clip"].mean() - 2.5) <= 4 * (3 / np.sqrt(12)) / np.sqrt(n)
        if level == "strong":
            assert abs(rec["fog_coef"].mean() - 0.65) <= 4 * (0.7 / np.sqrt(12)) / np.sqrt(n)
            two = (rec["n_poly"][rec["shadow"] == 1] == 2).mean()
            assert within(two, 0.5, int(rec["shadow"].sum()))
            # the haze points lie in the last round's window at the least; the vertices in the lower half
            sh = rec[rec["shadow"] == 1]
            assert sh["poly"][:, 0, :, 1].min() == 64 and sh["poly"][:, 0, :, 1].max() == 128
            assert sh["poly"][:, 0, :, 0].min() == 0 and sh["poly"][:, 0, :, 0].max() == 128


# ---- labels, determinism, errors -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["posnet", "shapenet"])
def test_labels_do_not_move_and_the_same_key_gives_the_same_bits(mctx, kind):
    from test_gpu_unet_resampling import scene
    sc = [scene((128, 128), 80, 5), scene((96, 160), 70, 6)]
    data = ut.ResidentSubset.from_arrays([s[0] for s in sc], [s[1] for s in sc], [s[2] for s in sc], 0)
    P, B, seed, epoch, batch = 64, 96, 21, 1, 2
    rng = np.random.default_rng(8)
    rows = [(i, int(rng.integers(0, sc[i][0].shape[0] + 1)), int(rng.integers(0, sc[i][0].shape[1] + 1)))
            for i in rng.integers(0, 2, size=B)]
    flags = hip_api.AUG_GEOMETRIC | hip_api.AUG_STRONG | hip_api.AUG_HISTMATCH | (hip_api.AUG_PERTURB if kind == "shapenet" else 0)
    builder = ut.BatchBuilder(mctx, ut.labels_struct(POS_CFG if kind == "posnet" else SHP_CFG, kind), P, 0, with_dist=kind == "posnet")
    a = {k: npy(v) for k, v in builder.build(data, desc_of(rows), flags, seed, epoch, batch, fresh=True).items()}
    b = {k: npy(v) for k, v in builder.build(data, desc_of(rows), flags | SPATIAL, seed, epoch, batch, fresh=True).items()}
    c = {k: npy(v) for k, v in builder.build(data, desc_of(rows), flags | SPATIAL, seed, epoch, batch, fresh=True).items()}
    assert set(a) == set(b) and len(a) >= 4
    for k in a:
        if k != "patch":
            assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(b[k], c[k]), k
    assert not np.array_equal(a["patch"], b["patch"])
    builder.check()


def test_a_patch_size_off_the_tile_grid_is_an_error(mctx):
    from test_gpu_unet_resampling import scene
    img = scene((160, 160), 30, 1)
    data = ut.ResidentSubset.from_arrays([img[0]], [img[1]], [img[2]], 0)
    flags = hip_api.AUG_GEOMETRIC | hip_api.AUG_STRONG
    for P in (100, 24):
        builder = ut.BatchBuilder(mctx, ut.labels_struct(POS_CFG, "posnet"), P, 0)
        out = dict(builder.buffers(2))
        out["status"] = builder.status
        desc = desc_of([(0, 50, 50), (0, 80, 90)])
        with pytest.raises(hip_api.MppError, match="MPP_AUG_SPATIAL"):
            mctx.train_batch(data.struct, builder.labels, desc, P, flags | SPATIAL, 1, 0, 0, out)
        with pytest.raises(hip_api.MppError, match="MPP_AUG_SPATIAL"):
            ut.aug_params(mctx, flags | SPATIAL, 1, 0, 0, 2, P, 1)
        # the context still builds: the same patch size without the flag, then a valid size with it
        plain = npy(builder.build(data, desc, flags, 1, 0, 0, fresh=True)["patch"])
        assert np.isfinite(plain).all() and plain.max() > 0
    builder = ut.BatchBuilder(mctx, ut.labels_struct(POS_CFG, "posnet"), 96, 0)
    ok = npy(builder.build(data, desc_of([(0, 50, 50), (0, 80, 90)]), flags | SPATIAL, 1, 0, 0, fresh=True)["patch"])
    assert np.isfinite(ok).all() and ok.min() >= 0 and ok.max() <= 1 and ok.max() > 0


# ---- the trainer -----------------------------------------------------------------------------------------------------------
def test_training_runs_with_the_whole_strong_recipe(tmp_path, monkeypatch):
    write_dataset(tmp_path)
    cfg = tiny_config("posnet", n_epochs=2, n_patches=256)
    assert cfg["data_loader"]["augment_params"]["aug_level"] == "strong"
    path = tmp_path / "cfg.json"
    with open(path, "w") as f:
        json.dump(cfg, f)
    r = run_main(tmp_path, ["-p", "train", "-m", "posnet", "-c", str(path), "-d", "SYNTH"], timeout=300)   # its own time limit
    assert r.returncode == 0, r.stderr[-3000:]
    d = tmp_path / "models_storage" / "posnet" / cfg["model_name"]
    log = json.load(open(d / "log.json"))
    assert log["epoch"] == [0, 1] and np.isfinite(log["train_loss"]).all() and np.isfinite(log["val_loss"]).all()
    assert (d / "model.pt").exists()

    # the trainer's first training batch carries the flag (stopped there)
    class Seen(Exception):
        pass

    def spy(self, data, desc, flags, *args, **kw):
        raise Seen(flags)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(ut.BatchBuilder, "build", spy)
    cfg["model_name"] = "second"
    with pytest.raises(Seen) as e:
        ut.train_unet(cfg, "posnet", dataset="SYNTH", model_base=str(tmp_path / "models_storage"))
    assert e.value.args[0] & SPATIAL and e.value.args[0] & hip_api.AUG_HISTMATCH
