"""Host side of the spatial ops of the augmentation recipe (no GPU): the flags, the record restated from the Philox words,
and the NumPy restatement's own ops against cases that can be checked by hand.  The GPU tests
(test_gpu_unet_augment.py) compare the kernels with this restatement, so it is pinned here first."""
import numpy as np
import pytest

from mpp_cnn_rs_object_detection_amd import hip_api
from mpp_cnn_rs_object_detection_amd import unet_training as ut
import unet_augment_ref as R

SPATIAL = hip_api.AUG_SPATIAL


# ---- flags -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["posnet", "shapenet"])
def test_aug_flags_gain_the_spatial_bit_only_when_asked(kind):
    cfg = ut.shipped_config(kind)
    assert SPATIAL == 32
    base = ut.aug_flags(cfg, kind)
    assert not base & SPATIAL and ut.aug_flags(cfg, kind, spatial=False) == base
    assert ut.aug_flags(cfg, kind, spatial=True) == base | SPATIAL
    assert ut.aug_flags(cfg, kind, histograms=True, spatial=True) == ut.aug_flags(cfg, kind, histograms=True) | SPATIAL
    assert base & hip_api.AUG_STRONG                                   # both shipped configs say "strong"
    cfg["data_loader"]["augment_params"]["aug_level"] = "medium"
    assert ut.aug_flags(cfg, kind, spatial=True) & (SPATIAL | hip_api.AUG_MEDIUM) == SPATIAL | hip_api.AUG_MEDIUM
    del cfg["data_loader"]["augment_params"]
    assert not ut.aug_flags(cfg, kind, histograms=True, spatial=True) & SPATIAL


def test_record_dtype_matches_the_header():
    d = hip_api.AUG_RECORD_DTYPE
    assert hip_api.AUG_MAX_HAZE == R.MAX_HAZE == 64
    assert d.itemsize == 16 * 4 + 6 * 4 + 4 * 8 + 2 * 5 * 2 * 2 + 64 * 2 * 2 and d.itemsize % 8 == 0
    assert d.fields["sigma"][1] == 88 and d.fields["poly"][1] == 120 and d.fields["haze"][1] == 160


# ---- Philox and the record ------------------------------------------------------------------------------------------------
def test_numpy_philox_equals_the_library():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, size=(200, 4), dtype=np.uint64)
    ctr[0] = 0
    ctr[1] = 2 ** 32 - 1
    for key in ((0, 0), (11, 2), (2 ** 32 - 1, 12345)):
        got = R.philox_many(ctr, key)
        for c, g in zip(ctr, got):
            assert np.array_equal(g, hip_api.philox(c, key))


def test_aug_params_host_is_a_function_of_its_key():
    flags = R.pool_flags("strong")
    a = R.aug_params_host(flags, 11, 2, 3, 32, 128, 5)
    assert a.tobytes() == R.aug_params_host(flags, 11, 2, 3, 32, 128, 5).tobytes()
    for other in ((12, 2, 3), (11, 3, 3), (11, 2, 4)):
        assert a.tobytes() != R.aug_params_host(flags, *other, 32, 128, 5).tobytes()
    assert a[:16].tobytes() == R.aug_params_host(flags, 11, 2, 3, 16, 128, 5).tobytes()       # patch b does not depend on B
    assert len({a[b].tobytes() for b in range(32)}) == 32                                      # ... but on b
    assert a.tobytes() != R.aug_params_host(flags, 11, 2, 3, 32, 64, 5).tobytes()              # vertices scale with P
    assert a.tobytes() != R.aug_params_host(flags, 11, 2, 3, 32, 128, 7).tobytes()             # the template draw
    # without the flag no record selects one of the six, and the other draws are the same
    plain = R.aug_params_host(flags & ~SPATIAL, 11, 2, 3, 32, 128, 5)
    assert not any(R.selects(r) for r in plain)
    for k in ("rot", "flip", "chan_op", "chan_arg", "bc", "color", "noise", "hm", "tmpl", "alpha", "beta", "shift", "sigma", "blend"):
        assert np.array_equal(plain[k], a[k]), k
    # medium never draws the strong-only ops
    med = R.aug_params_host(R.pool_flags("medium"), 11, 2, 3, 256, 128, 5)
    assert not (med["shadow"] | med["fog"] | med["downscale"] | med["chan_op"] | med["bc"]).any() and med["clahe"].any()
    for b, r in enumerate(a):
        # CLAHE is the draw that used to pick "CLAHE, not built": the colour OneOf fired and chose its first member
        u = R._draw(11, 2, 3, b, 0, 2)
        assert bool(r["clahe"]) == bool(u[2] < 0.5 and u[3] * 1.1 < 0.5)
        assert 1.0 <= r["clip"] <= 4.0 and 0.3 <= r["fog_coef"] <= 1.0
        for k in range(int(r["n_poly"])):
            assert (r["poly"][k, :, 0] >= 0).all() and (r["poly"][k, :, 0] <= 128).all()
            assert (r["poly"][k, :, 1] >= 64).all() and (r["poly"][k, :, 1] <= 128).all()


def test_haze_loop_never_exceeds_the_kernels_cap():
    worst = 0
    for P in range(32, 513, 8):
        for coef in np.linspace(0.3, 1.0, 71):
            rounds, hw = R.haze_plan(P, float(coef))
            n = sum(c for c, _, _ in rounds)
            assert n == R.haze_count(P, hw)
            worst = max(worst, n)
            for _, midx, midy in rounds:                              # randint's ranges are never empty
                assert midx <= P - midx - hw and midy <= P - midy - hw
        # the count depends on (P, hw) alone, and fog_coef in [0.3, 1] gives the integers hw = max(1, int(P // 3 * coef)):
        # every case there is
        lo = max(1, int(P // 3 * 0.3))
        worst = max(worst, max(R.haze_count(P, hw) for hw in range(lo, P // 3 + 1)))
    assert worst == 51 and worst <= hip_api.AUG_MAX_HAZE
    assert sum(c for c, _, _ in R.haze_plan(128, 0.3)[0]) == 10       # rounds of 1, 2, 3, 4 (hw 12)
    assert sum(c for c, _, _ in R.haze_plan(128, 0.999)[0]) == 12     # rounds of 4 and 8 (hw 41)


# ---- CLAHE -----------------------------------------------------------------------------------------------------------------
def scalar_clip(hist, limit):
    """the clip / redistribute step as a scalar loop (OpenCV's CLAHE_CalcLut_Body)"""
    h = [int(v) for v in hist]
    clipped = 0
    for i in range(256):
        if h[i] > limit:
            clipped += h[i] - limit
            h[i] = limit
    batch, residual = clipped // 256, clipped % 256
    for i in range(256):
        h[i] += batch
    if residual:
        step = max(256 // residual, 1)
        i = 0
        while i < 256 and residual > 0:
            h[i] += 1
            i += step
            residual -= 1
    return np.array(h), clipped


def test_clahe_clip_equals_the_scalar_loop():
    rng = np.random.default_rng(1)
    for case in range(300):
        area = int(rng.choice([64, 256, 1024, 4096]))
        spread = int(rng.choice([1, 3, 20, 256]))
        hist = np.bincount(rng.integers(0, spread, size=area) * (256 // spread) % 256, minlength=256)
        limit = max(1, int(rng.uniform(1, 4) * area / 256))
        want, clipped = scalar_clip(hist, limit)
        got = R.clahe_clip(hist, limit)
        assert np.array_equal(got, want), case
        assert got.sum() == area                                       # the bin sum is preserved
        assert got.max() <= limit + clipped // 256 + 1


def test_clahe_of_one_value_per_tile_is_that_values_lut_entry():
    # every tile holds one value v: hist[v] = area.  clip 1, P 128: area 256, limit 1, excess 255 -> +0 to every bin and +1
    # to bins 0, 1, ..., 254 (step 1): bin v has 2 (v < 255), the others 1 except bin 255 with 0;
    # cumsum[v] = (v + 1) + 1, lut[v] = rint((v + 2) * 255 / 256)
    P, ts = 128, 16
    rng = np.random.default_rng(2)
    vals = rng.integers(0, 255, size=(8, 8))
    L8 = np.repeat(np.repeat(vals, ts, 0), ts, 1)
    lut1 = np.rint((vals + 2) * 255.0 / 256.0)
    # clip 4: limit 4, excess 252 -> bins 0 .. 251 get +1 (step 1); cumsum[v] = min(v + 1, 252) + 4
    lut4 = np.rint((np.minimum(vals + 1, 252) + 4) * 255.0 / 256.0)
    for clip, lut in ((1.0, lut1), (4.0, lut4)):
        assert int(R.clahe_lut(np.bincount([int(vals[0, 0])] * 256, minlength=256), clip, 256)[vals[0, 0]]) == lut[0, 0]
        got = R.clahe_l8(L8, clip)
        # at a tile's centre rows / columns the blend weights are 1/32-steps; the pixel nearest the centre of tile (ty, tx)
        # mixes its own table 31/32 : 1/32 per axis, so compare where all four tables agree: patches of one value
        flat = R.clahe_l8(np.full((P, P), int(vals[3, 3])), clip)
        assert np.allclose(flat, lut[3, 3], rtol=0, atol=1e-12)
        # the corners of the patch read one tile only (both indices clamp)
        assert got[0, 0] == lut[0, 0] and got[P - 1, P - 1] == lut[7, 7] and got[0, P - 1] == lut[0, 7]
        # between the centres of tiles (0, 0) and (0, 1), on row 0: a linear ramp of their entries for value vals[0, 0]
        j = np.arange(ts // 2, ts)
        xa = j / ts - 0.5
        l_own = lut[0, 0]
        l_next = R.clahe_lut(np.bincount([int(vals[0, 1])] * 256, minlength=256), clip, 256)[vals[0, 0]]
        assert np.allclose(got[0, j], l_own * (1 - xa) + l_next * xa, rtol=0, atol=1e-12)


def test_lab_and_hls_round_trips():
    rng = np.random.default_rng(3)
    x = rng.uniform(0, 255, size=(5000, 3))
    x[:256] = np.arange(256)[:, None]                                  # the grays
    back = R.lab_to_rgb(R.rgb_to_lab(x))
    # OpenCV's two matrices are inverses to 6 digits: 1e-5 of linear light, times 255, times the gamma's slope of 12.92
    # at the dark end
    assert np.abs(back - x).max() < 1e-5 * 255 * 12.92
    lab = R.rgb_to_lab(np.array([[255.0, 255.0, 255.0], [0.0, 0.0, 0.0]]))
    assert abs(lab[0, 0] - 100.0) < 1e-3 and abs(lab[0, 1]) < 1e-2 and abs(lab[0, 2]) < 1e-2 and np.all(lab[1] == 0)
    s = R.shadow_rgb(x)
    assert np.allclose(s.max(-1) + s.min(-1), (x.max(-1) + x.min(-1)) / 2, rtol=0, atol=1e-9)    # L halves
    assert np.array_equal(np.argsort(s, -1, kind="stable")[256:], np.argsort(x, -1, kind="stable")[256:])   # the hue's order stays
    assert np.allclose(R.shadow_rgb(np.array([[200.0, 200.0, 200.0]])), 100.0)
    assert np.allclose(R.shadow_rgb(np.array([[255.0, 0.0, 0.0]])), [[127.5, 0.0, 0.0]])       # S stays 1


# ---- downscale, fog, blur --------------------------------------------------------------------------------------------------
def test_downscale_map_at_the_shipped_patch_size():
    m = R.down_map(128)
    assert len(np.unique(m)) == 115 and m.max() == 126 and m[0] == 0 and (np.diff(m) >= 0).all()
    assert (R.down_map(64) <= 63).all() and len(np.unique(R.down_map(64))) == 58


def test_fog_closed_form_equals_the_sequential_blend():
    rng = np.random.default_rng(4)
    P, coef = 128, 0.73
    haze = np.stack([rng.integers(-40, 150, size=12), rng.integers(-10, 120, size=12)], 1)
    hw2 = max(int(P // 3 * coef), 10)
    x = rng.uniform(0, 255, size=(P, P, 3))
    seq = x.copy()
    yy, xx = np.mgrid[:P, :P]
    alpha, rad = 0.08 * coef, hw2 // 2
    for hx, hy in haze:
        disc = (xx - (hx + rad)) ** 2 + (yy - (hy + rad)) ** 2 <= rad * rad
        seq[disc] = alpha * 255.0 + (1 - alpha) * seq[disc]
    k = R.fog_counts(P, haze, hw2)
    assert k.max() >= 2
    closed = 255.0 - (255.0 - x) * ((1 - alpha) ** k)[..., None]
    assert np.abs(closed - seq).max() < 1e-10
    assert hw2 // 10 == 3
    assert np.abs(R.fog(x, P, coef, haze) - R.box_mean(closed, 3)).max() < 1e-10


def test_box_median_and_blur_borders():
    x = np.arange(25, dtype=np.float64).reshape(5, 5, 1).repeat(3, -1)
    b = R.box_mean(x, 3)
    assert b[2, 2, 0] == 12 and b[0, 0, 0] == np.mean([6, 5, 6, 1, 0, 1, 6, 5, 6])             # REFLECT_101: row -1 is row 1
    b2 = R.box_mean(x, 2)                                                                      # anchor 1: rows i - 1, i
    assert b2[1, 1, 0] == np.mean([0, 1, 5, 6]) and b2[0, 0, 0] == np.mean([6, 5, 1, 0])
    m = R.median3(x)
    assert m[2, 2, 0] == 12 and m[0, 0, 0] == np.median([0, 0, 1, 0, 0, 1, 5, 5, 6])           # REPLICATE
    flat = np.full((16, 16, 3), 90.0)
    flat[4, 4] = 255.0
    flat[9, 12] = 0.0
    assert np.all(R.median3(flat) == 90.0)
    assert np.allclose(R.blur3(np.full((8, 8, 3), 77.0)), 77.0, rtol=0, atol=1e-12)


# ---- the inputs of the GPU comparison stay under the issue's caps, on the restatement alone --------------------------------
def test_the_gpu_tests_inputs_stay_under_the_exemption_caps():
    imgs = R.test_images()
    only, only_out = {}, {}
    for level, P, batches in R.POOLS:
        pool = R.restate_pool(level, P, batches, imgs)
        out = sum(1 for p in pool if p[5] > R.CLAHE_FLIP_CAP)
        assert out <= R.LEFT_OUT_SHARE * len(pool), (level, P, out)
        for _, _, rec, x, _, n_flip in pool:
            assert np.isfinite(x).all() and x.min() >= 0 and x.max() <= 1
            s = R.selects(rec)
            key = s[0] if len(s) == 1 else ("none" if not s else None)
            if key:
                only[key] = only.get(key, 0) + 1
                only_out[key] = only_out.get(key, 0) + (n_flip > R.CLAHE_FLIP_CAP)
    assert only["none"] >= 5
    for op in ("shadow", "fog", "clahe", "downscale", "median", "blur"):
        assert only[op] >= 8, (op, only)
        assert only_out[op] <= R.LEFT_OUT_SHARE * only[op], (op, only_out[op], only[op])
