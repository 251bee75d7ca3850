"""Restarts on the GPU: R independent chains per tile, the one whose returned state has the lowest total energy is kept.

* ``mpp_total_energy_all`` gives every chain's ``mpp_total_energy`` bit for bit (scan and candidate grids, hand-set and
  sampled states, chains in LDS and in device memory);
* the replicas are the plain chains of their (seed, chain id) keys, the winner is ``select_replicas`` of their energies,
  and replica 0 is the chain a launch without restarts runs;
* ``MPPModel`` hands the winners, and only them, to the merge; the dataset path gives what the image path gives.

Small on purpose: 64-px tiles, a few thousand steps, at most a dozen workgroups per launch."""
import json
import os

import numpy as np
import pytest

from helpers import REPO, log_model
from test_gpu_pipeline import image_data
from mpp_cnn_rs_object_detection_amd import energies as E
from mpp_cnn_rs_object_detection_amd import hip_api, kernels, mappings, synth
from mpp_cnn_rs_object_detection_amd.custom_types import ImageWMaps
from mpp_cnn_rs_object_detection_amd.sampler import (TileBatchSampler, replica_chain_ids, resolve_schedule,
                                                      sample_rjmcmc_batch, select_replicas)
from mpp_cnn_rs_object_detection_amd.shapes import Rectangle

pytestmark = pytest.mark.gpu

TILE = 64


# ---- 1. the batched energy call ---------------------------------------------------------------------------------------

MAPS, REPLICAS = 3, 4
COUNTS = [0, 1, 5, 90, 17, 33, 64, 15, 16, 48, 7, 81]          # chain 0 empty, chain 1 one point; 15 / 16: around the grid's threshold


def map_tiles():
    return [synth.make_tile(TILE, 16, tile_id=70 + k, noise=0.1) for k in range(MAPS)]


def hand_set_points(chain, tile):
    """the tile's objects first (they outlive the steps of the second half), then rectangles at random"""
    rng = np.random.default_rng([41, chain])
    n = COUNTS[chain]
    pix = rng.permutation(TILE * TILE)[:n]
    xy = np.stack([pix // TILE, pix % TILE], axis=1).astype(np.int32)
    marks = np.stack([rng.uniform(4.0, 9.0, n), rng.uniform(0.3, 0.9, n), rng.uniform(0.0, np.pi, n)], axis=1)
    k = min(n, len(tile.gt_xy))
    xy[:k], marks[:k] = tile.gt_xy[:k], tile.gt_marks[:k]
    return xy, marks


def energy_context(**options):
    setup, comb = log_model()
    unit, pair = setup.make_energies()
    tiles = map_tiles()
    ctx = hip_api.MppContext(0, point_capacity=256, spec_waves=8, replicas=REPLICAS, **options)
    ctx.set_maps(np.stack([t.det for t in tiles]), [np.stack([t.marks[k] for t in tiles]) for k in range(3)])
    ctx.set_model(E.build_model_desc(unit, pair, comb), mappings.default_mappings())
    assert ctx.get_option("n_chains") == MAPS * REPLICAS == len(COUNTS)
    for c in range(len(COUNTS)):
        ctx.set_points(c, *hand_set_points(c, tiles[c % MAPS]))
    ctx.set_kernels(kernels.make_kernels(mappings.default_mappings(), 1.0), intensity=np.maximum(1.0, COUNTS))
    ctx.set_schedule(0.05, 0.999, 0.0)           # (cold: the chains keep the objects and shed the random rectangles)
    return ctx


def assert_all_equals_each(ctx, what, grid_mins=(0, 16)):
    for grid_min in grid_mins:                                  # the scan; candidate grids from 16 points on
        ctx.set_option("scratch_grid_min_points", grid_min)
        each = np.array([ctx.total_energy(t) for t in range(ctx.get_option("n_chains"))])
        got = ctx.total_energy_all()
        print(f"{what}, scratch_grid_min_points {grid_min}: counts {ctx.counts().tolist()}, "
              f"max |all - each| {np.max(np.abs(got - each))!r}")
        assert got.dtype == np.float64 and got.shape == each.shape
        assert np.all(np.isfinite(each))
        assert np.all(got == each), (what, grid_min, got.tolist(), each.tolist())
    return got


def test_total_energy_all_equals_total_energy_of_every_chain():
    ctx = energy_context()
    e0 = assert_all_equals_each(ctx, "hand-set")
    assert e0[0] == 0.0 and ctx.count(0) == 0                   # an empty chain
    assert len(set(e0.tolist())) == len(COUNTS)                 # (every chain has an energy of its own: no slot is read twice)
    ctx.run(2000, seed=3)
    # (the chains shed the random rectangles: grids from 4 points on as well, so that sampled states go through them too)
    e1 = assert_all_equals_each(ctx, "after 2000 steps", (0, 16, 4))
    assert ctx.counts().max() >= 4 and np.count_nonzero(e1 != e0) >= len(COUNTS) - 2
    ctx.close()


def test_total_energy_all_reads_the_written_back_state_of_chains_in_device_memory():
    ctx = energy_context(chain_state=2)
    ctx.run(2000, seed=3)
    assert ctx.get_option("hbm_chains") == len(COUNTS)
    assert_all_equals_each(ctx, "chain_state 2, after 2000 steps", (0, 16, 4))
    assert ctx.counts().max() >= 4
    ctx.close()


# ---- 2. / 3. replicas are the plain chains; the winner ------------------------------------------------------------------

# (seed 8 at T0 = 0.3: the CPU oracle's chains of these keys end with 4 to 8 rectangles each and with the lowest energy in
#  replica 2 for tile 0 and in replica 0 for tile 1 -- a fixture in which the choice changes what is returned)
T, R, SEED, T0 = 2, 3, 8, 0.3
SCHEDULE = dict(num_samples=1, init_temperature=T0, alpha_t=0.998, burn_in=1500, samples_interval=500,
                target_temperature=0.0)


def two_tiles():
    return [image_data(synth.make_tile(TILE, 9, tile_id=80 + k, noise=0.2)) for k in range(T)]


def plain_chain(data, setup, comb, seed, chain_id, T0=T0):
    """one chain in a context of its own, without replicas: -> (xy, marks, total energy of the returned state)"""
    alpha, Tt, total, snaps = resolve_schedule(1, T0, SCHEDULE["alpha_t"], 1500, 500, 0.0)
    assert snaps[-1] + 1 == total                               # (no trailing steps: the context holds the returned state)
    s = TileBatchSampler([data], setup, comb, spec_waves=8, point_capacity=256)
    assert s.ctx.get_option("replicas") == 1 and s.ctx.get_option("n_chains") == 1
    s.init("naive")
    (xy, marks), = s.run(total, snaps, 1, T0, alpha, Tt, seed=seed, chain0=chain_id, as_arrays=True)[0]
    e = s.ctx.total_energy(0)
    s.ctx.close()
    return xy.copy(), marks.copy(), e


@pytest.fixture(scope="module")
def restarted():
    """the two tiles with three restarts, and every (replica, tile) as a plain chain of its own"""
    setup, comb = log_model()
    tiles = two_tiles()
    alpha, Tt, total, snaps = resolve_schedule(1, T0, SCHEDULE["alpha_t"], 1500, 500, 0.0)
    s = TileBatchSampler(tiles, setup, comb, spec_waves=8, point_capacity=256, restarts=R)
    s.init("naive")
    out = s.run(total, snaps, 1, T0, alpha, Tt, seed=SEED, chain0=0, as_arrays=True)
    chains = s.ctx.get_points_all()
    ids = replica_chain_ids(T, R)
    plain = {(r, i): plain_chain(tiles[i], setup, comb, SEED, int(ids[r * T + i])) for r in range(R) for i in range(T)}
    res = dict(sampler=s, out=out, chains=[(xy.copy(), mk.copy()) for xy, mk in chains], plain=plain, tiles=tiles,
               setup=setup, comb=comb)
    yield res
    s.ctx.close()


def test_replicas_are_the_plain_chains_of_their_keys(restarted):
    s, plain = restarted["sampler"], restarted["plain"]
    assert s.ctx.get_option("replicas") == R and len(restarted["chains"]) == R * T
    assert s.replica_energy.shape == (R, T) and s.replica_winner.shape == (T,)
    for (r, i), (xy, marks, e) in plain.items():
        cxy, cmk = restarted["chains"][r * T + i]
        assert len(xy) >= 3
        assert cxy.tobytes() == xy.tobytes() and cmk.tobytes() == marks.tobytes(), (r, i)
        assert s.replica_energy[r, i] == e, (r, i)
    # (the replicas of a tile are different chains: the choice below is a choice)
    for i in range(T):
        assert len({restarted["chains"][r * T + i][1].tobytes() for r in range(R)}) == R


def test_the_winner_is_the_lowest_energy_replica(restarted):
    s, out = restarted["sampler"], restarted["out"]
    print("replica energies", s.replica_energy.tolist(), "winners", s.replica_winner.tolist())
    assert s.replica_winner.tolist() == select_replicas(s.replica_energy, T).tolist()
    assert s.replica_winner[0] != 0                             # (see SEED)
    assert len(out) == T
    for i in range(T):
        w = int(s.replica_winner[i])
        assert len(out[i]) == 1
        xy, marks = out[i][-1]
        wxy, wmk = restarted["chains"][w * T + i]
        assert xy.tobytes() == wxy.tobytes() and marks.tobytes() == wmk.tobytes()
        assert s.replica_energy[w, i] <= s.replica_energy[0, i]
        assert s.replica_energy[w, i] == s.replica_energy[:, i].min()


def test_one_restart_is_todays_sampler_and_replica_zero_of_three(restarted):
    setup, comb, tiles = restarted["setup"], restarted["comb"], restarted["tiles"]
    got = {}
    for name, kw in (("omitted", {}), ("one", {"restarts": 1})):
        s = TileBatchSampler(tiles, setup, comb, spec_waves=8, point_capacity=256, **kw)
        s.init("naive")
        alpha, Tt, total, snaps = resolve_schedule(1, T0, SCHEDULE["alpha_t"], 1500, 500, 0.0)
        got[name] = s.run(total, snaps, 1, T0, alpha, Tt, seed=SEED, chain0=0, as_arrays=True)
        assert s.ctx.get_option("replicas") == 1 and s.replica_energy is None and s.replica_winner is None
        s.ctx.close()
    for i in range(T):
        (axy, amk), (bxy, bmk) = got["omitted"][i][-1], got["one"][i][-1]
        assert axy.tobytes() == bxy.tobytes() and amk.tobytes() == bmk.tobytes()
        zxy, zmk = restarted["chains"][i]                       # replica 0 of tile i
        assert axy.tobytes() == zxy.tobytes() and amk.tobytes() == zmk.tobytes()


def test_rectangles_and_the_drop_in_signature(restarted):
    """``sample_rjmcmc_batch(restarts=R)`` hands back lists of ``Rectangle`` of the shapes callers get today; several
    samples cannot be combined with restarts."""
    setup, comb, tiles = restarted["setup"], restarted["comb"], restarted["tiles"]
    seed = int(np.random.default_rng(4).integers(0, 2 ** 63 - 1))
    res = sample_rjmcmc_batch(tiles, np.random.default_rng(4), energy_combinator=comb, init_config="naive", energy_setup=setup,
                              spec_waves=8, point_capacity=256, restarts=2, **SCHEDULE)
    one = sample_rjmcmc_batch(tiles, np.random.default_rng(4), energy_combinator=comb, init_config="naive", energy_setup=setup,
                              spec_waves=8, point_capacity=256, **SCHEDULE)
    assert len(res) == T and all(len(r) == 1 and all(isinstance(p, Rectangle) for p in r[-1]) for r in res)
    ids = replica_chain_ids(T, 2)
    for i in range(T):
        rows = lambda pts: [(p.x, p.y, p.size, p.ratio, p.angle) for p in pts]
        second = plain_chain(tiles[i], setup, comb, seed, int(ids[T + i]))
        second = [(int(x), int(y), s, r, a) for (x, y), (s, r, a) in zip(second[0].tolist(), second[1].tolist())]
        assert rows(res[i][-1]) in (rows(one[i][-1]), second)    # replica 0 = the result without restarts, or replica 1
    with pytest.raises(ValueError, match="num_samples"):
        sample_rjmcmc_batch(tiles, np.random.default_rng(4), energy_combinator=comb, init_config="naive", energy_setup=setup,
                            restarts=2, **dict(SCHEDULE, num_samples=2))


# ---- 4. MPPModel ---------------------------------------------------------------------------------------------------------

def model_with(restarts):
    from mpp_cnn_rs_object_detection_amd.mpp_model import MPPModel
    cfg = json.load(open(os.path.join(REPO, "model_configs", "mpp", "config_mpp_log.json")))
    # (a short, cool schedule: per the CPU oracle 7 to 8 rectangles per tile, and replica 1 ahead in one tile of each image)
    cfg["inference"]["rjmcmc_params"].update(burn_in=2500, alpha_t=0.998, init_temperature=0.2)
    if restarts is not None:
        cfg["inference"]["restarts"] = restarts
    cwd = os.getcwd()
    os.chdir(REPO)                       # paths_config.json is resolved from the working directory, as upstream
    try:
        return MPPModel(cfg, phase="val", load=True)
    finally:
        os.chdir(cwd)


def two_images():
    """two 96 x 160 images: two overlapping 96-px tiles each"""
    out = []
    for k in range(2):
        gt_xy, gt_marks = synth.make_gt(96, 14, tile_id=90 + k)
        more_xy, more_marks = synth.make_gt(96, 10, tile_id=95 + k)
        sel = more_xy[:, 1] < 54
        gt_xy, gt_marks = np.concatenate([gt_xy, more_xy[sel] + np.array([0, 96])]), np.concatenate([gt_marks, more_marks[sel]])
        det, marks = synth.render_maps((96, 160), gt_xy, gt_marks, noise=0.2, noise_seed=k)
        out.append(ImageWMaps(name=f"{k:04}", shape=(96, 160), image=None, detection_map=det, param_dist_maps=marks,
                              mappings=mappings.default_mappings(), param_names=Rectangle.PARAMETERS, gt_config=[]))
    return out


def rows(detections, scores):
    return [(p.x, p.y, p.size, p.ratio, p.angle) for p in detections], np.asarray(scores, dtype=np.float64).tolist()


@pytest.fixture(scope="module")
def images():
    return two_images()


def test_model_merges_the_winners_and_the_dataset_path_equals_the_image_path(images):
    from mpp_cnn_rs_object_detection_amd.data_loaders import merge_score_images
    seeds = [21, 22]
    model = model_with(2)
    base = model_with(1)
    per_image = []
    for data, seed in zip(images, seeds):
        det, scores = model.infer_image(data, seed=seed)
        run = model.last_run
        e, w = run["replica_energy"], run["replica_winner"]
        n = len(run["anchors"])
        assert n == 2 and e.shape == (2, n) and w.tolist() == select_replicas(e, n).tolist()
        print(f"image {data.name}: replica energies {e.tolist()}, winners {w.tolist()}")
        # merging the recorded winners gives what infer_image returned
        agg = (np.concatenate([np.asarray(r.xy, dtype=np.int32) + np.asarray(a, dtype=np.int32)
                               for r, a in zip(run["tile_results"], run["anchors"])]),
               np.concatenate([r.marks for r in run["tile_results"]]))
        again = merge_score_images([model.region_maps(data)], [agg], model.energy_model, model.energy_setup, 3)[0]
        assert rows(det, scores) == rows(*again) and len(det) > 5
        # ... and the recorded winners are the winners: a tile that keeps replica 0 keeps the result without restarts
        base.infer_image(data, seed=seed)
        assert base.last_run["replica_energy"] is None and base.last_run["replica_winner"] is None
        for i in range(n):
            same = (run["tile_results"][i].xy.tobytes() == base.last_run["tile_results"][i].xy.tobytes()
                    and run["tile_results"][i].marks.tobytes() == base.last_run["tile_results"][i].marks.tobytes())
            assert same == (w[i] == 0), (i, w.tolist())
            assert e[w[i], i] <= e[0, i]
        per_image.append(rows(det, scores))
    batch = model.infer_images(images, image_seeds=seeds)
    for k in range(2):
        assert rows(*batch[k]) == per_image[k]


def test_model_with_one_restart_is_the_model_without_the_key(images):
    seeds = [21, 22]
    one, none = model_with(1), model_with(None)
    a = [rows(*one.infer_image(d, seed=s)) for d, s in zip(images, seeds)]
    b = [rows(*none.infer_image(d, seed=s)) for d, s in zip(images, seeds)]
    assert a == b and all(len(x[0]) > 5 for x in a)
    assert [rows(*r) for r in one.infer_images(images, image_seeds=seeds)] == a
    assert [rows(*r) for r in none.infer_images(images, image_seeds=seeds)] == a


# ---- 5. the contrast setup --------------------------------------------------------------------------------------------

def test_restarts_under_the_contrast_setup():
    """One 64 x 64 tile with a picture-reading energy (craciun2), two restarts, eight waves: the replicas share their
    tile's picture, the result is the winning replica's plain chain."""
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "classics_golden.npz"))
    image = np.ascontiguousarray(G["image"][:TILE, :TILE])
    setup = E.ContrastMeasureEnergySetup(contrast_type="craciun2", manual_threshold=-0.05)
    setup.energy_cal = {"detection_thresh": -0.05, "min_area": 20.0, "max_area": 90.0}
    rng = np.random.default_rng(3)
    det = np.clip(0.05 + 0.9 * (np.abs(image.mean(-1) - 0.5) > 0.3) + rng.normal(0, 0.02, (TILE, TILE)), 0.01, 1).astype(np.float32)
    marks = [rng.dirichlet(np.ones(32) * 0.5, size=(TILE, TILE)).astype(np.float32) for _ in range(3)]
    data = ImageWMaps(name="0", shape=(TILE, TILE), image=image, detection_map=det, param_dist_maps=marks,
                      mappings=mappings.default_mappings(), param_names=["size", "ratio", "angle"], labels=None, gt_config=[])
    comb = E.ManualHierarchicalEnergyCombinator(dict(zip(setup.NAMES, [1.0, 2.0, 0.5, 0.25, 0.75])), "ContrastEnergy", 0.0)
    alpha, Tt, total, snaps = resolve_schedule(1, 1.0, SCHEDULE["alpha_t"], 1500, 500, 0.0)
    s = TileBatchSampler([data], setup, comb, spec_waves=8, point_capacity=256, restarts=2)
    s.init("naive")
    (xy, mk), = s.run(total, snaps, 1, 1.0, alpha, Tt, seed=11, chain0=0, as_arrays=True)[0]
    assert s.ctx.get_option("spec_waves") == 8 and s.ctx.get_option("n_chains") == 2
    w = int(s.replica_winner[0])
    assert s.replica_winner.tolist() == select_replicas(s.replica_energy, 1).tolist()
    assert s.replica_energy[w, 0] <= s.replica_energy[0, 0]
    ids = replica_chain_ids(1, 2)
    for r in range(2):
        pxy, pmk, e = plain_chain(data, setup, comb, 11, int(ids[r]), T0=1.0)
        cxy, cmk = s.ctx.get_points(r)
        assert cxy.tobytes() == pxy.tobytes() and cmk.tobytes() == pmk.tobytes() and s.replica_energy[r, 0] == e
        if r == w:
            assert xy.tobytes() == pxy.tobytes() and mk.tobytes() == pmk.tobytes() and len(xy) > 0
    s.ctx.close()
