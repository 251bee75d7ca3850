"""Parallel tempering on the GPU: the replicas of a tile on a temperature ladder, exchanging schedules every K steps.

* the per-chain schedules and the ladder are what the header says, bit for bit;
* with ratio 1 the run is the restarts run; with no boundary reached the chains are plain chains on their rungs' schedules;
* the device loop (``mpp_run_tempered``) makes the decisions, and leaves the chains, of a host loop built from ``run``,
  ``total_energy_all``, ``get_schedules``, the rule of ``tempering_ref`` and ``set_schedules``;
* cutting the run into calls, chains in device memory and a short log change nothing;
* ``MPPModel``: the dataset path gives what the image path gives, restarts without the key are untouched.

Small on purpose: 64-px tiles, about 2 000 steps, at most a dozen workgroups per launch."""
import numpy as np
import pytest

import tempering_ref as ref
from helpers import log_model
from test_gpu_restarts import R as R3, SCHEDULE, SEED, T as N, T0, images, model_with, plain_chain, rows, two_tiles  # noqa: F401
from mpp_cnn_rs_object_detection_amd import hip_api
from mpp_cnn_rs_object_detection_amd.sampler import (TileBatchSampler, exchange_rates, replica_chain_ids, resolve_schedule,
                                                      rungs_after, select_replicas)

pytestmark = pytest.mark.gpu

ALPHA, EVERY, STEPS, RATIO = 0.998, 256, 2048, 2.0
# The seed of every R, picked from runs of host_loop below (run, total_energy_all, get / set_schedules and the NumPy rule:
# nothing of the code under test) over seeds 1, 2, ...: the first whose log holds every kind of decision.  Counts of
# (swaps accepted with d < 0, rejections, swaps with d >= 0) among the records of the 8 exchanges:
#   R = 2: seed 5, 16 records, (1, 12, 3)      R = 3: seed 2, 16 records, (1, 10, 5)      R = 4: seed 1, 24 records, (1, 12, 11)
# (the closest a draw comes to exp(d) in these three logs is 2e-2)
SEEDS = {2: 5, 3: 2, 4: 1}


def new_sampler(R, **ctx_options):
    setup, comb = log_model()
    ctx = hip_api.MppContext(0, point_capacity=256, spec_waves=8, replicas=R, **ctx_options) if ctx_options else None
    s = TileBatchSampler(two_tiles(), setup, comb, spec_waves=8, point_capacity=256, restarts=R, ctx=ctx)
    s.init("naive")
    return s


def start(ctx, R, seed):
    """keys of the replicas and the common schedule: what ``TileBatchSampler.run`` sets before it steps"""
    ids = replica_chain_ids(N, R)
    ctx.set_chain_keys(np.full(R * N, seed, np.uint64), ids)
    ctx.set_schedule(T0, ALPHA, 0.0)
    return (np.full(N, seed, np.uint64), ids[:N])


def state(ctx):
    return [(xy.copy(), mk.copy()) for xy, mk in ctx.get_points_all()]


def same_states(a, b):
    return len(a) == len(b) and all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() for x, y in zip(a, b))


def host_loop(R, seed, steps=STEPS, every=EVERY, ratio=RATIO):
    """the reference: plain runs of ``every`` steps, the energies and schedules through the host, the rule in NumPy"""
    s = new_sampler(R)
    ctx = s.ctx
    keys = start(ctx, R, seed)
    sched, rung = ref.ladder(T0, ALPHA, 0.0, ratio, R, N)
    ctx.set_schedules(sched)
    recs = []
    for at in range(every, steps + 1, every):
        ctx.run(every, seed)
        energy, sched = ctx.total_energy_all(), ctx.get_schedules()
        recs.append(ref.exchange(sched, rung, energy, at, every, N, R, keys))
        ctx.set_schedules(sched)
    out = dict(log=np.concatenate(recs), chains=state(ctx), sched=ctx.get_schedules(), rung=rung.reshape(R, N))
    ctx.close()
    return out


def kinds(log):
    """(swaps accepted with d < 0, rejections, swaps with d >= 0) of a reference log"""
    acc = log["accepted"] != 0
    return int(np.sum(acc & (log["d"] < 0))), int(np.sum(~acc)), int(np.sum(acc & (log["d"] >= 0)))


def device_loop(R, seed, cuts=(STEPS,), every=EVERY, ratio=RATIO, log=True, log_cap=None, **ctx_options):
    s = new_sampler(R, **ctx_options)
    ctx = s.ctx
    start(ctx, R, seed)
    ctx.set_ladder(ratio)
    logs, counts, ms = [], [], 0.0
    for c in cuts:
        logs.append(ctx.run_tempered(c, seed, 0, every=every, log=log, log_cap=log_cap))
        counts.append(ctx.exchange_records)
        ms += ctx.last_kernel_ms()
    out = dict(log=np.concatenate(logs) if log else None, counts=counts, chains=state(ctx), sched=ctx.get_schedules(),
               stats=ctx.tempering_stats(), hbm=ctx.get_option("hbm_chains"), step=ctx.step_index(0), kernel_ms=ms)
    ctx.close()
    return out


@pytest.fixture(scope="module")
def host3():
    return host_loop(3, SEEDS[3])


@pytest.fixture(scope="module")
def device3():
    return device_loop(3, SEEDS[3])


def assert_log_equals(got, want):
    assert len(got) == len(want)
    for f in ("step", "tile", "k", "chain_a", "chain_b", "accepted"):
        assert got[f].tolist() == want[f].tolist(), f
    for f in ("Ea", "Eb", "Ta", "Tb", "u"):
        assert got[f].tobytes() == want[f].tobytes(), f


# ---- 1. schedules and ladder --------------------------------------------------------------------------------------------

def test_schedules_and_ladder():
    s = new_sampler(3)
    ctx = s.ctx
    ctx.set_schedule(0.3, 0.998, 0.01)
    got = ctx.get_schedules()
    assert got.shape == (3 * N, 3) and got.dtype == np.float64
    assert np.all(got == np.array([0.3, 0.998, 0.01]))
    ctx.set_ladder(2.0)
    want, _ = ref.ladder(0.3, 0.998, 0.01, 2.0, 3, N)
    assert ctx.get_schedules().tobytes() == want.tobytes()
    ctx.set_ladder(1.3)                                          # (a ratio whose powers are rounded)
    want, _ = ref.ladder(0.3, 0.998, 0.01, 1.3, 3, N)
    assert ctx.get_schedules().tobytes() == want.tobytes() and want[2 * N, 0] == 0.3 * (1.3 * 1.3)
    assert ctx.tempering_stats() == {"exchanges": 0, "attempts": 0, "accepted": 0, "ms": 0.0}
    # a round trip of triples of one's own; a refused set writes nothing
    mine = np.random.default_rng(1).uniform(0.5, 1.0, (3 * N, 3)) * np.array([1.0, 1.0, 0.1])
    ctx.set_schedules(mine)
    assert ctx.get_schedules().tobytes() == mine.tobytes()
    for bad in ((0, 0, np.nan), (1, 1, np.inf), (2, 0, 0.01)):  # (chain 2: T below its T_target)
        worse = mine.copy()
        worse[bad[0], bad[1]] = bad[2]
        with pytest.raises(hip_api.MppError, match="set_schedules"):
            ctx.set_schedules(worse)
    assert ctx.get_schedules().tobytes() == mine.tobytes()
    # the ladder's refusals
    for ratio in (0.5, float("nan"), float("inf")):
        with pytest.raises(hip_api.MppError, match="ratio"):
            ctx.set_ladder(ratio)
    with pytest.raises(hip_api.MppError, match="every"):
        ctx.run_tempered(100, 1, every=0)
    ctx.set_schedule(0.3, 0.998, 0.0)                            # ... clears the ladder
    with pytest.raises(hip_api.MppError, match="no ladder"):
        ctx.run_tempered(100, 1, every=10)
    ctx.close()
    one = new_sampler(1)
    one.ctx.set_schedule(0.3, 0.998, 0.0)
    with pytest.raises(hip_api.MppError, match="replicas"):
        one.ctx.set_ladder(2.0)
    with pytest.raises(hip_api.MppError, match="no ladder"):
        one.ctx.run_tempered(100, 1, every=10)
    one.ctx.close()


def test_chains_at_different_steps_are_refused():
    setup, comb = log_model()
    ctx = hip_api.MppContext(0, point_capacity=256, spec_waves=8, replicas=2)
    s = TileBatchSampler(two_tiles()[:1], setup, comb, spec_waves=8, point_capacity=256, restarts=2, ctx=ctx)
    s.init("naive")
    start_keys = replica_chain_ids(1, 2)
    ctx.set_chain_keys(np.full(2, 5, np.uint64), start_keys)
    ctx.set_schedule(T0, ALPHA, 0.0)
    ctx.set_ladder(2.0)
    assert len(ctx.run_tempered(16, 5, every=8)) == 2 and ctx.step_index(0) == ctx.step_index(1) == 16
    tape = np.zeros(1, hip_api.PROPOSAL_DTYPE)                    # one uniform birth, replayed on chain 1 alone
    tape["kernel"], tape["target"], tape["ax"], tape["ay"] = 0, -1, 10, 10
    tape["as"], tape["ar"], tape["aa"], tape["u_accept"] = 6.0, 0.5, 0.3, 0.5
    ctx.replay(1, tape)
    assert ctx.step_index(1) == 17
    with pytest.raises(hip_api.MppError, match="same step"):
        ctx.run_tempered(16, 5, every=8)
    ctx.close()


# ---- 2. ratio 1 is restarts ---------------------------------------------------------------------------------------------

def test_ratio_one_is_restarts():
    setup, comb = log_model()
    alpha, Tt, total, snaps = resolve_schedule(1, T0, SCHEDULE["alpha_t"], 1500, 500, 0.0)
    got = {}
    for name, kw in (("restarts", {}), ("tempered", {"tempering": {"ratio": 1.0, "every": 256}})):
        s = TileBatchSampler(two_tiles(), setup, comb, spec_waves=8, point_capacity=256, restarts=R3, **kw)
        s.init("naive")
        out = s.run(total, snaps, 1, T0, alpha, Tt, seed=SEED, chain0=0, as_arrays=True)
        got[name] = dict(out=out, chains=state(s.ctx), energy=s.replica_energy.copy(), winner=s.replica_winner.copy(),
                         log=s.exchange_log, rung=s.replica_rung, rate=s.exchange_rate)
        s.ctx.close()
    a, b = got["restarts"], got["tempered"]
    assert a["log"] is None and a["rung"] is None and a["rate"] is None
    assert same_states(a["chains"], b["chains"]) and len(a["chains"]) == R3 * N
    assert a["energy"].tobytes() == b["energy"].tobytes() and a["winner"].tolist() == b["winner"].tolist()
    for i in range(N):
        assert same_states(a["out"][i], b["out"][i])
    log = b["log"]
    assert len(log) == N * (total // 256) and total // 256 >= 7  # one pair of three per tile and exchange
    d = np.array([ref.decide(r["Ea"], r["Eb"], r["Ta"], r["Tb"], r["u"])[1] for r in log])
    assert np.all(log["Ta"] == log["Tb"]) and np.all(d == 0.0) and np.all(log["accepted"] == 1)
    assert b["rate"].tolist() == [1.0, 1.0]
    assert b["rung"].shape == (R3, N) and sorted(b["rung"][:, 0].tolist()) == [0, 1, 2]
    assert b["rung"].tolist() == rungs_after(log, N, R3).tolist() and b["rung"].tolist() != [[0, 0], [1, 1], [2, 2]]


# ---- 3. no boundary reached: plain chains on the rungs' schedules -----------------------------------------------------

def test_no_boundary_reached_is_a_set_of_plain_chains():
    setup, comb = log_model()
    tiles = two_tiles()
    alpha, Tt, total, snaps = resolve_schedule(1, T0, SCHEDULE["alpha_t"], 1500, 500, 0.0)
    s = TileBatchSampler(tiles, setup, comb, spec_waves=8, point_capacity=256, restarts=R3,
                         tempering={"ratio": 2.0, "every": total + 1})
    s.init("naive")
    s.run(total, snaps, 1, T0, alpha, Tt, seed=SEED, chain0=0, as_arrays=True)
    chains, energy = state(s.ctx), s.replica_energy.copy()
    assert len(s.exchange_log) == 0 and s.replica_rung.tolist() == [[0, 0], [1, 1], [2, 2]]
    assert s.ctx.tempering_stats()["exchanges"] == 0
    s.ctx.close()
    ids = replica_chain_ids(N, R3)
    for r in range(R3):
        for i in range(N):
            xy, marks, e = plain_chain(tiles[i], setup, comb, SEED, int(ids[r * N + i]), T0=T0 * 2.0 ** r)
            assert chains[r * N + i][0].tobytes() == xy.tobytes() and chains[r * N + i][1].tobytes() == marks.tobytes(), (r, i)
            assert energy[r, i] == e


# ---- 4. the device loop equals a host loop ----------------------------------------------------------------------------

@pytest.mark.parametrize("R", [2, 3, 4])
def test_device_loop_equals_host_loop(R, host3, device3):
    want = host3 if R == 3 else host_loop(R, SEEDS[R])
    got = device3 if R == 3 else device_loop(R, SEEDS[R])
    log, wl = got["log"], want["log"]
    n_acc_neg, n_rej, n_acc_pos = kinds(wl)
    print(f"R {R} seed {SEEDS[R]}: {len(wl)} records, accepted with d < 0: {n_acc_neg}, rejected: {n_rej}, "
          f"swapped with d >= 0: {n_acc_pos}")
    # the fixture exercises the rule, and no decision hangs on the last bit of exp
    assert n_acc_neg >= 1 and n_rej >= 1 and n_acc_pos >= 1
    with np.errstate(over="ignore"):
        assert not np.any(np.abs(wl["u"] - np.exp(wl["d"])) <= 1e-12)
    assert len(wl) == sum(N * len(ref.pairs_of(R, e)) for e in range(1, STEPS // EVERY + 1))
    assert_log_equals(log, wl)
    assert same_states(got["chains"], want["chains"])
    assert got["sched"].tobytes() == want["sched"].tobytes()
    assert rungs_after(log, N, R).tolist() == want["rung"].tolist()
    # the triples moved as wholes: a chain's T_target / alpha say which rung's schedule it follows (T_target is 0 here: by T)
    for i in range(N):
        order = np.argsort(got["sched"][i::N, 0], kind="stable")
        assert want["rung"][order, i].tolist() == list(range(R))
    assert got["counts"] == [len(wl)] and got["step"] == STEPS
    st = got["stats"]
    assert st["exchanges"] == STEPS // EVERY and st["attempts"] == len(wl) and st["accepted"] == int(np.sum(wl["accepted"]))
    assert st["ms"] > 0.0 and got["kernel_ms"] > 0.0
    assert exchange_rates(log, R).tolist() == [np.mean(wl["accepted"][wl["k"] == k]) for k in range(R - 1)]


# ---- 5. / 6. / 7. cutting the run, chains in device memory, the log's capacity -----------------------------------------

def test_cutting_the_run_changes_nothing(device3):
    cut = device_loop(3, SEEDS[3], cuts=(700, 1348))
    assert cut["counts"][0] == N * 2 and sum(cut["counts"]) == len(device3["log"])      # exchanges at 256 and 512
    assert_log_equals(cut["log"], device3["log"])
    assert same_states(cut["chains"], device3["chains"]) and cut["sched"].tobytes() == device3["sched"].tobytes()
    assert cut["stats"]["accepted"] == device3["stats"]["accepted"] and cut["step"] == STEPS
    # a call that ends on a boundary makes that exchange, the next call does not repeat it
    ends = device_loop(3, SEEDS[3], cuts=(512, 1536))
    assert ends["counts"] == [N * 2, len(device3["log"]) - N * 2]
    assert_log_equals(ends["log"], device3["log"])
    assert same_states(ends["chains"], device3["chains"])


def test_chains_in_device_memory(device3):
    hbm = device_loop(3, SEEDS[3], chain_state=2)
    assert hbm["hbm"] == 3 * N and device3["hbm"] == 0
    assert_log_equals(hbm["log"], device3["log"])
    assert same_states(hbm["chains"], device3["chains"]) and hbm["sched"].tobytes() == device3["sched"].tobytes()


def test_log_capacity(device3):
    full = device3["log"]
    short = device_loop(3, SEEDS[3], log_cap=5)
    assert short["counts"] == [len(full)] and len(short["log"]) == 5 < len(full)
    assert_log_equals(short["log"], full[:5])
    none = device_loop(3, SEEDS[3], log=False)
    assert none["log"] is None and none["counts"] == [len(full)]
    for other in (short, none):
        assert same_states(other["chains"], device3["chains"]) and other["sched"].tobytes() == device3["sched"].tobytes()
        assert other["stats"]["accepted"] == device3["stats"]["accepted"]


# ---- 8. MPPModel ------------------------------------------------------------------------------------------------------

def tempered_model(restarts, tempering):
    model = model_with(restarts)
    if tempering is not None:
        model.config["inference"]["tempering"] = tempering
    return model


def test_model_dataset_path_equals_image_path(images):
    seeds = [21, 22]
    model = tempered_model(2, {"ratio": 2.0, "every": 512})
    per_image, runs = [], []
    for data, seed in zip(images, seeds):
        det, scores = model.infer_image(data, seed=seed)
        run = model.last_run
        t = run["tempering"]
        n = len(run["anchors"])
        assert n == 2 and t["ratio"] == 2.0 and t["every"] == 512
        assert t["exchange_rate"].shape == (1,) and 0.0 <= t["exchange_rate"][0] <= 1.0
        assert t["winner_rung"].shape == (n,) and set(t["winner_rung"].tolist()) <= {0, 1}
        assert t["exchanges"] == run["total_steps"] // 512 >= 4 and run["replica_winner"].tolist() == select_replicas(run["replica_energy"], n).tolist()
        print(f"image {data.name}: exchange rate {t['exchange_rate'].tolist()}, winners {run['replica_winner'].tolist()} "
              f"on rungs {t['winner_rung'].tolist()}")
        per_image.append(rows(det, scores))
        runs.append(t)
        assert len(det) > 5
    batch = model.infer_images(images, image_seeds=seeds)
    assert len(model.last_tempering) == 2
    for k in range(2):
        assert rows(*batch[k]) == per_image[k]
        t = model.last_tempering[k]                              # per image: its own tiles' pairs, drawn from its own key
        assert t["winner_rung"].tolist() == runs[k]["winner_rung"].tolist() and t["exchanges"] == runs[k]["exchanges"]
        assert t["exchange_rate"].tolist() == runs[k]["exchange_rate"].tolist()


def test_model_restarts_without_the_key_are_untouched(images):
    seeds = [21, 22]
    plain, off = tempered_model(2, None), tempered_model(2, False)
    a = [rows(*plain.infer_image(d, seed=s)) for d, s in zip(images, seeds)]
    assert plain.last_run["tempering"] is None and plain.last_tempering == [None]
    assert [rows(*off.infer_image(d, seed=s)) for d, s in zip(images, seeds)] == a
    assert [rows(*r) for r in plain.infer_images(images, image_seeds=seeds)] == a
    # ... and tempering does change what the replicas do (a ladder of ratio 2 is not two restarts)
    tempered = tempered_model(2, {"ratio": 2.0, "every": 512})
    tempered.infer_image(images[0], seed=seeds[0])
    plain.infer_image(images[0], seed=seeds[0])
    assert tempered.last_run["replica_energy"][1].tolist() != plain.last_run["replica_energy"][1].tolist()


def test_model_tempering_needs_restarts(images):
    for restarts in (1, None):
        model = tempered_model(restarts, True)
        with pytest.raises(ValueError, match="restarts"):
            model.infer_image(images[0], seed=21)
        with pytest.raises(ValueError, match="restarts"):
            model.infer_images(images, image_seeds=[21, 22])
