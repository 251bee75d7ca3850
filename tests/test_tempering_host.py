"""The exchange rule of parallel tempering on the host: the NumPy statement of ``tempering_ref`` behaves as the header says,
the rule keeps the product of Boltzmann laws invariant (a toy system, exact), and the option parses and is refused where
the spec says so.  No GPU: the Philox draw is the library's host entry point."""
import json
import os

import numpy as np
import pytest

import tempering_ref as ref
from helpers import REPO
from mpp_cnn_rs_object_detection_amd import build as hip_build
from mpp_cnn_rs_object_detection_amd import hip_api
from mpp_cnn_rs_object_detection_amd.mpp_model import check_tempering, format_tempering_summary
from mpp_cnn_rs_object_detection_amd.sampler import TEMPERING_EVERY, TEMPERING_RATIO, exchange_rates, resolve_tempering


@pytest.fixture(scope="module")
def lib():
    return hip_build.build()


# ---- the rule -----------------------------------------------------------------------------------------------------------

def test_a_hotter_chain_with_the_lower_energy_always_swaps():
    # a: rung k (colder), b: rung k + 1 (hotter, lower energy): d > 0, whatever the draw
    for u in (0.0, 0.5, 1.0 - 2.0 ** -53):
        ok, d = ref.decide(Ea=3.0, Eb=1.0, Ta=0.1, Tb=0.2, u=u)
        assert ok and d == (1.0 / 0.1 - 1.0 / 0.2) * 2.0 > 0
    ok, d = ref.decide(2.0, 2.0, 0.1, 0.2, 1.0 - 2.0 ** -53)   # equal energies: d == 0 takes the d >= 0 branch
    assert ok and d == 0.0
    ok, d = ref.decide(1.0, 3.0, 0.3, 0.3, 1.0 - 2.0 ** -53)   # equal temperatures (ratio 1) too
    assert ok and d == 0.0
    # the colder chain has the lower energy: Metropolis on d < 0
    d = (1.0 / 0.1 - 1.0 / 0.2) * (1.0 - 1.5)
    assert ref.decide(1.0, 1.5, 0.1, 0.2, np.exp(d) * 0.999)[0] and not ref.decide(1.0, 1.5, 0.1, 0.2, np.exp(d) * 1.001)[0]


def test_non_finite_energies_and_dead_temperatures_never_swap():
    for Ea, Eb in ((np.inf, 1.0), (1.0, -np.inf), (np.nan, 1.0), (3.0, np.nan), (np.inf, np.inf)):
        assert not ref.decide(Ea, Eb, 0.1, 0.2, 0.0)[0]
    for Ta, Tb in ((0.0, 0.2), (0.1, 0.0), (0.0, 0.0), (-0.1, 0.2), (np.nan, 0.2)):
        assert not ref.decide(3.0, 1.0, Ta, Tb, 0.0)[0]
    assert ref.decide(3.0, 1.0, 0.1, 0.2, 0.0)[0]                 # (the same pair with live values does)


def test_pair_sets():
    assert [ref.pairs_of(2, e) for e in range(1, 5)] == [[0]] * 4                       # R = 2: its pair, every time
    assert [ref.pairs_of(3, e) for e in range(1, 5)] == [[1], [0], [1], [0]]
    assert [ref.pairs_of(4, e) for e in range(1, 5)] == [[1], [0, 2], [1], [0, 2]]
    assert [ref.pairs_of(5, e) for e in range(2)] == [[0, 2], [1, 3]]
    for R in range(2, 9):
        for e in range(4):
            ks = ref.pairs_of(R, e)
            assert all(k + 1 < R for k in ks) and all(b - a >= 2 for a, b in zip(ks, ks[1:]))      # in range and disjoint
            assert len(ks) == (R - (0 if R == 2 else e % 2)) // 2                                  # the launcher's count


def test_ladder_is_repeated_multiplication():
    sched, rung = ref.ladder(0.3, 0.998, 0.01, 1.3, 4, 2)
    f = [1.0, 1.3, 1.3 * 1.3, 1.3 * 1.3 * 1.3]
    assert sched[::2, 0].tolist() == [0.3 * v for v in f] and sched[1::2, 2].tolist() == [0.01 * v for v in f]
    assert np.all(sched[:, 1] == 0.998) and rung.tolist() == [0, 0, 1, 1, 2, 2, 3, 3]


def test_exchange_swaps_triples_and_rungs_of_the_attempted_pairs_only(lib):
    R, n, every, s = 4, 2, 256, 512                              # e = 2: pairs (0, 1) and (2, 3)
    sched, rung = ref.ladder(0.4, 0.99, 0.02, 2.0, R, n)
    rung[[0, 2]] = rung[[2, 0]]                                   # tile 0: replica 0 on rung 1, replica 1 on rung 0
    sched[[0, 2]] = sched[[2, 0]]
    before, rung0 = sched.copy(), rung.copy()
    energy = np.array([5.0, 1.0, 9.0, 2.0, 1.0, 3.0, 0.5, np.inf])    # chain r * n + i
    keys = (np.array([11, 12], np.uint64), np.array([7, 8], np.uint32))
    log = ref.exchange(sched, rung, energy, s, every, n, R, keys)
    assert log["tile"].tolist() == [0, 0, 1, 1] and log["k"].tolist() == [0, 2, 0, 2] and np.all(log["step"] == s)
    # tile 0, k = 0: a is the chain ON rung 0 (replica 1, chain 2), b the one on rung 1 (replica 0, chain 0)
    assert (log["chain_a"][0], log["chain_b"][0]) == (2, 0) and (log["Ea"][0], log["Eb"][0]) == (9.0, 5.0)
    assert (log["Ta"][0], log["Tb"][0]) == (0.4, 0.8) and log["accepted"][0] == 1          # hotter and lower: swaps
    assert rung[[0, 2]].tolist() == [0, 1] and sched[0].tolist() == before[2].tolist() and sched[2].tolist() == before[0].tolist()
    # tile 0, k = 2: chains 4 and 6, the hotter one lower again
    assert (log["chain_a"][1], log["chain_b"][1], log["accepted"][1]) == (4, 6, 1) and rung[[4, 6]].tolist() == [3, 2]
    # tile 1, k = 2: an infinite energy never swaps; the records hold the values read before the swap
    assert (log["chain_a"][3], log["chain_b"][3], log["accepted"][3]) == (5, 7, 0) and rung[[5, 7]].tolist() == [2, 3]
    for r in log:
        ok, d = ref.decide(r["Ea"], r["Eb"], r["Ta"], r["Tb"], r["u"])
        assert bool(ok) == bool(r["accepted"]) and float(d) == r["d"]
    # the draw: block 0x80000000 | k of the tile's replica-0 key at the absolute step
    w = hip_api.philox([s, 0, 0x80000002, 8], [12, 0])
    assert log["u"][3] == ref.u53(w[0], w[1]) == ref.draw(s, 2, 8, 12) and 0.0 <= log["u"][3] < 1.0
    assert len({float(u) for u in log["u"]}) == 4
    # nothing but the accepted pairs moved
    moved = sorted(np.flatnonzero(rung != rung0).tolist())
    assert moved == sorted(np.concatenate([[r["chain_a"], r["chain_b"]] for r in log[log["accepted"] == 1]]).tolist())
    assert exchange_rates(log, R).tolist()[0] in (0.5, 1.0) and np.isnan(exchange_rates(log, R)[1])


def test_u53_and_step_words(lib):
    assert ref.u53(0, 0) == 0.0 and ref.u53(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53
    s = (3 << 32) | 5                                            # a step past 2^32: both words of the counter
    w = hip_api.philox([5, 3, 0x80000001, 9], [0xdeadbeef, 0x12345678])
    assert ref.draw(s, 1, 9, (0x12345678 << 32) | 0xdeadbeef) == ref.u53(w[0], w[1])


# ---- the rule keeps the product of Boltzmann laws: a toy system -----------------------------------------------------------

def toy_chi2(decide, sweeps=200_000, seed=1):
    """Three levels, three fixed temperatures.  A sweep: every rung's state drawn afresh from its own Boltzmann law (an exact
    Gibbs move), then the exchange of the sweep's pair set, as a swap of the two states.  The joint occupation AFTER the
    exchange against the product of the three laws: chi-square over the 27 cells."""
    E, T = np.array([0.0, 1.0, 2.5]), np.array([0.5, 1.0, 2.0])
    p = np.exp(-E[None, :] / T[:, None])
    p /= p.sum(axis=1, keepdims=True)
    rng = np.random.default_rng(seed)
    x = np.stack([rng.choice(3, size=sweeps, p=p[k]) for k in range(3)], axis=1)          # [sweeps, rung]
    u = rng.random(sweeps)
    k = np.array([ref.pairs_of(3, e)[0] for e in range(2)])[np.arange(sweeps) % 2]        # the pair of sweep e
    rows = np.arange(sweeps)
    ok, _ = decide(E[x[rows, k]], E[x[rows, k + 1]], T[k], T[k + 1], u)
    xa, xb = x[rows, k].copy(), x[rows, k + 1].copy()
    x[rows, k], x[rows, k + 1] = np.where(ok, xb, xa), np.where(ok, xa, xb)
    got = np.bincount(x[:, 0] * 9 + x[:, 1] * 3 + x[:, 2], minlength=27).astype(np.float64)
    want = sweeps * (p[0][:, None, None] * p[1][None, :, None] * p[2][None, None, :]).reshape(-1)
    assert want.min() > 5.0                                       # (every cell is populated enough for the statistic)
    return float(np.sum((got - want) ** 2 / want)), float(np.mean(ok))


def test_the_rule_keeps_the_product_of_boltzmann_laws():
    # 27 cells, probabilities fixed beforehand: 26 degrees of freedom, whose 0.999 quantile is 54.05.  The sweeps are
    # independent (every state is drawn afresh), so the statistic has that law; the seed is fixed.
    chi2, rate = toy_chi2(ref.decide)
    print(f"chi-square {chi2:.2f} (26 degrees of freedom, bound 54.05), {rate:.3f} of the exchanges accepted")
    assert chi2 < 54.05 and 0.2 < rate < 0.95

    # the statistic sees a wrong rule: the sign of d flipped, and a rule that always swaps
    def flipped(Ea, Eb, Ta, Tb, u):
        return ref.decide(Eb, Ea, Ta, Tb, u)

    def always(Ea, Eb, Ta, Tb, u):
        return np.ones(len(u), bool), None
    assert toy_chi2(flipped)[0] > 1000.0 and toy_chi2(always)[0] > 1000.0


# ---- the option -----------------------------------------------------------------------------------------------------------

def config(**inference):
    return {"inference": inference}


def test_check_tempering():
    assert check_tempering({}) is None and check_tempering(config(restarts=4)) is None
    assert check_tempering(config(restarts=4, tempering=False)) is None
    assert check_tempering(config(restarts=1, tempering=False)) is None
    assert check_tempering(config(restarts=2, tempering=True)) == {"ratio": TEMPERING_RATIO, "every": TEMPERING_EVERY}
    assert TEMPERING_EVERY == 4096 == hip_api.TEMPERING_EVERY
    assert check_tempering(config(restarts=8, tempering={"ratio": 1.5})) == {"ratio": 1.5, "every": 4096}
    assert check_tempering(config(restarts=8, tempering={"every": 1024, "ratio": 1})) == {"ratio": 1.0, "every": 1024}
    for restarts in ({}, {"restarts": 1}):
        with pytest.raises(ValueError, match="restarts"):
            check_tempering(config(tempering=True, **restarts))
        with pytest.raises(ValueError, match="restarts"):
            check_tempering(config(tempering={"ratio": 2.0}, **restarts))
    # what restarts refuses: a bad count, several ranks sharing one image
    with pytest.raises(ValueError, match="restarts"):
        check_tempering(config(restarts=0, tempering=True))
    with pytest.raises(ValueError, match="ranks"):
        check_tempering(config(restarts=2, tempering=True), world_size=2)
    for bad in (3, "on", 2.0, [2.0], {"ratio": 0.5}, {"ratio": float("nan")}, {"ratio": float("inf")}, {"ratio": "2"},
                {"ratio": True}, {"every": 0}, {"every": 2.5}, {"every": True}, {"rate": 2.0}):
        with pytest.raises(ValueError, match="tempering"):
            check_tempering(config(restarts=4, tempering=bad))
    assert resolve_tempering(None, 1) is None and resolve_tempering(False, 1) is None
    with pytest.raises(ValueError, match="restarts"):
        resolve_tempering(True, 1)


def test_the_shipped_configs_leave_it_off():
    for name in ("config_mpp_log.json", "mpp_hrcM.json"):
        cfg = json.load(open(os.path.join(REPO, "model_configs", "mpp", name)))
        assert check_tempering(cfg) is None


def test_summary_line():
    line = format_tempering_summary({"ratio": 2.0, "every": 4096, "exchanges": 7, "exchange_rate": np.array([0.25, np.nan, 1.0]),
                                     "winner_rung": np.array([0, 2, 0])})
    assert "ratio 2" in line and "7 exchange" in line and "[0.25, -, 1.00]" in line and "2 of 3" in line


def test_main_flag():
    import main
    parser = main.build_parser()
    base = ["-p", "infer", "-m", "mpp", "-c", "x"]
    assert parser.parse_args(base).tempering is None
    assert parser.parse_args(base + ["--tempering"]).tempering is True
    assert parser.parse_args(base + ["--tempering", "1.5"]).tempering == 1.5
    assert parser.parse_args(base + ["--tempering", "--restarts", "4"]).restarts == 4
    for bad in ("0.5", "nan", "inf", "x"):
        with pytest.raises(SystemExit):
            parser.parse_args(base + ["--tempering", bad])
    # off by default; on, it keeps an interval the config gives; a ratio on the command line replaces the config's
    cfg = main.apply_tempering(parser.parse_args(base), {"inference": {"restarts": 2}})
    assert "tempering" not in cfg["inference"]
    cfg = main.apply_tempering(parser.parse_args(base + ["--tempering"]), {"inference": {"restarts": 2}})
    assert cfg["inference"]["tempering"] is True
    cfg = main.apply_tempering(parser.parse_args(base + ["--tempering"]), {"inference": {"tempering": {"every": 512}}})
    assert cfg["inference"]["tempering"] == {"every": 512}
    cfg = main.apply_tempering(parser.parse_args(base + ["--tempering", "3"]), {"inference": {"tempering": {"every": 512, "ratio": 2}}})
    assert cfg["inference"]["tempering"] == {"every": 512, "ratio": 3.0}
    cfg = main.apply_tempering(parser.parse_args(base + ["--tempering", "3"]), {})
    assert cfg["inference"]["tempering"] == {"ratio": 3.0} and check_tempering(dict(cfg, inference=dict(cfg["inference"], restarts=2)))
    cfg = main.apply_tempering(parser.parse_args(["-p", "train", "-m", "mpp", "-c", "x", "--tempering"]), {})
    assert cfg == {}
