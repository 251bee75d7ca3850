"""Restarts (R independent chains per tile, the lowest-energy one is kept): the host-side rules.

``select_replicas`` against a plain double loop written here, ``replica_chain_ids``' layout, the validation of
``inference.restarts`` and the command line's ``--restarts``."""
import importlib.util
import math
import os

import numpy as np
import pytest

from helpers import REPO
from mpp_cnn_rs_object_detection_amd.mpp_model import check_restarts
from mpp_cnn_rs_object_detection_amd.sampler import replica_chain_ids, select_replicas

NAN, INF = float("nan"), float("inf")


def walk(energy, n_tiles):
    """the rule as the issue states it, one tile and one replica at a time"""
    e = [float(v) for v in np.asarray(energy, dtype=np.float64).reshape(-1)]
    R = len(e) // n_tiles
    out = []
    for i in range(n_tiles):
        best = 0
        for r in range(1, R):
            cur, new = e[best * n_tiles + i], e[r * n_tiles + i]
            if new < cur or (not math.isfinite(cur) and math.isfinite(new)):
                best = r
        out.append(best)
    return out


CASES = {
    "one replica": ([[3.0, -1.0, NAN]], [0, 0, 0]),
    "strict minimum in each position": ([[-5.0, 1.0, 2.0], [0.0, -7.0, 2.5], [1.0, 1.5, -3.0]], [0, 1, 2]),
    "tie of 1 and 2": ([[4.0], [-2.0], [-2.0]], [1]),
    "tie of 0 and 2": ([[-2.0], [3.0], [-2.0]], [0]),
    "nan in replica 0": ([[NAN], [5.0], [-1.0], [2.0]], [2]),
    "+inf in replica 0": ([[INF], [5.0], [7.0]], [1]),
    "nan later never wins": ([[1.0], [NAN], [0.5], [NAN]], [2]),
    "all non-finite": ([[NAN, INF, INF], [INF, NAN, INF], [NAN, NAN, INF]], [0, 0, 0]),
    "signed zeros tie": ([[0.0, -0.0], [-0.0, 0.0]], [0, 0]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_select_replicas(name):
    energy, want = CASES[name]
    e = np.array(energy, dtype=np.float64)
    T = e.shape[1]
    assert walk(e, T) == want                                   # (the loop above says what the issue says)
    for given in (e, e.reshape(-1), e.tolist()):                # [R, T], flat in chain order, plain lists
        got = select_replicas(given, T)
        assert got.shape == (T,) and np.issubdtype(got.dtype, np.integer)
        assert got.tolist() == want


def test_select_replicas_equals_the_walk_on_random_energies_with_ties_and_holes():
    rng = np.random.default_rng(5)
    for R, T in ((1, 4), (2, 1), (3, 7), (16, 40)):
        e = rng.integers(-3, 4, size=(R, T)).astype(np.float64)                  # few values: many exact ties
        e[rng.random((R, T)) < 0.2] = NAN
        e[rng.random((R, T)) < 0.1] = INF
        assert select_replicas(e, T).tolist() == walk(e, T)


def test_replica_chain_ids():
    ids = replica_chain_ids(5, 3)
    assert ids.dtype == np.uint32 and ids.shape == (15,)
    for r in range(3):
        for i in range(5):
            assert ids[r * 5 + i] == i + r * 5
    ids = replica_chain_ids(4, 3, chain0=7)
    assert ids[:4].tolist() == [7, 8, 9, 10]                    # replica 0 keeps the ids of a launch without restarts
    assert ids.reshape(3, 4)[2].tolist() == [15, 16, 17, 18]
    assert len(set(ids.tolist())) == 12
    assert replica_chain_ids(6, 1, 2).tolist() == [2, 3, 4, 5, 6, 7]
    top = replica_chain_ids(2, 2, chain0=2 ** 32 - 4)           # the last id that fits
    assert int(top[-1]) == 2 ** 32 - 1
    with pytest.raises(ValueError):
        replica_chain_ids(2, 2, chain0=2 ** 32 - 3)
    with pytest.raises(ValueError):
        replica_chain_ids(2 ** 31, 3)


def config(value):
    return {"inference": {"restarts": value, "rjmcmc_params": {}}}


@pytest.mark.parametrize("bad", [0, -1, 2.5, "2"])
def test_check_restarts_refuses(bad):
    with pytest.raises(ValueError, match="restarts"):
        check_restarts(config(bad), 1)


def test_check_restarts():
    assert check_restarts({"inference": {}}, 1) == 1            # the default
    assert check_restarts(config(1), 1) == 1 and check_restarts(config(4), 1) == 4
    assert check_restarts(config(1), 2) == 1                    # ranks that share an image: fine without restarts
    with pytest.raises(ValueError, match="restarts"):
        check_restarts(config(2), 2)


def test_the_command_line_refuses_restarts_below_one(capsys):
    spec = importlib.util.spec_from_file_location("mpp_main_cli", os.path.join(REPO, "main.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    parser = cli.build_parser()
    assert parser.parse_args(["-p", "infer", "-m", "mpp", "-c", "mpp_hrcM", "--restarts", "4"]).restarts == 4
    assert parser.parse_args(["-p", "infer", "-m", "mpp", "-c", "mpp_hrcM"]).restarts is None
    for bad in ("0", "-2"):
        with pytest.raises(SystemExit) as e:
            parser.parse_args(["--restarts", bad])
        assert e.value.code == 2
    assert "--restarts" in capsys.readouterr().err
