"""The greedy completion's host-side rules: the numpy selection rule of ``birth_complete_ref`` against the definition, the
command line's ``--birth-complete``, ``inference.birth_complete`` of a config and its refusals, the log line, and the
binding's prototypes and record layout against the header."""
import ctypes
import importlib.util
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from birth_complete_ref import numpy_summary, select_minima_definition, select_minima_ref
from helpers import REPO
from mpp_cnn_rs_object_detection_amd import hip_api
from mpp_cnn_rs_object_detection_amd.mpp_model import MPPModel, check_birth_complete, format_complete_summary

NAN, INF = float("nan"), float("inf")


def same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2] == b[2]
    assert a[0].dtype == np.int32 and a[1].dtype == np.float64


# ---- the rule ---------------------------------------------------------------------------------------------------------------

def test_the_loop_equals_the_definition_on_random_maps():
    rng = np.random.default_rng(7)
    for shape, below, distance in [((23, 31), -0.5, 4.0), ((40, 17), 0.0, 2.5), ((12, 12), 5.0, 0.0), ((30, 30), -1.0, 100.0),
                                   ((9, 50), 0.2, 1.0)]:
        d = rng.normal(0.0, 1.0, shape)
        d[rng.integers(0, shape[0], 5), rng.integers(0, shape[1], 5)] = NAN
        d[rng.integers(0, shape[0], 3), rng.integers(0, shape[1], 3)] = -INF
        d = np.round(d, 1)                                   # many equal values: the index decides
        got = select_minima_ref(d, below, distance)
        same(got, select_minima_definition(d, below, distance))
        flat = got[0][:, 0].astype(np.int64) * shape[1] + got[0][:, 1]
        assert np.all(np.diff(flat) > 0)                     # ascending row-major order
        if distance == 0.0:                                  # every candidate stands alone
            assert len(got[0]) == got[2] == int(np.sum(d < below))


def test_the_rule_on_hand_made_maps():
    d = np.zeros((10, 12))
    d[2, 3], d[5, 7] = -1.0, -2.0                            # (3, 4): exactly 5 apart
    xy, v, n = select_minima_ref(d, 0.0, 5.0)
    assert xy.tolist() == [[5, 7]] and v.tolist() == [-2.0] and n == 2
    same((xy, v, n), select_minima_definition(d, 0.0, 5.0))
    d[:] = 0.0
    d[2, 3], d[3, 8] = -1.0, -2.0                            # (1, 5): d^2 = 26 = distance^2 + 1
    xy, v, n = select_minima_ref(d, 0.0, 5.0)
    assert xy.tolist() == [[2, 3], [3, 8]] and n == 2
    d[:] = 0.0
    d[4, 4], d[4, 6], d[1, 1] = -1.0, -1.0, -1.0             # equal values: the smaller index wins, the far one stands
    assert select_minima_ref(d, 0.0, 2.0)[0].tolist() == [[1, 1], [4, 4]]
    d[:] = 0.0
    d[3, 3], d[3, 4], d[7, 7], d[7, 8] = NAN, -1.0, -INF, -INF
    xy, v, n = select_minima_ref(d, 0.0, 1.0)
    assert xy.tolist() == [[3, 4], [7, 7]] and n == 3 and v[1] == -INF
    # the rule is order-free, not a walk: a < b < c in a row, each within reach of the next only -- b loses to a, c to b
    d[:] = 0.0
    d[0, 0], d[0, 2], d[0, 4] = -3.0, -2.0, -1.0
    assert select_minima_ref(d, 0.0, 2.0)[0].tolist() == [[0, 0]]
    assert select_minima_ref(np.ones((4, 5)), 0.0, 3.0)[0].shape == (0, 2)          # no candidate at all
    assert select_minima_ref(np.full((4, 5), NAN), 0.0, 3.0)[2] == 0


def test_the_summary_helper():
    d = np.array([[1.0, NAN, -2.0], [-2.0, 0.0, -INF]])
    assert numpy_summary(d) == (-INF, 1, 2, 3, 1)
    assert numpy_summary(np.full((2, 2), NAN)) == (INF, -1, -1, 0, 4)


# ---- the config key and the flag ------------------------------------------------------------------------------------------------

def config(value):
    return {"inference": {"birth_complete": value, "rjmcmc_params": {}}}


def test_the_config_key_is_read():
    assert check_birth_complete({}) is None and check_birth_complete({"inference": {}}) is None        # the default: off
    assert check_birth_complete(config(False)) is None and check_birth_complete(config(False), 4) is None
    assert check_birth_complete(config(True)) == {"max_rounds": 16, "min_gain": 0.0}
    assert check_birth_complete(config({})) == {"max_rounds": 16, "min_gain": 0.0}
    assert check_birth_complete(config({"max_rounds": 3})) == {"max_rounds": 3, "min_gain": 0.0}
    assert check_birth_complete(config({"max_rounds": 1024, "min_gain": 0.25})) == {"max_rounds": 1024, "min_gain": 0.25}
    assert check_birth_complete(config({"min_gain": 1})) == {"max_rounds": 16, "min_gain": 1.0}
    for bad in (1, 0, "true", None, 2.0, [3], {"rounds": 3}, {"max_rounds": 0}, {"max_rounds": 1025}, {"max_rounds": 2.0},
                {"max_rounds": True}, {"min_gain": -0.1}, {"min_gain": NAN}, {"min_gain": INF}, {"min_gain": "0"}):
        with pytest.raises(ValueError, match="birth_complete"):
            check_birth_complete(config(bad))


def test_ranks_that_share_an_image_refuse_it_before_any_collective():
    for on in (True, {"max_rounds": 2}):
        with pytest.raises(ValueError, match="birth_complete"):
            check_birth_complete(config(on), 2)
        stub = SimpleNamespace(config=config(on))            # (nothing but a config: a step further fails with AttributeError)
        for rank in (0, 1):
            with pytest.raises(ValueError, match="birth_complete"):
                MPPModel.infer_image(stub, None, rank, 2)
    with pytest.raises(AttributeError):
        MPPModel.infer_image(SimpleNamespace(config=config(False)), None, 0, 2)


def cli():
    spec = importlib.util.spec_from_file_location("mpp_main_cli_complete", os.path.join(REPO, "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_command_line_flag_reaches_the_config():
    main = cli()
    parser = main.build_parser()
    assert parser.parse_args([]).birth_complete is False
    for proc in ("infer", "infereval", "detect"):
        off = parser.parse_args(["-p", proc, "-m", "mpp", "-c", "x"])
        on = parser.parse_args(["-p", proc, "-m", "mpp", "-c", "x", "--birth-complete"])
        assert off.birth_complete is False and on.birth_complete is True
        assert main.apply_birth_complete(off, {"inference": {"figures": True}}) == {"inference": {"figures": True}}   # untouched
        assert main.apply_birth_complete(on, {}) == {"inference": {"birth_complete": True}}
        assert main.apply_birth_complete(on, config(False))["inference"]["birth_complete"] is True
        kept = main.apply_birth_complete(on, config({"max_rounds": 4}))
        assert kept["inference"]["birth_complete"] == {"max_rounds": 4}        # the config's parameters stay
        assert check_birth_complete(kept) == {"max_rounds": 4, "min_gain": 0.0}
    other = parser.parse_args(["-p", "eval", "-m", "mpp", "-c", "x", "--birth-complete"])
    assert main.apply_birth_complete(other, {}) == {}


def test_the_log_line():
    s = {"n_added": 7, "rounds": 3, "gain": -12.3456, "status": 0, "min_dE": 0.1, "argmin": (4, 5), "n_negative": 0, "n_nan": 0}
    assert format_complete_summary(s) == "birth completion: +7 object(s) in 3 round(s), energy -12.35, 0 pixel(s) still below 0"
    s.update(n_added=0, rounds=0, gain=0.0, n_negative=57)
    assert format_complete_summary(s) == "birth completion: +0 object(s) in 0 round(s), energy -0.00, 57 pixel(s) still below 0"


# ---- the binding ----------------------------------------------------------------------------------------------------------------

def test_header_prototypes_and_record_agree():
    text = open(os.path.join(REPO, "include", "mpp_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} mpp_complete_report;", text)
    want = "int32_t status, rounds, n_added, n_after; double gain, min_dE; int32_t x, y; int64_t n_negative, n_nan;"
    assert m and " ".join(m.group(1).split()) == want
    dt = hip_api.COMPLETE_REPORT_DTYPE

    class Rec(ctypes.Structure):
        _fields_ = [("status", ctypes.c_int32), ("rounds", ctypes.c_int32), ("n_added", ctypes.c_int32), ("n_after", ctypes.c_int32),
                    ("gain", ctypes.c_double), ("min_dE", ctypes.c_double), ("x", ctypes.c_int32), ("y", ctypes.c_int32),
                    ("n_negative", ctypes.c_int64), ("n_nan", ctypes.c_int64)]
    assert dt.names == tuple(n for n, _ in Rec._fields_)
    assert [dt.fields[n][1] for n in dt.names] == [getattr(Rec, n).offset for n in dt.names] == [0, 4, 8, 12, 16, 24, 32, 36, 40, 48]
    assert dt.itemsize == ctypes.sizeof(Rec) == 56
    assert [dt.fields[n][0].itemsize for n in dt.names] == [getattr(Rec, n).size for n in dt.names]

    flat = " ".join(text.split())
    assert ("int mpp_select_minima(mpp_ctx *ctx, int H, int W, int ld, const double *dE_dev, double below, double distance, int cap, "
            "int32_t *xy, double *values, int64_t *n_candidates, int64_t *n_kept);") in flat
    assert "int mpp_birth_complete(mpp_ctx *ctx, int max_rounds, double min_gain, mpp_complete_report *report);" in flat
    vp, i32, dbl, p64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_int64)
    assert hip_api.PROTOTYPES["mpp_select_minima"] == (i32, [vp, i32, i32, i32, vp, dbl, dbl, i32, vp, vp, p64, p64])
    assert hip_api.PROTOTYPES["mpp_birth_complete"] == (i32, [vp, i32, dbl, vp])
    assert {"mpp_select_minima", "mpp_birth_complete"} <= set(hip_api.ABI_SYMBOLS)
    assert (hip_api.COMPLETE_CONVERGED, hip_api.COMPLETE_ROUND_LIMIT, hip_api.COMPLETE_CAPACITY) == (0, 1, 2)
    # the change only adds symbols: the version the ABI test pins stays
    assert re.search(r'extern "C" int mpp_abi_version\(void\) \{ return 10; \}',
                     open(os.path.join(REPO, "mpp_cnn_rs_object_detection_amd", "csrc", "mpp_api.hip")).read())
