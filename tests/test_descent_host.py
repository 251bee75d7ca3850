"""The local descent's host-side rules: the selection rule among points (``descent_ref.select_points_ref``) against the
definition, the death walk on the CPU oracle's float64 Papangelou values for the two states the GPU tests use, the command
line's ``--descent``, ``inference.descent`` of a config and its refusals, the log line, and the binding's prototypes and
record layout against the header."""
import ctypes
import importlib.util
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from descent_ref import death_walk, papangelou_summary, select_points_definition, select_points_ref, state_d
from helpers import REPO, hrc_model, log_model
from mpp_cnn_rs_object_detection_amd import energies as E
from mpp_cnn_rs_object_detection_amd import hip_api, synth
from mpp_cnn_rs_object_detection_amd.mpp_model import MPPModel, check_descent, format_descent_summary

NAN, INF = float("nan"), float("inf")
MAX_INTER = 32
MODELS = ["mpp_hrcM", "mpp_log"]


# ---- the rule ---------------------------------------------------------------------------------------------------------------

def test_the_loop_equals_the_definition_on_random_lists():
    rng = np.random.default_rng(11)
    for n, side, above, distance in [(60, 12, 0.0, 4.0), (200, 40, -0.5, 2.5), (90, 9, 0.3, 0.0), (120, 30, 0.0, 100.0),
                                     (75, 50, 1.0, 1.0), (1, 5, 0.0, 3.0), (0, 5, 0.0, 3.0)]:
        xy = rng.integers(0, side, (n, 2))                       # (more points than pixels in some: duplicates on one pixel)
        v = np.round(rng.normal(0.0, 1.0, n), 1)                 # many equal values: the slot decides
        if n > 10:
            v[rng.integers(0, n, 4)] = NAN
            v[rng.integers(0, n, 3)] = INF
            xy[1] = xy[0]
            v[1] = v[0] = 2.0                                    # equal values on one pixel
        keep, n_cand = select_points_ref(xy, v, above, distance)
        keep2, n_cand2 = select_points_definition(xy, v, above, distance)
        np.testing.assert_array_equal(keep, keep2)
        assert n_cand == n_cand2 == int(np.sum(v > above)) and keep.dtype == np.uint8 and len(keep) == n
        assert not np.any(keep[np.isnan(v)]) and not np.any(keep[~(v > above)])
        if distance == 0.0 and n > 10:                           # only points of one pixel are rivals
            assert keep[0] == 1 and keep[1] == 0


def test_the_rule_on_hand_made_lists():
    sel = lambda xy, v, above, d: select_points_ref(np.array(xy).reshape(-1, 2), np.array(v, float), above, d)[0].tolist()
    assert sel([[5, 3], [5, 67]], [1.0, 2.0], 0.0, 64.0) == [0, 1]                   # exactly 64 apart: only the better one
    assert sel([[140, 60], [141, 124]], [3.0, 4.0], 0.0, 64.0) == [1, 1]             # d^2 = 64^2 + 1: both
    assert sel([[2, 3], [5, 7]], [1.0, 2.0], 0.0, 5.0) == [0, 1]                     # the 3-4-5 edge
    assert sel([[2, 3], [3, 8]], [1.0, 2.0], 0.0, 5.0) == [1, 1]                     # (1, 5): 26 = 5^2 + 1
    assert sel([[4, 4], [4, 4]], [1.0, 1.0], 0.0, 3.0) == [1, 0]                     # equal values on one pixel: the smaller slot
    assert sel([[4, 4], [4, 4]], [1.0, 1.0], 0.0, 0.0) == [1, 0]                     # ... at distance 0 too
    assert sel([[1, 1], [1, 2], [9, 9], [9, 9]], [NAN, 1.0, INF, 5.0], 0.0, 1.0) == [0, 1, 1, 0]
    # order-free, not a walk: b loses to a and c to b although a does not reach c
    assert sel([[1, 0], [1, 2], [1, 4]], [3.0, 2.0, 1.0], 0.0, 2.0) == [1, 0, 0]
    assert sel([[1, 0], [1, 2], [1, 4]], [3.0, 2.0, 1.0], 3.0, 2.0) == [0, 0, 0]     # above every value (3.0 > 3.0 is false)
    assert sel([[1, 0], [1, 2], [1, 4]], [3.0, 2.0, 1.0], 0.0, 0.0) == [1, 1, 1]     # distance 0 on distinct pixels
    keep, n = select_points_ref(np.zeros((0, 2), int), np.zeros(0), 0.0, 3.0)
    assert keep.shape == (0,) and n == 0


def test_the_summary_helper():
    assert papangelou_summary([1.0, NAN, 3.0, 3.0, -2.0]) == (3.0, 2, 3)
    assert papangelou_summary([]) == (-INF, -1, 0) and papangelou_summary([NAN]) == (-INF, -1, 0)
    assert papangelou_summary([-INF, NAN]) == (-INF, 0, 0)


# ---- the death walk on the oracle's values ------------------------------------------------------------------------------------

def model_desc(name):
    setup, comb = hrc_model() if name == "mpp_hrcM" else log_model()
    unit, pair = setup.make_energies()
    return E.build_model_desc(unit, pair, comb)


def oracle_source(shape, det, marks, desc):
    o = oracle.Oracle(shape, det, marks, desc)

    def papangelou_of(xy, mk):
        o.set_points(xy, mk)
        return o.papangelou()
    return papangelou_of


def assert_rounds_are_sparse(per_round):
    for _, rxy, _ in per_round:
        p = rxy.astype(np.int64)
        d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        d2[np.arange(len(p)), np.arange(len(p))] = 1 << 40
        assert len(p) >= 1 and d2.min() > (2 * MAX_INTER) ** 2


@pytest.mark.parametrize("name", MODELS)
def test_state_b_loses_nine_points_one_per_round(name):
    from test_gpu_birth_map import H, POINT_MARKS, POINTS, W, tile_maps
    det, marks = tile_maps()
    assert (H - 1) ** 2 + (W - 1) ** 2 < (2 * MAX_INTER) ** 2        # the tile's diagonal: one removal per round
    source = oracle_source((H, W), det, marks, model_desc(name))
    first = source(POINTS, POINT_MARKS)
    assert int(np.sum(first > 0)) == (9 if name == "mpp_hrcM" else 10)
    walk = death_walk(source, POINTS, POINT_MARKS, MAX_INTER)
    print(f"state (b), {name}: -{walk['n_removed']} in {walk['rounds']} round(s), gain {walk['gain_deaths']!r}")
    assert (walk["status"], walk["n_removed"], walk["rounds"], len(walk["xy"])) == (0, 9, 9, 3)
    assert all(len(g[0]) == 1 for g in walk["per_round"])
    np.testing.assert_array_equal(walk["xy"], POINTS[walk["src"]])
    assert np.all(np.diff(walk["src"]) > 0)                          # the survivors keep their order
    assert not np.any(source(walk["xy"], walk["marks"]) > 0)         # a fixed point of the rule
    assert walk["gain_deaths"] > 0


@pytest.mark.parametrize("name", MODELS)
def test_state_d_loses_thirty_points_two_in_some_rounds(name):
    det, marks, xy, mk = state_d(synth.render_maps, synth.make_gt)
    assert xy.shape == (50, 2) and mk.shape == (50, 3)
    source = oracle_source((96, 96), det, marks, model_desc(name))
    walk = death_walk(source, xy, mk, MAX_INTER, max_rounds=64)
    sizes = [len(g[0]) for g in walk["per_round"]]
    print(f"state (d), {name}: -{walk['n_removed']} in {walk['rounds']} round(s), per round {sizes}")
    assert (walk["status"], walk["n_removed"], len(walk["xy"])) == (0, 30, 20)
    assert walk["rounds"] == (22 if name == "mpp_hrcM" else 27) and max(sizes) == 2 and sizes.count(2) >= 2
    assert_rounds_are_sparse(walk["per_round"])
    assert not np.any(source(walk["xy"], walk["marks"]) > 0)
    assert death_walk(source, xy, mk, MAX_INTER, max_rounds=16)["status"] == 1      # the default 16 rounds do not finish it


# ---- the config key and the flag ------------------------------------------------------------------------------------------------

def config(value, **more):
    return {"inference": dict({"descent": value, "rjmcmc_params": {}}, **more)}


ALL = {"max_rounds": 16, "min_gain": 0.0, "births": True, "deaths": True}


def test_the_config_key_is_read():
    assert check_descent({}) is None and check_descent({"inference": {}}) is None                      # the default: off
    assert check_descent(config(False)) is None and check_descent(config(False), 4) is None
    assert check_descent(config(False, birth_complete=True)) is None
    assert check_descent(config(True)) == ALL and check_descent(config({})) == ALL
    assert check_descent(config({"max_rounds": 3})) == dict(ALL, max_rounds=3)
    assert check_descent(config({"max_rounds": 1024, "min_gain": 0.25})) == dict(ALL, max_rounds=1024, min_gain=0.25)
    assert check_descent(config({"min_gain": 1, "births": False})) == dict(ALL, min_gain=1.0, births=False)
    assert check_descent(config({"deaths": False})) == dict(ALL, deaths=False)
    assert check_descent(config(True, birth_complete=False)) == ALL
    for bad in (1, 0, "true", None, 2.0, [3], {"rounds": 3}, {"max_rounds": 0}, {"max_rounds": 1025}, {"max_rounds": 2.0},
                {"max_rounds": True}, {"min_gain": -0.1}, {"min_gain": NAN}, {"min_gain": INF}, {"min_gain": "0"},
                {"births": 1}, {"deaths": "no"}, {"births": False, "deaths": False}):
        with pytest.raises(ValueError, match="descent"):
            check_descent(config(bad))
    for on in (True, {"max_rounds": 2}):                             # the descent contains the completion
        for complete in (True, {"max_rounds": 4}):
            with pytest.raises(ValueError, match="descent contains the completion"):
                check_descent(config(on, birth_complete=complete))


def test_ranks_that_share_an_image_refuse_it_before_any_collective():
    for on in (True, {"deaths": False}):
        with pytest.raises(ValueError, match="descent"):
            check_descent(config(on), 2)
        stub = SimpleNamespace(config=config(on))                # (nothing but a config: a step further fails with AttributeError)
        for rank in (0, 1):
            with pytest.raises(ValueError, match="descent"):
                MPPModel.infer_image(stub, None, rank, 2)
    with pytest.raises(AttributeError):
        MPPModel.infer_image(SimpleNamespace(config=config(False)), None, 0, 2)
    with pytest.raises(ValueError, match="descent contains the completion"):
        MPPModel.infer_image(SimpleNamespace(config=config(True, birth_complete=True)), None, 0, 1)


def cli():
    spec = importlib.util.spec_from_file_location("mpp_main_cli_descent", os.path.join(REPO, "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_command_line_flag_reaches_the_config():
    main = cli()
    parser = main.build_parser()
    assert parser.parse_args([]).descent is False
    for proc in ("infer", "infereval", "detect"):
        off = parser.parse_args(["-p", proc, "-m", "mpp", "-c", "x"])
        on = parser.parse_args(["-p", proc, "-m", "mpp", "-c", "x", "--descent"])
        assert off.descent is False and on.descent is True and on.birth_complete is False
        assert main.apply_descent(off, {"inference": {"figures": True}}) == {"inference": {"figures": True}}          # untouched
        assert main.apply_descent(on, {}) == {"inference": {"descent": True}}
        assert main.apply_descent(on, config(False))["inference"]["descent"] is True
        kept = main.apply_descent(on, config({"max_rounds": 4, "births": False}))
        assert kept["inference"]["descent"] == {"max_rounds": 4, "births": False}    # the config's parameters stay
        assert check_descent(kept) == dict(ALL, max_rounds=4, births=False)
    other = parser.parse_args(["-p", "eval", "-m", "mpp", "-c", "x", "--descent"])
    assert main.apply_descent(other, {}) == {}


def test_the_log_line():
    s = {"n_added": 7, "n_removed": 4, "rounds": 3, "gain": -12.3456, "n_negative": 0, "n_positive": 0}
    assert format_descent_summary(s) == ("descent: +7 -4 object(s) in 3 round(s), energy -12.35, 0 pixel(s) below 0, "
                                         "0 point(s) above 0")
    s.update(n_added=0, n_removed=0, rounds=0, gain=0.0, n_negative=57, n_positive=2)
    assert format_descent_summary(s) == ("descent: +0 -0 object(s) in 0 round(s), energy -0.00, 57 pixel(s) below 0, "
                                         "2 point(s) above 0")


# ---- the binding ----------------------------------------------------------------------------------------------------------------

def test_header_prototypes_and_record_agree():
    text = open(os.path.join(REPO, "include", "mpp_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} mpp_descent_report;", text)
    want = ("int32_t status, rounds, n_added, n_removed, n_after, slot_max; double gain_births, gain_deaths, max_p, min_dE; "
            "int32_t x, y; int64_t n_positive, n_negative, n_nan;")
    assert m and " ".join(m.group(1).split()) == want
    dt = hip_api.DESCENT_REPORT_DTYPE
    i32, f64, i64 = ctypes.c_int32, ctypes.c_double, ctypes.c_int64

    class Rec(ctypes.Structure):
        _fields_ = [("status", i32), ("rounds", i32), ("n_added", i32), ("n_removed", i32), ("n_after", i32), ("slot_max", i32),
                    ("gain_births", f64), ("gain_deaths", f64), ("max_p", f64), ("min_dE", f64), ("x", i32), ("y", i32),
                    ("n_positive", i64), ("n_negative", i64), ("n_nan", i64)]
    assert dt.names == tuple(n for n, _ in Rec._fields_)
    assert [dt.fields[n][1] for n in dt.names] == [getattr(Rec, n).offset for n in dt.names] == \
        [0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56, 60, 64, 72, 80]
    assert dt.itemsize == ctypes.sizeof(Rec) == 88
    assert [dt.fields[n][0].itemsize for n in dt.names] == [getattr(Rec, n).size for n in dt.names]

    flat = " ".join(text.split())
    assert "#define MPP_DESCEND_DEATHS 1 #define MPP_DESCEND_BIRTHS 2" in flat
    assert "int mpp_papangelou_all(mpp_ctx *ctx, double *dE);" in flat
    assert ("int mpp_select_points(mpp_ctx *ctx, int n, const int32_t *xy_dev, const double *values_dev, double above, "
            "double distance, uint8_t *keep_dev, int64_t *n_candidates, int64_t *n_kept);") in flat
    assert ("int mpp_descend(mpp_ctx *ctx, int what, int max_rounds, double min_gain, mpp_descent_report *report, "
            "int32_t *src_or_null);") in flat
    vp, i, dbl, p64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_int64)
    assert hip_api.PROTOTYPES["mpp_papangelou_all"] == (i, [vp, vp])
    assert hip_api.PROTOTYPES["mpp_select_points"] == (i, [vp, i, vp, vp, dbl, dbl, vp, p64, p64])
    assert hip_api.PROTOTYPES["mpp_descend"] == (i, [vp, i, i, dbl, vp, vp])
    assert {"mpp_papangelou_all", "mpp_select_points", "mpp_descend"} <= set(hip_api.ABI_SYMBOLS)
    assert (hip_api.DESCEND_DEATHS, hip_api.DESCEND_BIRTHS) == (1, 2)
    assert (hip_api.DESCENT_FIXED_POINT, hip_api.DESCENT_ROUND_LIMIT, hip_api.DESCENT_CAPACITY) == (0, 1, 2)
    # the change only adds symbols: the version the ABI test pins stays
    assert re.search(r'extern "C" int mpp_abi_version\(void\) \{ return 10; \}',
                     open(os.path.join(REPO, "mpp_cnn_rs_object_detection_amd", "csrc", "mpp_api.hip")).read())
