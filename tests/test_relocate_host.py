"""The relocation's host-side rules: ``inference.relocate`` of a config and its refusals, the command line's ``--relocate``,
the log line, the binding's prototypes and record layout against the header, the selection distance, and -- on the CPU
oracle's float64 deltas -- the additivity of two moves further apart than that distance and the one-move-per-round walk of
state (m) back to the rendered objects."""
import ctypes
import importlib.util
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
import relocate_ref as RR
from descent_ref import select_points_ref
from helpers import REPO, hrc_model, log_model
from mpp_cnn_rs_object_detection_amd import energies as E
from mpp_cnn_rs_object_detection_amd import hip_api, synth
from mpp_cnn_rs_object_detection_amd.mpp_model import MPPModel, check_relocate, format_relocate_summary

NAN, INF = float("nan"), float("inf")
MAX_INTER = 32
MODELS = ["mpp_hrcM", "mpp_log"]
U = 2.0 ** -53


def model_desc(name):
    setup, comb = hrc_model() if name == "mpp_hrcM" else log_model()
    unit, pair = setup.make_energies()
    return E.build_model_desc(unit, pair, comb)


# ---- the config key and the flag ------------------------------------------------------------------------------------------------

def config(value, **more):
    return {"inference": dict({"relocate": value, "rjmcmc_params": {}}, **more)}


ALL = {"max_rounds": 16, "min_gain": 0.0, "radius": 2, "cycles": 4}


def test_the_config_key_is_read():
    assert check_relocate({}) is None and check_relocate({"inference": {}}) is None                    # the default: off
    assert check_relocate(config(False)) is None and check_relocate(config(False), 4) is None
    assert check_relocate(config(True)) == ALL and check_relocate(config({})) == ALL
    assert check_relocate(config({"radius": 7})) == dict(ALL, radius=7)
    assert check_relocate(config({"radius": 1, "cycles": 16})) == dict(ALL, radius=1, cycles=16)
    assert check_relocate(config({"max_rounds": 1024, "min_gain": 0.25})) == dict(ALL, max_rounds=1024, min_gain=0.25)
    assert check_relocate(config({"min_gain": 1, "cycles": 1})) == dict(ALL, min_gain=1.0, cycles=1)
    assert check_relocate(config(True, descent=True)) == ALL                                            # the two go together
    for bad in (1, 0, "true", None, 2.0, [3], {"rounds": 3}, {"max_rounds": 0}, {"max_rounds": 1025}, {"max_rounds": 2.0},
                {"max_rounds": True}, {"min_gain": -0.1}, {"min_gain": NAN}, {"min_gain": INF}, {"min_gain": "0"},
                {"radius": 0}, {"radius": 8}, {"radius": 2.0}, {"radius": True}, {"radius": "2"}, {"cycles": 0}, {"cycles": 17},
                {"cycles": 1.5}, {"cycles": False}, {"births": True}):
        with pytest.raises(ValueError, match="relocate"):
            check_relocate(config(bad))


def test_ranks_that_share_an_image_refuse_it_before_any_collective():
    for on in (True, {"radius": 3}):
        with pytest.raises(ValueError, match="relocate"):
            check_relocate(config(on), 2)
        stub = SimpleNamespace(config=config(on))                # (nothing but a config: a step further fails with AttributeError)
        for rank in (0, 1):
            with pytest.raises(ValueError, match="relocate"):
                MPPModel.infer_image(stub, None, rank, 2)
    with pytest.raises(AttributeError):
        MPPModel.infer_image(SimpleNamespace(config=config(False)), None, 0, 2)


def cli():
    spec = importlib.util.spec_from_file_location("mpp_main_cli_relocate", os.path.join(REPO, "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_command_line_flag_reaches_the_config():
    main = cli()
    parser = main.build_parser()
    assert parser.parse_args([]).relocate is None
    for proc in ("infer", "infereval", "detect"):
        off = parser.parse_args(["-p", proc, "-m", "mpp", "-c", "x"])
        on = parser.parse_args(["-p", proc, "-m", "mpp", "-c", "x", "--relocate"])
        r3 = parser.parse_args(["-p", proc, "-m", "mpp", "-c", "x", "--relocate", "3"])
        assert off.relocate is None and on.relocate is True and r3.relocate == 3 and on.descent is False
        assert main.apply_relocate(off, {"inference": {"figures": True}}) == {"inference": {"figures": True}}         # untouched
        assert main.apply_relocate(on, {}) == {"inference": {"relocate": True}}
        assert main.apply_relocate(on, config(False))["inference"]["relocate"] is True
        kept = main.apply_relocate(on, config({"max_rounds": 4, "radius": 5}))
        assert kept["inference"]["relocate"] == {"max_rounds": 4, "radius": 5}       # the config's parameters stay
        assert check_relocate(kept) == dict(ALL, max_rounds=4, radius=5)
        assert main.apply_relocate(r3, {}) == {"inference": {"relocate": {"radius": 3}}}
        assert check_relocate(main.apply_relocate(r3, config({"max_rounds": 4, "radius": 5}))) == dict(ALL, max_rounds=4, radius=3)
    for bad in ("0", "8", "x"):
        with pytest.raises(SystemExit):
            parser.parse_args(["-p", "infer", "-m", "mpp", "-c", "x", "--relocate", bad])
    other = parser.parse_args(["-p", "eval", "-m", "mpp", "-c", "x", "--relocate"])
    assert main.apply_relocate(other, {}) == {}


def test_the_log_line():
    s = {"n_moved": 7, "rounds": 3, "gain": 12.3456, "n_positive": 0}
    assert format_relocate_summary(s) == "relocation: ~7 object(s) in 3 round(s), energy -12.35, 0 point(s) above 0"
    s.update(n_moved=0, rounds=0, gain=0.0, n_positive=2)
    assert format_relocate_summary(s) == "relocation: ~0 object(s) in 0 round(s), energy -0.00, 2 point(s) above 0"


# ---- the binding ----------------------------------------------------------------------------------------------------------------

def test_header_prototypes_and_record_agree():
    text = open(os.path.join(REPO, "include", "mpp_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} mpp_relocate_report;", text)
    assert m and " ".join(m.group(1).split()) == ("int32_t status, rounds, n_moved, n_after, slot_max, n_positive; "
                                                  "double gain, max_gain;")
    dt, Rec = hip_api.RELOCATE_REPORT_DTYPE, hip_api.RelocateReportC
    assert dt.names == tuple(n for n, _ in Rec._fields_)
    assert [dt.fields[n][1] for n in dt.names] == [getattr(Rec, n).offset for n in dt.names] == [0, 4, 8, 12, 16, 20, 24, 32]
    assert dt.itemsize == ctypes.sizeof(Rec) == 40
    assert [dt.fields[n][0].itemsize for n in dt.names] == [getattr(Rec, n).size for n in dt.names]
    flat = " ".join(text.split())
    assert f"#define MPP_MOVE_CHUNK {hip_api.MOVE_CHUNK} " in flat and f"#define MPP_MOVE_RADIUS_MAX {hip_api.MOVE_RADIUS_MAX} " in flat
    assert "int mpp_move_gains(mpp_ctx *ctx, int radius, double *gain, int32_t *to);" in flat
    assert ("int mpp_relocate(mpp_ctx *ctx, int radius, int max_rounds, double min_gain, mpp_relocate_report *report, "
            "int32_t *moved_or_null);") in flat
    vp, i, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert hip_api.PROTOTYPES["mpp_move_gains"] == (i, [vp, i, vp, vp])
    assert hip_api.PROTOTYPES["mpp_relocate"] == (i, [vp, i, i, dbl, vp, vp])
    assert {"mpp_move_gains", "mpp_relocate"} <= set(hip_api.ABI_SYMBOLS)
    assert (hip_api.RELOCATE_FIXED_POINT, hip_api.RELOCATE_ROUND_LIMIT) == (0, 1)
    # the change only adds symbols: the version the ABI test pins stays, and the descent's record is untouched
    assert re.search(r'extern "C" int mpp_abi_version\(void\) \{ return 10; \}',
                     open(os.path.join(REPO, "mpp_cnn_rs_object_detection_amd", "csrc", "mpp_api.hip")).read())
    assert hip_api.DESCENT_REPORT_DTYPE.itemsize == 88


def test_the_selection_distance():
    for radius in range(1, 8):
        d = hip_api.relocate_distance(MAX_INTER, radius)
        assert d == RR.distance(MAX_INTER, radius) == 2.0 * (32.0 + radius * np.sqrt(2.0))
        # two windows' farthest pixels plus both interaction ranges
        assert d >= 2 * MAX_INTER + 2 * np.hypot(radius, radius) - 1e-12
    assert np.hypot(40, 48) < RR.distance(MAX_INTER, 2) < np.hypot(160, 160)


# ---- the rule on the CPU oracle ---------------------------------------------------------------------------------------------------

def oracle_gains(o, xy, cand, radius, shape):
    """per point: (window pixels, g = -delta of the replacement by the pixel's candidate) from the oracle's from-scratch delta"""
    out = []
    for i, v in enumerate(xy):
        pix = RR.window_pixels(v, radius, shape)
        out.append((pix, np.array([-o.delta([i], c[None], cand[c[0], c[1]][None]) for c in pix])))
    return out


@pytest.mark.parametrize("name", MODELS)
def test_state_m_walks_back_to_the_objects_one_move_per_round(name):
    from test_gpu_birth_map import GT_MARKS, GT_XY, H, W, host_candidate_marks, point_energy_bound, tile_maps
    det, marks = tile_maps()
    cand = host_candidate_marks(marks)
    o = oracle.Oracle((H, W), det, marks, model_desc(name))
    xy, mk = RR.state_m(GT_XY, GT_MARKS)
    o.set_points(xy, mk)
    e0, total, rounds = o.total_energy(), 0.0, 0
    while True:
        gains = oracle_gains(o, xy, cand, 2, (H, W))
        best = np.array([g.max() for _, g in gains])
        to = np.array([pix[int(np.argmax(g))] for pix, g in gains])
        if rounds == 0:
            print(f"state (m), {name}: first gains {np.round(best, 3).tolist()}")
            assert np.all(best > 0)
        keep, _ = select_points_ref(xy, best, 0.0, RR.distance(MAX_INTER, 2))
        idx = np.flatnonzero(keep)
        if len(idx) == 0:
            break
        assert len(idx) == 1                                 # the tile's diagonal is shorter than the distance
        total += float(best[idx[0]])
        xy[idx], mk[idx] = to[idx], cand[to[idx, 0], to[idx, 1]]
        o.set_points(xy, mk)
        rounds += 1
        assert rounds <= 16
    print(f"state (m), {name}: {rounds} rounds, sum of gains {total!r}, E0 - E1 {e0 - o.total_energy()!r}")
    assert rounds == 5
    np.testing.assert_array_equal(xy, GT_XY)
    desc = model_desc(name)
    B = 2.0 if desc.combinator == E.C_LOGISTIC else 2.0 * point_energy_bound(desc, det, mk)
    assert abs(total - (e0 - o.total_energy())) <= RR.walk_bound(len(xy), rounds, B)


@pytest.mark.parametrize("name", MODELS)
def test_two_moves_out_of_reach_add_up(name):
    from test_gpu_birth_map import host_candidate_marks, point_energy_bound
    desc = model_desc(name)
    det, marks, xy, mk = RR.shifted_scene()
    cand = host_candidate_marks(marks)
    o = oracle.Oracle((160, 160), det, marks, desc)
    o.set_points(xy, mk)
    gains = oracle_gains(o, xy, cand, 2, (160, 160))
    to = np.array([pix[int(np.argmax(g))] for pix, g in gains])
    single = np.array([-g.max() for _, g in gains])          # the delta of each point's best move alone
    n = len(xy)
    # both sides sum at most n + 2 terms of magnitude B in different orders (the module docstring of test_gpu_relocate)
    B = 2.0 if desc.combinator == E.C_LOGISTIC else 2.0 * point_energy_bound(desc, det, mk)
    m = n + 2
    bound = 2.0 * 2.0 * (m - 1) * U / (1.0 - (m - 1) * U) * m * B
    d2 = RR.distance(MAX_INTER, 2) ** 2
    far, near_err, worst = 0, 0.0, 0.0
    for i in range(n):
        for j in range(i + 1, n):
            both = o.delta([i, j], to[[i, j]], cand[to[[i, j], 0], to[[i, j], 1]])
            err = abs(both - (single[i] + single[j]))
            if float(((xy[i].astype(np.int64) - xy[j]) ** 2).sum()) > d2:
                far, worst = far + 1, max(worst, err)
                assert err <= bound, (i, j, err, bound)
            else:
                near_err = max(near_err, err)
    print(f"{name}: {far} pairs out of reach, max |joint - sum| {worst!r} (bound {bound!r}); within reach up to {near_err!r}")
    assert far >= 10 and near_err > bound                    # the distance matters: pairs within reach do not add up
