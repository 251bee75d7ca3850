"""The host side of the recombination of restarts (``inference.recombine``) where no GPU is needed: the
binding's prototypes and report layout against the header, the config check, the command-line flag, the summary and its log
line.  Every test here needs the feature: none can pass without ``mpp_recombine``."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import REPO
from mpp_cnn_rs_object_detection_amd import hip_api


def header():
    return open(os.path.join(REPO, "include", "mpp_hip.h")).read()


def test_the_binding_declares_both_entry_points_as_the_header_does():
    text = header()
    for name, n_args in (("mpp_recombine", 3), ("mpp_point_energies_all", 2)):
        assert name in hip_api.PROTOTYPES and name in hip_api.ABI_SYMBOLS
        res, args = hip_api.PROTOTYPES[name]
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        assert res is ctypes.c_int and len(args) == n_args == len(m.group(1).split(","))
        assert all(a is ctypes.c_void_p for a in args)            # (the context and pointers to host arrays)


def test_the_report_dtype_is_the_headers_struct():
    text = header()
    m = re.search(r"typedef struct \{([^}]*)\} mpp_recombine_report;", text)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), {"int32_t": "<i4", "double": "<f8"}[ctype]) for n in names.split(",")]
    dt = hip_api.RECOMBINE_REPORT_DTYPE
    assert [(n, dt.fields[n][0].str) for n in dt.names] == fields
    assert dt.itemsize == 48 and dt.fields["E_winner"][1] == 24   # six int32, then three doubles: no padding
    assert (hip_api.RECOMBINE_UNCHANGED, hip_api.RECOMBINE_DONE, hip_api.RECOMBINE_CAPACITY) == (0, 1, 2)
    bound = re.search(r"#define MPP_RECOMBINE_LDS_POINTS (\d+)", text)
    assert bound and int(bound.group(1)) == hip_api.RECOMBINE_LDS_POINTS


def test_the_library_exports_the_entry_points():
    from mpp_cnn_rs_object_detection_amd import build as hip_build
    L = ctypes.CDLL(hip_build.build())
    assert hasattr(L, "mpp_recombine") and hasattr(L, "mpp_point_energies_all")
    assert L.mpp_abi_version() == 10                              # the addition is additive


def test_check_recombine():
    from mpp_cnn_rs_object_detection_amd.mpp_model import check_recombine
    assert check_recombine({}) is False and check_recombine({"inference": {}}) is False
    assert check_recombine({"inference": {"restarts": 4}}) is False
    assert check_recombine({"inference": {"restarts": 1, "recombine": False}}) is False
    assert check_recombine({"inference": {"restarts": 2, "recombine": True}}) is True
    assert check_recombine({"inference": {"restarts": 2, "recombine": True, "tempering": True}}) is True
    with pytest.raises(ValueError, match="inference.restarts to 2 or more"):
        check_recombine({"inference": {"recombine": True}})
    with pytest.raises(ValueError, match="inference.restarts to 2 or more"):
        check_recombine({"inference": {"restarts": 1, "recombine": True}})
    with pytest.raises(ValueError, match="ranks share"):
        check_recombine({"inference": {"restarts": 2, "recombine": True}}, world_size=2)
    with pytest.raises(ValueError, match="ranks share"):             # (restarts alone refuses several ranks already)
        check_recombine({"inference": {"restarts": 2}}, world_size=4)
    for bad in (1, "yes", {"on": True}):
        with pytest.raises(ValueError, match="true or false"):
            check_recombine({"inference": {"restarts": 2, "recombine": bad}})


def test_the_summary_and_its_log_line():
    from mpp_cnn_rs_object_detection_amd.mpp_model import format_recombine_summary, recombine_summary

    class Sampler:
        recombine_report = np.zeros(5, hip_api.RECOMBINE_REPORT_DTYPE)
    rep = Sampler.recombine_report
    rep["status"] = [1, 0, 2, 1, 1]
    rep["n_clusters"] = [10, 7, 9, 4, 12]
    rep["n_taken"] = [3, 0, 5, 1, 2]
    rep["E_winner"] = [-30.0, -20.0, -10.0, -5.0, np.nan]
    rep["E_after"] = [-32.5, -20.0, -10.0, -5.25, -1.0]
    assert recombine_summary(None) is None and recombine_summary(object()) is None
    s = recombine_summary(Sampler, 0, 4)                          # the first image's four tiles
    assert set(s) == {"status", "n_clusters", "n_taken", "E_winner", "E_after"} and all(len(v) == 4 for v in s.values())
    assert format_recombine_summary(s) == "recombine: 9 of 30 cluster(s) in 2 of 4 tile(s) taken from another replica, energy -2.750"
    last = recombine_summary(Sampler, 4, 1)                       # a tile whose winner's energy is not finite adds no gain
    assert format_recombine_summary(last) == "recombine: 2 of 12 cluster(s) in 1 of 1 tile(s) taken from another replica, energy -0.000"
    assert len(recombine_summary(Sampler)["status"]) == 5
    s["status"][0] = 7
    assert rep["status"][0] == 1                                  # (copies: the pickle does not alias the sampler's array)


def test_the_command_line_flag():
    import main
    parser = main.build_parser()
    for procedure in ("infer", "infereval", "detect"):
        args = parser.parse_args(["-p", procedure, "-m", "mpp", "-c", "x", "--restarts", "4", "--recombine"])
        assert args.recombine is True
        assert main.apply_recombine(args, {"inference": {"restarts": 4}})["inference"]["recombine"] is True
        assert main.apply_recombine(args, {})["inference"] == {"recombine": True}
    args = parser.parse_args(["-p", "infer", "-m", "mpp", "-c", "x"])
    assert args.recombine is False and main.apply_recombine(args, {"inference": {}}) == {"inference": {}}
    args = parser.parse_args(["-p", "train", "-m", "mpp", "-c", "x", "--recombine"])
    assert main.apply_recombine(args, {}) == {}                   # (only the inference procedures read it)


def test_the_sampler_refuses_recombine_without_restarts_before_it_touches_a_device():
    from mpp_cnn_rs_object_detection_amd.sampler import TileBatchSampler, sample_rjmcmc_batch
    with pytest.raises(ValueError, match="restarts >= 2"):
        TileBatchSampler([], None, None, recombine=True)
    with pytest.raises(ValueError, match="restarts >= 2"):
        TileBatchSampler([], None, None, restarts=1, recombine=True)
    with pytest.raises(ValueError, match="restarts >= 2"):
        sample_rjmcmc_batch([], np.random.default_rng(0), 1, None, "naive", 1.0, 0.99, 10, None, 5, 0.0, recombine=True)
