"""Steps that propose the values their target already holds, counted on the CPU oracle's own chains (tests/same_value_cases.py).
No GPU.

The bench chain's counts are the table the skip of such steps in the deep-round kernel was estimated from
(profiles/deep_skip_same.md): they are pinned.  The chains of tests/test_gpu_deep_skip_same.py are held to floors: a case whose
chain holds no such step would compare two runs that never skip.  The floors are conditions on the cases, not measurements."""
import numpy as np
import pytest

import same_value_cases as sv
from mpp_cnn_rs_object_detection_amd import kernels as K


def test_the_bench_chain_from_its_handover_on():
    c = sv.bench_chain_counts()
    assert (c[K.K_DTRANSF]["steps"], c[K.K_DTRANSF]["same"], c[K.K_DTRANSF]["changing"]) == (21730, 17229, 1145)
    assert (c[K.K_DTRANS]["steps"], c[K.K_DTRANS]["same"], c[K.K_DTRANS]["changing"]) == (21754, 1473, 333)
    assert (c[K.K_GTRANS]["steps"], c[K.K_GTRANS]["same"], c[K.K_GTRANS]["changing"]) == (10759, 411, 94)
    assert sum(v["steps"] for v in c.values()) == 97307
    assert sum(v["same"] for v in c.values()) == 19113 and sum(v["changing"] for v in c.values()) == 3098
    assert all(c[k]["same"] == 0 for k in sv.BIRTHS + sv.DEATHS)


@pytest.mark.parametrize("name", sv.CASES)
def test_every_gpu_case_holds_such_steps(name):
    c = sv.case_counts(name)
    assert c[K.K_DTRANSF]["same"] >= 100, c
    assert sum(c[k]["same"] for k in sv.TRANSLATIONS) >= 5, c
    assert sum(v["changing"] for v in c.values()) > 0, c        # (and the chain moves: the runs compared are not all rejects)


def test_what_the_cases_are_there_for():
    # off-class: no initial mark is the edge of its class, so the first transform into a mark's own class changes the value
    b = sv.build("off-class")
    for j, m in enumerate(b.maps):
        assert not np.isin(b.mk[:, j], np.asarray(m.feature_mapping)).any()
    assert sv.case_counts("off-class")[K.K_DTRANSF]["own_class_moved"] >= 20
    assert sv.case_counts("tile112")[K.K_DTRANSF]["own_class_moved"] < sv.case_counts("off-class")[K.K_DTRANSF]["own_class_moved"]
    # contrast: the NaN rule is at work; empty: steps are drawn without a target; capacity: a cell of the 32-px grid gets crowded
    out, _, _ = sv.oracle_chain("contrast")
    assert int(np.isnan(out["dE"]).sum()) > 1000
    out, _, _ = sv.oracle_chain("empty")
    n_before = np.concatenate([[0], out["n_after"][:-1]])
    assert int((n_before == 0).sum()) >= 50
    out, _, fin = sv.oracle_chain("capacity")
    cells = fin[0] // 32
    assert int(out["n_after"].max()) > 40 and np.unique(cells, axis=0, return_counts=True)[1].max() > 3
