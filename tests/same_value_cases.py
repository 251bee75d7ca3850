"""Steps that re-write a point with the values it already holds (host side: no GPU is used here).

A move / transform whose proposal equals its target in all five values -- pixel, size, ratio, angle -- leaves the
configuration as it is, accepted or not.  The deep-round kernel does not evaluate such a step in an untraced chain
(csrc/mpp_deep.hip, ``deep_same_values``; option ``deep_skip_same``).  ``count`` walks the oracle's trace of a chain, keeping
``order[]`` and the five values of every point as the kernels keep them (tests/hot_commit_walk.py does the same for the
pixels), and counts per kernel type the proposals identical to their target -- compared on the VALUES, as the kernel does.

``CASES`` are the chains of tests/test_gpu_deep_skip_same.py; tests/test_same_value_cases_host.py holds each of them to a
floor of such steps, so that no case compares two runs that never skip."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

import hot_commit_walk as hw
from helpers import model_for
from mpp_cnn_rs_object_detection_amd import kernels, mappings, synth

K = kernels
BIRTHS, DEATHS = (K.K_UBIRTH, K.K_DBIRTH), (K.K_UDEATH, K.K_DDEATH)
TRANSLATIONS = (K.K_GTRANS, K.K_DTRANS)


def count(props, out, xy0, mk0, first=0, maps=None):
    """-> {kernel: dict(steps, same, changing)} over the steps from `first` on: steps of that kernel type, proposals identical
    to their target, accepted steps that change the configuration.  With `maps` (the mark mappings) also ``own_class_moved``:
    data-driven transforms that draw the class their mark sits in and yet propose another value -- the mark was off the edge"""
    order = list(range(len(xy0)))
    val = {i: (int(xy0[i][0]), int(xy0[i][1]), float(mk0[i][0]), float(mk0[i][1]), float(mk0[i][2])) for i in range(len(xy0))}
    next_id = len(order)
    c = {k: dict(steps=0, same=0, changing=0) for k in range(8)}
    if maps is not None:
        c[K.K_DTRANSF]["own_class_moved"] = 0
    kern, targ, acc = props["kernel"], props["target"], out["accepted"]
    for st in range(len(props)):
        k, a, t = int(kern[st]), bool(acc[st]), int(targ[st])
        late = st >= first
        c[k]["steps"] += late
        new = (int(props["ax"][st]), int(props["ay"][st]), float(props["as"][st]), float(props["ar"][st]), float(props["aa"][st]))
        if k in BIRTHS:
            if a:
                order.append(next_id); val[next_id] = new; next_id += 1
                c[k]["changing"] += late
        elif t >= 0:
            slot = order[t]
            if k in DEATHS:
                if a:
                    order[t] = order[-1]; order.pop(); del val[slot]
                    c[k]["changing"] += late
            else:
                same = val[slot] == new
                c[k]["same"] += late and same
                if maps is not None and k == K.K_DTRANSF:
                    pid = int(props["param_id"][st])
                    cls = int(np.searchsorted(np.asarray(maps[pid].feature_mapping), val[slot][2 + pid], side="right")) - 1
                    c[k]["own_class_moved"] += late and not same and int(props["new_class"][st]) == max(cls, 0)
                if a and not same:
                    val[slot] = new
                    c[k]["changing"] += late
    assert len(order) == int(out["n_after"][-1])
    return c


def bench_chain_counts(n_steps=100001, first=2694):
    """the chain bench.py times (512 x 512, 200 objects, seed 0), from the step at which its hot start hands over"""
    props, out, xy0, _, _ = hw.oracle_trace(512, 200, n_steps, seed=0, T0=1.0, alpha=0.999)
    t = synth.make_tile(512, 200, tile_id=0)
    import oracle
    setup, _, model = model_for("legacy")
    o = oracle.Oracle(t.shape, t.det, t.marks, model, kernels.make_kernels(mappings.default_mappings(), 1.0))
    _, mk0 = o.naive_detection(setup.detection_threshold, 6.0)
    return count(props, out, xy0, np.asarray(mk0).reshape(-1, 3), first)


# ---- the GPU cases ------------------------------------------------------------------------------------------------------
@dataclass
class Built:
    name: str
    shape: tuple
    det: np.ndarray
    marks: list
    maps: list
    model: object
    kd: object
    xy: np.ndarray
    mk: np.ndarray
    T0: float
    alpha: float
    steps: int
    seed: int
    chain: int = 0
    image: Optional[np.ndarray] = None      # the picture of a classic image energy


# At T0 = 5 nearly every proposal is accepted and the marks wander: a data-driven transform re-writes its mark only when the
# mark sits on a class edge AND the row draws that class again -- 3 % of them where the mark maps are flat.  The cases that are
# hot, or small enough for the population to collapse, therefore run a mixture that is mostly data-driven transform (about
# three steps in four; a Gaussian transform, which moves a mark off the edges, one in 55), with twice the usual share of
# translations.  Seeds were chosen on the oracle so that every case meets the floors of tests/test_same_value_cases_host.py.
TRANSFORM_HEAVY = dict(transformation_weight=14, gaussian_transformation_weight=0.1, data_transformation_weight=4, translation_weight=2)


def _synthetic(name, tile, n_obj, T0, alpha, steps, seed, tile_id=0, intensity=None, chain=0, weights=TRANSFORM_HEAVY):
    """a synthetic tile from its naive initialisation, as tests/test_gpu_chain.py's setup_case builds it"""
    import oracle
    t = synth.make_tile(tile, n_obj, tile_id=tile_id, noise=0.1)
    setup, _, model = model_for("legacy")
    maps = mappings.default_mappings()
    o = oracle.Oracle(t.shape, t.det, t.marks, model, kernels.make_kernels(maps, 1.0))
    xy, mk = o.naive_detection(setup.detection_threshold, 6.0)
    kd = kernels.make_kernels(maps, float(max(1, len(xy))) if intensity is None else intensity,
                              kernel_weights=dict(kernels.BASE_KERNEL_WEIGHTS, **(weights or {})))
    return Built(name, t.shape, t.det, list(t.marks), maps, model, kd, np.asarray(xy, np.int32).reshape(-1, 2),
                 np.asarray(mk, np.float64).reshape(-1, 3), T0, alpha, steps, seed, chain)


def _tile():
    return _synthetic("tile112", 112, 28, 1.0, 0.9985, 3000, 3)


def _packed():
    """the packed tile of tests/test_gpu_deep_live_state.py: 30 strongly overlapping rectangles at T0 = 5"""
    b = _synthetic("packed", 96, 30, 5.0, 0.9995, 4000, 6)
    rng = np.random.default_rng(3)
    b.xy = rng.integers(24, 72, (30, 2)).astype(np.int32)
    b.mk = np.stack([rng.uniform(20.0, 30.0, 30), rng.uniform(0.3, 0.6, 30), rng.uniform(0.0, np.pi, 30)], axis=1)
    return b


def _off_class():
    """every initial mark sits 0.37 of a class width above its class edge: a data-driven transform that draws the class the
    mark sits in proposes the EDGE, which is another value -- the first such transform of a mark is no re-write"""
    b = _synthetic("off-class", 112, 28, 1.0, 0.9985, 3000, 3)
    mk = b.mk.copy()
    for j, m in enumerate(b.maps):
        edges = np.asarray(m.feature_mapping, dtype=np.float64)
        cls = np.clip(np.searchsorted(edges, mk[:, j], side="right") - 1, 0, len(edges) - 1)
        mk[:, j] = edges[cls] + 0.37 * (m.range / m.n_classes)
    b.mk = mk
    b.name = "off-class"
    return b


def _contrast():
    """the contrast energy setup of tests/test_gpu_classics.py with the measure whose value is +inf for a one-pixel fill
    ("craciun": E(after) - E(before) over a neighbourhood of such a point is NaN, and the step is rejected)"""
    from mpp_cnn_rs_object_detection_amd import energies as E
    from test_gpu_classics import G, setup_and_data
    setup, data = setup_and_data("craciun")
    np.random.seed(5)
    unit, pair = setup.make_energies(data)
    comb = E.ManualHierarchicalEnergyCombinator(dict(zip(setup.NAMES, [1.0, 2.0, 0.5, 0.25, 0.75])), "ContrastEnergy", 0.0)
    model = E.build_model_desc(unit, pair, comb)
    kd = kernels.make_kernels(data.mappings, 12.0, kernel_weights=dict(kernels.BASE_KERNEL_WEIGHTS, **TRANSFORM_HEAVY))
    xy = G["setup_cfg_craciun2"][:12, :2].astype(np.int32)
    # nine steps in ten are rejected for a NaN here, and a mark that never moves never reaches a class edge: every initial mark
    # is the edge of the likeliest class of its pixel's row
    mk = np.stack([np.asarray(m.feature_mapping, np.float64)[data.param_dist_maps[j][xy[:, 0], xy[:, 1]].argmax(1)]
                   for j, m in enumerate(data.mappings)], axis=1)
    return Built("contrast", tuple(data.shape), data.detection_map, list(data.param_dist_maps), data.mappings, model, kd,
                 xy, np.ascontiguousarray(mk), 0.05, 0.999, 3000, 4, image=E.classic_image(unit))


def _capacity():
    """the hot tile of tests/test_gpu_capacity.py: a birth intensity of 150 at T0 = 5 piles points up until a cell is full"""
    return _synthetic("capacity", 96, 14, 5.0, 0.9995, 4000, 3, tile_id=71, intensity=150.0, chain=3)


def _empty():
    b = _synthetic("empty", 64, 6, 5.0, 0.9995, 4000, 1)
    b.xy, b.mk = np.zeros((0, 2), np.int32), np.zeros((0, 3), np.float64)
    return b


def _hot():
    """a call long enough to start hot (4 096 steps or more); the test hands over at the first chance"""
    return _synthetic("hot-start", 128, 40, 1.0, 0.9985, 5000, 77, weights=None)      # (the usual mixture)


_BUILDERS = {"tile112": _tile, "packed": _packed, "off-class": _off_class, "contrast": _contrast, "capacity": _capacity,
             "empty": _empty, "hot-start": _hot}
CASES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def build(name) -> Built:
    return _BUILDERS[name]()


def make_oracle(b: Built):
    import oracle
    o = oracle.Oracle(b.shape, b.det, b.marks, b.model, b.kd)
    if b.image is not None:
        o.set_image(b.image)
    o.set_points(b.xy, b.mk)
    o.set_temperature(b.T0, b.alpha, 0.0)
    return o


@functools.lru_cache(maxsize=None)
def oracle_chain(name):
    """the oracle's chain of the case: (out, props, final points)"""
    b = build(name)
    o = make_oracle(b)
    out, props = o.run(b.steps, b.seed, chain=b.chain, trace=True)
    return out, props, o.get_points()


def case_counts(name):
    b = build(name)
    out, props, _ = oracle_chain(name)
    return count(props, out, b.xy, b.mk, maps=b.maps)
