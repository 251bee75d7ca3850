"""ctypes binding of ``libmppgpu.so`` (C ABI: ``include/mpp_hip.h``).

This is the only door between the Python host code and the HIP kernels.  There
is no CPU fallback: if the library is missing or no GPU is visible, importing
the symbols or creating a context raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from .energies import ModelDesc
from .kernels import KernelDesc

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPP_LIB_PATH") or os.path.join(_HERE, "libmppgpu.so")   # override: diagnostic builds only

MAX_UNIT, MAX_PAIR, NCLASS, NKERNEL = 8, 2, 32, 10

class UnitTermC(C.Structure):
    _fields_ = [("kind", C.c_int32), ("gated", C.c_int32), ("coef", C.c_double), ("p", C.c_double * 8)]


class PairTermC(C.Structure):
    _fields_ = [("kind", C.c_int32), ("gated", C.c_int32), ("reduce", C.c_int32), ("_pad", C.c_int32),
                ("coef", C.c_double), ("max_dist", C.c_double), ("p", C.c_double * 2)]


class ModelC(C.Structure):
    _fields_ = [("n_unit", C.c_int32), ("n_pair", C.c_int32), ("combinator", C.c_int32), ("gate_term", C.c_int32),
                ("gate_thr", C.c_double), ("lin0", C.c_double),
                ("unit", UnitTermC * MAX_UNIT), ("pair", PairTermC * MAX_PAIR)]


class MappingsC(C.Structure):
    _fields_ = [("cyclic", C.c_int32 * 3), ("_pad", C.c_int32), ("vmin", C.c_double * 3), ("vmax", C.c_double * 3),
                ("edges", (C.c_double * NCLASS) * 3)]


class KernelsC(C.Structure):
    _fields_ = [("p_kernel", C.c_double * NKERNEL), ("sigma_trans", C.c_double), ("sigma_transform", C.c_double),
                ("max_delta", C.c_int32), ("_pad", C.c_int32), ("split_radius", C.c_double), ("split_sigma", C.c_double)]


class TrainDataC(C.Structure):
    """mpp_train_data: the resident training images and their object tables (device pointers)"""
    _fields_ = [("images", C.c_void_p), ("img_off", C.c_void_p), ("img_hw", C.c_void_p), ("obj_start", C.c_void_p),
                ("centers", C.c_void_p), ("params", C.c_void_p), ("n_images", C.c_int32), ("_pad", C.c_int32)]


class TrainLabelsC(C.Structure):
    """mpp_train_labels: kind 0 PosNet (uvec, max_distance, sigma_dil), 1 ShapeNet (n_classes, cyclic, lower bin edges)"""
    _fields_ = [("kind", C.c_int32), ("uvec", C.c_int32), ("max_distance", C.c_double), ("sigma_dil", C.c_double),
                ("n_classes", C.c_int32), ("cyclic", C.c_int32 * 3), ("edges", (C.c_double * NCLASS) * 3)]


class TrainOutC(C.Structure):
    """mpp_train_out: device pointers of the batch builder's outputs (None: not written)"""
    _fields_ = [(k, C.c_void_p) for k in ("patch", "vec", "mask", "dil", "dist", "cls", "cover", "sums", "status")]


#: mpp_train_batch flags (include/mpp_hip.h MPP_AUG_*) and its geometry
AUG_GEOMETRIC, AUG_MEDIUM, AUG_STRONG, AUG_PERTURB, AUG_HISTMATCH = 1, 2, 4, 8, 16
#: shadow, fog, CLAHE, downscale, median / box blur: the ops of the recipe that need neighbours or the whole patch
AUG_SPATIAL = 32
#: haze points of one patch (MPP_AUG_MAX_HAZE) and mpp_aug_record, what mpp_train_aug_params writes per patch
AUG_MAX_HAZE = 64
AUG_RECORD_DTYPE = np.dtype([(k, "<i4") for k in ("rot", "flip", "chan_op", "chan_arg", "bc", "color", "noise", "hm", "tmpl",
                                                  "shadow", "n_poly", "fog", "n_haze", "clahe", "downscale", "blur")]
                            + [("alpha", "<f4"), ("beta", "<f4"), ("shift", "<f4", (3,)), ("_pad", "<f4"),
                               ("sigma", "<f8"), ("blend", "<f8"), ("clip", "<f8"), ("fog_coef", "<f8"),
                               ("poly", "<i2", (2, 5, 2)), ("haze", "<i2", (AUG_MAX_HAZE, 2))], align=True)
#: side of a density cell in pixels (mpp_posnet_error_map), the reference's rescale_fac 1/8
DENSITY_CELL = 8
TRAIN_BAND, TRAIN_MAX_OBJ = 16, 1024
#: default workspace limit of MppContext.rescale in bytes: tables plus one band of horizontally filtered rows
RESCALE_WORKSPACE = 512 << 20


PROPOSAL_DTYPE = np.dtype([("kernel", "<i4"), ("target", "<i4"), ("ax", "<i4"), ("ay", "<i4"),
                           ("as", "<f8"), ("ar", "<f8"), ("aa", "<f8"), ("aux0", "<f8"), ("aux1", "<f8"),
                           ("param_id", "<i4"), ("new_class", "<i4"), ("u_accept", "<f8")], align=True)
STEPOUT_DTYPE = np.dtype([("dE", "<f8"), ("fwd", "<f8"), ("bwd", "<f8"), ("log_alpha", "<f8"), ("T", "<f8"),
                          ("accepted", "<i4"), ("n_after", "<i4")], align=True)
#: mpp_birth_summary, one per chain, and MPP_BIRTH_CHUNK: the points a block of the birth-energy map stages per pass
BIRTH_SUMMARY_DTYPE = np.dtype([("min_dE", "<f8"), ("x", "<i4"), ("y", "<i4"), ("n_negative", "<i8"), ("n_nan", "<i8")], align=True)
BIRTH_CHUNK = 256
#: mpp_complete_report, one per chain (``MppContext.birth_complete``); status: 0 converged, 1 round limit, 2 capacity
COMPLETE_REPORT_DTYPE = np.dtype([("status", "<i4"), ("rounds", "<i4"), ("n_added", "<i4"), ("n_after", "<i4"), ("gain", "<f8"),
                                  ("min_dE", "<f8"), ("x", "<i4"), ("y", "<i4"), ("n_negative", "<i8"), ("n_nan", "<i8")], align=True)
COMPLETE_CONVERGED, COMPLETE_ROUND_LIMIT, COMPLETE_CAPACITY = 0, 1, 2
#: mpp_recombine_report, one per tile (``MppContext.recombine``); status: 0 the winner stays as it is, 1 recombined, 2 the
#: composite does not fit point_capacity.  RECOMBINE_LDS_POINTS: the points of a tile whose labels fit the LDS
RECOMBINE_REPORT_DTYPE = np.dtype([("status", "<i4"), ("winner", "<i4"), ("n_clusters", "<i4"), ("n_taken", "<i4"), ("n_before", "<i4"),
                                   ("n_after", "<i4"), ("E_winner", "<f8"), ("E_sum", "<f8"), ("E_after", "<f8")], align=True)
RECOMBINE_UNCHANGED, RECOMBINE_DONE, RECOMBINE_CAPACITY = 0, 1, 2
RECOMBINE_LDS_POINTS = 2048
#: mpp_descent_report, one per chain (``MppContext.descend``); status: 0 joint fixed point, 1 round limit, 2 capacity
DESCENT_REPORT_DTYPE = np.dtype([("status", "<i4"), ("rounds", "<i4"), ("n_added", "<i4"), ("n_removed", "<i4"), ("n_after", "<i4"),
                                 ("slot_max", "<i4"), ("gain_births", "<f8"), ("gain_deaths", "<f8"), ("max_p", "<f8"),
                                 ("min_dE", "<f8"), ("x", "<i4"), ("y", "<i4"), ("n_positive", "<i8"), ("n_negative", "<i8"),
                                 ("n_nan", "<i8")], align=True)
DESCEND_DEATHS, DESCEND_BIRTHS = 1, 2
DESCENT_FIXED_POINT, DESCENT_ROUND_LIMIT, DESCENT_CAPACITY = 0, 1, 2
#: mpp_relocate_report, one per chain (``MppContext.relocate``); status: 0 a round moved nothing, 1 round limit.  MOVE_CHUNK:
#: the points a workgroup of the move-gain kernel stages per pass; MOVE_RADIUS_MAX: the largest window radius
RELOCATE_REPORT_DTYPE = np.dtype([("status", "<i4"), ("rounds", "<i4"), ("n_moved", "<i4"), ("n_after", "<i4"), ("slot_max", "<i4"),
                                  ("n_positive", "<i4"), ("gain", "<f8"), ("max_gain", "<f8")], align=True)
RELOCATE_FIXED_POINT, RELOCATE_ROUND_LIMIT = 0, 1
MOVE_CHUNK = 256
MOVE_RADIUS_MAX = 7


class RelocateReportC(C.Structure):
    """mpp_relocate_report"""
    _fields_ = [("status", C.c_int32), ("rounds", C.c_int32), ("n_moved", C.c_int32), ("n_after", C.c_int32), ("slot_max", C.c_int32),
                ("n_positive", C.c_int32), ("gain", C.c_double), ("max_gain", C.c_double)]


def relocate_distance(max_inter: float, radius: int) -> float:
    """The selection distance of a relocation round, ``2 * (max_inter + radius * sqrt(2))`` in float64: two points further
    apart neither interact before or after their moves nor share an affected neighbour"""
    return 2.0 * (float(max_inter) + float(int(radius)) * float(np.sqrt(np.float64(2.0))))
#: mpp_exchange_record, one per attempted exchange of ``MppContext.run_tempered``: the values as read before the swap
EXCHANGE_RECORD_DTYPE = np.dtype([("step", "<i8"), ("tile", "<i4"), ("k", "<i4"), ("chain_a", "<i4"), ("chain_b", "<i4"),
                                  ("accepted", "<i4"), ("_pad", "<i4"), ("Ea", "<f8"), ("Eb", "<f8"), ("Ta", "<f8"),
                                  ("Tb", "<f8"), ("u", "<f8")], align=True)
#: steps between two exchanges unless told otherwise: a segment of a run gets its hot start only from 4096 steps on
TEMPERING_EVERY = 4096
E_OUTPUT_FULL = -13     # mpp_select_minima: more minima kept than the output holds


_vp, _i32, _i64, _dbl = C.c_void_p, C.c_int, C.c_int64, C.c_double
#: (result, arguments) of every function include/mpp_hip.h declares
PROTOTYPES = {
    "mpp_create": (_i32, [_i32, C.POINTER(_vp)]),
    "mpp_destroy": (_i32, [_vp]),
    "mpp_last_error": (C.c_char_p, [_vp]),
    "mpp_set_stream": (_i32, [_vp, _vp]),
    "mpp_synchronize": (_i32, [_vp]),
    "mpp_set_option": (_i32, [_vp, C.c_char_p, _i64]),
    "mpp_get_option": (_i64, [_vp, C.c_char_p]),
    "mpp_set_maps": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32]),
    "mpp_set_image": (_i32, [_vp, _i32, _i32, _vp, _i32]),
    "mpp_set_model": (_i32, [_vp, C.POINTER(ModelC), C.POINTER(MappingsC)]),
    "mpp_set_kernels": (_i32, [_vp, C.POINTER(KernelsC), _vp]),
    "mpp_set_points": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "mpp_get_points": (_i32, [_vp, _i32, _i32, C.POINTER(C.c_int32), _vp, _vp]),
    "mpp_count": (_i32, [_vp, _i32, C.POINTER(C.c_int32)]),
    "mpp_get_points_all": (_i32, [_vp, _i32, _vp, _vp, _vp]),
    "mpp_pack_detections": (_i32, [_vp, _i32, _vp, _vp, _i32, _vp, C.POINTER(C.c_int32)]),
    "mpp_total_energy": (_i32, [_vp, _i32, C.POINTER(_dbl), _vp]),
    "mpp_total_energy_all": (_i32, [_vp, _vp]),
    "mpp_point_energies_all": (_i32, [_vp, _vp]),
    "mpp_delta_batch": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mpp_delta_vectors": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "mpp_papangelou": (_i32, [_vp, _i32, _vp]),
    "mpp_birth_energy_map": (_i32, [_vp, _vp, _vp, _vp]),
    "mpp_select_minima": (_i32, [_vp, _i32, _i32, _i32, _vp, _dbl, _dbl, _i32, _vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mpp_birth_complete": (_i32, [_vp, _i32, _dbl, _vp]),
    "mpp_recombine": (_i32, [_vp, _vp, _vp]),
    "mpp_papangelou_all": (_i32, [_vp, _vp]),
    "mpp_select_points": (_i32, [_vp, _i32, _vp, _vp, _dbl, _dbl, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mpp_descend": (_i32, [_vp, _i32, _i32, _dbl, _vp, _vp]),
    "mpp_move_gains": (_i32, [_vp, _i32, _vp, _vp]),
    "mpp_relocate": (_i32, [_vp, _i32, _i32, _dbl, _vp, _vp]),
    "mpp_conv3x3_c32": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "mpp_conv3x3_stem": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mpp_merge_score": (_i32, [_vp, C.c_double, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mpp_naive_init": (_i32, [_vp, _dbl, _dbl]),
    "mpp_set_schedule": (_i32, [_vp, _dbl, _dbl, _dbl]),
    "mpp_replay": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "mpp_run": (_i32, [_vp, _i64, C.c_uint64, C.c_uint32, _i32, _vp, _vp]),
    "mpp_set_chain_keys": (_i32, [_vp, _i32, _vp, _vp]),
    "mpp_step_index": (_i32, [_vp, _i32, C.POINTER(C.c_int64)]),
    "mpp_last_kernel_ms": (_i32, [_vp, C.POINTER(_dbl)]),
    "mpp_get_schedules": (_i32, [_vp, _vp]),
    "mpp_set_schedules": (_i32, [_vp, _vp]),
    "mpp_set_ladder": (_i32, [_vp, _dbl]),
    "mpp_run_tempered": (_i32, [_vp, _i64, C.c_uint64, C.c_uint32, _i64, _vp, _i64, C.POINTER(C.c_int64)]),
    "mpp_affine_relu": (_i32, [_vp, _vp, _i32, _i32, _i64, _i32, _vp, _vp]),
    "mpp_posnet_epilogue_win": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _dbl, _dbl, _i32, _i32, _i32, _i32, _vp, _i32]),
    "mpp_shapenet_epilogue_win": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _i32]),
    "mpp_posnet_epilogue_nhwc_win": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _dbl, _dbl, _i32, _i32, _i32, _i32, _vp, _i32]),
    "mpp_shapenet_epilogue_nhwc_win": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32]),
    "mpp_shapenet_heads_win": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32]),
    "mpp_nhwc_glue": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "mpp_quad_iou": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _i32]),
    "mpp_detect_centers": (_i32, [_vp, _i32, _i32, _i32, _vp, _dbl, _i32, _dbl, _i32, _vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mpp_mark_classes": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp]),
    "mpp_train_batch": (_i32, [_vp, C.POINTER(TrainDataC), C.POINTER(TrainLabelsC), _i32, _i32, _vp, _i32, C.c_uint32, C.c_uint32,
                               C.c_uint32, C.POINTER(TrainOutC)]),
    "mpp_posnet_loss": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "mpp_shapenet_loss": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mpp_philox4x32": (None, [_vp, _vp, _vp]),
    "mpp_image_histograms": (_i32, [_vp, C.POINTER(TrainDataC), _vp]),
    "mpp_train_set_histograms": (_i32, [_vp, _vp, _i32]),
    "mpp_train_aug_params": (_i32, [_vp, _i32, C.c_uint32, C.c_uint32, C.c_uint32, _i32, _i32, _i32, _vp]),
    "mpp_posnet_error_map": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _dbl, _vp, _vp, _vp]),
    "mpp_density_prefix": (_i32, [_vp, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "mpp_density_anchors": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, C.c_uint32, C.c_uint32, _vp]),
    "mpp_rescale": (_i32, [_vp, _vp, _i32, _i32, _i64, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _i64]),
    "mpp_draw_outlines": (_i32, [_vp, _i32, _i32, _vp, _vp, _dbl, _dbl, _vp, _i32, _vp, _vp, _vp]),
    "mpp_abi_version": (_i32, []),
}
#: every symbol include/mpp_hip.h declares (tests check that the header agrees and that the library exports all of them)
ABI_SYMBOLS = list(PROTOTYPES)


class MppError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libmppgpu error {code}: {message}")
        self.code = code


_lib = None


def _torch_runtime_first():
    """PyTorch-ROCm wheels bundle their own HIP/HSA runtime under the SAME sonames (libamdhip64.so.7,
    libhsa-runtime64.so.1) as the system one libmppgpu.so is linked against.  Whichever is loaded first serves both:
    with torch first the process has ONE runtime (and device pointers are shared freely); with /opt/rocm's first, torch
    later stacks its own HIP on the foreign HSA and reports "No HIP GPUs are available".  So torch, when installed, is
    imported before the library is opened."""
    try:
        import torch  # noqa: F401
    except Exception:                     # torch missing: the sampler itself does not need it
        pass


def load_library(path: Optional[str] = None):
    """Load libmppgpu.so and declare the prototypes (``PROTOTYPES``).  Raises if it was not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback for the sampler")
    _torch_runtime_first()
    L = C.CDLL(path)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    if path == LIB_PATH:
        _lib = L
    return L


def model_struct(desc: ModelDesc) -> ModelC:
    m = ModelC()
    m.n_unit, m.n_pair = len(desc.unit), len(desc.pair)
    m.combinator, m.gate_term, m.gate_thr, m.lin0 = desc.combinator, desc.gate_term, desc.gate_thr, desc.lin0
    for i, (kind, gated, coef, params) in enumerate(desc.unit):
        m.unit[i].kind, m.unit[i].gated, m.unit[i].coef = kind, gated, coef
        for j, p in enumerate(params):
            m.unit[i].p[j] = p
    for i, (kind, gated, red, coef, max_dist, params) in enumerate(desc.pair):
        t = m.pair[i]
        t.kind, t.gated, t.reduce, t.coef, t.max_dist = kind, gated, red, coef, max_dist
        for j, p in enumerate(params):
            t.p[j] = p
    return m


def mappings_struct(mappings) -> MappingsC:
    s = MappingsC()
    for j, mp in enumerate(mappings):
        if mp.n_classes != NCLASS:
            raise ValueError("marks must have 32 classes")
        s.cyclic[j], s.vmin[j], s.vmax[j] = int(mp.is_cyclic), float(mp.v_min), float(mp.v_max)
        for i in range(NCLASS):
            s.edges[j][i] = float(mp.feature_mapping[i])
    return s


def kernels_struct(kd: KernelDesc) -> KernelsC:
    k = KernelsC()
    for i in range(NKERNEL):
        k.p_kernel[i] = float(kd.p_kernel[i]) if i < len(kd.p_kernel) else 0.0
    k.sigma_trans, k.sigma_transform, k.max_delta = float(kd.sigma_trans), float(kd.sigma_transform), int(kd.max_delta)
    k.split_radius, k.split_sigma = float(getattr(kd, "split_radius", 16.0)), float(getattr(kd, "split_sigma", 0.1))
    return k


def _is_torch(a) -> bool:
    return hasattr(a, "data_ptr") and hasattr(a, "device")


def _ptr(a):
    if a is None:
        return None
    if _is_torch(a):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


class MppContext:
    """One GPU context holding ``n_tiles`` tiles of equal shape (thin, 1:1 over the C ABI)."""

    def __init__(self, device: int = 0, point_capacity: Optional[int] = None, cell_capacity: Optional[int] = None,
                 spec_waves: Optional[int] = None, spec_lanes: Optional[int] = None, replicas: Optional[int] = None,
                 deep: Optional[int] = None, chain_state: Optional[int] = None):
        """chain_state: where a chain's state lives -- 0 auto (LDS; a chain that outgrows it continues in device memory),
        1 LDS only (such a chain stops with -12 / -11), 2 device memory for every chain (tests, diagnosis)."""
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.mpp_create(int(device), C.byref(h))
        if rc != 0:
            raise MppError(rc, "mpp_create failed: no usable MI355X/HIP device" if rc == -3 else "mpp_create failed")
        self._h = h
        self.device = int(device)
        self._keep = []          # keeps borrowed device tensors / host arrays alive
        self.n_tiles = 0
        self.exchange_records = 0       # records the last run_tempered made
        self.shape = (0, 0)
        self.n_terms = 0
        self.names: List[str] = []
        for name, value in (("point_capacity", point_capacity), ("cell_capacity", cell_capacity), ("spec_waves", spec_waves),
                            ("spec_lanes", spec_lanes), ("replicas", replicas), ("deep", deep), ("chain_state", chain_state)):
            if value is not None:
                self.set_option(name, value)
        if os.environ.get("MPP_HANDOVER_TILES"):           # (experiments: the largest launch that starts hot)
            self.set_option("handover_tiles", int(os.environ["MPP_HANDOVER_TILES"]))
        if os.environ.get("MPP_HANDOVER_AT"):
            self.set_option("handover_at", int(os.environ["MPP_HANDOVER_AT"]))

    # -- plumbing ------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != 0:
            raise MppError(rc, self._L.mpp_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.mpp_destroy(self._h)
            self._h = None
            self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name: str, value: int):
        self._check(self._L.mpp_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        return int(self._L.mpp_get_option(self._h, name.encode()))

    def set_stream(self, stream_handle: Optional[int]):
        self._check(self._L.mpp_set_stream(self._h, C.c_void_p(stream_handle) if stream_handle else None))

    def synchronize(self):
        self._check(self._L.mpp_synchronize(self._h))

    # -- inputs --------------------------------------------------------------------------------
    def set_maps(self, det, marks: Sequence):
        """det: [T,H,W] or [H,W]; marks: three [T,H,W,32] or [H,W,32]; numpy (copied) or torch
        tensors already on this GPU (borrowed, zero-copy)."""
        on_device = _is_torch(det)
        if on_device:
            if any(not _is_torch(m) for m in marks):
                raise TypeError("det and marks must all be device tensors or all be numpy arrays")
            import torch
            arrs = [a.contiguous() if a.dtype == torch.float32 else a.float().contiguous() for a in [det] + list(marks)]
            if not all(a.is_cuda for a in arrs):
                raise TypeError("torch maps must live on the GPU")
            if any(a.device.index != self.device for a in arrs):
                # borrowed pointers are dereferenced by kernels launched on this ctx's GPU; peer access is never enabled
                raise ValueError(f"borrowed maps live on {arrs[0].device} but this context is bound to GPU {self.device}")
            shape = tuple(arrs[0].shape)
        else:
            arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in [det] + list(marks)]
            shape = arrs[0].shape
        if len(shape) == 2:
            T, (H, W) = 1, shape
        else:
            T, H, W = shape
        for a in arrs[1:]:
            if tuple(a.shape[-3:]) != (H, W, NCLASS):
                raise ValueError(f"mark map of shape {tuple(a.shape)} does not match tile {H}x{W}x32")
        self._check(self._L.mpp_set_maps(self._h, T, H, W, _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), _ptr(arrs[3]),
                                         1 if on_device else 0))
        self._keep = arrs if on_device else []
        self.n_tiles, self.shape = self.get_option("n_chains"), (H, W)     # = T * replicas

    def set_image(self, img):
        """The picture behind the classic image energies (``energies/classics.py``): [T,H,W,C] or [H,W,C] float32, numpy
        (copied) or a torch tensor on this GPU (borrowed); after :meth:`set_maps`."""
        on_device = _is_torch(img)
        if on_device:
            import torch
            a = img.contiguous() if img.dtype == torch.float32 else img.float().contiguous()
            if not a.is_cuda or a.device.index != self.device:
                raise ValueError(f"a borrowed image must live on GPU {self.device}")
        else:
            a = np.ascontiguousarray(img, dtype=np.float32)
        if a.ndim == 3:
            a = a.reshape((1,) + tuple(a.shape))
        if a.ndim != 4 or tuple(a.shape[1:3]) != tuple(self.shape):
            raise ValueError(f"image of shape {tuple(a.shape)} does not match tiles {self.shape}")
        self._check(self._L.mpp_set_image(self._h, int(a.shape[0]), int(a.shape[3]), _ptr(a), 1 if on_device else 0))
        self._keep_img = a if on_device else None

    def set_model(self, desc: ModelDesc, mappings):
        m, mp = model_struct(desc), mappings_struct(mappings)
        self._check(self._L.mpp_set_model(self._h, C.byref(m), C.byref(mp)))
        self.n_terms = len(desc.unit) + len(desc.pair)
        self.names = list(desc.names)

    def set_kernels(self, kd: KernelDesc, intensity=None):
        k = kernels_struct(kd)
        inten = np.ascontiguousarray(np.broadcast_to(np.asarray(kd.intensity if intensity is None else intensity,
                                                                dtype=np.float64), (max(self.n_tiles, 1),)))
        self._check(self._L.mpp_set_kernels(self._h, C.byref(k), _ptr(inten)))

    def set_schedule(self, T0: float, alpha: float, T_target: float = 0.0):
        self._check(self._L.mpp_set_schedule(self._h, float(T0), float(alpha), float(T_target)))

    # -- configuration -------------------------------------------------------------------------
    def set_points(self, tile: int, xy, marks):
        xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        marks = np.ascontiguousarray(marks, dtype=np.float64).reshape(-1, 3)
        self._check(self._L.mpp_set_points(self._h, tile, len(xy), _ptr(xy), _ptr(marks)))

    def count(self, tile: int = 0) -> int:
        n = C.c_int32()
        self._check(self._L.mpp_count(self._h, tile, C.byref(n)))
        return n.value

    def get_points(self, tile: int = 0):
        n = self.count(tile)
        xy, marks = np.zeros((n, 2), np.int32), np.zeros((n, 3), np.float64)
        nn = C.c_int32()
        self._check(self._L.mpp_get_points(self._h, tile, n, C.byref(nn), _ptr(xy), _ptr(marks)))
        return xy, marks

    def counts(self) -> np.ndarray:
        """number of points of every tile (one device read)"""
        n = np.zeros(self.get_option("n_chains"), np.int32)
        self._check(self._L.mpp_get_points_all(self._h, 0, _ptr(n), None, None))
        return n

    def get_points_all(self):
        """[(xy, marks)] of every tile with five strided device reads in total"""
        n = self.counts()
        cap = int(n.max()) if len(n) else 0
        xy, marks = np.zeros((len(n), cap, 2), np.int32), np.zeros((len(n), cap, 3), np.float64)
        if cap:
            self._check(self._L.mpp_get_points_all(self._h, cap, _ptr(n), _ptr(xy), _ptr(marks)))
        return [(xy[t, :n[t]], marks[t, :n[t]]) for t in range(len(n))]

    def pack_detections(self, tile_ids, anchors, capacity: int, out) -> int:
        """Every tile's configuration as records (tile id, x + anchor_x, y + anchor_y, size, ratio, angle, 0) in the
        device tensor ``out`` [capacity+1, 7] float64 (row 0 = count): the all-gather's send buffer, filled without a
        host round trip.  Returns the number of records."""
        tile_ids = np.ascontiguousarray(tile_ids, dtype=np.int32).reshape(-1)
        anchors = np.ascontiguousarray(anchors, dtype=np.int32).reshape(-1, 2)
        if len(tile_ids) != len(anchors) or len(tile_ids) > self.n_tiles:
            raise ValueError("pack_detections: one id and one anchor per tile of the context")
        if not (_is_torch(out) and out.is_cuda and out.device.index == self.device and out.is_contiguous()
                and tuple(out.shape) == (capacity + 1, 7) and out.element_size() == 8):
            raise ValueError(f"pack_detections: out must be a contiguous [{capacity + 1}, 7] float64 tensor on GPU {self.device}")
        n = C.c_int32()
        self._check(self._L.mpp_pack_detections(self._h, len(tile_ids), _ptr(tile_ids), _ptr(anchors), int(capacity),
                                                _ptr(out), C.byref(n)))
        return n.value

    def naive_init(self, threshold: float, nms_distance: float = 6.0):
        self._check(self._L.mpp_naive_init(self._h, float(threshold), float(nms_distance)))

    # -- energies ------------------------------------------------------------------------------
    def total_energy(self, tile: int = 0, return_vectors: bool = False):
        e = C.c_double()
        vec = np.zeros((self.count(tile), self.n_terms), np.float64) if return_vectors else None
        self._check(self._L.mpp_total_energy(self._h, tile, C.byref(e), _ptr(vec)))
        return (e.value, vec) if return_vectors else e.value

    def total_energy_all(self) -> np.ndarray:
        """``total_energy(t)`` of every chain of the context, bit for bit, with one device read (``mpp_total_energy_all``)"""
        e = np.zeros(self.get_option("n_chains"), np.float64)
        self._check(self._L.mpp_total_energy_all(self._h, _ptr(e)))
        return e

    def point_energies_all(self) -> np.ndarray:
        """The per-point energies behind :meth:`total_energy_all`, float64 ``[n_chains, point_capacity]``: row c holds the
        energies of chain c's points in slot order, 0.0 behind its count; the row summed in that order from 0.0 is
        ``total_energy_all()[c]`` bit for bit (``mpp_point_energies_all``)"""
        e = np.zeros((max(self.get_option("n_chains"), 1), self.get_option("point_capacity")), np.float64)
        self._check(self._L.mpp_point_energies_all(self._h, _ptr(e)))
        return e[:self.get_option("n_chains")]

    def recombine(self, src: bool = False):
        """``mpp_recombine``: per tile, the winning replica's chain takes, for every interaction cluster of the union of the
        tile's replicas, the points of the replica that spends the least energy there (the rules: ``include/mpp_hip.h``).
        Returns one record of ``RECOMBINE_REPORT_DTYPE`` per tile; with ``src`` also int32 ``[n_tiles, point_capacity, 2]``,
        the (replica, slot) every slot of the returned winner chain came from, (-1, -1) behind its count."""
        n = self.get_option("n_chains") // max(self.get_option("replicas"), 1)
        rep = np.zeros(max(n, 1), RECOMBINE_REPORT_DTYPE)
        where = np.full((max(n, 1), self.get_option("point_capacity"), 2), -1, np.int32) if src else None
        self._check(self._L.mpp_recombine(self._h, _ptr(rep), _ptr(where)))
        return (rep[:n], where[:n]) if src else rep[:n]

    @staticmethod
    def _pack_cases(removals, add_xy, add_marks):
        n = len(removals)
        rem_off = np.zeros(n + 1, np.int32)
        add_off = np.zeros(n + 1, np.int32)
        rem_off[1:] = np.cumsum([len(r) for r in removals])
        add_off[1:] = np.cumsum([len(a) for a in add_xy])
        rem = np.ascontiguousarray(np.concatenate([np.asarray(r, np.int32).reshape(-1) for r in removals] +
                                                  [np.zeros(0, np.int32)]), dtype=np.int32)
        axy = np.ascontiguousarray(np.concatenate([np.asarray(a, np.int32).reshape(-1, 2) for a in add_xy] +
                                                  [np.zeros((0, 2), np.int32)]), dtype=np.int32)
        am = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float64).reshape(-1, 3) for a in add_marks] +
                                                 [np.zeros((0, 3))]), dtype=np.float64)
        if len(rem) == 0:
            rem = np.zeros(1, np.int32)
        if len(axy) == 0:
            axy, am = np.zeros((1, 2), np.int32), np.zeros((1, 3))
        return n, rem_off, rem, add_off, axy, am

    def delta_batch(self, tile: int, removals: Sequence[Sequence[int]], add_xy: Sequence, add_marks: Sequence):
        n, rem_off, rem, add_off, axy, am = self._pack_cases(removals, add_xy, add_marks)
        out = np.zeros(n, np.float64)
        self._check(self._L.mpp_delta_batch(self._h, tile, n, _ptr(rem_off), _ptr(rem), _ptr(add_off), _ptr(axy),
                                            _ptr(am), _ptr(out)))
        return out

    def delta_vectors(self, tile: int, removals: Sequence[Sequence[int]], add_xy: Sequence, add_marks: Sequence,
                      n_terms: int):
        """before, after [n_cases][stride][n_terms] and mask [n_cases][stride] (see mpp_delta_vectors)"""
        n, rem_off, rem, add_off, axy, am = self._pack_cases(removals, add_xy, add_marks)
        stride = self.count(tile) + (int(np.max(np.diff(add_off))) if n else 0)
        stride = max(stride, 1)
        before = np.zeros((n, stride, n_terms), np.float64)
        after = np.zeros((n, stride, n_terms), np.float64)
        mask = np.zeros((n, stride), np.uint8)
        self._check(self._L.mpp_delta_vectors(self._h, tile, n, _ptr(rem_off), _ptr(rem), _ptr(add_off), _ptr(axy),
                                              _ptr(am), stride, _ptr(before), _ptr(after), _ptr(mask)))
        return before, after, mask

    def papangelou(self, tile: int = 0) -> np.ndarray:
        out = np.zeros(max(self.count(tile), 1), np.float64)
        self._check(self._L.mpp_papangelou(self._h, tile, _ptr(out)))
        return out[:self.count(tile)]

    def birth_energy_map(self, out=None, marks=False, summary: bool = True):
        """``mpp_birth_energy_map``: dE(c) = E(X + u_c) - E(X) for every pixel c of every chain, u_c the rectangle ShapeNet
        proposes at c.  Returns ``(dE, marks, summary)``: dE a float64 CUDA tensor [n_chains,H,W] on the ctx's GPU (``out``:
        written there), marks [n_chains,H,W,3] (size, ratio, angle of the candidates) when ``marks`` is True or a tensor to
        write, else None; summary a structured array of ``BIRTH_SUMMARY_DTYPE`` per chain, or None -- then the call does not
        wait for the device."""
        import torch
        T, (H, W) = self.get_option("n_chains"), self.shape
        if not self.n_tiles:
            self._check(self._L.mpp_birth_energy_map(self._h, None, None, None))       # (no maps: the library's message)
        dev = torch.device("cuda", self.device)

        def dev_out(name, t, shape):
            if not (_is_torch(t) and t.is_cuda and t.device.index == self.device and t.dtype == torch.float64
                    and t.is_contiguous() and tuple(t.shape) == shape):
                raise ValueError(f"birth_energy_map: {name} must be a contiguous float64 tensor of shape {shape} on GPU {self.device}")
            return t
        out = torch.empty((T, H, W), dtype=torch.float64, device=dev) if out is None else dev_out("out", out, (T, H, W))
        if marks is True:
            marks = torch.empty((T, H, W, 3), dtype=torch.float64, device=dev)
        elif marks is False or marks is None:
            marks = None
        else:
            marks = dev_out("marks", marks, (T, H, W, 3))
        # (the ctx's stream reads and writes tensors torch made: what torch has queued on them is complete first)
        torch.cuda.current_stream(dev).synchronize()
        s = np.zeros(T, BIRTH_SUMMARY_DTYPE) if summary else None
        self._check(self._L.mpp_birth_energy_map(self._h, _ptr(out), _ptr(marks), _ptr(s)))
        return out, marks, s

    def select_minima(self, dE, below: float, distance: float):
        """``mpp_select_minima``: the local minima below ``below`` of a float64 CUDA tensor [H,W] on the ctx's GPU (a view
        with unit column stride will do) -- the candidates ``dE < below`` that no other candidate within ``distance`` beats
        on the key (value, row-major index).  Returns ``(xy, values, n_candidates)``: xy [k,2] int32 (row, col) and values
        [k] float64 tensors on the device, in ascending row-major order."""
        import torch
        if not (_is_torch(dE) and dE.is_cuda and dE.device.index == self.device and dE.dtype == torch.float64 and dE.dim() == 2
                and dE.shape[0] >= 1 and dE.shape[1] >= 1 and dE.stride(1) == 1 and (dE.shape[0] == 1 or dE.stride(0) >= dE.shape[1])):
            raise ValueError(f"select_minima: dE must be a float64 [H,W] tensor with unit column stride on GPU {self.device}")
        H, W = int(dE.shape[0]), int(dE.shape[1])
        ld = int(dE.stride(0)) if H > 1 else W
        dev = torch.device("cuda", self.device)
        torch.cuda.current_stream(dev).synchronize()
        nc, nk = C.c_int64(), C.c_int64()
        cap = 256
        while True:
            xy = torch.empty((cap, 2), dtype=torch.int32, device=dev)
            values = torch.empty((cap,), dtype=torch.float64, device=dev)
            rc = self._L.mpp_select_minima(self._h, H, W, ld, _ptr(dE), float(below), float(distance), cap, _ptr(xy), _ptr(values),
                                           C.byref(nc), C.byref(nk))
            if rc != E_OUTPUT_FULL:
                break
            cap = int(nk.value)                      # (the call says how many it keeps: the second one fits)
        self._check(rc)
        return xy[:nk.value], values[:nk.value], int(nc.value)

    def birth_complete(self, max_rounds: int = 16, min_gain: float = 0.0) -> np.ndarray:
        """``mpp_birth_complete``: every chain of the context takes the births of its birth-energy map -- the local minima
        below ``-min_gain``, no two within twice the model's interaction range -- round after round until none is left,
        ``max_rounds`` rounds have added points, or a round does not fit ``point_capacity``.  The chains' configurations are
        changed on the device.  Returns one record of ``COMPLETE_REPORT_DTYPE`` per chain."""
        rep = np.zeros(max(self.get_option("n_chains"), 1), COMPLETE_REPORT_DTYPE)
        self._check(self._L.mpp_birth_complete(self._h, int(max_rounds), float(min_gain), _ptr(rep)))
        return rep[:self.get_option("n_chains")]

    def papangelou_all(self) -> np.ndarray:
        """``papangelou(t)`` of every chain of the context, bit for bit, with one device read (``mpp_papangelou_all``): float64
        ``[n_chains, point_capacity]``, row c the values of chain c's points in slot order, 0.0 behind its count"""
        d = np.zeros((max(self.get_option("n_chains"), 1), self.get_option("point_capacity")), np.float64)
        self._check(self._L.mpp_papangelou_all(self._h, _ptr(d)))
        return d[:self.get_option("n_chains")]

    def select_points(self, xy, values, above: float, distance: float):
        """``mpp_select_points``: the descent's selection on a list of points -- the candidates ``values > above`` that no
        other candidate within ``distance`` beats on the key (-value, slot).  ``xy`` [n,2] int32 and ``values`` [n] float64:
        arrays, or contiguous CUDA tensors on the ctx's GPU.  Returns ``(keep, n_candidates, n_kept)``, keep a uint8 tensor
        [n] on the device."""
        import torch
        dev = torch.device("cuda", self.device)

        def on_device(name, a, dtype, shape):
            t = a if _is_torch(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).reshape(shape)).to(dev)
            if not (t.is_cuda and t.device.index == self.device and t.dtype == getattr(torch, np.dtype(dtype).name)
                    and t.is_contiguous() and t.dim() == len(shape) and (len(shape) == 1 or t.shape[1] == 2)):
                raise ValueError(f"select_points: {name} must be a contiguous {np.dtype(dtype).name} tensor on GPU {self.device}")
            return t
        xy, values = on_device("xy", xy, np.int32, (-1, 2)), on_device("values", values, np.float64, (-1,))
        if xy.shape[0] != values.shape[0]:
            raise ValueError("select_points: one value per point")
        n = int(values.shape[0])
        keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        nc, nk = C.c_int64(), C.c_int64()
        self._check(self._L.mpp_select_points(self._h, n, _ptr(xy), _ptr(values), float(above), float(distance), _ptr(keep),
                                              C.byref(nc), C.byref(nk)))
        return keep, int(nc.value), int(nk.value)

    def descend(self, what: int = 3, max_rounds: int = 16, min_gain: float = 0.0, src: bool = False):
        """``mpp_descend``: every chain of the context alternates death rounds -- the points whose removal lowers the energy
        by more than ``min_gain``, no two within twice the model's interaction range, leave by stable compaction -- and birth
        rounds (one round of :meth:`birth_complete`) until a whole round changes nothing, ``max_rounds`` rounds have changed
        the chain, or a birth round does not fit ``point_capacity``.  ``what``: ``DESCEND_DEATHS``, ``DESCEND_BIRTHS`` or
        both.  Returns one record of ``DESCENT_REPORT_DTYPE`` per chain; with ``src`` also int32 ``[n_chains,
        point_capacity]``: the slot every final slot's point had when the call began, -1 for a born point and behind the count."""
        T = self.get_option("n_chains")
        rep = np.zeros(max(T, 1), DESCENT_REPORT_DTYPE)
        where = np.full((max(T, 1), self.get_option("point_capacity")), -1, np.int32) if src else None
        self._check(self._L.mpp_descend(self._h, int(what), int(max_rounds), float(min_gain), _ptr(rep), _ptr(where)))
        return (rep[:T], where[:T]) if src else rep[:T]

    def move_gains(self, radius: int = 2):
        """``mpp_move_gains``: for every point of every chain the largest energy gain of replacing it by the map's candidate
        at a pixel of the ``(2 radius + 1)^2`` window around it, and that pixel.  Returns ``(gain, to)``: float64
        ``[n_chains, point_capacity]`` (NaN: every pixel's value is NaN; 0.0 behind a chain's count) and int32 ``[n_chains,
        point_capacity, 2]`` (``(-1, -1)`` where there is none)."""
        T, cap = self.get_option("n_chains"), self.get_option("point_capacity")
        gain = np.zeros((max(T, 1), cap), np.float64)
        to = np.full((max(T, 1), cap, 2), -1, np.int32)
        self._check(self._L.mpp_move_gains(self._h, int(radius), _ptr(gain), _ptr(to)))
        return gain[:T], to[:T]

    def relocate(self, radius: int = 2, max_rounds: int = 16, min_gain: float = 0.0, moved: bool = False):
        """``mpp_relocate``: every chain of the context moves, round after round, the points whose best replacement by a map
        candidate within ``radius`` pixels lowers the energy by more than ``min_gain`` -- no two within
        ``relocate_distance(max_inter, radius)`` in one round -- until a round moves nothing or ``max_rounds`` rounds have
        moved something.  The points are rewritten in place on the device: slots, counts and order stay.  Returns one record
        of ``RELOCATE_REPORT_DTYPE`` per chain; with ``moved`` also int32 ``[n_chains, point_capacity]``: how often each slot
        was rewritten."""
        T = self.get_option("n_chains")
        rep = np.zeros(max(T, 1), RELOCATE_REPORT_DTYPE)
        count = np.zeros((max(T, 1), self.get_option("point_capacity")), np.int32) if moved else None
        self._check(self._L.mpp_relocate(self._h, int(radius), int(max_rounds), float(min_gain), _ptr(rep), _ptr(count)))
        return (rep[:T], count[:T]) if moved else rep[:T]

    # -- the chain -----------------------------------------------------------------------------
    def merge_score(self, distance: float):
        """``merge_patches(method='distance')`` and the two scorings around it for every tile of the ctx on the device
        (``mpp_merge_score``): -> [(xy, marks, dE)] of the survivors per tile (score = exp(-dE)), and the removed counts."""
        T = self.get_option("n_chains")
        cap = int(max(1, self.counts()[:T].max(initial=0)))
        n = np.zeros(T, np.int32)
        xy, marks = np.zeros((T, cap, 2), np.int32), np.zeros((T, cap, 3), np.float64)
        dE, removed = np.zeros((T, cap), np.float64), np.zeros(T, np.int32)
        self._check(self._L.mpp_merge_score(self._h, float(distance), cap, _ptr(n), _ptr(xy), _ptr(marks), _ptr(dE), _ptr(removed)))
        return [(xy[t, :n[t]].copy(), marks[t, :n[t]].copy(), dE[t, :n[t]].copy()) for t in range(T)], removed

    def replay(self, tile: int, tape: np.ndarray) -> np.ndarray:
        tape = np.ascontiguousarray(tape, dtype=PROPOSAL_DTYPE)
        out = np.zeros(len(tape), STEPOUT_DTYPE)
        self._check(self._L.mpp_replay(self._h, tile, len(tape), _ptr(tape), _ptr(out)))
        return out

    def run(self, n_steps: int, seed: int, chain0: int = 0, trace_tile: int = -1):
        if trace_tile >= 0:
            out = np.zeros(n_steps, STEPOUT_DTYPE)
            props = np.zeros(n_steps, PROPOSAL_DTYPE)
            self._check(self._L.mpp_run(self._h, int(n_steps), int(seed), int(chain0), trace_tile, _ptr(out),
                                        _ptr(props)))
            return out, props
        self._check(self._L.mpp_run(self._h, int(n_steps), int(seed), int(chain0), -1, None, None))
        return None

    # -- parallel tempering ---------------------------------------------------
    def get_schedules(self) -> np.ndarray:
        """Every chain's (current T, alpha, T_target) as the last launch left it, float64 ``[n_chains, 3]``"""
        sched = np.zeros((max(self.get_option("n_chains"), 1), 3), np.float64)
        self._check(self._L.mpp_get_schedules(self._h, _ptr(sched)))
        return sched[:self.get_option("n_chains")]

    def set_schedules(self, sched):
        """Replace every chain's (current T, alpha, T_target); nothing else changes (``mpp_set_schedules``)."""
        sched = np.ascontiguousarray(sched, dtype=np.float64)
        if sched.shape != (self.get_option("n_chains"), 3):
            raise ValueError(f"set_schedules: one (T, alpha, T_target) per chain of the context ({self.get_option('n_chains')})")
        self._check(self._L.mpp_set_schedules(self._h, _ptr(sched)))

    def set_ladder(self, ratio: float):
        """The temperature ladder over the replicas of every tile, after ``set_schedule``: replica r anneals ``ratio ** r``
        times hotter (``mpp_set_ladder``).  Zeroes the exchange counters."""
        self._check(self._L.mpp_set_ladder(self._h, float(ratio)))

    def run_tempered(self, n_steps: int, seed: int, chain0: int = 0, every: int = TEMPERING_EVERY, log: bool = True,
                     log_cap: Optional[int] = None) -> Optional[np.ndarray]:
        """``run`` with replica exchanges whenever the chains reach a multiple of ``every`` steps (``mpp_run_tempered``).
        Returns the call's attempted exchanges as records of ``EXCHANGE_RECORD_DTYPE`` in (exchange, tile, pair) order --
        at most ``log_cap`` of them (None: all) --, or None when ``log`` is False.  ``exchange_records`` holds the number
        of records the call made, kept or not."""
        n_logged = C.c_int64()
        if not log:
            self._check(self._L.mpp_run_tempered(self._h, int(n_steps), int(seed), int(chain0), int(every), None, 0,
                                                 C.byref(n_logged)))
            self.exchange_records = int(n_logged.value)
            return None
        if log_cap is None:                     # no more than one record per tile and pair of rungs at every boundary
            R = max(self.get_option("replicas"), 1)
            n = self.get_option("n_chains") // R
            log_cap = n * max(R - 1, 0) * (int(n_steps) // max(int(every), 1) + 1)
        rec = np.zeros(max(int(log_cap), 1), EXCHANGE_RECORD_DTYPE)
        self._check(self._L.mpp_run_tempered(self._h, int(n_steps), int(seed), int(chain0), int(every), _ptr(rec), int(log_cap),
                                             C.byref(n_logged)))
        self.exchange_records = int(n_logged.value)
        return rec[:min(self.exchange_records, int(log_cap))]

    def tempering_stats(self) -> dict:
        """Since the last ``set_ladder``: exchange steps, attempted and accepted pairs, ms of the energy and exchange launches"""
        return {"exchanges": self.get_option("tempering_exchanges"), "attempts": self.get_option("tempering_attempts"),
                "accepted": self.get_option("tempering_accepted"), "ms": self.get_option("tempering_us") / 1000.0}

    def set_chain_keys(self, seeds=None, chains=None):
        """Per-chain Philox key and chain id (``mpp_set_chain_keys``); ``None``: back to ``run``'s seed and chain0 + tile."""
        if seeds is None or chains is None:
            self._check(self._L.mpp_set_chain_keys(self._h, 0, None, None))
            return
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1)
        chains = np.ascontiguousarray(chains, dtype=np.uint32).reshape(-1)
        if len(seeds) != len(chains):
            raise ValueError("one seed and one chain id per chain")
        self._check(self._L.mpp_set_chain_keys(self._h, len(seeds), _ptr(seeds), _ptr(chains)))

    def deep_stats(self) -> dict:
        """counters of the last run's deep rounds (all tiles): rounds, steps evaluated, rounds with a change, steps committed"""
        v = [self.get_option(f"deep_stat{i}") for i in range(4)]
        return {"rounds": v[0], "evaluated": v[1], "rounds_with_change": v[2], "committed": v[3]}

    def step_index(self, tile: int = 0) -> int:
        s = C.c_int64()
        self._check(self._L.mpp_step_index(self._h, tile, C.byref(s)))
        return s.value

    def last_kernel_ms(self) -> float:
        ms = C.c_double()
        self._check(self._L.mpp_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    # -- U-Net epilogues (device tensors).  Each writes the window at (wx0, wy0) of the H x W crop whose size is the destination's:
    # a view of a larger map, e.g. ``det[a:a+h, b:b+w]``, or, at (0, 0), a dense [H,W] / [H,W,32] tensor for the whole crop ------
    def posnet_epilogue(self, pos_out, H: int, W: int, div_w: float, div_b: float, det, *, wx0: int = 0, wy0: int = 0):
        """``mpp_posnet_epilogue_win``: pos_out the crop's [3,ldh,ldw] float32 network output (contiguous); det an [h,w] float32
        view with unit column stride."""
        ldh, ldw = _planar_shape(pos_out, 3)
        h, w, ld = _window_view(det, 1)
        self._check(self._L.mpp_posnet_epilogue_win(self._h, H, W, ldh, ldw, _ptr(pos_out), float(div_w), float(div_b), int(wx0),
                                                    int(wy0), h, w, _ptr(det), ld))

    def shapenet_epilogue(self, logits, H: int, W: int, marks, *, wx0: int = 0, wy0: int = 0):
        """``mpp_shapenet_epilogue_win``: logits one head's [32,ldh,ldw] float32 crop output (contiguous); marks an [h,w,32]
        float32 view of a mark map with contiguous pixels."""
        ldh, ldw = _planar_shape(logits, NCLASS)
        h, w, ld = _window_view(marks, NCLASS)
        self._check(self._L.mpp_shapenet_epilogue_win(self._h, H, W, ldh, ldw, _ptr(logits), int(wx0), int(wy0), h, w,
                                                      _ptr(marks), ld))

    def posnet_epilogue_nhwc(self, pos_out, H: int, W: int, div_w: float, div_b: float, det, *, wx0: int = 0, wy0: int = 0):
        """``posnet_epilogue`` on a [1,3,ldh,ldw] channels-last (NHWC memory) float32 / bfloat16 network output"""
        ldh, ldw, ch = nhwc_shape(pos_out)
        if ch != 3:
            raise ValueError("posnet output must have 3 channels")
        h, w, ld = _window_view(det, 1)
        self._check(self._L.mpp_posnet_epilogue_nhwc_win(self._h, H, W, ldh, ldw, _ptr(pos_out), int(pos_out.element_size()),
                                                         float(div_w), float(div_b), int(wx0), int(wy0), h, w, _ptr(det), ld))

    def shapenet_epilogue_nhwc(self, logits, H: int, W: int, marks, *, wx0: int = 0, wy0: int = 0):
        """``shapenet_epilogue`` on a [1,32,ldh,ldw] channels-last (NHWC memory) float32 / bfloat16 head output"""
        ldh, ldw, ch = nhwc_shape(logits)
        if ch != NCLASS:
            raise ValueError(f"a shapenet head must have {NCLASS} channels")
        h, w, ld = _window_view(marks, NCLASS)
        self._check(self._L.mpp_shapenet_epilogue_nhwc_win(self._h, H, W, ldh, ldw, _ptr(logits), int(logits.element_size()),
                                                           int(wx0), int(wy0), h, w, _ptr(marks), ld))

    def affine_relu(self, x, scale, shift):
        """x <- max(0, x * scale[c] + shift[c]) in place; x: contiguous NCHW float32 / bfloat16 CUDA tensor"""
        n, ch = int(x.shape[0]), int(x.shape[1])
        hw = int(x.shape[2]) * int(x.shape[3])
        self._check(self._L.mpp_affine_relu(self._h, _ptr(x), n * ch, ch, hw, int(x.element_size()), _ptr(scale), _ptr(shift)))

    def nhwc_glue(self, x0, x1=None, pad: int = 1, pool: bool = False, scale=None, shift=None, out_dtype=None, out=None):
        """One pass between two convolutions on channels-last activations (``mpp_nhwc_glue``):
        reflect_pad(relu(affine(maxpool2(cat(x0, x1))))).  x0 / x1: [1,C,H,W] CUDA tensors with channels_last
        strides;
        returns a [1,C0+C1,H',W'] channels_last tensor (``out``: write there, e.g. ``x0`` itself for pad = 0)."""
        import torch
        h0, w0, c0 = nhwc_shape(x0)
        c1 = 0
        if x1 is not None:
            h1, w1, c1 = nhwc_shape(x1)
            if (h1, w1) != (h0, w0) or x1.dtype != x0.dtype:
                raise ValueError("nhwc_glue: the two sources differ in size or element type")
        H, W = (h0 // 2, w0 // 2) if pool else (h0, w0)
        if out is None:
            out = torch.empty((1, H + 2 * pad, W + 2 * pad, c0 + c1), dtype=out_dtype or x0.dtype, device=x0.device)
            out = out.permute(0, 3, 1, 2)
        self._check(self._L.mpp_nhwc_glue(self._h, _ptr(x0), _ptr(x1), _ptr(out), H, W, c0, c1, pad, 1 if pool else 0,
                                          int(x0.element_size()), int(out.element_size()), _ptr(scale), _ptr(shift)))
        return out

    def conv3x3_c32(self, x0, wp, x1=None, in_scale=None, in_shift=None, out_scale=None, out_shift=None, relu: bool = True, out=None):
        """3x3 reflect-padded convolution to 32 channels on channels-last float32 activations (``mpp_conv3x3_c32``):
        x0 (and x1, the second half of a concatenation): [1,32,H,W] CUDA tensors with channels_last strides; wp: the repacked
        weights [C_in/32, 9, 32, 32]; returns relu(conv * out_scale + out_shift) as a [1,32,H,W] channels_last tensor."""
        import torch
        h, w, c = nhwc_shape(x0)
        if c != 32 or x0.dtype != torch.float32 or (x1 is not None and nhwc_shape(x1) != (h, w, 32)):
            raise ValueError("conv3x3_c32: float32 channels-last sources of 32 channels")
        if out is None:
            out = torch.empty((1, h, w, 32), dtype=torch.float32, device=x0.device).permute(0, 3, 1, 2)
        self._check(self._L.mpp_conv3x3_c32(self._h, _ptr(x0), _ptr(x1), h, w, _ptr(wp), _ptr(in_scale), _ptr(in_shift),
                                            _ptr(out_scale), _ptr(out_shift), 1 if relu else 0, _ptr(out)))
        return out

    def conv3x3_stem(self, x, wp, scale, shift):
        """Conv2d(3 -> 32, 3x3, reflect) + folded BatchNorm + ReLU of a U-Net's stem (``mpp_conv3x3_stem``): x [1,3,H,W] float32
        with channels_last strides, wp [9,3,32]; returns a [1,32,H,W] channels_last tensor."""
        import torch
        h, w, c = nhwc_shape(x)
        if c != 3 or x.dtype != torch.float32 or tuple(wp.shape) != (9, 3, 32):
            raise ValueError("conv3x3_stem: a float32 channels-last picture of 3 channels, weights [9,3,32]")
        out = torch.empty((1, h, w, 32), dtype=torch.float32, device=x.device).permute(0, 3, 1, 2)
        self._check(self._L.mpp_conv3x3_stem(self._h, _ptr(x), h, w, _ptr(wp), _ptr(scale), _ptr(shift), _ptr(out)))
        return out

    def shapenet_heads(self, h, w, b, H: int, W: int, marks, *, wx0: int = 0, wy0: int = 0):
        """ShapeNet's three 1x1 heads + biases + softmax in one pass (``mpp_shapenet_heads_win``): h [1,32,ldh,ldw] float32
        channels_last, w [3,32,32] (head, class, input channel), b [3,32]; marks: three [h,w,32] float32 views of the mark maps
        with the same shape and strides (the window at (wx0, wy0), as for the epilogues above)."""
        import torch
        ldh, ldw, c = nhwc_shape(h)
        if c != 32 or h.dtype != torch.float32 or tuple(w.shape) != (3, 32, 32) or tuple(b.shape) != (3, 32) or len(marks) != 3:
            raise ValueError("shapenet_heads: float32 channels-last activations of 32 channels, w [3,32,32], b [3,32]")
        if not (w.is_contiguous() and b.is_contiguous()):
            raise ValueError("shapenet_heads: contiguous weights")
        views = [_window_view(m, NCLASS) for m in marks]
        if len(set(views)) != 1:
            raise ValueError("shapenet_heads: the three mark windows differ in shape or pitch")
        wh, ww, ld = views[0]
        self._check(self._L.mpp_shapenet_heads_win(self._h, H, W, ldh, ldw, _ptr(h), _ptr(w), _ptr(b), int(wx0), int(wy0), wh, ww,
                                                   _ptr(marks[0]), _ptr(marks[1]), _ptr(marks[2]), ld))

    # -- training the U-Nets (device tensors; asynchronous on the ctx's stream) -----------------------------------------
    def train_batch(self, data: TrainDataC, labels: TrainLabelsC, desc, P: int, flags: int, seed: int, epoch: int, batch: int,
                    out: dict):
        """``mpp_train_batch``: desc [B,3] int32 CUDA tensor (image, anchor row, anchor col); out: CUDA tensors by field name of
        ``TrainOutC`` (patch, sums and status required)."""
        import torch
        if desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != 3 or not desc.is_contiguous() or not desc.is_cuda:
            raise ValueError("desc must be a contiguous [B,3] int32 CUDA tensor")
        B = int(desc.shape[0])
        want = {"patch": (torch.float32, (B, 3, P, P)), "vec": (torch.float32, (B, 2, P, P)), "mask": (torch.float32, (B, P, P)),
                "dil": (torch.float32, (B, P, P)), "dist": (torch.float32, (B, P, P)), "cls": (torch.uint8, (3, B, P, P)),
                "cover": (torch.uint8, (B, P, P)), "sums": (torch.float64, (B, (P + TRAIN_BAND - 1) // TRAIN_BAND, 2)),
                "status": (torch.int32, (1,))}
        o = TrainOutC()
        for k, t in out.items():
            dt, shape = want[k]
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"train_batch: {k} must be a contiguous {dt} CUDA tensor of shape {shape}")
            setattr(o, k, t.data_ptr())
        self._check(self._L.mpp_train_batch(self._h, C.byref(data), C.byref(labels), B, int(P), _ptr(desc), int(flags),
                                            int(seed) & 0xffffffff, int(epoch) & 0xffffffff, int(batch) & 0xffffffff, C.byref(o)))

    def train_aug_params(self, flags: int, seed: int, epoch: int, batch: int, B: int, P: int, n_images: int) -> np.ndarray:
        """``mpp_train_aug_params``: what ``train_batch`` with the same arguments draws for each of its B patches, as a
        structured array of ``AUG_RECORD_DTYPE`` (synchronises the ctx's stream)"""
        import torch
        size = AUG_RECORD_DTYPE.itemsize
        out = torch.zeros((int(B), size), dtype=torch.uint8, device=torch.device("cuda", self.device))
        self._check(self._L.mpp_train_aug_params(self._h, int(flags), int(seed) & 0xffffffff, int(epoch) & 0xffffffff,
                                                 int(batch) & 0xffffffff, int(B), int(P), int(n_images), _ptr(out)))
        self.synchronize()
        return out.cpu().numpy().view(AUG_RECORD_DTYPE).reshape(int(B))

    def posnet_loss(self, out, vec, mask, dil, sums, res, grad=None, w=None, b=None):
        """``mpp_posnet_loss``: with w and b (float32 CUDA scalars) the training form with the divergence classifier"""
        B, P = int(out.shape[0]), int(out.shape[-1])
        with_div = w is not None
        self._check(self._L.mpp_posnet_loss(self._h, B, P, _ptr(out), _ptr(vec), _ptr(mask), _ptr(dil), _ptr(sums), int(with_div),
                                            _ptr(w), _ptr(b), _ptr(grad), _ptr(res)))

    def shapenet_loss(self, logits, cls, cover, sums, res, grads=None):
        """``mpp_shapenet_loss``: logits three [B,n,P,P] float32 CUDA tensors; grads three of the same shape or None"""
        B, nc, P = int(logits[0].shape[0]), int(logits[0].shape[1]), int(logits[0].shape[-1])
        g = list(grads) if grads is not None else [None, None, None]
        self._check(self._L.mpp_shapenet_loss(self._h, B, P, nc, _ptr(logits[0]), _ptr(logits[1]), _ptr(logits[2]), _ptr(cls),
                                              _ptr(cover), _ptr(sums), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(res)))

    # -- histogram matching and error-density resampling (device tensors; asynchronous on the ctx's stream) ---------------
    @staticmethod
    def _dev(name: str, t, dtype, shape=None):
        if t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
            raise ValueError(f"{name} must be a contiguous {dtype} CUDA tensor" + (f" of shape {tuple(shape)}" if shape else ""))
        return _ptr(t)

    def image_histograms(self, data: TrainDataC, hist):
        """``mpp_image_histograms``: hist [n_images,3,256] int32 CUDA tensor (the counts are unsigned)"""
        import torch
        self._check(self._L.mpp_image_histograms(self._h, C.byref(data), self._dev("hist", hist, torch.int32, (data.n_images, 3, 256))))

    def train_set_histograms(self, hist):
        """``mpp_train_set_histograms``: the table of ``image_histograms`` for the next ``train_batch`` calls (None: none);
        the caller keeps the tensor alive"""
        import torch
        if hist is None:
            self._check(self._L.mpp_train_set_histograms(self._h, None, 0))
            return
        if hist.dim() != 3 or tuple(hist.shape[1:]) != (3, 256):
            raise ValueError("hist must be [n_images,3,256]")
        self._check(self._L.mpp_train_set_histograms(self._h, self._dev("hist", hist, torch.int32), int(hist.shape[0])))

    def posnet_error_map(self, out, shape, centers, max_distance: float, dens, total, cell=None, crop=(0, 0), core=None):
        """``mpp_posnet_error_map``: out [3,ldh,ldw] float32 (the raw PosNet output of the crop whose pixel (0, 0) is image
        pixel ``crop``), shape (H, W) of the image, centers [n,2] int32 (None or empty: no objects), dens
        [ceil(H/8),ceil(W/8)] uint8, total [1] int64 (grows by the sum of the cells written), cell the float32 means or
        None; core (x0, x1, y0, y1): the cells to write (default: the whole image)."""
        import torch
        H, W = int(shape[0]), int(shape[1])
        ldh, ldw = _planar_shape(out, 3)
        cells = (-(-H // DENSITY_CELL), -(-W // DENSITY_CELL))
        x0, x1, y0, y1 = (0, H, 0, W) if core is None else (int(v) for v in core)
        n = 0 if centers is None else int(centers.shape[0])
        self._check(self._L.mpp_posnet_error_map(
            self._h, H, W, ldh, ldw, _ptr(out), int(crop[0]), int(crop[1]), x0, x1, y0, y1,
            self._dev("centers", centers, torch.int32) if n else None, n, float(max_distance),
            self._dev("dens", dens, torch.uint8, cells), self._dev("total", total, torch.int64, (1,)),
            None if cell is None else self._dev("cell", cell, torch.float32, cells)))

    def density_prefix(self, img_hw, cell_off, row_off, total_rows: int, dens, cellcum, rowcum):
        """``mpp_density_prefix``: img_hw [n,2] int32, cell_off / row_off [n] int64, dens uint8 and cellcum int32 (unsigned
        counts) of the same length, rowcum [total_rows] int64"""
        import torch
        n = int(img_hw.shape[0])
        self._check(self._L.mpp_density_prefix(
            self._h, n, self._dev("img_hw", img_hw, torch.int32, (n, 2)), self._dev("cell_off", cell_off, torch.int64, (n,)),
            self._dev("row_off", row_off, torch.int64, (n,)), int(total_rows), self._dev("dens", dens, torch.uint8),
            self._dev("cellcum", cellcum, torch.int32, dens.shape), self._dev("rowcum", rowcum, torch.int64, (int(total_rows),))))

    def density_anchors(self, img_hw, cell_off, row_off, cellcum, rowcum, rows, seed: int, epoch: int, anchors):
        """``mpp_density_anchors``: rows [n,2] int32 (image, plan row) -> anchors [n,2] int32"""
        import torch
        n_images, n = int(img_hw.shape[0]), int(rows.shape[0])
        self._check(self._L.mpp_density_anchors(
            self._h, n_images, self._dev("img_hw", img_hw, torch.int32, (n_images, 2)),
            self._dev("cell_off", cell_off, torch.int64, (n_images,)), self._dev("row_off", row_off, torch.int64, (n_images,)),
            self._dev("cellcum", cellcum, torch.int32), self._dev("rowcum", rowcum, torch.int64),
            n, self._dev("rows", rows, torch.int32, (n, 2)), int(seed) & 0xffffffff, int(epoch) & 0xffffffff,
            self._dev("anchors", anchors, torch.int32, (n, 2))))

    # -- dataset translation (device tensors; asynchronous on the ctx's stream) ----------------------------------------
    def rescale(self, src, tables, out=None, out_f64=None, workspace_limit: int = RESCALE_WORKSPACE):
        """``mpp_rescale``: src [H,W,3] uint8 CUDA tensor whose pixels are contiguous (rows may be further apart: a slice of
        a wider image); tables = (row_idx [oh,Tr] int32, row_w [oh,Tr] float64, col_idx [ow,Tc] int32, col_w [ow,Tc]
        float64), numpy, as ``dataset_translation.rescale_tables`` builds them; out [oh,ow,3] uint8 (made if None), out_f64
        the unquantised float64 values (True: made; a tensor: written).  Returns out, or (out, out_f64)."""
        import torch
        if not (_is_torch(src) and src.is_cuda and src.device.index == self.device and src.dtype == torch.uint8 and src.dim() == 3
                and src.shape[2] == 3 and src.stride(2) == 1 and src.stride(1) == 3 and (src.shape[0] == 1 or src.stride(0) >= 3 * src.shape[1])):
            raise ValueError(f"rescale: src must be a [H,W,3] uint8 tensor on GPU {self.device} with contiguous pixels")
        H, W = int(src.shape[0]), int(src.shape[1])
        ri, rw, ci, cw = tables
        ri, ci = np.ascontiguousarray(ri, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32)
        rw, cw = np.ascontiguousarray(rw, dtype=np.float64), np.ascontiguousarray(cw, dtype=np.float64)
        if ri.ndim != 2 or ci.ndim != 2 or ri.shape != rw.shape or ci.shape != cw.shape:
            raise ValueError("rescale: tables must be (row_idx, row_w, col_idx, col_w) with [n_out, taps] each")
        (oh, tr), (ow, tc) = ri.shape, ci.shape
        if out is None:
            out = torch.empty((oh, ow, 3), dtype=torch.uint8, device=src.device)
        if out_f64 is True:
            out_f64 = torch.empty((oh, ow, 3), dtype=torch.float64, device=src.device)
        elif out_f64 is False:
            out_f64 = None
        self._check(self._L.mpp_rescale(self._h, _ptr(src), H, W, int(src.stride(0)) if H > 1 else 3 * W, _ptr(ri), _ptr(rw), oh, tr,
                                        _ptr(ci), _ptr(cw), ow, tc, self._dev("out", out, torch.uint8, (oh, ow, 3)),
                                        None if out_f64 is None else self._dev("out_f64", out_f64, torch.float64, (oh, ow, 3)),
                                        int(workspace_limit)))
        return out if out_f64 is None else (out, out_f64)

    # -- the result pictures (synchronous: the picture is complete on return) ------------------------------------------
    def draw_outlines(self, base, corners=None, colors=None, lut=None, vmin: float = 0.0, vmax: float = 1.0, out=None):
        """``mpp_draw_outlines``: base a contiguous float32 CUDA tensor, [H,W,3] (the picture, 0..1) or [H,W] (a scalar map:
        clipped to [vmin, vmax] and looked up in ``lut`` [256,3] float32, numpy); corners [n,4,2] int32 (row, col) and colors
        [n,3] float32, numpy (None or empty: the base picture alone).  Returns out, [H,W,3] uint8 CUDA tensor (made if None)."""
        import torch
        if not (_is_torch(base) and base.is_cuda and base.device.index == self.device and base.dtype == torch.float32
                and base.is_contiguous() and (base.dim() == 2 or (base.dim() == 3 and base.shape[2] == 3))):
            raise ValueError(f"draw_outlines: base must be a contiguous float32 [H,W,3] or [H,W] tensor on GPU {self.device}")
        H, W = int(base.shape[0]), int(base.shape[1])
        scalar = base.dim() == 2
        if scalar:
            if lut is None:
                raise ValueError("draw_outlines: a scalar base needs a lut")
            lut = np.ascontiguousarray(lut, dtype=np.float32)
            if lut.shape != (256, 3):
                raise ValueError("draw_outlines: lut must be [256,3]")
        corners = np.zeros((0, 4, 2), np.int32) if corners is None else np.ascontiguousarray(corners, dtype=np.int32)
        colors = np.zeros((0, 3), np.float32) if colors is None else np.ascontiguousarray(colors, dtype=np.float32)
        n = int(corners.shape[0])
        if corners.shape != (n, 4, 2) or colors.shape != (n, 3):
            raise ValueError("draw_outlines: corners must be [n,4,2] and colors [n,3]")
        if out is None:
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=base.device)
        self._check(self._L.mpp_draw_outlines(self._h, H, W, None if scalar else _ptr(base), _ptr(base) if scalar else None,
                                              float(vmin), float(vmax), _ptr(lut) if scalar else None, n,
                                              _ptr(corners) if n else None, _ptr(colors) if n else None,
                                              self._dev("out", out, torch.uint8, (H, W, 3))))
        return out

    # -- evaluation --------------------------------------------------------------------------------
    def quad_iou(self, a, b) -> np.ndarray:
        """IoU matrix [n][m] of convex quads a [n][8] and b [m][8] (-1: axis-aligned extents apart)."""
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 8))
        b = np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1, 8))
        out = np.zeros((len(a), len(b)), np.float64)
        self._check(self._L.mpp_quad_iou(self._h, len(a), _ptr(a), len(b), _ptr(b), _ptr(out), 0))
        return out


def nhwc_shape(x):
    """(H, W, C) of a [1,C,H,W] tensor whose memory is NHWC (channels_last strides); raises otherwise."""
    import torch
    if x.dim() != 4 or x.shape[0] != 1 or not x.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("expected a [1,C,H,W] tensor in channels_last memory format")
    return int(x.shape[2]), int(x.shape[3]), int(x.shape[1])


def _planar_shape(x, channels: int):
    """(ldh, ldw) of a contiguous float32 [channels,ldh,ldw] (or [1,channels,ldh,ldw]) tensor; raises otherwise."""
    import torch
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[0] != 1) \
            or x.shape[-3] != channels:
        raise ValueError(f"expected a contiguous float32 [{channels},H,W] tensor")
    return int(x.shape[-2]), int(x.shape[-1])


def _window_view(v, channels: int):
    """(h, w, row pitch in pixels) of a float32 window view: [h,w] with unit column stride (channels 1) or [h,w,channels] with
    contiguous pixels (a slice of a larger map); raises otherwise."""
    import torch
    shape = (int(v.shape[0]), int(v.shape[1])) if v.dim() >= 2 else None
    ok = v.dtype == torch.float32 and v.is_cuda and shape is not None and v.dim() == (2 if channels == 1 else 3)
    if ok and channels > 1:
        ok = int(v.shape[2]) == channels and v.stride(2) == 1 and v.stride(1) == channels and v.stride(0) % channels == 0
    elif ok:
        ok = v.stride(1) == 1
    if not ok or (shape[0] > 1 and v.stride(0) < channels * shape[1]):
        raise ValueError(f"expected a float32 CUDA window view [h,w{',' + str(channels) if channels > 1 else ''}] with contiguous "
                         "pixels and rows at least one window row apart")
    return shape[0], shape[1], max(v.stride(0) // channels, shape[1])


def philox(ctr, key) -> np.ndarray:
    L = load_library()
    c = np.ascontiguousarray(ctr, dtype=np.uint32)
    k = np.ascontiguousarray(key, dtype=np.uint32)
    o = np.zeros(4, np.uint32)
    L.mpp_philox4x32(_ptr(c), _ptr(k), _ptr(o))
    return o
