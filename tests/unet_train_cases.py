"""Inputs of the U-Net training fixture (tests/golden/unet_train_golden.npz): regenerated from seeded generators by the
fixture's generator and by the tests, so that only recorded outputs are stored."""
import numpy as np

LOSS_B, LOSS_P = 3, 24          # PosNet loss cases: the last patch has no object (mask and dil all zero)
CE_B, CE_P = 3, 16              # ShapeNet loss cases: the last patch has no object (loss_mask all zero)
DIV_W, DIV_B = -10.812359809875488, -2.128434181213379
LABEL_P = 48


def posnet_loss_inputs(seed=11):
    rng = np.random.default_rng(seed)
    B, P = LOSS_B, LOSS_P
    out = (rng.normal(0, 1.5, size=(B, 3, P, P))).astype(np.float32)
    mask = (rng.random((B, P, P)) < 0.3).astype(np.float32)
    ang = rng.uniform(0, 2 * np.pi, size=(B, P, P))
    vec = (np.stack([np.cos(ang), np.sin(ang)], axis=1) * mask[:, None]).astype(np.float32)
    dil = (rng.random((B, P, P)) * (rng.random((B, P, P)) < 0.1)).astype(np.float32)
    mask[-1] = 0
    vec[-1] = 0
    dil[-1] = 0
    return out, vec, mask, dil


def shapenet_loss_inputs(seed=12):
    rng = np.random.default_rng(seed)
    B, P = CE_B, CE_P
    logits = [rng.normal(0, 2.0, size=(B, 32, P, P)).astype(np.float32) for _ in range(3)]
    cls = rng.integers(0, 32, size=(3, B, P, P)).astype(np.int64)
    cover = rng.random((B, P, P)) < 0.25
    cover[-1] = False
    loss_mask = np.zeros((B, P, P))
    for b in range(B - 1):
        loss_mask[b] = cover[b] / np.sum(cover[b])
    return logits, cls, cover, loss_mask


def label_patches():
    """three P x P patches as (centres [n,2] int64, params [n,3] (a, b, angle)): touching objects, objects cut by the border,
    and an empty patch"""
    P = LABEL_P
    c0 = np.array([[20, 20], [20, 29], [29, 20], [31, 31], [10, 40]], dtype=np.int64)
    p0 = np.array([[4.0, 9.0, 0.0], [4.5, 9.5, np.pi / 2], [5.0, 8.0, 0.3], [3.5, 10.0, 2.4], [6.0, 12.0, 1.1]])
    c1 = np.array([[0, 5], [2, P - 1], [P - 1, 20], [P - 3, P - 2], [24, 0], [23, 3]], dtype=np.int64)
    p1 = np.array([[6.0, 11.0, 0.7], [5.0, 9.0, 2.0], [4.0, 14.0, 0.1], [7.0, 9.0, 1.4], [4.0, 8.0, 3.0], [4.2, 8.4, 0.05]])
    c2 = np.zeros((0, 2), dtype=np.int64)
    p2 = np.zeros((0, 3))
    return [(c0, p0), (c1, p1), (c2, p2)]


def density_images():
    """image shapes and object counts for the patch-plan densities"""
    shapes = np.array([[300, 420], [1024, 768], [128, 2000], [512, 512]])
    n_objects = np.array([70, 5, 0, 1200])
    return shapes, n_objects
