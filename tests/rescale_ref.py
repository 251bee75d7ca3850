"""The scipy restatement of skimage 0.18.1 ``rescale(image, scale, anti_aliasing=True, multichannel=True)`` for scale <= 1,
from its published code (``skimage/transform/_warps.py``: ``rescale`` -> ``resize`` -> ``warp``), float64 throughout:

* output shape ``np.round(scale * (H, W))``; per axis ``f = n_in / n_out``;
* ``ndi.gaussian_filter(image, sigma=(max(0, (f - 1) / 2) per axis, 0 for the channels), mode='mirror')`` (skimage's
  'reflect' is ndimage's 'mirror'; truncate 4);
* order-1 warp with the map ``src = f (dst + 0.5) - 0.5`` per axis.  skimage gets that map from a least-squares
  ``AffineTransform.estimate`` on the corner points, whose coefficients carry rounding noise of a few ulps; the exact map is
  used here.  For scale <= 1 the sample points lie inside the image, so the warp's boundary mode never acts;
* ``clip=True``: to the input's own min / max.

``to_uint8`` is what ``plt.imsave`` stores: ``(v * 255).astype(uint8)``, a truncation.

``resize_ref`` is the same restatement with the output size given per axis; ``apply_tables`` evaluates the kernels' formula
for any tap tables in float64 or ``np.longdouble`` (``rescale_cases.py``).
"""
import numpy as np
from scipy import ndimage as ndi


def output_shape(H, W, scale):
    oh, ow = np.round(scale * np.array([H, W], dtype=np.float64)).astype(int)
    return int(oh), int(ow)


def _lerp_axis(a, n_out, axis):
    n_in = a.shape[axis]
    x = (n_in / n_out) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5
    i0 = np.floor(x).astype(np.int64)
    t = x - i0
    i1 = np.minimum(i0 + 1, n_in - 1)
    shape = [1] * a.ndim
    shape[axis] = n_out
    t = t.reshape(shape)
    return (1.0 - t) * np.take(a, i0, axis=axis) + t * np.take(a, i1, axis=axis)


def rescale_ref(u8, scale):
    """uint8 [H,W,C] -> float64 [oh,ow,C] in [0, 1]"""
    img = np.asarray(u8, dtype=np.float64) / 255
    H, W = img.shape[:2]
    oh, ow = output_shape(H, W, scale)
    sigma = (max(0.0, (H / oh - 1) / 2), max(0.0, (W / ow - 1) / 2), 0.0)
    blurred = ndi.gaussian_filter(img, sigma, cval=0, mode='mirror')
    out = _lerp_axis(_lerp_axis(blurred, oh, 0), ow, 1)
    return np.clip(out, img.min(), img.max())


def resize_ref(u8, oh, ow):
    """the same steps with the output size given per axis (skimage's ``resize(anti_aliasing=True)``, which ``rescale`` calls):
    the two axes may take different factors.  uint8 [H,W,C] -> float64 [oh,ow,C] in [0, 1]"""
    img = np.asarray(u8, dtype=np.float64) / 255
    H, W = img.shape[:2]
    sigma = (max(0.0, (H / oh - 1) / 2), max(0.0, (W / ow - 1) / 2), 0.0)
    blurred = ndi.gaussian_filter(img, sigma, cval=0, mode='mirror')
    out = _lerp_axis(_lerp_axis(blurred, oh, 0), ow, 1)
    return np.clip(out, img.min(), img.max())


def apply_tables(u8, row_idx, row_w, col_idx, col_w, dtype=np.float64):
    """The formula in the header of ``csrc/mpp_rescale.hip`` for any tables, without clip or truncation:
    ``out[i][j][c] = sum_t wr[i][t] * sum_s wc[j][s] * src[ir[i][t]][ic[j][s]][c] / 255``, evaluated in ``dtype`` by NumPy's own
    sums (pairwise, not the kernels' ascending fused chain).  ``dtype=np.longdouble`` is the yardstick for tables that no
    scipy restatement covers."""
    x = np.asarray(u8).astype(dtype) / dtype(255)
    ri, ci = np.asarray(row_idx, dtype=np.int64), np.asarray(col_idx, dtype=np.int64)
    rw, cw = np.asarray(row_w).astype(dtype), np.asarray(col_w).astype(dtype)
    across = (x[:, ci, :] * cw[None, :, :, None]).sum(axis=2)            # [H, ow, C]
    return (across[ri] * rw[:, :, None, None]).sum(axis=1)               # [oh, ow, C]


def to_uint8(v):
    return (np.asarray(v) * 255).astype(np.uint8)
