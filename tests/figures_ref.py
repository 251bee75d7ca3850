"""NumPy restatement of the result pictures: the line rule, list-order overwrite, compose and the 8-bit rule.

Written from the rules as DESIGN.md section 11 states them, not from the kernel: the rectangles are drawn one after another
in list order, each by walking its four edges pixel by pixel into the float picture, and the float picture is then turned
into bytes the way ``matplotlib.pyplot.imsave`` does it for a float32 array.
"""
import numpy as np


def line_pixels(p0, p1):
    """[(row, col)] of the integer 8-connected Bresenham walk from p0 to p1, both (row, col), end points included"""
    (y0, x0), (y1, x1) = (int(p0[0]), int(p0[1])), (int(p1[0]), int(p1[1]))
    dx, dy = abs(x1 - x0), -abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    err = dx + dy
    out = []
    while True:
        out.append((y0, x0))
        if x0 == x1 and y0 == y1:
            return out
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            x0 += sx
        if e2 <= dx:
            err += dx
            y0 += sy


def corners_of(polys):
    """float corners [n,4,2] -> int32, truncated toward zero"""
    return np.asarray(polys, dtype=np.float64).reshape(-1, 4, 2).astype(np.int32)


def outline_pixels(corners):
    """the pixels of one closed outline: edge k runs from corner k to corner (k + 1) % 4"""
    out = []
    for k in range(4):
        out += line_pixels(corners[k], corners[(k + 1) % 4])
    return out


def draw(base, corners, colors):
    """float32 picture [H,W,3] with the outlines drawn in list order (a later rectangle overwrites an earlier one);
    pixels outside the picture are skipped one by one"""
    img = np.array(base, dtype=np.float32, copy=True)
    H, W = img.shape[:2]
    for q, c in zip(np.asarray(corners).reshape(-1, 4, 2), np.asarray(colors, dtype=np.float32).reshape(-1, 3)):
        for (r, col) in outline_pixels(q):
            if 0 <= r < H and 0 <= col < W:
                img[r, col] = c
    return img


def to_bytes(img):
    """the 8-bit rule of ``plt.imsave`` for a float32 RGB array in 0..1: ``(x * 255).astype(np.uint8)`` in float32; a pixel
    with a NaN channel becomes 0"""
    x = np.array(img, dtype=np.float32, copy=True)
    x[np.any(np.isnan(x), axis=2)] = 0
    return (x * np.float32(255)).astype(np.uint8)


def scalar_base(m, lut, vmin, vmax):
    """a scalar map through a 256-entry table: clipped to [vmin, vmax], index min(255, int((v - vmin) / (vmax - vmin) * 256))
    in float64"""
    v = np.clip(np.asarray(m, dtype=np.float64), vmin, vmax)
    idx = np.minimum(255, ((v - vmin) / (vmax - vmin) * 256.0).astype(np.int64))
    return np.asarray(lut, dtype=np.float32)[idx]


def picture(base, corners, colors):
    """uint8 [H,W,3]: what the device composes for an RGB base"""
    return to_bytes(draw(base, corners, colors))


def score_colors(scores):
    """the reference's colour of a score: plasma(clip(score / max_score, 0, max_score))[:3], max_score the largest score"""
    from matplotlib import pyplot as plt
    scores = [float(s) for s in scores]
    max_score = 1.0 if len(scores) == 0 else max(scores)
    cm = plt.get_cmap("plasma")
    return np.array([cm(np.clip(s / max_score, 0, max_score))[:3] for s in scores], dtype=np.float32).reshape(-1, 3)
