"""NumPy restatement of the training loss of Modelbuilder.forward -- Heatmapcreator.get's targets and the criteria KEYPOINT.LOSS
names, joint / smoothmse / mse, with their gradients for the prediction -- in this project's own words, with the layouts of
et_heatmap_targets / et_heatmap_loss / et_heatmap_loss_bwd (include/epipolar_amd.h).  Pinned to what the real reference returned
(tests/golden/training/heatmap_loss.npz, made by tests/golden/make_heatmap_loss_golden.py) by tests/test_heatmap_loss_cpu.py.

  targets()   float64, bit-equal to Heatmapcreator.get; the kernels return them rounded once to float32
  terms()     the float32 term of every element, the reference's operations one by one, each rounded once
  loss()      float32(exactly rounded float64 sum of the terms / denominator)
  grad()      every element in float64 from the float32 difference, rounded once to float32
The reference sums in float32 in an order of its own and makes three float32 roundings per gradient element: the bounds between
it and this are the maker's conditions 3-5, restated by loss_bound() and the ulp helpers."""
import math

import numpy as np

KINDS = ("joint", "smoothmse", "mse")
CLIP = 4.60517019
THRESHOLD = 400.0
# the issue's cases: name -> (N, J, H, W, sigma, downsample); gradients are stored for all but `main`
CASES = {
    "tiny": (1, 1, 9, 7, 8.0, 4),
    "small": (3, 4, 10, 12, 8.0, 4),
    "odd": (2, 3, 17, 19, 12.0, 4),
    "main": (2, 17, 64, 64, 8.0, 4),
    "smooth_hot": (3, 4, 10, 12, 8.0, 4),
}
WEIGHT_VALUES = np.array([0, 0.25, 0.5, 0.7, 1], np.float32)


# ---- targets -------------------------------------------------------------------------------------------------------------------------
def grid_values(count, sigma, downsample):
    """float32: (float32 index * downsample + (downsample / 2.0 - 0.5)) / (sigma * 2**.5), every operation in float32."""
    s = np.float32(sigma * 2 ** .5)
    index = np.arange(count, dtype=np.float32)
    return (index * np.float32(downsample) + np.float32(downsample / 2.0 - 0.5)) / s


def targets(points, h, w, sigma, downsample):
    """points (N,J,2) float64 (u, v) -> (N,J,H,W) float64.  v pairs with the rows, u with the columns."""
    s = sigma * 2 ** .5
    r = points[..., 1, None] / s - grid_values(h, sigma, downsample).astype(np.float64)          # (N,J,H)
    c = points[..., 0, None] / s - grid_values(w, sigma, downsample).astype(np.float64)          # (N,J,W)
    q = (r * r)[..., :, None] + (c * c)[..., None, :]
    return np.exp(-np.clip(q, 0, CLIP))


def midpoint_distance(values):
    """The smallest relative distance of a float64 value from the middle between two neighbouring float32 values."""
    v = np.abs(np.asarray(values, np.float64)).reshape(-1)
    near = v.astype(np.float32)
    other = np.where(near.astype(np.float64) <= v, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf)))
    middle = (near.astype(np.float64) + other.astype(np.float64)) / 2
    return float((np.abs(v - middle) / v).min())


# ---- terms, loss, gradient -----------------------------------------------------------------------------------------------------------
def _weights(weight, n, j):
    return np.ones((n, j, 1, 1), np.float32) if weight is None else np.asarray(weight, np.float32).reshape(n, j, 1, 1)


def difference(kind, pred, gt, weight=None):
    """The float32 difference the term and the gradient are built from, and the weight broadcast to it."""
    n, j = pred.shape[:2]
    w = _weights(weight, n, j)
    if kind == "joint":
        return pred * w - gt * w, w
    return (gt - pred, w) if kind == "smoothmse" else (pred - gt, w)


def smooth_raw(d, w):
    return (d * d) * w


def terms(kind, pred, gt, weight=None):
    assert pred.dtype == np.float32 and gt.dtype == np.float32
    d, w = difference(kind, pred, gt, weight)
    if kind != "smoothmse":
        return d * d
    t = smooth_raw(d, w)
    hot = t > np.float32(THRESHOLD)
    # float32 pow as the correctly rounded value, times the scalar as float32
    replaced = np.power(t.astype(np.float64), 0.1, where=hot, out=np.ones(t.shape)).astype(np.float32) * np.float32(THRESHOLD ** 0.9)
    return np.where(hot, replaced, t)


def denominator(kind, shape, weight=None, per_joint=False):
    n, j, h, w = shape
    if kind == "joint":
        return float(n * h * w * (1 if per_joint else j))
    if kind == "mse":
        return float(n * j * h * w)
    total = float(n * j) if weight is None else math.fsum(np.asarray(weight, np.float32).reshape(-1).astype(np.float64))
    return float(h * w) * max(1.0, total)


def loss(kind, pred, gt, weight=None, per_joint=False):
    t = terms(kind, pred, gt, weight)
    return np.float32(math.fsum(t.astype(np.float64).reshape(-1)) / denominator(kind, pred.shape, weight, per_joint))


def grad(kind, pred, gt, weight=None, per_joint=False, grad_out=1.0):
    d, w = difference(kind, pred, gt, weight)
    c = float(np.float32(grad_out)) / denominator(kind, pred.shape, weight, per_joint)
    d64, w64 = d.astype(np.float64), w.astype(np.float64)
    if kind == "mse":
        return (2.0 * d64 * c).astype(np.float32)
    if kind == "joint":
        return (2.0 * d64 * w64 * c).astype(np.float32)
    g = -2.0 * d64 * w64 * c
    t = smooth_raw(d, w)
    hot = t > np.float32(THRESHOLD)
    factor = 0.1 * np.power(t.astype(np.float64), -0.9, where=hot, out=np.ones(t.shape)) * THRESHOLD ** 0.9
    return np.where(hot, g * factor, g).astype(np.float32)


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------
def loss_bound(kind, shape, value):
    """Condition 3: any float32 summation order of the M terms of one mean, the J means and the division stays within relative
    (M + J + 1) * 2**-24 of the exact sum.  M = N*H*W for joint, everything for the other two (one sum)."""
    n, j, h, w = shape
    m = n * h * w if kind == "joint" else n * j * h * w
    return (m + j + 1) * 2.0 ** -24 * abs(float(value))


def ulp32(x):
    """The spacing of float32 at |x| (at least the smallest normal's)."""
    x = np.maximum(np.abs(np.asarray(x, np.float32)), np.float32(2.0 ** -126))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def ulps_apart(a, b):
    """|a - b| in units of float32's spacing at b, elementwise (float64)."""
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / ulp32(b)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def case_inputs(name, seed):
    """pred (N,J,H,W) float32, points (N,J,2) float64, weight (N,J) float32 of a case.  Points run from 12 px outside the image to
    12 px inside along both axes, some lie anywhere inside and one far outside, so blobs are cut by every edge and a map is all
    background; weights come from WEIGHT_VALUES
    with at least one 0 and one fractional value (a single-map case takes a fractional one).  pred is a multiple of 2**-7 (it
    compresses, and its products with the weights stay inexact); `smooth_hot` scales part of it so that 2-3 % of the smoothmse
    terms exceed 400."""
    n, j, h, w, sigma, downsample = CASES[name]
    rng = np.random.default_rng(seed)
    pred = (rng.integers(-96, 160, (n, j, h, w)) / 128.0).astype(np.float32)
    extent = np.array([w * downsample, h * downsample], np.float64)
    points = rng.uniform(-12.0, 12.0, (n, j, 2)) + np.where(rng.random((n, j, 2)) < 0.5, 0.0, extent)
    inside = rng.random((n, j)) < 0.4                                  # some blobs in the middle of the map too
    points[inside] = rng.uniform(0, 1, (int(inside.sum()), 2)) * extent
    if n * j >= 6:                                                     # and one far outside: a map that is all background
        points.reshape(-1, 2)[rng.integers(0, n * j)] = (-60.0, extent[1] + 45.0)
    weight = WEIGHT_VALUES[rng.integers(0, 5, (n, j))]
    flat = weight.reshape(-1)
    if flat.size >= 2:
        flat[rng.permutation(flat.size)[:2]] = (0.0, 0.7)
    else:
        flat[0] = 0.7
    if name == "smooth_hot":
        hot = rng.random(pred.shape) < 0.055
        pred = np.where(hot, pred * np.float32(64.0), pred).astype(np.float32)
    return pred, points, weight
