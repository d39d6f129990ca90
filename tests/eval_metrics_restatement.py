"""NumPy restatement of the test-time metrics of Modelbuilder.forward -- JDR, the PCK counts of calculate_err / calc_pck, and
EPEmean -- in this project's own words, with the layouts of et_eval_jdr / et_eval_pck / et_eval_epe (include/epipolar_amd.h).
Pinned to what the real reference returned (tests/golden/lifting/eval_metrics.npz, made by tests/golden/make_eval_metrics_golden.py) by
tests/test_eval_metrics_cpu.py; where the reference tree is absent (the GPU tests) it stands in for it on random shapes.

Everything is float64 arithmetic on exactly the operands the reference uses, one rounding per operation, so the results are
bit-equal to the reference's -- except the mean of EPEmean, an exactly rounded sum here (math.fsum) against the reference's
unspecified summation order: `mean_bound` is the bound between any two orders of the same terms."""
import math

import numpy as np

THRESHOLDS = (1, 2, 5, 10, 20, 30, 40, 50, 60, 80, 100)      # the reference's cfg.TEST.THRESHOLDS
MAX_TH = 20                                                   # cfg.TEST.MAX_TH
MAPPING = (0, 1, 2, 3, 4, 5, 6, 7, 9, 11, 12, 14, 15, 16, 17, 18, 19)      # DATASETS.H36M.MAPPING: 17 of 20 channels


def curve_points(max_threshold=MAX_TH):
    return np.linspace(0, max_threshold, num=int(max_threshold))


def peaks(maps):
    """(N,J,H,W) float32 -> (N,J,2) float32: (x, y) of each map's first maximum, (0, 0) unless that maximum is > 0."""
    n, j, h, w = maps.shape
    flat = maps.reshape(n, j, h * w)
    idx = flat.argmax(-1)                                     # first occurrence; -0.0 == +0.0
    top = np.take_along_axis(flat, idx[..., None], -1)[..., 0]
    xy = np.stack([idx % w, idx // w], -1).astype(np.float32)
    return xy * (top > 0)[..., None].astype(np.float32)


def jdr(pred, target, thr=0.5):
    """-> dists (J,N) float64, acc (J+1,) float64, pred_xy, target_xy (N,J,2) float32.  A target at x <= 1 or y <= 1 does not
    count (-1).  normalize = (H / 10, W / 10) divides (x, y) in that order: x by the HEIGHT term, as the reference does."""
    n, j, h, w = pred.shape
    pxy, txy = peaks(pred), peaks(target)
    scale = np.array([h / 10, w / 10])
    d = pxy.astype(np.float64) / scale - txy.astype(np.float64) / scale
    dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    counts = (txy[..., 0] > 1) & (txy[..., 1] > 1)
    dists = np.where(counts, dist, -1.0).T.copy()
    acc = np.zeros(j + 1)
    total, used = 0.0, 0
    for c in range(j):
        row = dists[c][dists[c] != -1]
        acc[1 + c] = (row < thr).sum() / row.size if row.size else -1.0
        if acc[1 + c] >= 0:
            total += acc[1 + c]
            used += 1
    acc[0] = total / used if used else np.nan
    return dists, acc, pxy, txy


def jdr_margin(dists, thr=0.5):
    """Smallest |dist - thr| over the counted distances that are not exactly thr (inf: none)."""
    d = dists[(dists != -1) & (dists != thr)]
    return float(np.abs(d - thr).min()) if d.size else math.inf


def pck_errors(locs, gt, vis=None):
    """The errors calculate_err thresholds -- the x difference ALONE (its `[:1, j]` takes the first row) -- and which count."""
    err = np.abs(locs[..., 0].astype(np.float64) - gt[..., 0])
    counts = np.ones(err.shape, bool) if vis is None else vis != 0
    return err, counts


def pck(locs, gt, vis=None, thresholds=THRESHOLDS, curve=None):
    """locs (N,J,2) float32, gt (N,J,2) float64, vis (N,J) or None -> pck (T,), err_joints (N,M), total_joints (N,) float64."""
    curve = curve_points() if curve is None else np.asarray(curve, np.float64)
    err, counts = pck_errors(locs, gt, vis)
    total = counts.sum(1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        hit = np.array([np.float64(((err < th) & counts).sum()) * 100.0 / np.float64(counts.sum()) for th in thresholds], np.float64)
    err_joints = np.stack([((err < c) & counts).sum(1) for c in curve], 1).astype(np.float64) if len(curve) else np.zeros((len(err), 0))
    return hit.reshape(len(thresholds)), err_joints, total


def pck_margin(locs, gt, vis=None, thresholds=THRESHOLDS, curve=None):
    curve = curve_points() if curve is None else np.asarray(curve, np.float64)
    err, counts = pck_errors(locs, gt, vis)
    marks = np.concatenate([np.asarray(thresholds, np.float64).ravel(), curve])
    return float(np.abs(err[counts][:, None] - marks[None]).min()) if counts.any() and marks.size else math.inf


def epe_errors(pred, gt, unit=1.0, max_dist=150.0):
    d = pred.astype(np.float64) - gt.astype(np.float64)
    e = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * np.float64(unit)
    return np.where(e > max_dist, np.float64(max_dist), e)


def epe(pred, gt, vis=None, unit=1.0, max_dist=150.0):
    """pred, gt (F,J,3) float64 -> mean (float64, visibility does not enter it), per_joint (F,J) with invisible items 0."""
    e = epe_errors(pred, gt, unit, max_dist)
    per_joint = e if vis is None else np.where(vis != 0, e, 0.0)
    return np.float64(math.fsum(e.ravel().tolist()) / e.size), per_joint


def mean_bound(errors):
    """|difference| between two summation orders of the same n terms, divided by n: 2 (n - 1) 2^-53 sum / n."""
    n = errors.size
    return 2.0 * (n - 1) * 2.0 ** -53 * float(errors.sum()) / n


# ---- inputs for shapes the fixture does not hold -------------------------------------------------------------------------------
def blob_maps(rng, centres, h, w, height=1.0):
    """(N,J,H,W) float32: zeros with a 3 x 3 bump whose top sits at centres (N,J,2) = (x, y) -- sparse, as target heat maps are."""
    n, j, _ = centres.shape
    maps = np.zeros((n, j, h, w), np.float32)
    for a in range(n):
        for b in range(j):
            x, y = int(centres[a, b, 0]), int(centres[a, b, 1])
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if 0 <= y + dy < h and 0 <= x + dx < w:
                        maps[a, b, y + dy, x + dx] = np.float32(height * (0.5 if dx or dy else 1.0) * rng.uniform(0.9, 1.0))
            maps[a, b, y, x] = np.float32(height)
    return maps


def random_maps(n, j, h, w, seed):
    """Predicted and target maps with every kind of item: targets anywhere (those at x <= 1 or y <= 1 do not count), predictions
    0-3 pixels off, a few maps without a positive value, a few with their maximum twice (the first must win), sparse noise."""
    rng = np.random.default_rng(seed)
    t_xy = np.stack([rng.integers(0, w, (n, j)), rng.integers(0, h, (n, j))], -1)
    off = rng.integers(-3, 4, (n, j, 2)) * (rng.random((n, j, 1)) < 0.7)
    p_xy = np.clip(t_xy + off, 0, [w - 1, h - 1])
    target, pred = blob_maps(rng, t_xy, h, w), blob_maps(rng, p_xy, h, w, 0.8)
    pred += (rng.random(pred.shape) < 0.004) * rng.uniform(-0.3, 0.3, pred.shape).astype(np.float32)
    for maps in (pred, target):
        kind = rng.random((n, j))
        for a, b in zip(*np.nonzero(kind < 0.1)):                       # nothing positive: all zero, or all negative
            maps[a, b] = 0 if rng.random() < 0.5 else -np.abs(maps[a, b]) - np.float32(0.25)
        for a, b in zip(*np.nonzero(kind > 0.85)):                      # the maximum a second time, somewhere later or earlier
            flat = maps[a, b].reshape(-1)
            flat[rng.integers(0, flat.size)] = flat.max()
    return np.ascontiguousarray(pred, np.float32), np.ascontiguousarray(target, np.float32)


def random_points2d(n, j, seed, vis="mixed"):
    """locs float32, gt float64 with errors from a fraction of a pixel to beyond the largest threshold; vis None | zeros | mixed."""
    rng = np.random.default_rng(seed)
    locs = rng.uniform(0, 256, (n, j, 2)).astype(np.float32)
    gt = locs.astype(np.float64) + rng.normal(0, 1, (n, j, 2)) * rng.choice([0.5, 4.0, 30.0, 90.0], (n, j, 1))
    v = {"none": None, "zeros": np.zeros((n, j), np.float32), "mixed": (rng.random((n, j)) < 0.7).astype(np.float32)}[vis]
    return locs, gt, v


def random_points3d(f, j, seed, vis="mixed"):
    rng = np.random.default_rng(seed)
    gt = rng.normal(0, 500, (f, j, 3))
    pred = gt + rng.normal(0, 1, (f, j, 3)) * rng.choice([5.0, 30.0, 80.0], (f, j, 1))
    v = {"none": None, "zeros": np.zeros((f, j), np.float32), "mixed": (rng.random((f, j)) < 0.7).astype(np.float32)}[vis]
    return pred, gt, v
