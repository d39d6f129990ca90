"""NumPy float64 restatement of KEYPOINT.TRIANGULATION pymvg / naive / refine, written from the semantics of
include/epipolar_amd.h (et_triangulate_views) -- the oracle of the tests for shapes the reference-made fixtures
(tests/golden/triangulation.npz, tests/golden/lifting/triangulation_ransac.npz) do not hold.  Not a product path: plain loops and
numpy's SVD and inverse (`dlt`, `ray_distance` of triangulation_epipolar_restatement.py).

    X, info, margin = triangulate_views(pts, conf, krt, method=, conf_thres=, ransac_thres=)

pts (F,V,J,2), conf (F,V,J), krt (F,V,3,4), all float32.  X (F,J,3) float64, info (F,J) int32 (bits 0-7 views selected, 8-15 views
the point was computed from, 18 zeros written, 24-30 threshold steps of pymvg).  `margin`: the smallest |d - ransac_thres| /
ransac_thres over every inlier distance computed (inf for pymvg, which computes none) -- a test that compares decisions with
another implementation asserts that it is far above rounding."""
import numpy as np

from triangulation_epipolar_restatement import dlt, ray_distance

INFO_ZEROS = 1 << 18
STEPS_SHIFT = 24
METHODS = ("pymvg", "naive", "refine")


def bits(views):
    return sum(1 << v for v in views)


def pymvg_joint(pts, conf, P, conf_thres):
    """The threshold steps down by REPEATED float64 subtraction and is compared as a float32 with the float32 scores."""
    c = conf.astype(np.float32)
    t, steps = float(conf_thres), 0
    while True:
        sel = [v for v in range(len(c)) if c[v] > np.float32(t)]
        if t < -1 or len(sel) > 1:
            break
        t -= 0.05
        steps += 1
    word = bits(sel) | steps << STEPS_SHIFT
    if len(sel) < 2:
        return np.zeros(3), word | INFO_ZEROS
    return dlt([(P[v], pts[v, 0], pts[v, 1]) for v in sel]), word | bits(sel) << 8


def ransac_joint(pts, conf, P, conf_thres, ransac_thres, refine):
    """Returns X, info, the inlier distances computed."""
    sel = [v for v in range(len(conf)) if np.float32(conf[v]) > np.float32(conf_thres)]
    mask = bits(sel)
    if len(sel) < 2:
        return np.zeros(3), mask | INFO_ZEROS, []
    best, best_p, best_in, best_pair, dists = 0, None, [], None, []
    for i, a in enumerate(sel):
        for b in sel[i + 1:]:
            p = dlt([(P[a], pts[a, 0], pts[a, 1]), (P[b], pts[b, 0], pts[b, 1])])
            d = [ray_distance(P[v], pts[v, 0], pts[v, 1], p) for v in sel]
            dists += d
            inl = [v for v, dv in zip(sel, d) if dv < ransac_thres]
            if len(inl) > best:
                best, best_p, best_in, best_pair = len(inl), p, inl, (a, b)
    if best == 0:
        return np.zeros(3), mask | INFO_ZEROS, dists
    if refine and best > 1:
        return dlt([(P[v], pts[v, 0], pts[v, 1]) for v in best_in]), mask | bits(best_in) << 8, dists
    return best_p, mask | bits(best_pair) << 8, dists


def triangulate_views(pts, conf, krt, *, method, conf_thres, ransac_thres=3.0):
    assert method in METHODS
    F, V, J, _ = pts.shape
    X = np.zeros((F, J, 3))
    info = np.zeros((F, J), np.int32)
    margin = np.inf
    for f in range(F):
        P = krt[f].astype(np.float64)
        for j in range(J):
            p2 = pts[f, :, j].astype(np.float64)
            if method == "pymvg":
                X[f, j], info[f, j] = pymvg_joint(p2, conf[f, :, j], P, conf_thres)
                continue
            X[f, j], info[f, j], dists = ransac_joint(p2, conf[f, :, j], P, conf_thres, float(ransac_thres), method == "refine")
            if dists:
                margin = min(margin, float(np.min(np.abs(np.asarray(dists) - ransac_thres))) / ransac_thres)
    return X, info, margin


def random_scene(F, V, J, seed, conf_thres=0.85, size=1024.0):
    """Float32 inputs (pts, conf, krt) and the planted joints X_true (F,J,3): V jittered ring cameras per frame, detections
    with 1.5 px noise, and per joint one of eight kinds of scores around `conf_thres`:
      0 all views above            1 all above, one a confident outlier      2 all above, only two views right
      3 ONE view above, the others far below: several steps down             4 none above
      5 one score == float32(conf_thres) (not above it), one == nextafter of it (above), the rest below: one step down
        only if the boundary is handled in float32
      6 all-zero scores: the threshold ends negative                         7 mixed, wrong where the score is low"""
    from epipolar_transformers_amd import synthetic as syn

    rng = np.random.default_rng(seed)
    t32 = np.float32(conf_thres)
    pts = np.zeros((F, V, J, 2))
    conf = np.zeros((F, V, J), np.float32)
    krt = np.zeros((F, V, 3, 4))
    truth = np.zeros((F, J, 3))
    for f in range(F):
        krt[f] = syn.ring_cameras(V, size, jitter=(0.02, 5.0), rng=rng)
        truth[f] = X = np.array([0, 0, 900.0]) + rng.normal(0, 300, (J, 3))
        xh = np.einsum("vik,nk->vni", krt[f], np.concatenate([X, np.ones((J, 1))], 1))
        pts[f] = xh[..., :2] / xh[..., 2:] + rng.normal(0, 1.5, (V, J, 2))
        for j in range(J):
            kind = (f + j) % 8
            conf[f, :, j] = rng.uniform(conf_thres + 0.01, conf_thres + 0.15, V)
            if kind == 1:
                pts[f, rng.integers(V), j] += rng.uniform(60, 120, 2)
            elif kind == 2 and V > 2:
                wrong = rng.permutation(V)[2:]
                pts[f, wrong, j] += rng.choice([-1, 1], (len(wrong), 2)) * rng.uniform(90, 150, (len(wrong), 2))
            elif kind == 3:
                conf[f, :, j] = rng.uniform(conf_thres - 0.6, conf_thres - 0.2, V)
                conf[f, rng.integers(V), j] = conf_thres + 0.1
            elif kind == 4:
                conf[f, :, j] = rng.uniform(conf_thres - 0.7, conf_thres - 0.07, V)
            elif kind == 5:
                conf[f, :, j] = rng.uniform(conf_thres - 0.04, conf_thres - 0.01, V)
                conf[f, 0, j] = t32
                conf[f, V - 1, j] = np.nextafter(t32, np.float32(2))       # (V = 1: this one stands)
            elif kind == 6:
                conf[f, :, j] = 0.0
            elif kind == 7:
                conf[f, :, j] = rng.uniform(conf_thres - 0.25, conf_thres + 0.15, V)
                low = conf[f, :, j] <= t32
                pts[f, low, j] += rng.normal(0, 40, (int(low.sum()), 2))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return (f32(pts), f32(conf), f32(krt)), truth
