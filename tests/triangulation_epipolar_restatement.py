"""NumPy float64 restatement of KEYPOINT.TRIANGULATION epipolar / epipolar_dlt, written from the semantics of
include/epipolar_amd.h (et_triangulate_epipolar) -- the oracle of the tests for shapes the reference-made fixture
(tests/golden/lifting/triangulation_epipolar.npz) does not hold.  Not a product path: plain loops, numpy's SVD and inverse.

    X, info, margin = triangulate_epipolar(pts, conf, krt, other_krt, corr_pos, downsample=, resize=, conf_thres=,
                                           ransac_thres=, dlt=)

pts (F,V,J,2), conf (F,V,J), krt / other_krt (F,V,3,4), corr_pos (F,V,H,W,2), all float32.  X (F,J,3) float64, info (F,J) int32
(bits 0-7 selected views, 8-15 views the point was computed from, 16-17 branch, 18 no inlier, 19 lookup clamped).  `margin`:
the smallest |d - ransac_thres| / ransac_thres over every inlier distance computed -- a test that compares decisions with
another implementation asserts that it is far above rounding."""
import numpy as np

INFO_NO_INLIER = 1 << 18
INFO_CLAMPED = 1 << 19


def dlt(rows):
    """rows: list of (P (3,4), x, y).  Right singular vector of the smallest singular value, de-homogenised."""
    A = []
    for P, x, y in rows:
        A.append(x * P[2] - P[0])
        A.append(y * P[2] - P[1])
    vt = np.linalg.svd(np.asarray(A, dtype=np.float64))[2]
    return vt[-1, :3] / vt[-1, 3]


def ray_distance(P, x, y, p):
    A = P[:, :3]
    inv = np.linalg.inv(A)
    c = -inv @ P[:, 3]
    x1 = inv @ np.array([x, y, 1.0]) + c
    return np.linalg.norm(np.cross(x1 - p, c - p)) / np.linalg.norm(x1 - c)


def _index(q, size):
    """Python's int() on the map coordinate, clamped into [0, size) -> (index, clamped)."""
    if not np.isfinite(q):
        return (size - 1 if not q < size else 0), True
    i = int(q)
    if i < 0:
        return 0, True
    if i >= size:
        return size - 1, True
    return i, False


def triangulate_joint(pts, conf, krt, other_krt, corr_pos, ds, resize, conf_thres, ransac_thres, use_dlt):
    """One (frame, joint): pts (V,2), conf (V,), krt / other_krt (V,3,4), corr_pos (V,H,W,2).  Returns X, info, distances."""
    V = pts.shape[0]
    P = krt.astype(np.float64)
    p2 = pts.astype(np.float64)
    sel = [v for v in range(V) if np.float32(conf[v]) > np.float32(conf_thres)]
    branch = 0
    if not sel:
        sel, branch = [int(np.argmax(conf))], 2
    elif len(sel) == 1:
        branch = 1
    mask = sum(1 << v for v in sel)
    if branch:
        v = sel[0]
        H, W = corr_pos.shape[1:3]
        q = (p2[v] / resize + 0.5 - ds / 2.0) / ds
        ix, cx = _index(q[0], W)
        iy, cy = _index(q[1], H)
        o = (corr_pos[v, iy, ix].astype(np.float64) * ds + ds / 2.0 - 0.5) * resize
        X = dlt([(P[v], p2[v, 0], p2[v, 1]), (other_krt[v].astype(np.float64), o[0], o[1])])
        return X, mask | mask << 8 | branch << 16 | (INFO_CLAMPED if cx or cy else 0), []
    if use_dlt:
        return dlt([(P[v], p2[v, 0], p2[v, 1]) for v in sel]), mask | mask << 8, []
    best, best_p, best_in, best_pair, dists = 0, None, [], None, []
    for a in sel:
        for b in sel:
            if a == b:
                continue
            p = dlt([(P[a], p2[a, 0], p2[a, 1]), (P[b], p2[b, 0], p2[b, 1])])
            d = [ray_distance(P[v], p2[v, 0], p2[v, 1], p) for v in sel]
            dists += d
            inl = [v for v, dv in zip(sel, d) if dv < ransac_thres]
            if len(inl) > best:
                best, best_p, best_in, best_pair = len(inl), p, inl, (a, b)
    if best == 0:
        return np.zeros(3), mask | INFO_NO_INLIER, dists
    if best > 2:
        return dlt([(P[v], p2[v, 0], p2[v, 1]) for v in best_in]), mask | sum(1 << v for v in best_in) << 8, dists
    return best_p, mask | ((1 << best_pair[0]) | (1 << best_pair[1])) << 8, dists


def triangulate_epipolar(pts, conf, krt, other_krt, corr_pos, *, downsample, resize, conf_thres, ransac_thres, dlt=False):
    F, V, J, _ = pts.shape
    X = np.zeros((F, J, 3))
    info = np.zeros((F, J), np.int32)
    margin = np.inf
    ds, resize = float(np.float32(downsample)), float(np.float32(resize))
    for f in range(F):
        for j in range(J):
            X[f, j], word, dists = triangulate_joint(pts[f, :, j], conf[f, :, j], krt[f], other_krt[f], corr_pos[f], ds, resize,
                                                     conf_thres, float(ransac_thres), dlt)
            info[f, j] = word
            if dists:
                margin = min(margin, float(np.min(np.abs(np.asarray(dists) - ransac_thres))) / ransac_thres)
    return X, info, margin


def random_scene(F, V, J, seed, hw=16, ds=64.0, resize=1.0):
    """Float32 inputs (pts, conf, krt, other_krt, corr_pos) and the planted joints X_true (F,J,3) of F frames that take every branch: V jittered ring cameras per
    frame (view v's source is v+1), detections with 1.5 px noise, per joint one of: all views confident, a confident
    outlier, only two views right, one confident view, none confident -- and, for some of the last two, a detection far
    outside the image, so that the corr_pos lookup is clamped on every side."""
    from epipolar_transformers_amd import synthetic as syn

    rng = np.random.default_rng(seed)
    size = hw * ds * resize
    pts = np.zeros((F, V, J, 2))
    conf = np.zeros((F, V, J))
    krt = np.zeros((F, V, 3, 4))
    truth = np.zeros((F, J, 3))
    for f in range(F):
        krt[f] = syn.ring_cameras(V, size, jitter=(0.02, 5.0 * resize), rng=rng)
        truth[f] = X = np.array([0, 0, 900.0]) + rng.normal(0, 300, (J, 3))
        xh = np.einsum("vik,nk->vni", krt[f], np.concatenate([X, np.ones((J, 1))], 1))
        pts[f] = xh[..., :2] / xh[..., 2:] + rng.normal(0, 1.5 * resize, (V, J, 2))
        for j in range(J):
            kind = (f + j) % 6
            conf[f, :, j] = rng.uniform(0.86, 1.0, V)
            if kind == 1:
                pts[f, rng.integers(V), j] += rng.uniform(60, 120, 2) * resize
            elif kind == 2 and V > 2:
                wrong = rng.permutation(V)[2:]
                pts[f, wrong, j] += rng.choice([-1, 1], (len(wrong), 2)) * rng.uniform(90, 150, (len(wrong), 2)) * resize
            elif kind == 3:
                conf[f, :, j] = rng.uniform(0.6, 1.0, V)
            elif kind >= 4:
                conf[f, :, j] = rng.uniform(0.1, 0.8, V)
                v = rng.integers(V)
                if kind == 4:
                    conf[f, v, j] = 0.9
                if (f + j) % 4 < 2:
                    v = int(np.argmax(conf[f, :, j]))
                    pts[f, v, j] = [(-3.0, 0.4), (1.7, 0.5), (0.3, -0.02), (0.6, 1.2)][(f + j // 2) % 4] * np.array([size, size])
    corr = rng.uniform(0, hw - 1, (F, V, hw, hw, 2))
    src = np.roll(np.arange(V), -1)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return (f32(pts), f32(conf), f32(krt), f32(krt[:, src]), f32(corr)), truth
