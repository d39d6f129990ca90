"""NumPy float64 restatement of KEYPOINT.TRIANGULATION rpsm (modeling/pictorial_cuda.py:17-254), written from the recipe in
include/epipolar_amd.h (et_rpsm), not from the kernel.  Besides the pose and the chosen bins it reports how close every decision
on the chosen path was, so that a test can tell a float32 rounding from an error:

  margins[f, level]      the smallest relative gap (best - runner-up DISTINCT value) / best over every arg-max on the chosen path
                         (the root's, and for every limb the row of the parent's chosen bin); inf where best <= 0 or all equal
  band_margin[f, level]  in mm: over those rows, how far |d - L| is from the tolerance for the chosen child bin and for every
                         incompatible child bin whose energy would have tied or beaten the winner (>= best * (1 - 1e-4), > 0)

Level 0 is the first stage, level k the k-th recursion.  A (parent, child) compatibility test |sqrt(d2) + 1e-9 - L| < tol is
evaluated on d2 (lo^2 < d2 < hi^2, the same set in exact arithmetic); the reported band distances use the stated form.
"""
import numpy as np

H36M_PARENT = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)
PAIR_EPS, DIST_EPS = 1e-6, 1e-9
MARGIN, BAND_MARGIN = 1e-4, 1e-2


def tree(parent):
    parent = [int(p) for p in parent]
    J = len(parent)
    root = parent.index(-1)
    level = [0] * J
    for j in range(J):
        k, lv = j, 0
        while k != root:
            k, lv = parent[k], lv + 1
        level[j] = lv
    limb_of, e = [-1] * J, 0
    for j in range(J):
        if j != root:
            limb_of[j], e = e, e + 1
    children = [[k for k in range(J) if parent[k] == j] for j in range(J)]
    return root, level, limb_of, children


def grid_sample(img, gx, gy, align_corners):
    """F.grid_sample(img[None, None], grid, mode='bilinear', padding_mode='zeros') at normalised (gx, gy)."""
    H, W = img.shape
    if align_corners:
        ix, iy = (gx + 1) / 2 * (W - 1), (gy + 1) / 2 * (H - 1)
    else:
        ix, iy = ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2
    ok = np.isfinite(ix) & np.isfinite(iy) & (ix > -1) & (ix < W) & (iy > -1) & (iy < H)
    ix, iy = np.where(ok, ix, -1.0), np.where(ok, iy, -1.0)
    x0, y0 = np.floor(ix), np.floor(iy)
    out = np.zeros_like(ix)
    for xx, yy, wgt in ((x0, y0, (x0 + 1 - ix) * (y0 + 1 - iy)), (x0 + 1, y0, (ix - x0) * (y0 + 1 - iy)),
                        (x0, y0 + 1, (x0 + 1 - ix) * (iy - y0)), (x0 + 1, y0 + 1, (ix - x0) * (iy - y0))):
        inside = ok & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        xi, yi = np.clip(xx, 0, W - 1).astype(np.int64), np.clip(yy, 0, H - 1).astype(np.int64)
        out = out + np.where(inside, img[yi, xi] * wgt, 0.0)
    return out


def positions(axes):
    """axes (3, n) -> (n^3, 3), bin b = (ix * n + iy) * n + iz."""
    gx, gy, gz = np.meshgrid(axes[0], axes[1], axes[2], indexing="ij")
    return np.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], 1)


def unary(heat_fj, cams_f, trans_f, X, image_size, align_corners):
    """heat_fj (V,H,W) of one joint; X (B,3): the sum over the views, ascending, of one bilinear sample."""
    V, H, W = heat_fj.shape
    total = None
    for v in range(V):
        p = X @ cams_f[v][:, :3].T + cams_f[v][:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            xy = p[:, :2] / p[:, 2:3]
            xy = xy @ trans_f[v][:, :2].T + trans_f[v][:, 2]
            xy = xy * np.array([W, H], np.float64) / np.asarray(image_size, np.float64)
            g = xy / np.array([H - 1, W - 1], np.float64) * 2.0 - 1.0          # x by H - 1: the reference's
        s = grid_sample(heat_fj[v], g[:, 0], g[:, 1], align_corners)
        total = s if total is None else total + s
    return total


def band_distance(xa, xc, L):
    """|d - L| with d = ||x_a - x_c + 1e-6|| + 1e-9, xa (3,), xc (B,3)."""
    return np.abs(np.sqrt(((xa - xc + PAIR_EPS) ** 2).sum(-1)) + DIST_EPS - L)


def message(axes_p, axes_c, E_c, L, tol):
    """max_c compat(a, c) * E_c[c] and its first arg-max for every parent bin a."""
    n = axes_p.shape[1]
    lo, hi = L - tol - DIST_EPS, L + tol - DIST_EPS
    d2 = [(axes_p[k][:, None] - axes_c[k][None, :] + PAIR_EPS) ** 2 for k in range(3)]
    B = n ** 3
    best, arg = np.empty(B), np.empty(B, np.int64)
    Ec = E_c.reshape(1, 1, n, n, n)
    for ix in range(n):                                          # a slab of n^2 parent bins at a time
        dd = (d2[0][ix][None, None, :, None, None] + d2[1][:, None, None, :, None] + d2[2][None, :, None, None, :])
        ok = dd < hi * hi if hi > 0 else np.zeros(dd.shape, bool)
        if lo > 0:
            ok &= dd > lo * lo
        val = np.where(ok, Ec, 0.0).reshape(n * n, B)
        a = val.argmax(1)
        arg[ix * n * n:(ix + 1) * n * n] = a
        best[ix * n * n:(ix + 1) * n * n] = val[np.arange(n * n), a]
    return best, arg


def gap(values, best):
    """(best - runner-up distinct value) / best; inf where that says nothing."""
    lower = values[values < best]
    if not best > 0 or lower.size == 0:
        return np.inf
    return float((best - lower.max()) / best)


def stage(heat_f, cams_f, trans_f, axes, L, parent, image_size, tol, align_corners):
    """One level for one frame.  axes (J,3,n): every joint's grid (the first stage passes J copies of one).  Returns the chosen
    bins (J,), the new pose (J,3), the smallest arg-max gap and the smallest band distance."""
    root, level, limb_of, children = tree(parent)
    J = len(parent)
    pos = [positions(axes[j]) for j in range(J)]
    U = [unary(heat_f[:, j], cams_f, trans_f, pos[j], image_size, align_corners) for j in range(J)]
    E, M, BP = [None] * J, [None] * J, [None] * J
    for j in sorted(range(J), key=lambda q: -level[q]):          # deepest first
        e = U[j].copy()
        for c in children[j]:
            e = e * M[c]
        E[j] = e
        if j != root:
            M[j], BP[j] = message(axes[parent[j]], axes[j], e, L[limb_of[j]], tol)
    bins = np.zeros(J, np.int64)
    bins[root] = int(np.argmax(E[root]))
    margin, band = gap(E[root], E[root][bins[root]]), np.inf
    for j in sorted(range(J), key=lambda q: level[q]):
        if j == root:
            continue
        p = parent[j]
        a = bins[p]
        bins[j] = BP[j][a]
        dist = band_distance(pos[p][a], pos[j], L[limb_of[j]])
        ok = dist < tol
        row = np.where(ok, E[j], 0.0)
        best = row[bins[j]]
        if best != M[j][a] or bins[j] != int(np.argmax(row)):    # the d2 form and the stated form part only AT the band's edge
            band = 0.0
        margin = min(margin, gap(row, best))
        if ok[bins[j]]:
            band = min(band, float(tol - dist[bins[j]]))
        rivals = ~ok & (E[j] > 0) & (E[j] >= best * (1 - MARGIN))
        if rivals.any():
            band = min(band, float((dist[rivals] - tol).min()))
    return bins, np.stack([pos[j][bins[j]] for j in range(J)]), margin, band


def rpsm(heat, cams, trans, center, limb_length, *, first_limb_length=None, parent=H36M_PARENT, image_size, grid_size, first_nbins,
         recur_nbins, recur_depth, tolerance, align_corners=False):
    """heat (F,V,J,H,W), cams (F,V,3,4), trans (F,V,2,3), center (F,3), limb_length (F,E) or (E,).  Returns pose (F,J,3) float64,
    path (F,1+depth,J) int64, margins (F,1+depth), band_margin (F,1+depth)."""
    heat, cams, trans, center = [np.asarray(a, np.float64) for a in (heat, cams, trans, center)]
    F, V, J = heat.shape[:3]
    limb = np.broadcast_to(np.asarray(limb_length, np.float64), (F, J - 1))
    first = limb if first_limb_length is None else np.broadcast_to(np.asarray(first_limb_length, np.float64), (F, J - 1))
    pose = np.zeros((F, J, 3))
    path = np.zeros((F, 1 + recur_depth, J), np.int64)
    margins = np.full((F, 1 + recur_depth), np.inf)
    band = np.full((F, 1 + recur_depth), np.inf)
    for f in range(F):
        size = float(grid_size)
        axes = np.linspace(-size / 2, size / 2, first_nbins)[None, :] + center[f][:, None]
        axes = np.broadcast_to(axes, (J, 3, first_nbins))
        bins, cur, margins[f, 0], band[f, 0] = stage(heat[f], cams[f], trans[f], axes, first[f], parent, image_size, float(tolerance),
                                                     align_corners)
        path[f, 0] = bins
        size /= first_nbins
        for k in range(1, recur_depth + 1):
            axes = np.linspace(-size / 2, size / 2, recur_nbins)[None, None, :] + cur[:, :, None]
            bins, cur, margins[f, k], band[f, k] = stage(heat[f], cams[f], trans[f], axes, limb[f], parent, image_size,
                                                         float(tolerance), align_corners)
            path[f, k] = bins
            size /= recur_nbins
        pose[f] = cur
    return pose, path, margins, band


def level_size(grid_size, first_nbins, recur_nbins, k):
    """The grid size of level k (0: the first stage)."""
    return float(grid_size) if k == 0 else float(grid_size) / first_nbins / recur_nbins ** (k - 1)


def crop_transform_three_point(center, scale, image_size):
    """get_affine_transform(center, scale, 0, image_size) (data/transforms/image.py:226-258) with cv2.getAffineTransform
    replaced by the float64 solve of its three-point system; the points are rounded to float32 as the reference builds them."""
    scale = np.array([scale, scale], np.float64) if np.ndim(scale) == 0 else np.asarray(scale, np.float64)
    center = np.asarray(center, np.float64)
    src_w, dst_w, dst_h = scale[0] * 200.0, image_size[0], image_size[1]
    src, dst = np.zeros((3, 2), np.float32), np.zeros((3, 2), np.float32)
    src[0] = center
    src[1] = center + np.array([0.0, src_w * -0.5])
    dst[0] = [dst_w * 0.5, dst_h * 0.5]
    dst[1] = np.array([dst_w * 0.5, dst_h * 0.5]) + np.array([0, dst_w * -0.5], np.float32)
    third = lambda a, b: b + np.array([-(a - b)[1], (a - b)[0]], np.float32)
    src[2], dst[2] = third(src[0], src[1]), third(dst[0], dst[1])
    return affine_from_points(src, dst)


def affine_from_points(src, dst):
    """The 2 x 3 map that takes the three points src to dst: what cv2.getAffineTransform documents, solved in float64."""
    A = np.concatenate([np.asarray(src, np.float64), np.ones((3, 1))], 1)
    return np.linalg.solve(A, np.asarray(dst, np.float64)).T


# ---------------------------------------------------------------------------------------------------------------- scenes
def sample_pixel(X, cam, trans, image_size, H, W, align_corners=False):
    """Where the unary term samples heat map (H, W) for world points X (N,3): un-normalised (ix, iy), float64."""
    p = X @ cam[:, :3].T + cam[:, 3]
    xy = p[:, :2] / p[:, 2:3]
    xy = xy @ trans[:, :2].T + trans[:, 2]
    xy = xy * np.array([W, H], np.float64) / np.asarray(image_size, np.float64)
    g = xy / np.array([H - 1, W - 1], np.float64) * 2.0 - 1.0
    if align_corners:
        return (g[:, 0] + 1) / 2 * (W - 1), (g[:, 1] + 1) / 2 * (H - 1)
    return ((g[:, 0] + 1) * W - 1) / 2, ((g[:, 1] + 1) * H - 1) / 2


def ring_rig(V, rng):
    """V cameras on a ring of 5 m around (0, 0, 900) mm, 1024 x 1024 images: K (V,3,3), RT (V,3,4), float64."""
    Ks, RTs = [], []
    for i in range(V):
        ang = (2 * i + 0.5) * np.pi / V + rng.normal(0, 0.05)
        c = np.array([5000 * np.cos(ang), 5000 * np.sin(ang), 1500.0 + rng.normal(0, 50)])
        fwd = np.array([0, 0, 900.0]) - c
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, [0, 0, 1.0])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])
        f = 1145.0 + rng.normal(0, 5)
        Ks.append(np.array([[f, 0, 512.0 + rng.normal(0, 3)], [0, f, 515.0 + rng.normal(0, 3)], [0, 0, 1]]))
        RTs.append(np.concatenate([R, (-R @ c)[:, None]], 1))
    return np.stack(Ks), np.stack(RTs)


def frame(seed, V, J, H, W, *, image_size=(256, 256), box=500.0, shift_view=None, zero_joint=None, first_scale=None,
          align_corners=False, sigma=1.5, noise=0.02, parent=None):
    """One frame's float32 inputs: a random pose on `parent` (J entries, the root has -1; None: the first J joints of the H36M
    tree) with limbs of 200-400 mm -- limb e ends at the e-th non-root joint in ascending order --, Gaussians of
    `sigma` map pixels where the unary term will look for each joint plus `noise` * uniform clutter, rounded to float16 values
    (that is how the fixture stores them).  shift_view: that view's crop box is moved by 60 % of its width, so part of every grid
    samples outside the map; zero_joint: that joint's maps are zero in every view."""
    rng = np.random.default_rng(seed)
    parent = H36M_PARENT[:J] if parent is None else tuple(int(p) for p in parent)
    assert len(parent) == J
    root = parent.index(-1)
    K, RT = ring_rig(V, rng)
    X = np.zeros((J, 3))
    X[root] = np.array([0, 0, 900.0]) + rng.normal(0, 100, 3)
    placed, pending = {root}, [j for j in range(J) if j != root]
    while pending:                                               # ascending passes, a joint once its parent stands (H36M: one pass)
        before = len(pending)
        for j in list(pending):
            if parent[j] in placed:
                d = rng.normal(0, 1, 3)
                X[j] = X[parent[j]] + d / np.linalg.norm(d) * rng.uniform(200, 400)
                placed.add(j)
                pending.remove(j)
        assert len(pending) < before, "parent is not a tree with one root"
    cams = (K @ RT).astype(np.float32)
    trans = np.zeros((V, 2, 3), np.float32)
    centers = np.zeros((V, 2), np.float32)
    heat = np.zeros((V, J, H, W), np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    for v in range(V):
        p = X.mean(0) @ cams[v].astype(np.float64)[:, :3].T + cams[v].astype(np.float64)[:, 3]
        c = p[:2] / p[2] + rng.normal(0, 5, 2)
        if v == shift_view:
            c = c + np.array([0.6 * box, 0.0])
        centers[v] = c
        trans[v] = crop_transform_three_point(centers[v], box / 200.0, image_size)
        ix, iy = sample_pixel(X, cams[v].astype(np.float64), trans[v].astype(np.float64), image_size, H, W, align_corners)
        for j in range(J):
            heat[v, j] = np.exp(-((xx - ix[j]) ** 2 + (yy - iy[j]) ** 2) / (2 * sigma ** 2)) + noise * rng.uniform(0, 1, (H, W))
    if zero_joint is not None:
        heat[:, zero_joint] = 0
    heat = heat.astype(np.float16).astype(np.float32)
    limb = np.array([np.linalg.norm(X[j] - X[parent[j]]) for j in range(J) if j != root], np.float32)
    out = dict(heat=heat, cams=cams, trans=trans, center=(X[root] + rng.normal(0, 30, 3)).astype(np.float32), limb_length=limb, X_true=X,
               box_center=centers, box_scale=np.float32(box / 200.0))
    if first_scale is not None:
        out["first_limb_length"] = (limb * first_scale).astype(np.float32)
    return out


ARRAYS = ("heat", "cams", "trans", "center", "limb_length")


def run(fr, params, parent=None):
    """The restatement on one frame dict (or a stacked scene) with `params` (the keyword arguments of rpsm) on the tree `parent`
    (None: the H36M prefix of the scene's joint count)."""
    one = fr["heat"].ndim == 4
    args = [fr[k][None] if one else fr[k] for k in ARRAYS]
    first = fr.get("first_limb_length")
    return rpsm(*args, first_limb_length=None if first is None else (first[None] if one else first),
                parent=H36M_PARENT[:fr["heat"].shape[-3]] if parent is None else parent, **params)


def condition_holds(margins, band):
    return bool((margins >= MARGIN).all() and (band >= BAND_MARGIN).all())


def scene(seed, F, V, J, H, W, params, log=None, parent=None, **kw):
    """F frames whose every decision on the chosen path is clear (margins >= 1e-4, band_margin >= 1e-2 mm): frame i starts from
    seed + 1000 * i, and a seed that violates the condition is replaced by the next one (reported through `log`).  Returns the
    stacked float32 arrays and the restatement's (pose, path, margins, band_margin).  `parent`: the tree (None: the H36M prefix)."""
    frames, results = [], []
    for i in range(F):
        s = seed + 1000 * i
        while True:
            fr = frame(s, V, J, H, W, image_size=params["image_size"], align_corners=params.get("align_corners", False),
                       parent=parent, **kw)
            res = run(fr, params, parent)
            if condition_holds(res[2], res[3]):
                break
            if log is not None:
                log("seed %d replaced (margin %.2e, band %.2e mm)" % (s, res[2].min(), res[3].min()))
            s += 1
        frames.append(fr)
        results.append(res)
    stacked = {k: np.ascontiguousarray(np.stack([fr[k] for fr in frames])) for k in frames[0]}
    return stacked, tuple(np.concatenate([r[i] for r in results]) for i in range(4))
