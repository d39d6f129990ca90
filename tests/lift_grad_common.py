"""What tests/test_lift_grad_cpu.py and tests/test_gpu_lift_grad.py share: the scenes, the two float64 yardsticks of the liftings'
gradient, the condition on the inputs, the tolerance and the host hook's call.

The reference's liftings run in NumPy / cv2 / pymvg and have no autograd, so the gradient cannot be frozen from them (the forward
is pinned to them elsewhere).  The yardstick is float64 torch autograd through torch.linalg.svd on the DLT rows that the info word
of the NumPy RESTATEMENT names (triangulation_views_restatement / triangulation_epipolar_restatement) -- never a decision or a
value of the library.  A second, independent float64 route -- the implicit formula of include/epipolar_amd.h from np.linalg.svd --
is a condition on the inputs only: on every joint tested the two must agree within 2^-30 of the joint's largest gradient element
(a scene that breaks it gets another seed; the bound is not widened and no joint is excluded).

Tolerance of ONE joint, derived and not tuned:  |g - g_ref| <= 2^-23 x max |g_ref| over the joint's 2 V elements.  Half of it is the
single float32 rounding on the store (2^-24 of the element, at most of the largest); the other half is room for the float64
algorithm, which the condition shows to be about a thousand times smaller."""
import ctypes
import functools

import numpy as np
import torch

import triangulation_epipolar_restatement as epi
import triangulation_views_restatement as views

CONDITION = 2.0 ** -30
TOLERANCE = 2.0 ** -23
VIEWS_KW = dict(conf_thres=0.85, ransac_thres=35.0)
EPIPOLAR_KW = dict(downsample=64.0, resize=1.0, conf_thres=0.85, ransac_thres=35.0)
GX = (0.3, -1.1, 0.7)
NULL = ctypes.c_void_p(0)


def used_views(word):
    return [v for v in range(8) if word >> (8 + v) & 1]


def branch(word):
    return word >> 16 & 3


def grad_outs(F, J, seed=0):
    """The upstream gradients every scene is tested with: one constant, one random per joint; (F, J, 3) float64."""
    return [np.ascontiguousarray(np.broadcast_to(np.asarray(GX), (F, J, 3))),
            np.random.default_rng(1000 + seed).normal(0, 1, (F, J, 3))]


class Scene:
    """Inputs of one lifting call and the restatement's info word for them.  `arrays`: (pts, conf, krt) or (pts, conf, krt,
    other_krt, corr_pos); `method`: pymvg | naive | refine | epipolar | epipolar_dlt."""

    def __init__(self, arrays, method):
        self.arrays, self.method = arrays, method
        self.pts, self.conf, self.krt = arrays[:3]
        self.other, self.corr = (arrays[3], arrays[4]) if len(arrays) == 5 else (None, None)
        self.F, self.V, self.J, _ = self.pts.shape
        if self.other is None:
            self.X, self.info, margin = views.triangulate_views(*arrays, method=method, **VIEWS_KW)
        else:
            self.X, self.info, margin = epi.triangulate_epipolar(*arrays, dlt=method == "epipolar_dlt", **EPIPOLAR_KW)
        assert margin >= 1e-6                                 # no decision hangs on rounding
        self._refs = {}

    def rows(self, f, j):
        """The DLT the info word names, as a list of (P (3,4) float64, view or None, (x, y)): `view` None marks the constant
        correspondence row pair of the single-view branches.  Empty: no point was computed."""
        word = int(self.info[f, j])
        used = used_views(word)
        P = self.krt[f].astype(np.float64)
        p2 = self.pts[f, :, j].astype(np.float64)
        if branch(word):
            v, = used
            ds, resize = EPIPOLAR_KW["downsample"], EPIPOLAR_KW["resize"]
            H, W = self.corr.shape[2:4]
            q = (p2[v] / resize + 0.5 - ds / 2.0) / ds
            ix, iy = epi._index(q[0], W)[0], epi._index(q[1], H)[0]
            o = (self.corr[f, v, iy, ix].astype(np.float64) * ds + ds / 2.0 - 0.5) * resize
            return [(P[v], v, p2[v]), (self.other[f, v].astype(np.float64), None, o)]
        return [(P[v], v, p2[v]) for v in used] if len(used) >= 2 else []

    def reference(self, k):
        """(autograd yardstick, implicit yardstick) for grad_outs(F, J)[k], each (F, V, J, 2) float64; computed once."""
        if k not in self._refs:
            gout = grad_outs(self.F, self.J)[k]
            a, b = np.zeros((self.F, self.V, self.J, 2)), np.zeros((self.F, self.V, self.J, 2))
            for f in range(self.F):
                for j in range(self.J):
                    rows = self.rows(f, j)
                    if rows:
                        for out, fn in ((a, autograd_joint), (b, implicit_joint)):
                            for (_, v, _), g in zip(rows, fn(rows, gout[f, j])):
                                if v is not None:
                                    out[f, v, j] = g
            self._refs[k] = (a, b)
        return self._refs[k]


def autograd_joint(rows, gX):
    """float64 torch autograd through torch.linalg.svd -> one (gx, gy) per row pair."""
    xy = torch.tensor(np.array([r[2] for r in rows]), dtype=torch.float64, requires_grad=True)
    P = torch.tensor(np.array([r[0] for r in rows]), dtype=torch.float64)
    A = torch.cat([xy[:, 0:1] * P[:, 2] - P[:, 0], xy[:, 1:2] * P[:, 2] - P[:, 1]], 0)
    vt = torch.linalg.svd(A, full_matrices=False)[2]
    X = vt[-1, :3] / vt[-1, 3]
    g, = torch.autograd.grad(X, xy, torch.tensor(np.asarray(gX), dtype=torch.float64))
    return g.numpy()


def implicit_joint(rows, gX):
    """The implicit formula from np.linalg.svd: gv, w = -pinv(A^T A - s4^2 I) gv, gA = (A w) v^T + (A v) w^T."""
    A = np.array([r[2][0] * r[0][2] - r[0][0] for r in rows] + [r[2][1] * r[0][2] - r[0][1] for r in rows])
    _, s, vt = np.linalg.svd(A)
    v = vt[3]
    gX = np.asarray(gX, np.float64)
    gv = np.append(gX / v[3], -(gX @ v[:3]) / v[3] ** 2)
    w = -sum(vt[k] * (vt[k] @ gv) / (s[k] ** 2 - s[3] ** 2) for k in range(3))
    gA = np.outer(A @ w, v) + np.outer(A @ v, w)
    n = len(rows)
    return np.array([[gA[i] @ rows[i][0][2], gA[n + i] @ rows[i][0][2]] for i in range(n)])


def per_joint_max(g):
    """(F, V, J, 2) -> (F, J): the largest |element| of every joint."""
    return np.abs(g).max(axis=(1, 3))


def condition(scene, k):
    """The worst disagreement of the two yardsticks, relative to the joint's largest gradient element."""
    a, b = scene.reference(k)
    size = per_joint_max(a)
    diff = per_joint_max(a - b)
    assert ((size > 0) | (diff == 0)).all()
    return float(np.divide(diff, size, out=np.zeros_like(diff), where=size > 0).max())


def use_of_bound(got, want):
    """(all joints within TOLERANCE x their largest reference element, the worst use of that bound).  A joint whose reference is
    all zeros has the bound 0: it must be exactly zero."""
    err, tol = per_joint_max(np.asarray(got, np.float64) - want), TOLERANCE * per_joint_max(want)
    ok = bool((err <= tol).all())
    return ok, float(np.divide(err, tol, out=np.zeros_like(err), where=tol > 0).max())


def fp(a):
    return NULL if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_bwd(lib, scene, info, gout, other="scene"):
    """et_debug_host_triangulate_bwd -> (F, V, J, 2) float32; the output starts as NaN.  `other` None: NULL other_krt / corr_pos
    whatever the scene holds."""
    okrt, corr = (scene.other, scene.corr) if other == "scene" else (None, None)
    H, W = corr.shape[2:4] if corr is not None else (0, 0)
    ds, resize = (EPIPOLAR_KW["downsample"], EPIPOLAR_KW["resize"]) if corr is not None else (0.0, 0.0)
    grad = np.full(scene.pts.shape, np.nan, np.float32)
    info, gout = np.ascontiguousarray(info, np.int32), np.ascontiguousarray(gout, np.float64)
    rc = lib.et_debug_host_triangulate_bwd(scene.F, scene.V, scene.J, H, W, fp(scene.pts), fp(scene.krt), fp(okrt), fp(corr), ds,
                                           resize, fp(info), fp(gout), fp(grad))
    assert rc == 0, lib.et_last_error()
    return grad


METHODS = ("pymvg", "naive", "refine", "epipolar", "epipolar_dlt")


@functools.lru_cache(maxsize=None)
def scene(method, V, F=3, J=17):
    """The scenes of the existing forward tests: random_scene(3, V, 17, seed=20 + V) for the three methods of the views,
    random_scene(3, V, 17, seed=10 + V) for the epipolar ones.  Other sizes (the GPU test's F J = 1 and J = 257 at V = 2) take
    the same generators and seeds."""
    if method in views.METHODS:
        return Scene(views.random_scene(F, V, J, seed=20 + V)[0], method)
    return Scene(epi.random_scene(F, V, J, seed=10 + V)[0], method)
