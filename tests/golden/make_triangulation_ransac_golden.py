"""Generate tests/golden/lifting/triangulation_ransac.npz from the REAL reference `triangulate` and `triangulate_refine`
(vision/triangulation.py:99-154 and 162-232: KEYPOINT.TRIANGULATION naive -- the default of the key -- and refine).

Runs only where the reference tree is present (imported read-only through oracle/ref_harness.py, with the pymvg stand-in
oracle/pymvg_stub.py, exactly as make_triangulation_golden.py does).  What is executed is the reference's own code: the
selection `conf > CONF_THRES`, the loop over RANSAC_ITER = 100 pairs, camera_center / point2line for the inliers, `acc > best`,
and for refine build_multi_camera_system -> find3d over the best inliers when there is more than one.

Two things of the path are NOT the reference's.

`cv2.triangulatePoints` (triangulation.py:139, 156-160).  The harness's `cv2` is an empty stub (OpenCV is absent), so this script
installs `triangulate_points_standin` of make_triangulation_epipolar_golden.py in its place, as that script does.  It restates
what OpenCV documents for that call -- the homogeneous point minimising the algebraic error of the two views' four rows
x * P[2] - P[0], y * P[2] - P[1], i.e. the last right singular vector of that 4 x 4 matrix -- in float64.

The module's `random`.  The reference draws `a = random.randint(0, n-1); b = random.randint(0, n-1)` 100 times per joint and
skips a == b.  In this process `random` is replaced by a scripted source whose 200 draws per joint walk the ORDERED pairs (a, b)
in lexicographic order, cyclically.  For n <= 8 views n^2 <= 64 <= 100, so every pair is visited, and the first occurrences of the
unordered pairs come in lexicographic order ((1, 0) repeats (0, 1), which came first).  This is one sequence `random` can produce,
so every stored result is one the reference can return -- and it is the result of full enumeration with the first best
hypothesis winning, which is what et_triangulate_views computes (its documented deviation, the one ops.triangulate_epipolar
states for its own search).

    python tests/golden/make_triangulation_ransac_golden.py

Stored per case (arrays only): K (V,3,3), RT (V,3,4), KRT = K @ RT (V,3,4), pts (V,J,2), conf (V,J), all float32 as Modelbuilder
hands them over; conf_thres, ransac_thres; the reference's (J,3) float64 points X_ref_naive / X_ref_refine and the planted X_true.

Condition on the inputs (asserted; a seed that violates it is replaced by the next, no case is dropped): every inlier distance
of every hypothesis, computed in float64, is at least 3 % of the threshold away from it -- those to the winning hypothesis'
point, which decide what refine solves over, among them.  The reference does its ray arithmetic with a float32 inverse
(camera_center on the float32 KRT): estimated error ~0.5 mm at 5 m (condition ~1e3 x 2^-24; not measured) against 3 % of 35 mm =
1.05 mm.  The case with RANSAC_THRES 0.05 also replaces a seed in which two rays pass within 0.05 mm of each other, so that
every joint of it is a no-inlier joint.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]
from oracle import ref_harness as rh  # noqa: E402
import make_triangulation_golden as base  # noqa: E402
from make_triangulation_epipolar_golden import CONF_THRES, RANSAC_THRES, MARGIN, scene, triangulate_points_standin  # noqa: E402
import triangulation_views_restatement as restate  # noqa: E402

DRAWS_PER_JOINT = 200       # RANSAC_ITER = 100 iterations, two draws each, whether or not a == b


class LexicographicPairs:
    """Stands in for the `random` module inside vision.triangulation: iteration i of a joint gets the ordered pair number
    i mod n^2 in lexicographic order, (a, b) = divmod(i mod n^2, n).  A joint with at most one selected view draws nothing, so
    the count of draws stays a multiple of DRAWS_PER_JOINT between joints."""

    def __init__(self):
        self.draws = 0

    def randint(self, lo, hi):
        assert lo == 0
        n = hi + 1
        k = self.draws % DRAWS_PER_JOINT
        self.draws += 1
        a, b = divmod((k // 2) % (n * n), n)
        return b if k % 2 else a


def main():
    tri = base.reference_triangulate_pymvg()
    sys.modules["cv2"].triangulatePoints = triangulate_points_standin
    assert tri.cv2 is sys.modules["cv2"] and tri.RANSAC_ITER * 2 == DRAWS_PER_JOINT
    specs = [
        # name, kind (of make_triangulation_epipolar_golden.scene), V, ransac_thres
        ("all_confident_clean_first_pair_wins", "clean", 4, RANSAC_THRES),
        ("confident_outlier_rejected", "confident_outlier", 4, RANSAC_THRES),
        ("two_of_four_wrong", "two_of_four_wrong", 4, RANSAC_THRES),
        ("tiny_ransac_thres_no_inlier", "clean", 4, 0.05),
        ("one_confident_view_zeros", "one_confident", 4, RANSAC_THRES),
        ("eight_views_mixed", "mixed", 8, RANSAC_THRES),
    ]
    cases = {}
    for ci, (name, kind, V, thres) in enumerate(specs):
        seed = 500 + 20 * ci
        while True:
            s = scene(kind, V, seed, 1.0)
            args = [s[k][None] for k in ("pts", "conf", "KRT")]
            kw = dict(conf_thres=CONF_THRES, ransac_thres=thres)
            ours = {m: restate.triangulate_views(*args, method=m, **kw) for m in ("naive", "refine")}
            margin = min(ours["naive"][2], ours["refine"][2])      # (every hypothesis' distances, the winner's among them)
            info = ours["naive"][1]
            if margin >= MARGIN and (thres >= 1 or (info[0] & restate.INFO_ZEROS).all()):
                break
            print("%s: seed %d replaced (smallest distance to the threshold %.1f %% of it)" % (name, seed, 100 * margin))
            seed += 1
        assert margin >= MARGIN
        cfg = rh.load_cfg(None, ["KEYPOINT.CONF_THRES", str(CONF_THRES), "KEYPOINT.RANSAC_THRES", thres])
        assert float(cfg.KEYPOINT.RANSAC_THRES) == thres and float(cfg.KEYPOINT.CONF_THRES) == CONF_THRES
        tri.random = source = LexicographicPairs()
        pts, krt, conf = torch.from_numpy(s["pts"]), torch.from_numpy(s["KRT"]), torch.from_numpy(s["conf"])
        with contextlib.redirect_stdout(io.StringIO()):
            naive = tri.triangulate(pts, krt, conf)
            assert source.draws % DRAWS_PER_JOINT == 0
            refine = tri.triangulate_refine(pts, krt, s["K"], s["RT"], conf)
        assert source.draws % DRAWS_PER_JOINT == 0
        got = {"naive": np.stack([np.asarray(p, dtype=np.float64).reshape(3) for p in naive]),
               "refine": np.stack([np.asarray(p, dtype=np.float64).reshape(3) for p in refine])}
        e = {m: np.linalg.norm(got[m] - s["X_true"], axis=1) for m in got}
        dev = {m: np.linalg.norm(ours[m][0][0] - got[m], axis=1).max() for m in got}
        print("%-36s V=%d seed %d margin %.1f %%: |X_ref - X_true| naive mean %.1f max %.1f mm, refine mean %.1f max %.1f mm; "
              "restatement vs reference max %.2e / %.2e mm" % (name, V, seed, 100 * margin, e["naive"].mean(), e["naive"].max(),
                                                               e["refine"].mean(), e["refine"].max(), dev["naive"], dev["refine"]))
        if kind == "clean" and thres >= 1:
            assert ((info[0] >> 8 & 0xff) == 0b0011).all(), "every pair ties: the first must win"
        if thres < 1 or kind == "one_confident":
            assert (got["naive"] == 0).all() and (got["refine"] == 0).all() and (info[0] & restate.INFO_ZEROS).all()
        for key, val in [(k, s[k]) for k in ("K", "RT", "KRT", "pts", "conf", "X_true")] + [
                ("conf_thres", np.float64(CONF_THRES)), ("ransac_thres", np.float64(thres)),
                ("X_ref_naive", got["naive"]), ("X_ref_refine", got["refine"])]:
            cases["%s.%s" % (name, key)] = np.asarray(val)
    out = os.path.join(ROOT, "tests", "golden", "lifting", "triangulation_ransac.npz")
    np.savez_compressed(out, **cases)
    assert all(v.dtype != object for v in np.load(out, allow_pickle=False).values())
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
