"""Generate tests/golden/lifting/rpsm.npz from the REAL reference `rpsm` (modeling/pictorial_cuda.py:222-254:
KEYPOINT.TRIANGULATION rpsm, the recursive pictorial structure model).

Runs only where the reference tree is present (imported read-only through oracle/ref_harness.py).  What is executed is the
reference's own code, on the CPU, one frame at a time: compute_grid, compute_unary_term (with get_affine_transform and
F.grid_sample as this image's torch runs it), compute_pairwise / pdist2, infer, recursive_infer, with HumanBody's skeleton.  The
first stage's kw['pairwise'], which the reference unpickles from PICT_STRUCT.PAIRWISE_FILE, is built here with the reference's own
compute_pairwise(skeleton, first_limb_length, [grid] * J, tolerance): the distance band that ops.rpsm computes on the fly.

One function of the path is NOT the reference's: `cv2.getAffineTransform` (data/transforms/image.py:255-257).  The harness's `cv2`
is an empty stub (OpenCV is absent), so this script installs rpsm_restatement.affine_from_points in its place: the 2 x 3 map that
takes the three source points to the three destination points, which is what OpenCV documents for that call, solved in float64.

    python tests/golden/make_rpsm_golden.py

Stored per case: heat (V,17,H,W) float16 (the values are float16 numbers; every consumer widens them to float32), cams = K @ RT
(V,3,4), trans (V,2,3), center (3,), limb_length (16,), optionally first_limb_length (16,), the integer parameters, the reference's
pose X_ref (17,3) float32 and the planted X_true.

Condition on the inputs (asserted; a seed that violates it is replaced by the next and printed, no case is dropped): on the
float64 restatement's chosen path every arg-max wins by a relative margin >= 1e-4 at every level, and every band test that decides
one is >= 1e-2 mm away from the tolerance.  RECUR_DEPTH is 4: deeper levels are decided at float32 rounding.

Tolerance of the tests (tests/test_rpsm_cpu.py, tests/test_gpu_rpsm.py): with identical bins the poses differ only by the float32
rounding of grid positions.  This script prints the largest |restatement - reference| and |host hook - reference| over all cases;
the run that wrote the committed file printed 8.53e-05 mm and 3.05e-05 mm, and the tests use 4 x the larger: TOLERANCE_MM = 3.42e-4.
"""
import contextlib
import ctypes
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import ref_harness as rh  # noqa: E402
import rpsm_restatement as restate  # noqa: E402

J, DEPTH, TOLERANCE = 17, 4, 150

# name: (V, H, W, image_size, grid_size, first_nbins, recur_nbins, frame keywords)
SPECS = [
    ("four_views_clean", 4, 24, 24, (256, 256), 2000, 8, 2, dict(noise=0.0, box=450.0)),
    ("three_views_shifted_crop", 3, 24, 24, (256, 256), 2000, 8, 2, dict(shift_view=1)),
    ("non_square_map", 4, 20, 28, (256, 192), 2000, 8, 2, {}),
    ("first_nbins_6", 4, 24, 24, (256, 256), 1200, 6, 2, {}),
    ("first_nbins_16", 4, 24, 24, (256, 256), 2000, 16, 2, {}),
    ("first_limb_length_differs", 4, 24, 24, (256, 256), 2000, 8, 2, dict(first_scale=1.08)),
    ("recur_nbins_3", 4, 24, 24, (256, 256), 2000, 8, 3, {}),
    ("zero_heatmap_joint", 4, 24, 24, (256, 256), 2000, 8, 2, dict(zero_joint=16)),
]


def host_hook(lib, sc, params):
    """et_debug_host_rpsm on a stacked scene: (pose (F,J,3) float32, path (F,1+depth,J) int32)."""
    F, V, joints, H, W = sc["heat"].shape
    out = np.full((F, joints, 3), np.nan, np.float32)
    path = np.full((F, 1 + params["recur_depth"], joints), -1, np.int32)
    fp = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)
    parent = np.array(restate.H36M_PARENT[:joints], np.int32)
    rc = lib.et_debug_host_rpsm(F, V, joints, H, W, fp(sc["heat"]), fp(sc["cams"]), fp(sc["trans"]), fp(sc["center"]),
                                fp(sc["limb_length"]), fp(sc.get("first_limb_length")), fp(parent), params["image_size"][0],
                                params["image_size"][1], params["grid_size"], params["first_nbins"], params["recur_nbins"],
                                params["recur_depth"], params["tolerance"], int(params.get("align_corners", False)), fp(out), fp(path))
    assert rc == 0, lib.et_last_error()
    return out, path


def reference_rpsm(fr, params):
    """The reference on one frame dict: (J,3) float32."""
    V, joints, H, W = fr["heat"].shape
    cfg = rh.load_cfg(None, ["DATASETS.IMAGE_SIZE", tuple(params["image_size"]), "KEYPOINT.HEATMAP_SIZE", (W, H),
                             "PICT_STRUCT.GRID_SIZE", params["grid_size"], "PICT_STRUCT.FIRST_NBINS", params["first_nbins"],
                             "PICT_STRUCT.RECUR_NBINS", params["recur_nbins"], "PICT_STRUCT.RECUR_DEPTH", params["recur_depth"],
                             "PICT_STRUCT.LIMB_LENGTH_TOLERANCE", params["tolerance"], "KEYPOINT.ROOTIDX", 0])
    import data.transforms.image as rimage
    import modeling.pictorial_cuda as pc
    from modeling.layers.body import HumanBody

    sys.modules["cv2"].getAffineTransform = restate.affine_from_points
    assert rimage.cv2 is sys.modules["cv2"] and pc.cfg is cfg
    assert tuple(cfg.DATASETS.IMAGE_SIZE) == tuple(params["image_size"]) and cfg.PICT_STRUCT.FIRST_NBINS == params["first_nbins"]
    body = HumanBody()
    assert tuple(-1 if "parent" not in n else n["parent"] for n in body.skeleton) == restate.H36M_PARENT
    limbs = lambda arr: {(restate.H36M_PARENT[j], j): float(arr[j - 1]) for j in range(1, joints)}
    center = torch.from_numpy(fr["center"])
    grid = pc.compute_grid(params["grid_size"], center, params["first_nbins"])
    first = fr.get("first_limb_length", fr["limb_length"])
    kw = dict(body=body, center=center, limb_length=limbs(fr["limb_length"]),
              pairwise=pc.compute_pairwise(body.skeleton, limbs(first), [grid] * joints, params["tolerance"]),
              boxes=[dict(center=fr["box_center"][v].astype(np.float64), scale=float(fr["box_scale"])) for v in range(V)])
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        pose = pc.rpsm([torch.from_numpy(c) for c in fr["cams"]], torch.from_numpy(fr["heat"]), kw)
    return pose.numpy().astype(np.float32)


def main():
    from epipolar_transformers_amd import _lib, build

    build.build_library()
    lib = _lib.load()
    cases, worst_restate, worst_hook = {}, 0.0, 0.0
    for ci, (name, V, H, W, image_size, grid_size, first_nbins, recur_nbins, kw) in enumerate(SPECS):
        params = dict(image_size=image_size, grid_size=grid_size, first_nbins=first_nbins, recur_nbins=recur_nbins, recur_depth=DEPTH,
                      tolerance=TOLERANCE)
        sc, (pose, path, margins, band) = restate.scene(500 + 20 * ci, 1, V, J, H, W, params, log=lambda t: print(name + ": " + t), **kw)
        assert restate.condition_holds(margins, band)
        fr = {k: v[0] for k, v in sc.items()}
        ref = reference_rpsm(fr, params)
        got, hook_path = host_hook(lib, sc, params)
        d_restate, d_hook = np.abs(pose[0] - ref).max(), np.abs(got[0].astype(np.float64) - ref).max()
        worst_restate, worst_hook = max(worst_restate, d_restate), max(worst_hook, d_hook)
        print("%-28s V=%d %dx%d bins %d/%d margin %.1e band %.2f mm: |X_ref - X_true| mean %.1f mm; restatement vs reference %.2e mm, "
              "host hook vs reference %.2e mm, hook path == restatement path: %s" % (
                  name, V, H, W, first_nbins, recur_nbins, margins.min(), band.min(),
                  np.linalg.norm(ref - fr["X_true"], axis=1).mean(), d_restate, d_hook, np.array_equal(hook_path, path)))
        # identical bins: the poses differ by rounding only.  For the all-zero joint this also says that the reference takes the
        # FIRST index among equal values (torch.max over dim 1 and np.argmax), as the restatement does.
        assert d_restate < 1e-2, "the reference chose other bins than the restatement"
        if kw.get("zero_joint") is not None:
            assert (path[0][:, 0] == 0).all(), "an all-zero joint zeroes the root's energy: the first bin wins every level"
        for key, val in fr.items():
            if key in ("box_center", "box_scale"):
                continue
            cases["%s.%s" % (name, key)] = val.astype(np.float16) if key == "heat" else val
        for key, val in (("image_size", np.array(image_size, np.int32)), ("grid_size", np.int32(grid_size)),
                         ("first_nbins", np.int32(first_nbins)), ("recur_nbins", np.int32(recur_nbins)),
                         ("recur_depth", np.int32(DEPTH)), ("tolerance", np.int32(TOLERANCE)), ("X_ref", ref)):
            cases["%s.%s" % (name, key)] = val
    print("largest |restatement - reference| %.2e mm, |host hook - reference| %.2e mm -> TOLERANCE_MM = 4 x %.2e" % (
        worst_restate, worst_hook, max(worst_restate, worst_hook)))
    out = os.path.join(ROOT, "tests", "golden", "lifting", "rpsm.npz")
    np.savez_compressed(out, **cases)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
