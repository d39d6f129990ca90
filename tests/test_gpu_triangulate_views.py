"""KEYPOINT.TRIANGULATION pymvg / naive / refine on the GPU: the kernels (ops.triangulate_views) against the reference-made
fixtures and the NumPy restatement, their reproducibility, the wrapper's argument checks, and the model's dispatch under
EPIPOLAR_AMD.LIFT_KERNELS."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

import triangulation_views_restatement as restate
from test_triangulate_epipolar_cpu import within_tolerance
from test_triangulate_views_cpu import (PYMVG_CASES, RANDOM_KW, RANSAC_CASES, check_ransac_expectations, pymvg_case,
                                        ransac_case)

pytestmark = pytest.mark.gpu


def on_gpu(arrays):
    return [torch.from_numpy(a).cuda() for a in arrays]


def test_pymvg_kernel_matches_the_reference_fixture():
    from epipolar_transformers_amd import ops

    golden = np.load(os.path.join(GOLDEN_DIR, "triangulation.npz"), allow_pickle=False)
    for name in PYMVG_CASES:
        arrays, thres, g = pymvg_case(golden, name)
        X, info = ops.triangulate_views(*on_gpu(arrays), method="pymvg", conf_thres=thres, want_info=True)
        ok, worst = within_tolerance(X[0].cpu().numpy(), g("X_ref"), g("X_true"))
        print(name, "kernel vs reference: worst err / bound %.3g" % worst)
        assert ok, (name, worst)
        assert np.array_equal(info.cpu().numpy(), restate.triangulate_views(*arrays, method="pymvg", conf_thres=thres)[1]), name


@pytest.mark.parametrize("method", ["naive", "refine"])
def test_ransac_kernel_matches_the_reference_fixture(method):
    from epipolar_transformers_amd import ops

    golden = np.load(os.path.join(GOLDEN_DIR, "lifting", "triangulation_ransac.npz"), allow_pickle=False)
    for name in RANSAC_CASES:
        arrays, kw, g = ransac_case(golden, name)
        dev = on_gpu(arrays)
        X, info = [t.cpu().numpy() for t in ops.triangulate_views(*dev, method=method, want_info=True, **kw)]
        ok, worst = within_tolerance(X[0], g("X_ref_" + method), g("X_true"))
        print(name, method, "kernel vs reference: worst err / bound %.3g" % worst)
        assert ok, (name, worst)
        check_ransac_expectations(name, method, X, info, g, ops.triangulate_views(*dev, method="pymvg", **kw).cpu().numpy())
        assert np.array_equal(info, restate.triangulate_views(*arrays, method=method, **kw)[1]), name


@pytest.mark.parametrize("shape", [(33, 4, 17), (5, 8, 17), (1, 2, 1), (2, 1, 3)], ids=lambda s: "F%d_V%d_J%d" % s)
def test_kernels_match_the_restatement(shape):
    """561 items (pymvg: three blocks, a partly filled last wave; naive / refine: a ragged last block), eight views, the smallest
    problem, and one view (every joint flagged).  The outputs start as NaN (conftest: ops.POISON_OUTPUTS), so a joint a kernel did
    not write shows."""
    from epipolar_transformers_amd import ops

    assert ops.POISON_OUTPUTS
    arrays, truth = restate.random_scene(*shape, seed=sum(shape))
    dev = on_gpu(arrays)
    for method in restate.METHODS:
        Xr, info_r, margin = restate.triangulate_views(*arrays, method=method, **RANDOM_KW)
        assert margin >= 1e-6                               # no decision hangs on rounding: nothing is excluded
        X, info = ops.triangulate_views(*dev, method=method, want_info=True, **RANDOM_KW)
        assert X.dtype == torch.float64 and tuple(X.shape) == (shape[0], shape[2], 3)
        assert info.dtype == torch.int32 and tuple(info.shape) == (shape[0], shape[2])
        X = X.cpu().numpy()
        assert np.isfinite(X).all()
        assert np.array_equal(info.cpu().numpy(), info_r), method
        ok, worst = within_tolerance(X, Xr, truth)
        print(shape, "%s kernel vs restatement: worst err / bound %.3g" % (method, worst))
        assert ok, (method, worst)
        if shape[1] == 1:
            assert (info_r & restate.INFO_ZEROS).all() and (X == 0).all()
        assert torch.equal(ops.triangulate_views(*dev, method=method, **RANDOM_KW), torch.from_numpy(X).cuda())    # info is nullable


@pytest.mark.parametrize("method", restate.METHODS)
def test_repeated_calls_and_another_stream_give_the_same_bits(method):
    from epipolar_transformers_amd import ops

    arrays, _ = restate.random_scene(9, 8, 17, seed=77)
    dev = on_gpu(arrays)
    first = ops.triangulate_views(*dev, method=method, want_info=True, **RANDOM_KW)
    for _ in range(4):
        again = ops.triangulate_views(*dev, method=method, want_info=True, **RANDOM_KW)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ops.triangulate_views(*dev, method=method, want_info=True, **RANDOM_KW)
    side.synchronize()
    assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])


def test_argument_checks():
    from epipolar_transformers_amd import _lib, ops

    arrays, _ = restate.random_scene(2, 4, 3, seed=5)
    pts, conf, krt = on_gpu(arrays)
    call = lambda *a, method="naive": ops.triangulate_views(*a, method=method, **RANDOM_KW)
    with pytest.raises(_lib.EpipolarAmdError):
        call(pts.cpu(), conf, krt)
    with pytest.raises(_lib.EpipolarAmdError):
        call(pts, conf, krt.cpu())
    with pytest.raises(TypeError):
        call(pts.double(), conf, krt)
    with pytest.raises(TypeError):
        call(pts, conf.double(), krt)
    with pytest.raises(ValueError):
        call(pts, conf[:, :, :2].contiguous(), krt)                         # wrong shape
    with pytest.raises(ValueError):
        call(pts[..., :1].contiguous(), conf, krt)
    with pytest.raises(ValueError):
        call(pts, conf, krt.transpose(2, 3).contiguous().transpose(2, 3))   # right shape, not contiguous
    with pytest.raises(ValueError):
        call(pts, conf.transpose(0, 1).contiguous().transpose(0, 1), krt)
    with pytest.raises(ValueError, match="pymvg, naive, refine"):
        call(pts, conf, krt, method="epipolar")
    nine, _ = restate.random_scene(1, 9, 2, seed=5)
    for method in restate.METHODS:
        with pytest.raises(_lib.EpipolarAmdError, match="V=9"):
            call(*on_gpu(nine), method=method)
    with pytest.raises(_lib.EpipolarAmdError, match="conf_thres"):
        ops.triangulate_views(pts, conf, krt, method="pymvg", conf_thres=2.5)


def test_model_lifts_through_the_kernels_when_the_knob_is_set():
    """MultiViewPoseModel in eval mode with VIS.MULTIVIEW and EPIPOLAR_AMD.LIFT_KERNELS: pymvg / naive / refine return what the
    kernel gives for the model's own detections and scores; pymvg agrees with the torch path it replaces; EPIPOLAR.MULTITEST works."""
    from epipolar_transformers_amd import ops, synthetic as syn
    from epipolar_transformers_amd.model import ring_sources
    from epipolar_transformers_amd.triangulate import triangulate_dlt
    from test_gpu_model import _cfg, _model

    cfg, size, hs = _cfg(**{"KEYPOINT.TRIANGULATION": "pymvg", "KEYPOINT.CONF_THRES": 0.05, "KEYPOINT.RANSAC_THRES": 400,
                            "EPIPOLAR_AMD.LIFT_KERNELS": True})
    m = _model(cfg)
    frames, V, J = 2, 4, 17
    # Per-frame jittered cameras (the data set's crops), not the exactly symmetric ring: an untrained network peaks at the same pixel
    # in every view for some joints, and with cameras that are rotations of one another about the vertical axis the DLT solution of
    # such a joint lies at infinity (fourth component 0 up to rounding).  No float64 SVD determines that point -- torch on the CPU
    # and torch on the GPU differ by 1e19 mm there -- so it cannot be compared with anything.
    rng = np.random.default_rng(3)
    P = torch.from_numpy(np.concatenate([syn.ring_cameras(V, size, jitter=(0.02, 1.0), rng=rng) for _ in range(frames)])).float()
    img =torch.randn(frames * V, 3, size, size, device="cuda")
    batch = {"img": img, "KRT": P, "other_index": ring_sources(frames, V, "cuda"), "num_views": V}
    with torch.no_grad():
        out = m(batch, is_train=False)[2]
    # a threshold inside the scores' range, so that joints differ in how many views they select
    thres = float(out["batch_scos"].median())
    cfg.merge_from_list(["KEYPOINT.CONF_THRES", thres])
    scale = float(cfg.DATASETS.IMAGE_RESIZE) * float(cfg.DATASETS.PREDICT_RESIZE)
    krt = P.cuda().view(frames, V, 3, 4).contiguous()
    selected = set()
    for method in restate.METHODS:
        cfg.merge_from_list(["KEYPOINT.TRIANGULATION", method])
        with torch.no_grad():
            out = m(batch, is_train=False)[2]
        pts = (out["batch_locs"] * scale).view(frames, V, J, 2).contiguous()
        conf = out["batch_scos"].view(frames, V, J).contiguous()
        want, info = ops.triangulate_views(pts, conf, krt, method=method, conf_thres=thres, ransac_thres=400.0, want_info=True)
        assert out["points-3d"].dtype == torch.float64 and tuple(out["points-3d"].shape) == (frames, J, 3)
        assert torch.equal(out["points-3d"], want), method
        selected |= set((info & 0xff).flatten().tolist())
        if method == "pymvg":
            torch_path = triangulate_dlt(pts, krt, conf, conf_thres=thres).cpu().numpy()
            ok, worst = within_tolerance(want.cpu().numpy(), torch_path, torch_path)      # bound: 2e-3 mm
            print("pymvg kernel vs torch path: worst err / bound %.3g" % worst)
            assert ok, worst
    assert len(selected) > 1
    cfg.merge_from_list(["KEYPOINT.TRIANGULATION", "pymvg", "EPIPOLAR.MULTITEST", True])
    with torch.no_grad():
        pred = m(batch, is_train=False)[2]["points-3d"]
    assert pred.dtype == torch.float64 and tuple(pred.shape) == (frames, J, 3) and torch.isfinite(pred).all()
