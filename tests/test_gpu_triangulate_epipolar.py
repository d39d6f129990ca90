"""KEYPOINT.TRIANGULATION epipolar / epipolar_dlt on the GPU: the kernel (ops.triangulate_epipolar) against the reference-made
fixture and the NumPy restatement, its reproducibility, the wrapper's argument checks, and the model's dispatch."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

import triangulation_epipolar_restatement as restate
from test_triangulate_epipolar_cpu import CASES, case_inputs, within_tolerance

pytestmark = pytest.mark.gpu

KW = dict(downsample=64.0, resize=1.0, conf_thres=0.85, ransac_thres=35.0)


def on_gpu(arrays):
    return [torch.from_numpy(a).cuda() for a in arrays]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "lifting", "triangulation_epipolar.npz"))


@pytest.mark.parametrize("dlt", [False, True], ids=["epipolar", "epipolar_dlt"])
def test_kernel_matches_the_reference_fixture(golden, dlt):
    from epipolar_transformers_amd import ops

    for name in CASES:
        arrays, kw, g = case_inputs(golden, name)
        X, info = ops.triangulate_epipolar(*on_gpu(arrays), dlt=dlt, want_info=True, **kw)
        ok, worst = within_tolerance(X[0].cpu().numpy(), g("X_ref_dlt" if dlt else "X_ref_epipolar"), g("X_true"))
        print(name, "kernel vs reference: worst err / bound %.3g" % worst)
        assert ok, (name, worst)
        assert np.array_equal(info.cpu().numpy(), restate.triangulate_epipolar(*arrays, dlt=dlt, **kw)[1]), name


@pytest.mark.parametrize("shape", [(33, 4, 17), (5, 8, 17), (1, 2, 1)], ids=lambda s: "F%d_V%d_J%d" % s)
def test_kernel_matches_the_restatement(shape):
    """561 waves (more than one block, a ragged last block), eight views, and the smallest problem.  The outputs start as NaN
    (conftest: ops.POISON_OUTPUTS), so a joint the kernel did not write shows."""
    from epipolar_transformers_amd import ops

    assert ops.POISON_OUTPUTS
    arrays, truth = restate.random_scene(*shape, seed=sum(shape))
    dev = on_gpu(arrays)
    for dlt in (False, True):
        Xr, info_r, margin = restate.triangulate_epipolar(*arrays, dlt=dlt, **KW)
        assert margin >= 1e-6                               # no decision hangs on rounding: nothing is excluded
        X, info = ops.triangulate_epipolar(*dev, dlt=dlt, want_info=True, **KW)
        assert X.dtype == torch.float64 and tuple(X.shape) == (shape[0], shape[2], 3) and info.dtype == torch.int32
        X = X.cpu().numpy()
        assert np.isfinite(X).all()
        assert np.array_equal(info.cpu().numpy(), info_r)
        ok, worst = within_tolerance(X, Xr, truth)
        print(shape, "dlt=%d kernel vs restatement: worst err / bound %.3g" % (dlt, worst))
        assert ok, worst


def test_repeated_calls_and_another_stream_give_the_same_bits():
    from epipolar_transformers_amd import ops

    arrays, _ = restate.random_scene(9, 8, 17, seed=77)
    dev = on_gpu(arrays)
    first = ops.triangulate_epipolar(*dev, want_info=True, **KW)
    for _ in range(4):
        again = ops.triangulate_epipolar(*dev, want_info=True, **KW)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ops.triangulate_epipolar(*dev, want_info=True, **KW)
    side.synchronize()
    assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])


def test_argument_checks():
    from epipolar_transformers_amd import _lib, ops

    arrays, _ = restate.random_scene(2, 4, 3, seed=5)
    pts, conf, krt, okrt, corr = on_gpu(arrays)
    call = lambda *a: ops.triangulate_epipolar(*a, **KW)
    with pytest.raises(_lib.EpipolarAmdError):
        call(pts.cpu(), conf, krt, okrt, corr)
    with pytest.raises(_lib.EpipolarAmdError):
        call(pts, conf, krt, okrt, corr.cpu())
    with pytest.raises(TypeError):
        call(pts.double(), conf, krt, okrt, corr)
    with pytest.raises(TypeError):
        call(pts, conf.half(), krt, okrt, corr)
    with pytest.raises(ValueError):
        call(pts, conf[:, :, :2].contiguous(), krt, okrt, corr)             # wrong shape
    with pytest.raises(ValueError):
        call(pts, conf, krt, okrt[:1], corr)
    with pytest.raises(ValueError):
        call(pts, conf, krt.transpose(2, 3).contiguous().transpose(2, 3), okrt, corr)   # right shape, not contiguous
    with pytest.raises(ValueError):
        call(pts, conf, krt, okrt, corr[:, :, :, ::2])
    nine, _ = restate.random_scene(1, 9, 2, seed=5)
    with pytest.raises(_lib.EpipolarAmdError, match="V=9"):
        call(*on_gpu(nine))


def test_model_lifts_by_the_configured_method():
    """MultiViewPoseModel in eval mode with VIS.MULTIVIEW: KEYPOINT.TRIANGULATION epipolar / epipolar_dlt return what the kernel
    gives for the model's own detections, scores, corr_pos and source projections; pymvg still returns triangulate_dlt."""
    from epipolar_transformers_amd import ops, synthetic as syn
    from epipolar_transformers_amd.model import ring_sources
    from epipolar_transformers_amd.triangulate import triangulate_dlt
    from test_gpu_model import _cfg, _model

    cfg, size, hs = _cfg(**{"KEYPOINT.TRIANGULATION": "pymvg", "KEYPOINT.CONF_THRES": 0.05, "KEYPOINT.RANSAC_THRES": 400})
    m = _model(cfg)
    frames, V, J = 2, 4, 17
    P = torch.from_numpy(syn.ring_cameras(V, size)).float().repeat(frames, 1, 1)
    img = torch.randn(frames * V, 3, size, size, device="cuda")
    src = ring_sources(frames, V, "cuda")
    batch = {"img": img, "KRT": P, "other_index": src, "num_views": V}
    with torch.no_grad():
        out = m(batch, is_train=False)[2]
    pts = out["batch_locs"].view(frames, V, J, 2)
    want = triangulate_dlt(pts, P.cuda().view(frames, V, 3, 4), out["batch_scos"].view(frames, V, J), conf_thres=0.05)
    assert torch.equal(out["points-3d"], want)                             # the existing path, unchanged
    # a threshold inside the scores' range, so that joints differ in how many views they select
    cfg.merge_from_list(["KEYPOINT.CONF_THRES", float(out["batch_scos"].median())])
    branches = set()
    for method in ("epipolar", "epipolar_dlt"):
        cfg.merge_from_list(["KEYPOINT.TRIANGULATION", method])
        with torch.no_grad():
            out = m(batch, is_train=False)[2]
        planes = lambda t: t.cuda().view(frames, V, 3, 4).contiguous()
        want, info = ops.triangulate_epipolar(
            out["batch_locs"].view(frames, V, J, 2).contiguous(), out["batch_scos"].view(frames, V, J).contiguous(), planes(P),
            planes(P[src.cpu()]), out["corr_pos"].view(frames, V, hs, hs, 2).contiguous(), downsample=float(cfg.BACKBONE.DOWNSAMPLE),
            resize=1.0, conf_thres=float(cfg.KEYPOINT.CONF_THRES), ransac_thres=400.0, dlt=method == "epipolar_dlt", want_info=True)
        assert out["points-3d"].dtype == torch.float64 and tuple(out["points-3d"].shape) == (frames, J, 3)
        assert torch.equal(out["points-3d"], want)
        branches |= set(((info >> 16) & 3).flatten().tolist())
    assert 0 in branches
    # EPIPOLAR.MULTITEST keeps no corr_pos: the epipolar methods say so
    cfg.merge_from_list(["EPIPOLAR.MULTITEST", True])
    with pytest.raises(ValueError, match="MULTITEST"), torch.no_grad():
        m(batch, is_train=False)
