"""KEYPOINT.TRIANGULATION rpsm on the GPU: the kernels (ops.rpsm) against the reference-made fixture and the NumPy restatement,
one run at the config defaults (depth 10), reproducibility, workspace handling, the wrapper's argument checks and the model's
dispatch.  TOLERANCE_MM and the margin condition: tests/test_rpsm_cpu.py, tests/rpsm_restatement.py."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

import rpsm_restatement as restate
from test_rpsm_cpu import CASES, TOLERANCE_MM, case

pytestmark = pytest.mark.gpu


def on_gpu(sc):
    return [torch.from_numpy(sc[k]).cuda() for k in restate.ARRAYS]


def run(sc, params, **kw):
    from epipolar_transformers_amd import ops

    first = sc.get("first_limb_length")
    return ops.rpsm(*on_gpu(sc), first_limb_length=None if first is None else torch.from_numpy(first).cuda(),
                    parent=restate.H36M_PARENT[:sc["heat"].shape[2]], want_path=True, **params, **kw)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "lifting", "rpsm.npz"))


@pytest.fixture(scope="module")
def two_scenes():
    """Two scenes of different shapes with the restatement's answers, shared by the tests that only need SOME correct input."""
    pa = dict(image_size=(256, 256), grid_size=1200, first_nbins=6, recur_nbins=2, recur_depth=4, tolerance=150.0)
    pb = dict(image_size=(256, 256), grid_size=900, first_nbins=4, recur_nbins=3, recur_depth=2, tolerance=150.0)
    a, ra = restate.scene(11, 3, 4, 17, 24, 24, pa)
    b, rb = restate.scene(12, 2, 3, 9, 16, 20, pb)
    return (a, pa, ra), (b, pb, rb)


def test_kernel_matches_the_reference_fixture(golden):
    for name in CASES:
        sc, params, ref, (pose, path, margins, band) = case(golden, name)
        X, p = run(sc, params)
        err = np.abs(X[0].cpu().numpy().astype(np.float64) - ref).max()
        print(name, "kernel vs reference: %.3g mm" % err)
        assert err <= TOLERANCE_MM, (name, err)
        assert np.array_equal(p.cpu().numpy(), path), name


@pytest.mark.parametrize("F,V,J,first_nbins,grid_size", [(1, 2, 2, 2, 300), (5, 4, 17, 6, 1200), (2, 8, 17, 16, 2000),
                                                         (33, 3, 17, 4, 900)], ids=lambda v: str(v))
def test_kernel_matches_the_restatement(F, V, J, first_nbins, grid_size):
    """The smallest problem (one limb, 8 bins); 216 bins (a ragged last wave); 4096 bins and eight views; 33 frames of 64 bins.
    Every scene meets the margin condition (restate.scene), so the bins must be the restatement's.  The outputs start as NaN
    (conftest: ops.POISON_OUTPUTS), so a joint the kernels did not write shows."""
    from epipolar_transformers_amd import ops

    assert ops.POISON_OUTPUTS
    params = dict(image_size=(256, 256), grid_size=grid_size, first_nbins=first_nbins, recur_nbins=2, recur_depth=4, tolerance=150.0)
    sc, (pose, path, margins, band) = restate.scene(100 + F + V, F, V, J, 22, 26, params)
    assert restate.condition_holds(margins, band)
    X, p = run(sc, params)
    assert X.dtype == torch.float32 and tuple(X.shape) == (F, J, 3) and p.dtype == torch.int32 and tuple(p.shape) == (F, 5, J)
    X = X.cpu().numpy()
    assert np.isfinite(X).all()
    assert np.array_equal(p.cpu().numpy(), path)
    err = np.abs(X - pose).max()
    print((F, V, J, first_nbins), "kernel vs restatement: %.3g mm" % err)
    assert err <= TOLERANCE_MM, err


def test_config_defaults_depth_10():
    """FIRST_NBINS 16, RECUR_NBINS 2, RECUR_DEPTH 10, GRID_SIZE 2000, tolerance 150: the deep levels are decided at float32
    rounding, so the bins must agree up to the first level k* whose margin in the float64 restatement is below 1e-4, and the pose
    within sqrt(3) x that level's grid size (or within TOLERANCE_MM when no level is that close)."""
    from epipolar_transformers_amd import default_cfg

    ps = default_cfg().PICT_STRUCT
    params = dict(image_size=(256, 256), grid_size=ps.GRID_SIZE, first_nbins=ps.FIRST_NBINS, recur_nbins=ps.RECUR_NBINS,
                  recur_depth=ps.RECUR_DEPTH, tolerance=float(ps.LIMB_LENGTH_TOLERANCE))
    assert (params["first_nbins"], params["recur_depth"]) == (16, 10)
    fr = restate.frame(2024, 4, 17, 32, 32)
    sc = {k: np.ascontiguousarray(fr[k][None]) for k in restate.ARRAYS}
    pose, path, margins, band = restate.run(sc, params)
    close = np.nonzero(margins[0] < restate.MARGIN)[0]
    k_star = int(close[0]) if close.size else 11
    X, p = run(sc, params)
    print("margins", margins[0], "k* =", k_star)
    assert np.array_equal(p.cpu().numpy()[0, :k_star], path[0, :k_star])
    bound = TOLERANCE_MM if k_star == 11 else np.sqrt(3.0) * restate.level_size(params["grid_size"], 16, 2, k_star)
    err = np.linalg.norm(X[0].cpu().numpy() - pose[0], axis=1).max()
    print("kernel vs restatement: %.3g mm, bound %.3g mm" % (err, bound))
    assert err <= bound


def test_repeated_calls_and_a_side_stream_give_the_same_bits(two_scenes):
    (sc, params, (pose, path, _, _)), _ = two_scenes
    X0, p0 = run(sc, params)
    assert np.array_equal(p0.cpu().numpy(), path)
    for _ in range(3):
        X, p = run(sc, params)
        assert torch.equal(X, X0) and torch.equal(p, p0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        X, p = run(sc, params)
    side.synchronize()
    assert torch.equal(X, X0) and torch.equal(p, p0)


def test_workspace_reused_across_shapes_and_misaligned(two_scenes):
    from epipolar_transformers_amd import ops

    (a, pa, ra), (b, pb, rb) = two_scenes
    need = max(ops.rpsm_workspace_bytes(3, 17, 6, 2), ops.rpsm_workspace_bytes(2, 9, 4, 3))
    ws = torch.empty(need + 4, dtype=torch.uint8, device="cuda")
    fresh_a, fresh_b = run(a, pa), run(b, pb)
    assert np.array_equal(fresh_a[1].cpu().numpy(), ra[1]) and np.array_equal(fresh_b[1].cpu().numpy(), rb[1])
    for sc, params, fresh in ((a, pa, fresh_a), (b, pb, fresh_b), (a, pa, fresh_a)):
        X, p = run(sc, params, workspace=ws)
        assert torch.equal(X, fresh[0]) and torch.equal(p, fresh[1])
    for sc, params, fresh in ((b, pb, fresh_b), (a, pa, fresh_a)):
        X, p = run(sc, params, workspace=ws[4:])          # 4 bytes off whatever alignment the allocator gave
        assert torch.equal(X, fresh[0]) and torch.equal(p, fresh[1])
    with pytest.raises(ValueError, match="workspace"):
        run(a, pa, workspace=ws[:16])


def test_wrapper_argument_checks(two_scenes):
    from epipolar_transformers_amd import _lib, ops

    _, (sc, params, _) = two_scenes
    kw = dict(parent=restate.H36M_PARENT[:9], **params)
    good = on_gpu(sc)
    ops.rpsm(*good, **kw)
    with pytest.raises(_lib.EpipolarAmdError):
        ops.rpsm(good[0].cpu(), *good[1:], **kw)
    with pytest.raises(TypeError):
        ops.rpsm(good[0].double(), *good[1:], **kw)
    with pytest.raises(TypeError):
        ops.rpsm(*good[:4], good[4].half(), **kw)
    with pytest.raises(ValueError):
        ops.rpsm(good[0], good[1][:, :2].contiguous(), *good[2:], **kw)
    with pytest.raises(ValueError):
        ops.rpsm(good[0][0], *good[1:], **kw)
    with pytest.raises(ValueError):
        ops.rpsm(good[0].transpose(3, 4).contiguous().transpose(3, 4), *good[1:], **kw)      # right shape, not contiguous
    with pytest.raises(ValueError):
        ops.rpsm(*good, **dict(kw, parent=restate.H36M_PARENT[:8]))
    nine = [t.repeat_interleave(3, 1).contiguous() for t in good[:3]]
    with pytest.raises(_lib.EpipolarAmdError, match="V=9"):
        ops.rpsm(*nine, *good[3:], **kw)


def test_model_lifts_by_rpsm():
    """MultiViewPoseModel in eval mode with VIS.MULTIVIEW and KEYPOINT.TRIANGULATION rpsm: with the batch's `rpsm` dict it returns
    exactly what ops.rpsm gives for the model's own heat maps; the same batch without the dict returns triangulate_dlt's bits."""
    from epipolar_transformers_amd import ops, pictorial, synthetic as syn
    from epipolar_transformers_amd.model import ring_sources
    from epipolar_transformers_amd.triangulate import triangulate_dlt
    from test_gpu_model import _cfg, _model

    cfg, size, hs = _cfg(**{"KEYPOINT.TRIANGULATION": "rpsm", "KEYPOINT.CONF_THRES": 0.05, "PICT_STRUCT.FIRST_NBINS": 8,
                            "PICT_STRUCT.RECUR_DEPTH": 3})
    m = _model(cfg)
    frames, V, J = 2, 4, 17
    P = torch.from_numpy(syn.ring_cameras(V, size)).float().repeat(frames, 1, 1)
    img = torch.randn(frames * V, 3, size, size, device="cuda")
    batch = {"img": img, "KRT": P, "other_index": ring_sources(frames, V, "cuda"), "num_views": V}
    with torch.no_grad():
        out = m(batch, is_train=False)[2]
    want = triangulate_dlt(out["batch_locs"].view(frames, V, J, 2), P.cuda().view(frames, V, 3, 4),
                           out["batch_scos"].view(frames, V, J), conf_thres=0.05)
    assert torch.equal(out["points-3d"], want)                             # no dict: the existing path, unchanged
    gen = torch.Generator().manual_seed(3)
    extra = dict(cameras=P, crop_center=torch.full((frames * V, 2), size / 2.0) + torch.randn(frames * V, 2, generator=gen),
                 crop_scale=torch.full((frames * V, 2), size / 200.0), center=torch.randn(frames, 3, generator=gen) * 50,
                 limb_length=200 + 200 * torch.rand(frames, J - 1, generator=gen))
    with torch.no_grad():
        out = m(dict(batch, rpsm=extra), is_train=False)[2]
    cuda = lambda t, *shape: t.cuda().view(*shape).contiguous()
    direct = ops.rpsm(out["heatmaps"].view(frames, V, J, hs, hs).contiguous(), cuda(P, frames, V, 3, 4),
                      pictorial.crop_transform(cuda(extra["crop_center"], frames, V, 2), cuda(extra["crop_scale"], frames, V, 2),
                                               (size, size)),
                      extra["center"].cuda(), extra["limb_length"].cuda(), image_size=(size, size), grid_size=2000.0, first_nbins=8,
                      recur_nbins=2, recur_depth=3, tolerance=150.0)
    assert out["points-3d"].dtype == torch.float32 and tuple(out["points-3d"].shape) == (frames, J, 3)
    assert torch.equal(out["points-3d"], direct) and torch.isfinite(direct).all()
    cfg.merge_from_list(["EPIPOLAR.MULTITEST", True])                      # no heat maps: rpsm says so
    with pytest.raises(ValueError, match="MULTITEST"), torch.no_grad():
        m(dict(batch, rpsm=extra), is_train=False)
