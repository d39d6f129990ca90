"""The test-time metrics of Modelbuilder.forward on the GPU: the kernels (ops.eval_jdr / eval_pck / eval_epe) against the
reference-made fixture, the NumPy restatement and the library's host hooks, their reproducibility, the wrappers' argument
checks, and MultiViewPoseModel.forward under EPIPOLAR_AMD.EVAL_METRICS.  Everything is compared for equal bits (test_eval_metrics_cpu
says why) except EPEmean's mean: equal bits with the host hook, which sums in the kernel's order, and within the bound between two
summation orders of the restatement's and the reference's."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

import eval_metrics_restatement as restate
from test_eval_metrics_cpu import JDR_CASES, case, host_epe, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "lifting", "eval_metrics.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def lib():
    from epipolar_transformers_amd import _lib

    return _lib.load()


def gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(tensors):
    return [t.cpu().numpy() for t in tensors]


def kernel_jdr(pred, target, thr=0.5):
    from epipolar_transformers_amd import ops

    assert ops.POISON_OUTPUTS                                 # every output starts as NaN: an unwritten element shows
    return host(ops.eval_jdr(gpu(pred), gpu(target), thr, want_xy=True))


def kernel_pck(locs, gt, vis, thresholds=restate.THRESHOLDS, max_threshold=restate.MAX_TH):
    from epipolar_transformers_amd import ops

    pck, ej, tj = host(ops.eval_pck(gpu(locs), gpu(gt), gpu(vis), thresholds=thresholds, max_threshold=max_threshold))
    assert tj.shape == (len(locs), 1)
    return pck, ej, tj[:, 0]


def kernel_epe(pred, gt, vis, unit, max_dist):
    from epipolar_transformers_amd import ops

    mean, rows = ops.eval_epe(gpu(pred), gpu(gt), gpu(vis), unit=unit, max_dist=max_dist)
    assert mean.dim() == 0 and mean.dtype == torch.float64
    return np.float64(mean.item()), rows.cpu().numpy()


def test_kernels_match_the_reference_fixture(golden, lib):
    for name in JDR_CASES:
        g = case(golden, name)
        for key, value in zip(("dists", "acc", "pred_xy", "target_xy"), kernel_jdr(g("pred"), g("target"))):
            assert same_bits(value, g(key)), (name, key)
    g = case(golden, "jdr_nonsquare")
    assert same_bits(kernel_jdr(g("pred"), g("target"), 0.9)[1], g("acc_thr09"))           # x over the HEIGHT term
    g = case(golden, "pck_main")
    for key, value in zip(("pck", "err_joints", "total_joints"), kernel_pck(g("locs"), g("gt"), g("vis"))):
        assert same_bits(value, g(key)), key
    g = case(golden, "epe_main")
    unit, max_dist = float(g("unit")), float(g("max_dist"))
    mean, rows = kernel_epe(g("pred"), g("gt"), g("vis"), unit, max_dist)
    assert same_bits(rows, g("per_joint"))
    bound = restate.mean_bound(restate.epe_errors(g("pred"), g("gt"), unit, max_dist))
    print("kernel mean - reference: %.3g (bound %.3g)" % (mean - float(g("mean")), bound))
    assert abs(mean - float(g("mean"))) <= bound
    assert same_bits(mean, host_epe(lib, g("pred"), g("gt"), g("vis"), unit, max_dist)[0])


@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (5, 3, 10, 12), (3, 2, 3, 86), (7, 17, 64, 64), (2, 20, 96, 96), (3, 2, 128, 128)], ids=str)
def test_jdr_kernels_match_the_restatement(shape):
    """The smallest map (a partly filled wave), a non-square one, 258 elements (one past a 256-thread stride), the usual size, 20
    channels, and the map limit."""
    pred, target = restate.random_maps(*shape, seed=sum(shape))
    want = restate.jdr(pred, target)
    for key, a, b in zip(("dists", "acc", "pred_xy", "target_xy"), kernel_jdr(pred, target), want):
        assert same_bits(a, b), key
    from epipolar_transformers_amd import ops

    dists, acc = ops.eval_jdr(gpu(pred), gpu(target))                                       # the coordinates are nullable
    assert same_bits(dists.cpu().numpy(), want[0]) and same_bits(acc.cpu().numpy(), want[1])


def test_equal_maxima_the_lower_index_wins_and_nothing_positive_is_masked():
    h, w = 24, 30                                              # 720 elements: three strides of the block
    maps = np.zeros((1, 8, h, w), np.float32)
    flat = maps.reshape(8, h * w)
    flat[0, [70, 70 + 64]] = 0.5                               # i and i + 64: the next wave
    flat[1, [70, 70 + 256]] = 0.5                              # i and i + 256: the same thread, one stride on
    flat[2, [h * w - 1]] = 0.5                                 # the last element
    flat[3, [300, h * w - 1]] = 0.5
    flat[4] = 0.0                                              # all zero
    flat[5] = -0.0                                             # -0.0 with one +0.0: a tie, and not > 0
    flat[5, 400] = 0.0
    flat[6] = -np.linspace(1, 2, h * w, dtype=np.float32)      # all negative
    flat[7, [5, 6, 7, 500]] = [0.25, 0.5, 0.5, 0.5]
    target = np.zeros_like(maps)
    target[0, :, 10, 10] = 1.0
    want = restate.jdr(maps, target)
    got = kernel_jdr(maps, target)
    first = [70, 70, h * w - 1, 300, None, None, None, 6]
    for j, i in enumerate(first):
        assert got[2][0, j].tolist() == ([i % w, i // w] if i is not None else [0, 0]), j
    for key, a, b in zip(("dists", "acc", "pred_xy", "target_xy"), got, want):
        assert same_bits(a, b), key
    # a target without a positive value does not count: every joint -1, the average NaN
    got = kernel_jdr(target, -np.abs(maps) - np.float32(1))
    assert (got[0] == -1).all() and (got[1][1:] == -1).all() and np.isnan(got[1][0]) and (got[3] == 0).all()


@pytest.mark.parametrize("items", [(1, 1), (9, 7), (5, 13), (33, 17), (128, 17)], ids=lambda s: "%dx%d" % s)
def test_pck_and_epe_kernels_match_the_restatement(lib, items):
    """N * J = F * J = 1, 63, 65, 561 and 2176; T in {0, 1, 11}, M in {0, 20}; vis null, all zero (NaN percentages, zero totals)
    and mixed."""
    n, j = items
    assert n * j in (1, 63, 65, 561, 2176)
    for vis in ("none", "zeros", "mixed"):
        locs, gt, v = restate.random_points2d(n, j, seed=n + j, vis=vis)
        for th, max_th in (((), 0), ((5,), 20), (restate.THRESHOLDS, 20)):
            want = restate.pck(locs, gt, v, th, restate.curve_points(max_th))
            assert want[0].shape == (len(th),) and want[1].shape == (n, max_th)
            for key, a, b in zip(("pck", "err_joints", "total_joints"), kernel_pck(locs, gt, v, th, max_th), want):
                assert same_bits(a, b), (vis, th, key)
            if vis == "zeros":
                assert np.isnan(want[0]).all() and (want[2] == 0).all()
        pred, gt3, v = restate.random_points3d(n, j, seed=n * j, vis=vis)
        mean, rows = kernel_epe(pred, gt3, v, 2.5, 150.0)
        want_mean, want_rows = restate.epe(pred, gt3, v, 2.5, 150.0)
        assert same_bits(rows, want_rows), vis
        assert abs(mean - want_mean) <= restate.mean_bound(restate.epe_errors(pred, gt3, 2.5, 150.0))
        assert same_bits(mean, host_epe(lib, pred, gt3, v, 2.5, 150.0)[0])              # the same summation order


def test_repeated_calls_and_another_stream_give_the_same_bits():
    from epipolar_transformers_amd import ops

    pred, target = [gpu(a) for a in restate.random_maps(4, 17, 64, 64, seed=9)]
    locs, gt, vis = [gpu(a) for a in restate.random_points2d(33, 17, seed=9)]
    p3, g3, v3 = [gpu(a) for a in restate.random_points3d(128, 17, seed=9)]

    def run():
        return list(ops.eval_jdr(pred, target, want_xy=True)) + list(ops.eval_pck(locs, gt, vis)) + \
            list(ops.eval_epe(p3, g3, v3, unit=2.5, max_dist=150.0))

    first = run()
    for _ in range(3):
        assert all(torch.equal(a, b) for a, b in zip(first, run()))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = run()
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, other))


def test_argument_checks():
    from epipolar_transformers_amd import _lib, ops

    pred, target = [gpu(a) for a in restate.random_maps(2, 3, 6, 5, seed=1)]
    with pytest.raises(_lib.EpipolarAmdError):
        ops.eval_jdr(pred.cpu(), target)
    with pytest.raises(_lib.EpipolarAmdError):
        ops.eval_jdr(pred, target.cpu())
    with pytest.raises(TypeError):
        ops.eval_jdr(pred.double(), target)
    with pytest.raises(TypeError):
        ops.eval_jdr(pred, target.half())
    with pytest.raises(ValueError):
        ops.eval_jdr(pred, target[:, :2].contiguous())
    with pytest.raises(ValueError):
        ops.eval_jdr(pred[0], target[0])
    with pytest.raises(ValueError):
        ops.eval_jdr(pred, target.transpose(2, 3).contiguous().transpose(2, 3))             # right shape, not contiguous
    with pytest.raises(_lib.EpipolarAmdError, match="map 1 x 30"):
        ops.eval_jdr(pred.view(2, 3, 1, 30), target.view(2, 3, 1, 30))
    big = torch.zeros(1, 1, 128, 129, device="cuda")
    with pytest.raises(_lib.EpipolarAmdError, match="16384"):
        ops.eval_jdr(big, big)
    locs, gt, vis = [gpu(a) for a in restate.random_points2d(2, 3, seed=1)]
    with pytest.raises(_lib.EpipolarAmdError):
        ops.eval_pck(locs.cpu(), gt)
    with pytest.raises(_lib.EpipolarAmdError):
        ops.eval_pck(locs, gt, vis.cpu())
    with pytest.raises(TypeError):
        ops.eval_pck(locs, gt.float())                                                      # gt is float64
    with pytest.raises(TypeError):
        ops.eval_pck(locs.double(), gt)
    with pytest.raises(TypeError):
        ops.eval_pck(locs, gt, vis.bool())
    with pytest.raises(ValueError):
        ops.eval_pck(locs, gt[:, :2].contiguous())
    with pytest.raises(ValueError):
        ops.eval_pck(locs, gt, vis[:1])
    with pytest.raises(ValueError):
        ops.eval_pck(locs[..., :1].contiguous(), gt)
    p3, g3, v3 = [gpu(a) for a in restate.random_points3d(2, 3, seed=1)]
    with pytest.raises(_lib.EpipolarAmdError):
        ops.eval_epe(p3, g3.cpu())
    with pytest.raises(TypeError):
        ops.eval_epe(p3.float(), g3)
    with pytest.raises(TypeError):
        ops.eval_epe(p3, g3.float())
    with pytest.raises(ValueError):
        ops.eval_epe(p3, g3[:1])
    with pytest.raises(ValueError):
        ops.eval_epe(p3, g3, v3.view(3, 2))
    with pytest.raises(ValueError):
        ops.eval_epe(p3[..., :2].contiguous(), g3)


def _eval_batch(frames, V, channels, joints, size, hs, seed=3):
    from epipolar_transformers_amd import synthetic as syn
    from epipolar_transformers_amd.model import ring_sources

    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    m = frames * V
    P = torch.from_numpy(np.concatenate([syn.ring_cameras(V, size, jitter=(0.02, 1.0), rng=rng) for _ in range(frames)])).float()
    centres = np.stack([rng.integers(0, hs, (m, channels)), rng.integers(0, hs, (m, channels))], -1)
    return {"img": torch.randn(m, 3, size, size, generator=g).cuda(), "KRT": P, "other_index": ring_sources(frames, V, "cuda"),
            "num_views": V, "heatmap": gpu(restate.blob_maps(rng, centres, hs, hs)),
            "visibility": (torch.rand(m, channels, 1, generator=g) < 0.7).float().cuda(),
            "points-2d": (torch.rand(m, joints, 2, generator=g) * size).double().cuda(),
            "points-3d": (torch.randn(m, joints, 3, generator=g) * 300).double().cuda(), "unit": 0.5}


def _check_metrics(metrics, out, heat, target, locs, vis, gt2, pred3, gt3, vis3, unit, lib):
    """Every new key against the restatement applied to the tensors the model itself produced."""
    n = lambda t: np.array(t.detach().cpu().numpy(), order="C")            # (keeps a 0-d value 0-d)
    dists, acc, _, _ = restate.jdr(n(heat), n(target))
    assert same_bits(n(metrics["JDR"]), acc[0]) and same_bits(n(out["jdr_per_joint"]), acc[1:])
    pck, ej, tj = restate.pck(n(locs), n(gt2), n(vis))
    for i, th in enumerate(restate.THRESHOLDS):
        assert same_bits(n(metrics["PCK@%d" % th]), pck[i]), th
    assert same_bits(n(out["err_joints"]), ej) and same_bits(n(out["total_joints"])[:, 0], tj)
    want_mean, want_rows = restate.epe(n(pred3), n(gt3), n(vis3), unit, 150.0)
    assert same_bits(n(out["epe_per_joint"]), want_rows)
    assert abs(float(metrics["EPEmean_global"]) - want_mean) <= restate.mean_bound(restate.epe_errors(n(pred3), n(gt3), unit, 150.0))
    assert same_bits(np.float64(metrics["EPEmean_global"].item()), host_epe(lib, n(pred3), n(gt3), n(vis3), unit, 150.0)[0])


def test_model_computes_the_metrics_when_the_knob_is_set(lib):
    from test_gpu_model import _cfg, _model

    cfg, size, hs = _cfg(**{"KEYPOINT.TRIANGULATION": "pymvg", "KEYPOINT.CONF_THRES": 0.05})
    m = _model(cfg)
    frames, V, J = 2, 4, 17
    batch = _eval_batch(frames, V, J, J, size, hs)
    with torch.no_grad():
        _, metrics, out = m(batch, is_train=False)
    assert list(metrics) == ["MPJPE"]                                  # knob off (the default): exactly today's keys
    assert not {"epe_per_joint", "jdr_per_joint", "err_joints", "total_joints"} & set(out)
    cfg.merge_from_list(["EPIPOLAR_AMD.EVAL_METRICS", True])
    with torch.no_grad():
        _, on, out_on = m(batch, is_train=False)
    assert list(on) == ["MPJPE", "EPEmean_global", "JDR"] + ["PCK@%d" % t for t in restate.THRESHOLDS]
    assert sorted(out_on) == sorted(list(out) + ["epe_per_joint", "jdr_per_joint", "err_joints", "total_joints"])
    assert all(v.is_cuda for v in on.values())
    _check_metrics(on, out_on, out_on["heatmaps"], batch["heatmap"], out_on["batch_locs"], batch["visibility"].view(-1, J),
                   batch["points-2d"], out_on["points-3d"], batch["points-3d"].view(frames, V, J, 3)[:, 0],
                   batch["visibility"].view(frames, V, J)[:, 0], 0.5, lib)


def test_model_maps_twenty_channels_to_the_seventeen_joints(lib):
    from epipolar_transformers_amd.config import LenientCfgNode
    from test_gpu_model import _cfg, _model

    keep = list(restate.MAPPING)
    cfg, size, hs = _cfg(**{"KEYPOINT.TRIANGULATION": "pymvg", "KEYPOINT.CONF_THRES": 0.05, "KEYPOINT.NUM_PTS": 20})
    cfg.DATASETS.H36M = LenientCfgNode({"MAPPING": True})
    m = _model(cfg)
    frames, V = 2, 4
    batch = _eval_batch(frames, V, 20, 17, size, hs)
    with torch.no_grad():
        # knob off: the 20 channels, lifted as they are (without the 17-joint ground truth, which cannot be compared with them)
        out20 = m({k: v for k, v in batch.items() if k != "points-3d"}, is_train=False)[2]
        assert tuple(out20["points-3d"].shape) == (frames, 20, 3)
        cfg.merge_from_list(["EPIPOLAR_AMD.EVAL_METRICS", True])
        _, metrics, out = m(batch, is_train=False)
        # the same call made by hand on the 17 channels (of the same forward pass: equal bits)
        lifted = m.lift(out["batch_locs"], out["batch_scos"], batch["KRT"], V)
    assert tuple(out["points-3d"].shape) == (frames, 17, 3) and torch.equal(out["points-3d"], lifted)
    assert tuple(out["heatmaps"].shape) == (frames * V, 17, hs, hs) and tuple(out["batch_locs"].shape) == (frames * V, 17, 2)
    # ... which are channels MAPPING of the 20 (another forward pass: equal to the trunk's rounding)
    assert (out["heatmaps"] - out20["heatmaps"][:, keep]).abs().max().item() <= 1e-4
    assert (out["batch_scos"] - out20["batch_scos"][:, keep]).abs().max().item() <= 1e-4
    vis = batch["visibility"].view(-1, 20)[:, keep]
    _check_metrics(metrics, out, out["heatmaps"], batch["heatmap"][:, keep], out["batch_locs"], vis, batch["points-2d"], lifted,
                   batch["points-3d"].view(frames, V, 17, 3)[:, 0], vis.reshape(frames, V, 17)[:, 0], 0.5, lib)
    # a 19-channel head under MAPPING True is an error that names the key
    cfg19, _, _ = _cfg(**{"KEYPOINT.NUM_PTS": 19, "EPIPOLAR_AMD.EVAL_METRICS": True})
    cfg19.DATASETS.H36M = LenientCfgNode({"MAPPING": True})
    with pytest.raises(ValueError, match="DATASETS.H36M.MAPPING"):
        with torch.no_grad():
            _model(cfg19)(_eval_batch(1, 4, 19, 17, size, hs), is_train=False)
