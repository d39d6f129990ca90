"""The test-time metrics of Modelbuilder.forward on the CPU: the library's host hooks (et_debug_host_eval_jdr / _pck / _epe: the
kernels' own per-item routines in serial loops) and the NumPy restatement against what the reference's JDR, calculate_err /
calc_pck and EPEmean returned (tests/golden/lifting/eval_metrics.npz, made by make_eval_metrics_golden.py), the hooks against the
restatement where the reference has no answer, the ABI's argument checks, and the wiring of MultiViewPoseModel.forward under
EPIPOLAR_AMD.EVAL_METRICS.

Everything but the mean of EPEmean is compared for EQUAL BITS: integer counts, or correctly rounded float64 operations on the
reference's operands in the reference's order.  The mean is within 2 (n - 1) 2^-53 sum(err) / n of the reference's, the bound
between two summation orders of the same n terms (torch's CPU mean does not sum in index order)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

import eval_metrics_restatement as restate
from epipolar_transformers_amd import _lib, build, default_cfg, model, ops
from epipolar_transformers_amd.config import LenientCfgNode

JDR_CASES = {"jdr_main": (7, 17, 64, 64), "jdr_nonsquare": (5, 3, 10, 12), "jdr_exact_half": (4, 2, 20, 20)}
NEW_SYMBOLS = ("et_eval_jdr", "et_eval_pck", "et_eval_epe", "et_debug_host_eval_jdr", "et_debug_host_eval_pck",
               "et_debug_host_eval_epe")
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "lifting", "eval_metrics.npz"), allow_pickle=False)


def case(golden, name):
    return lambda k: golden["%s.%s" % (name, k)]


def same_bits(a, b):
    """Equal shape, dtype and bits; a NaN equals a NaN whatever its sign and payload (0 / 0 differs between processors)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.where(np.isnan(a), 0, a).tobytes() == np.where(np.isnan(b), 0, b).tobytes()


def fp(a):
    return NULL if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_jdr(lib, pred, target, thr=0.5, want_xy=True):
    n, j, h, w = pred.shape
    dists, acc = np.full((j, n), np.nan), np.full(j + 1, np.nan)
    pxy = np.full((n, j, 2), np.nan, np.float32) if want_xy else None
    txy = np.full((n, j, 2), np.nan, np.float32) if want_xy else None
    rc = lib.et_debug_host_eval_jdr(n, j, h, w, fp(pred), fp(target), thr, fp(dists), fp(acc), fp(pxy), fp(txy))
    assert rc == 0, lib.et_last_error()
    return dists, acc, pxy, txy


def host_pck(lib, locs, gt, vis, thresholds=restate.THRESHOLDS, curve=None):
    curve = restate.curve_points() if curve is None else np.asarray(curve, np.float64)
    th = np.asarray(thresholds, np.float64).reshape(-1)
    n, j, _ = locs.shape
    pck, ej, tj = np.full(len(th), -7.0), np.full((n, len(curve)), -7.0), np.full(n, -7.0)
    rc = lib.et_debug_host_eval_pck(n, j, fp(locs), fp(gt), fp(vis), len(th), fp(th) if len(th) else NULL, len(curve),
                                    fp(curve) if len(curve) else NULL, fp(pck) if len(th) else NULL,
                                    fp(ej) if len(curve) else NULL, fp(tj))
    assert rc == 0, lib.et_last_error()
    return pck, ej, tj


def host_epe(lib, pred, gt, vis, unit, max_dist):
    f, j, _ = pred.shape
    mean, rows = np.full(1, np.nan), np.full((f, j), np.nan)
    rc = lib.et_debug_host_eval_epe(f, j, fp(pred), fp(gt), fp(vis), unit, max_dist, fp(mean), fp(rows))
    assert rc == 0, lib.et_last_error()
    return mean[0], rows


def test_fixture_holds_every_case_and_the_makers_conditions(golden):
    assert sorted({k.split(".")[0] for k in golden.files}) == sorted(list(JDR_CASES) + ["pck_main", "epe_main"])
    for name, shape in JDR_CASES.items():
        g = case(golden, name)
        assert g("pred").shape == shape and g("target").shape == shape and g("pred").dtype == np.float32
        assert g("dists").shape == (shape[1], shape[0]) and g("acc").shape == (shape[1] + 1,) and float(g("thr")) == 0.5
        assert restate.jdr_margin(g("dists")) >= 1e-6
    g = case(golden, "jdr_main")
    assert g("acc")[1 + 5] == -1 and (g("dists") == -1).any() and (g("dists")[g("dists") != -1] < 0.5).any()
    assert (g("pred").reshape(7 * 17, -1).max(1) <= 0).any() and (g("target").reshape(7 * 17, -1).max(1) <= 0).any()
    g = case(golden, "jdr_exact_half")
    assert set(np.unique(g("dists"))) == {0.0, 0.5}                 # the designed exact distances: 0.5 is not below 0.5
    assert g("acc")[1] == (g("dists")[0] == 0).mean() and g("acc")[2] == (g("dists")[1] == 0).mean()
    g = case(golden, "pck_main")
    assert restate.pck_margin(g("locs"), g("gt"), g("vis")) >= 1e-6 and (g("vis") == 0).any() and (g("vis")[3] == 0).all()
    assert same_bits(g("curve"), np.linspace(0, 20, num=20)) and g("thresholds").tolist() == list(restate.THRESHOLDS)
    g = case(golden, "epe_main")
    assert float(g("unit")) != 1 and (g("per_joint") == float(g("max_dist"))).any() and (g("vis") == 0).any()
    assert ((g("per_joint") > 0) & (g("per_joint") < float(g("max_dist")))).any()


@pytest.mark.parametrize("name", list(JDR_CASES))
def test_jdr_matches_the_reference_to_the_bit(lib, golden, name):
    g = case(golden, name)
    for who, got in (("restatement", restate.jdr(g("pred"), g("target"))), ("host hook", host_jdr(lib, g("pred"), g("target")))):
        for key, value in zip(("dists", "acc", "pred_xy", "target_xy"), got):
            assert same_bits(value, g(key)), (name, who, key)
    assert host_jdr(lib, g("pred"), g("target"), want_xy=False)[2] is None      # the coordinates are nullable
    if name == "jdr_nonsquare":
        # thr 0.9 separates one pixel along x (1 / (H/10) = 1) from one along y (1 / (W/10) = 0.83): x is divided by the HEIGHT term
        assert same_bits(restate.jdr(g("pred"), g("target"), 0.9)[1], g("acc_thr09"))
        assert same_bits(host_jdr(lib, g("pred"), g("target"), 0.9)[1], g("acc_thr09"))
        assert not same_bits(g("acc_thr09"), g("acc"))


def test_pck_matches_the_reference_to_the_bit(lib, golden):
    g = case(golden, "pck_main")
    for who, got in (("restatement", restate.pck(g("locs"), g("gt"), g("vis"))), ("host hook", host_pck(lib, g("locs"), g("gt"), g("vis")))):
        for key, value in zip(("pck", "err_joints", "total_joints"), got):
            assert same_bits(value, g(key)), (who, key)
    # the error is the x difference alone: moving every y changes nothing
    moved = g("gt").copy()
    moved[..., 1] += 1000.0
    assert same_bits(host_pck(lib, g("locs"), moved, g("vis"))[0], g("pck"))


def test_epe_matches_the_reference(lib, golden):
    g = case(golden, "epe_main")
    unit, max_dist = float(g("unit")), float(g("max_dist"))
    bound = restate.mean_bound(restate.epe_errors(g("pred"), g("gt"), unit, max_dist))
    assert 0 < bound < 1e-11
    for who, (mean, rows) in (("restatement", restate.epe(g("pred"), g("gt"), g("vis"), unit, max_dist)),
                              ("host hook", host_epe(lib, g("pred"), g("gt"), g("vis"), unit, max_dist))):
        assert same_bits(rows, g("per_joint")), who
        print("%s mean - reference: %.3g (bound %.3g)" % (who, mean - float(g("mean")), bound))
        assert abs(mean - float(g("mean"))) <= bound, who


def test_hooks_match_the_restatement_where_the_reference_raises(lib):
    """No joint that counts (JDR's average is 0 / 0) and no visible item (the PCK percentages are 0 / 0): NaN, not an error."""
    pred, target = restate.random_maps(3, 2, 8, 9, seed=1)
    target[:] = -np.abs(target)
    for got in (restate.jdr(pred, target), host_jdr(lib, pred, target)):
        assert (got[0] == -1).all() and (got[1][1:] == -1).all() and np.isnan(got[1][0]) and (got[3] == 0).all()
    locs, gt, vis = restate.random_points2d(3, 5, seed=2, vis="zeros")
    for got in (restate.pck(locs, gt, vis), host_pck(lib, locs, gt, vis)):
        assert np.isnan(got[0]).all() and got[0].shape == (11,) and (got[1] == 0).all() and (got[2] == 0).all()
    # vis NULL: every item counts
    assert same_bits(host_pck(lib, locs, gt, None)[2], np.full(3, 5.0))
    for a, b in zip(host_pck(lib, locs, gt, None), restate.pck(locs, gt, None)):
        assert same_bits(a, b)


@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (5, 3, 10, 12), (3, 2, 3, 86), (2, 20, 96, 96), (3, 2, 128, 128)], ids=str)
def test_jdr_hook_matches_the_restatement_on_random_maps(lib, shape):
    pred, target = restate.random_maps(*shape, seed=sum(shape))
    for a, b in zip(host_jdr(lib, pred, target), restate.jdr(pred, target)):
        assert same_bits(a, b)


def test_signed_zeros_tie_and_the_first_maximum_wins(lib):
    maps = np.full((1, 4, 6, 7), -0.0, np.float32)
    maps[0, 0, 3, 4] = 0.0                                       # -0.0 everywhere, one +0.0: a tie, index 0 -- and masked anyway
    maps[0, 1] = -1.5                                            # all negative
    maps[0, 2] = 0.0
    maps[0, 2, 2, 3] = maps[0, 2, 5, 6] = 0.75                   # twice: the first
    maps[0, 3, 5, 6] = 0.25                                      # the last element
    target = np.zeros_like(maps)
    target[0, :, 2, 3] = 1.0
    for got in (restate.jdr(maps, target), host_jdr(lib, maps, target)):
        assert got[2].tolist() == [[[0, 0], [0, 0], [3, 2], [6, 5]]] and (got[3] == [3, 2]).all()
        a, b = 3 / (6 / 10), 2 / (7 / 10)                       # x over the height term, y over the width term
        assert got[0][:3, 0].tolist() == [np.sqrt(a * a + b * b), np.sqrt(a * a + b * b), 0.0]


@pytest.mark.parametrize("items", [(1, 1), (9, 7), (5, 13), (33, 17), (128, 17)], ids=str)
def test_pck_and_epe_hooks_match_the_restatement(lib, items):
    n, j = items
    for vis in ("none", "zeros", "mixed"):
        locs, gt, v = restate.random_points2d(n, j, seed=n + j, vis=vis)
        for th, curve in (((), ()), ((5,), restate.curve_points()), (restate.THRESHOLDS, restate.curve_points())):
            for a, b in zip(host_pck(lib, locs, gt, v, th, curve), restate.pck(locs, gt, v, th, curve)):
                assert same_bits(a, b), (vis, th)
        pred, gt3, v = restate.random_points3d(n, j, seed=n * j, vis=vis)
        mean, rows = host_epe(lib, pred, gt3, v, 2.5, 150.0)
        want_mean, want_rows = restate.epe(pred, gt3, v, 2.5, 150.0)
        assert same_bits(rows, want_rows)
        assert abs(mean - want_mean) <= restate.mean_bound(restate.epe_errors(pred, gt3, 2.5, 150.0))


def test_header_ctypes_and_exports_agree_and_bad_arguments_are_errors(lib):
    text = open(os.path.join(ROOT, "include", "epipolar_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert ("int %s(" % name) in text and name in _lib.exported_symbols() and hasattr(lib, name)
    assert lib.et_abi_version() == 14 and _lib.ET_ABI_VERSION == 14      # additive: the version stays
    assert "NaN" in text[text.index("et_eval_jdr:"):text.index("int et_eval_jdr(")]
    err = lambda: lib.et_last_error()
    # (the device entry points report these before any launch: no GPU is touched)
    maps = np.zeros((1, 1, 4, 4), np.float32)
    d, a = np.zeros((1, 1)), np.zeros(2)
    for entry, extra in ((lib.et_debug_host_eval_jdr, ()), (lib.et_eval_jdr, (NULL,))):
        bad = lambda n, j, h, w, p=fp(maps), t=fp(maps), dd=fp(d), aa=fp(a): entry(n, j, h, w, p, t, 0.5, dd, aa, NULL, NULL, *extra) != 0
        assert bad(1, 1, 1, 16) and b"map 1 x 16" in err()
        assert bad(1, 1, 16, 1) and b"map 16 x 1" in err()
        assert bad(1, 1, 128, 129) and b"16384" in err()
        assert bad(0, 1, 4, 4) and b"bad sizes" in err()
        assert bad(1, -1, 4, 4) and b"bad sizes" in err()
        for k in ("p", "t", "dd", "aa"):
            assert bad(1, 1, 4, 4, **{k: NULL}) and b"NULL" in err()
        assert extra or not bad(1, 1, 4, 4)                 # (valid arguments: only the host hook can run here)
    locs, gt, tj = np.zeros((1, 1, 2), np.float32), np.zeros((1, 1, 2)), np.zeros(1)
    th, out = np.ones(2), np.zeros(2)
    for entry, extra in ((lib.et_debug_host_eval_pck, ()), (lib.et_eval_pck, (NULL,))):
        bad = lambda n, j, T, M, l=fp(locs), g=fp(gt), t=fp(th), c=fp(th), p=fp(out), e=fp(out), tt=fp(tj): \
            entry(n, j, l, g, NULL, T, t, M, c, p, e, tt, *extra) != 0
        assert bad(0, 1, 2, 2) and b"bad sizes" in err()
        assert bad(1, 0, 2, 2) and b"bad sizes" in err()
        assert bad(1, 1, -1, 2) and b"T=-1" in err()
        assert bad(1, 1, 2, -1) and b"M=-1" in err()
        for k in ("l", "g", "t", "c", "p", "e", "tt"):
            assert bad(1, 1, 2, 2, **{k: NULL}) and b"NULL" in err()
    # T == 0 and M == 0 are valid, write nothing, and their arrays may be NULL
    assert lib.et_debug_host_eval_pck(1, 1, fp(locs), fp(gt), NULL, 0, NULL, 0, NULL, NULL, NULL, fp(tj)) == 0 and tj[0] == 1
    pts, mean, rows = np.zeros((1, 1, 3)), np.zeros(1), np.zeros((1, 1))
    for entry, extra in ((lib.et_debug_host_eval_epe, ()), (lib.et_eval_epe, (NULL,))):
        bad = lambda f, j, p=fp(pts), g=fp(pts), m=fp(mean), r=fp(rows): entry(f, j, p, g, NULL, 1.0, 150.0, m, r, *extra) != 0
        assert bad(0, 1) and b"bad sizes F=0" in err()
        assert bad(1, 0) and b"bad sizes" in err()
        for k in ("p", "g", "m", "r"):
            assert bad(1, 1, **{k: NULL}) and b"NULL" in err()


def test_ops_wrappers_reject_cpu_tensors():
    assert default_cfg().EPIPOLAR_AMD.EVAL_METRICS is False
    pred, target = [torch.from_numpy(a) for a in restate.random_maps(1, 1, 4, 4, seed=0)]
    with pytest.raises(_lib.EpipolarAmdError):
        ops.eval_jdr(pred, target)
    locs, gt, _ = restate.random_points2d(1, 2, seed=0)
    with pytest.raises(_lib.EpipolarAmdError):
        ops.eval_pck(torch.from_numpy(locs), torch.from_numpy(gt))
    p3, g3, _ = restate.random_points3d(1, 2, seed=0)
    with pytest.raises(_lib.EpipolarAmdError):
        ops.eval_epe(torch.from_numpy(p3), torch.from_numpy(g3))


# ---- the wiring of MultiViewPoseModel.forward, with the kernels and the network replaced by recorders -----------------------------
class _Stub(model.MultiViewPoseModel):
    """forward() with a canned backbone result: heat (M,C,H,W), locs (M,C,2), scos (M,C)."""

    def __init__(self, cfg, channels, frames=2, views=2, hw=(6, 5)):
        torch.nn.Module.__init__(self)
        self.cfg, self.sharded, self.criterion = cfg, None, model.JointsMSELoss()
        m = frames * views
        g = torch.Generator().manual_seed(0)
        self.canned = (None, [torch.rand(m, channels, *hw, generator=g)], torch.rand(m, channels, 2, generator=g) * 20,
                       torch.rand(m, channels, generator=g), None, None, None, None)

    def forward_views(self, *a, **k):
        return self.canned

    def forward_multitest(self, *a, **k):
        return self.canned[2], self.canned[3]


def _wiring_cfg(channels=17, mapping=None, knob=True, **test_keys):
    cfg = default_cfg()
    cfg.merge_from_list(["BACKBONE.BODY", "epipolarposeR-18", "KEYPOINT.NUM_PTS", channels, "VIS.MULTIVIEW", True,
                         "KEYPOINT.TRIANGULATION", "pymvg", "EPIPOLAR_AMD.EVAL_METRICS", knob])
    if mapping is not None:
        cfg.DATASETS.H36M = LenientCfgNode({"MAPPING": mapping})
    if test_keys:
        cfg.TEST = LenientCfgNode(test_keys)
    return cfg


def _batch(stub, joints, frames=2, views=2):
    m = frames * views
    g = torch.Generator().manual_seed(1)
    heat = stub.canned[1][0]
    return {"img": torch.zeros(m, 3, 8, 8), "KRT": torch.rand(m, 3, 4, generator=g), "other_index": torch.arange(m), "num_views": views,
            "heatmap": torch.rand(m, heat.shape[1], *heat.shape[2:], generator=g), "points-2d": torch.rand(m, joints, 3, generator=g),
            "visibility": (torch.rand(m, heat.shape[1], 1, generator=g) < 0.7), "points-3d": torch.rand(m, joints, 3, generator=g),
            "unit": 2.0}


@pytest.fixture
def recorded(monkeypatch):
    calls = []
    monkeypatch.setattr(model, "triangulate_dlt", lambda pts, krt, conf, **k: calls.append(("lift", (pts, krt, conf), k)) or
                        torch.zeros(pts.shape[0], pts.shape[2], 3, dtype=torch.float64))
    monkeypatch.setattr(ops, "eval_jdr", lambda *a, **k: calls.append(("jdr", a, k)) or
                        (None, torch.arange(a[0].shape[1] + 1.0, dtype=torch.float64)))
    monkeypatch.setattr(ops, "eval_pck", lambda *a, **k: calls.append(("pck", a, k)) or
                        (torch.arange(float(len(k["thresholds"])), dtype=torch.float64), "EJ", "TJ"))
    monkeypatch.setattr(ops, "eval_epe", lambda *a, **k: calls.append(("epe", a, k)) or (torch.tensor(3.0, dtype=torch.float64), "ROWS"))
    return calls


def test_knob_off_keeps_todays_keys(recorded):
    stub = _Stub(_wiring_cfg(knob=False), 17)
    _, metrics, out = stub(_batch(stub, 17), is_train=False)
    assert list(metrics) == ["MPJPE"] and [c[0] for c in recorded] == ["lift"]
    assert sorted(out) == sorted(["heatmap_pred", "batch_locs", "score_pred", "batch_scos", "heatmaps", "points-3d"])
    # ... also when DATASETS.H36M.MAPPING is set: the mapping belongs to the knob
    stub = _Stub(_wiring_cfg(20, mapping=True, knob=False), 20)
    _, metrics, out = stub(_batch(stub, 20), is_train=False)
    assert list(metrics) == ["MPJPE"] and tuple(out["points-3d"].shape) == (2, 20, 3)


def test_knob_on_calls_the_three_metrics_with_the_references_arguments(recorded):
    stub = _Stub(_wiring_cfg(), 17)
    batch = _batch(stub, 17)
    _, metrics, out = stub(batch, is_train=False)
    assert [c[0] for c in recorded] == ["lift", "epe", "jdr", "pck"]
    assert list(metrics) == ["MPJPE", "EPEmean_global", "JDR"] + ["PCK@%d" % t for t in restate.THRESHOLDS]
    assert float(metrics["EPEmean_global"]) == 3.0 and float(metrics["JDR"]) == 0.0 and float(metrics["PCK@100"]) == 10.0
    assert out["epe_per_joint"] == "ROWS" and out["err_joints"] == "EJ" and out["total_joints"] == "TJ"
    assert torch.equal(out["jdr_per_joint"], torch.arange(1.0, 18.0, dtype=torch.float64))
    by = {c[0]: c for c in recorded}
    pred, gt = by["epe"][1]
    assert gt.dtype == torch.float64 and torch.equal(gt, batch["points-3d"].view(2, 2, 17, 3)[:, 0].double())
    assert by["epe"][2]["unit"] == 2.0 and by["epe"][2]["max_dist"] == 150.0
    assert torch.equal(by["epe"][2]["vis"], batch["visibility"].view(2, 2, 17)[:, 0].float())
    heat, target = by["jdr"][1]
    assert torch.equal(heat, stub.canned[1][0]) and torch.equal(target, batch["heatmap"])
    locs, gt2 = by["pck"][1]
    assert torch.equal(locs, stub.canned[2]) and gt2.dtype == torch.float64 and torch.equal(gt2, batch["points-2d"][..., :2].double())
    assert torch.equal(by["pck"][2]["vis"], batch["visibility"].view(4, 17).float())
    assert by["pck"][2]["thresholds"] == restate.THRESHOLDS and by["pck"][2]["max_threshold"] == 20
    # training is untouched by the knob
    del recorded[:]
    assert stub(batch, is_train=True)[1] == {} and not recorded


def test_test_keys_are_read_and_pck_can_be_switched_off(recorded):
    stub = _Stub(_wiring_cfg(PCK=True, THRESHOLDS=(2, 7.5), MAX_TH=30, EPEMEAN_MAX_DIST=99), 17)
    batch = _batch(stub, 17)
    del batch["unit"], batch["visibility"]
    _, metrics, _ = stub(batch, is_train=False)
    by = {c[0]: c for c in recorded}
    assert by["pck"][2] == dict(vis=None, thresholds=(2, 7.5), max_threshold=30) and "PCK@7.5" in metrics and "PCK@2" in metrics
    assert by["epe"][2] == dict(vis=None, unit=1.0, max_dist=99.0)
    del recorded[:]
    stub = _Stub(_wiring_cfg(PCK=False), 17)
    _, metrics, out = stub(_batch(stub, 17), is_train=False)
    assert list(metrics) == ["MPJPE", "EPEmean_global"] and [c[0] for c in recorded] == ["lift", "epe"] and "err_joints" not in out
    # without the ground truths nothing is computed; EPIPOLAR.MULTITEST keeps no heat maps, so no JDR
    del recorded[:]
    stub = _Stub(_wiring_cfg(), 17)
    batch = _batch(stub, 17)
    for key in ("heatmap", "points-2d", "points-3d"):
        del batch[key]
    assert stub(batch, is_train=False)[1] == {} and [c[0] for c in recorded] == ["lift"]
    del recorded[:]
    stub.cfg.merge_from_list(["EPIPOLAR.MULTITEST", True])
    _, metrics, _ = stub(_batch(stub, 17), is_train=False)
    assert "JDR" not in metrics and "PCK@1" in metrics and [c[0] for c in recorded] == ["lift", "epe", "pck"]


def test_mapping_reduces_twenty_channels_to_seventeen_before_the_lift(recorded):
    stub = _Stub(_wiring_cfg(20, mapping=True), 20)
    batch = _batch(stub, 17)                                  # points-2d / points-3d: the 17 joints
    keep = list(restate.MAPPING)
    _, metrics, out = stub(batch, is_train=False)
    by = {c[0]: c for c in recorded}
    pts, _, conf = by["lift"][1]
    assert tuple(pts.shape) == (2, 2, 17, 2) and torch.equal(conf.reshape(4, 17), stub.canned[3][:, keep])
    assert tuple(out["points-3d"].shape) == (2, 17, 3)
    heat, target = by["jdr"][1]
    assert torch.equal(heat, stub.canned[1][0][:, keep]) and heat.is_contiguous() and torch.equal(target, batch["heatmap"][:, keep])
    locs, gt2 = by["pck"][1]
    assert torch.equal(locs, stub.canned[2][:, keep]) and torch.equal(gt2, batch["points-2d"][..., :2].double())
    assert torch.equal(by["pck"][2]["vis"], batch["visibility"].view(4, 20)[:, keep].float())
    assert torch.equal(out["batch_locs"], stub.canned[2][:, keep]) and tuple(out["heatmaps"].shape) == (4, 17, 6, 5)
    # MAPPING False, or absent: nothing is reduced
    for mapping in (False, None):
        del recorded[:]
        stub = _Stub(_wiring_cfg(20, mapping=mapping), 20)
        stub(_batch(stub, 20), is_train=False)
        assert tuple(recorded[0][1][0].shape) == (2, 2, 20, 2)
    # any other head under MAPPING True is an error that names the key
    stub = _Stub(_wiring_cfg(19, mapping=True), 19)
    with pytest.raises(ValueError, match="DATASETS.H36M.MAPPING"):
        stub(_batch(stub, 19), is_train=False)
