"""KEYPOINT.TRIANGULATION pymvg / naive / refine on the CPU: the NumPy restatement and the library's host hook
(et_debug_host_triangulate_views: the kernels' own per-joint routine in a serial loop) against what the reference's
`triangulate_pymvg`, `triangulate` and `triangulate_refine` returned (tests/golden/triangulation.npz, made by
make_triangulation_golden.py; tests/golden/lifting/triangulation_ransac.npz, made by make_triangulation_ransac_golden.py), the hook
against the restatement on random scenes, the ABI's argument checks, and the dispatch of MultiViewPoseModel.lift under
EPIPOLAR_AMD.LIFT_KERNELS.  Every comparison of points uses the project's rule for reference-frozen triangulation
(`within_tolerance`)."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

import triangulation_views_restatement as restate
from test_triangulate_epipolar_cpu import _lift_cfg, within_tolerance
from epipolar_transformers_amd import _lib, build, model, ops

PYMVG_CASES = ["all_scores_tiny", "all_views_default_thres", "eight_views", "thres085_drops_low_views",
               "thres085_lowered_until_two_views", "thres_boundary_float32"]
RANSAC_CASES = ["all_confident_clean_first_pair_wins", "confident_outlier_rejected", "two_of_four_wrong",
                "tiny_ransac_thres_no_inlier", "one_confident_view_zeros", "eight_views_mixed"]
METHOD_ID = {"pymvg": 0, "naive": 1, "refine": 2}
RANDOM_KW = dict(conf_thres=0.85, ransac_thres=35.0)


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


@pytest.fixture(scope="module")
def pymvg_golden():
    return np.load(os.path.join(GOLDEN_DIR, "triangulation.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def ransac_golden():
    return np.load(os.path.join(GOLDEN_DIR, "lifting", "triangulation_ransac.npz"), allow_pickle=False)


def pymvg_case(golden, name):
    """(pts, conf, krt) with a frame axis, the threshold, and the case's getter; krt = float32 of the float64 K @ RT."""
    g = lambda k: golden["%s.%s" % (name, k)]
    krt = (g("K").astype(np.float64) @ g("RT").astype(np.float64)).astype(np.float32)
    return [np.ascontiguousarray(a[None]) for a in (g("pts"), g("conf"), krt)], float(g("thres")), g


def ransac_case(golden, name):
    g = lambda k: golden["%s.%s" % (name, k)]
    arrays = [np.ascontiguousarray(g(k)[None]) for k in ("pts", "conf", "KRT")]
    return arrays, dict(conf_thres=float(g("conf_thres")), ransac_thres=float(g("ransac_thres"))), g


def host_hook(lib, arrays, *, method, conf_thres, ransac_thres=3.0):
    pts, conf, krt = arrays
    F, V, J, _ = pts.shape
    out = np.full((F, J, 3), np.nan)
    info = np.full((F, J), -1, np.int32)
    fp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.et_debug_host_triangulate_views(F, V, J, fp(pts), fp(conf), fp(krt), METHOD_ID[method], conf_thres, ransac_thres,
                                             fp(out), fp(info))
    assert rc == 0, lib.et_last_error()
    return out, info


def check_ransac_expectations(name, method, X, info, g, pymvg_X):
    """The named expectations of the RANSAC fixture, for whichever implementation produced X (1,J,3) and info (1,J)."""
    if name == "all_confident_clean_first_pair_wins" and method == "naive":
        assert ((info >> 8 & 0xff) == 0b0011).all()           # every pair ties: the first wins
    if name in ("tiny_ransac_thres_no_inlier", "one_confident_view_zeros"):
        assert (X == 0).all() and (info & restate.INFO_ZEROS).all() and ((info >> 8 & 0xff) == 0).all()
    if name == "confident_outlier_rejected" and method == "refine":
        assert np.linalg.norm(X[0] - g("X_true"), axis=1).max() < 20          # mm
        assert np.linalg.norm(pymvg_X[0] - g("X_true"), axis=1).max() > 20    # the DLT over all views cannot reject it


def test_fixtures_hold_every_case(pymvg_golden, ransac_golden):
    assert sorted({k.split(".")[0] for k in pymvg_golden.files}) == sorted(PYMVG_CASES)
    assert sorted({k.split(".")[0] for k in ransac_golden.files}) == sorted(RANSAC_CASES)
    for name in RANSAC_CASES:
        arrays, kw, g = ransac_case(ransac_golden, name)
        assert g("pts").shape == (8 if name == "eight_views_mixed" else 4, 7, 2)
        for method in ("naive", "refine"):
            assert restate.triangulate_views(*arrays, method=method, **kw)[2] >= 0.03      # the maker's condition on the inputs


@pytest.mark.parametrize("name", PYMVG_CASES)
def test_pymvg_matches_the_reference(lib, pymvg_golden, name):
    arrays, thres, g = pymvg_case(pymvg_golden, name)
    Xr, info_r, _ = restate.triangulate_views(*arrays, method="pymvg", conf_thres=thres)
    X, info = host_hook(lib, arrays, method="pymvg", conf_thres=thres)
    for who, got in (("restatement", Xr), ("host hook", X)):
        ok, worst = within_tolerance(got[0], g("X_ref"), g("X_true"))
        print(name, "%s vs reference: worst err / bound %.3g" % (who, worst))
        assert ok, (name, who, worst)
    assert np.array_equal(info, info_r)
    steps = info >> restate.STEPS_SHIFT & 0x7f
    if name == "thres085_lowered_until_two_views":
        assert (steps >= 1).all() and (steps[0, :5] == 1).all()
    if name == "thres_boundary_float32":
        assert (steps == 0).all() and not (info & 0b0100).any()       # a score == float32(threshold) is not above it
        assert ((info[0, ::2] & 0b1000) != 0).all()                   # ... and its nextafter is
    if name == "all_scores_tiny":
        # all-zero scores: 0.05 -> 0.0 (0 is not above it) -> -0.05, the threshold ends negative and every view is selected
        assert (info[0, 3] & 0xff) == 0b1111 and (info[0, 3] >> restate.STEPS_SHIFT & 0x7f) == 2
    assert not (info & restate.INFO_ZEROS).any()


@pytest.mark.parametrize("method", ["naive", "refine"])
@pytest.mark.parametrize("name", RANSAC_CASES)
def test_naive_and_refine_match_the_reference(lib, ransac_golden, name, method):
    arrays, kw, g = ransac_case(ransac_golden, name)
    Xr, info_r, _ = restate.triangulate_views(*arrays, method=method, **kw)
    X, info = host_hook(lib, arrays, method=method, **kw)
    pymvg_X, _ = host_hook(lib, arrays, method="pymvg", **kw)
    for who, got, word in (("restatement", Xr, info_r), ("host hook", X, info)):
        ok, worst = within_tolerance(got[0], g("X_ref_" + method), g("X_true"))
        print(name, method, "%s vs reference: worst err / bound %.3g" % (who, worst))
        assert ok, (name, who, worst)
        check_ransac_expectations(name, method, got, word, g, pymvg_X)
    assert np.array_equal(info, info_r)


@pytest.mark.parametrize("V", [4, 8])
def test_host_hook_matches_the_restatement_on_random_scenes(lib, V):
    arrays, truth = restate.random_scene(3, V, 17, seed=20 + V)
    for method in restate.METHODS:
        Xr, info_r, margin = restate.triangulate_views(*arrays, method=method, **RANDOM_KW)
        if method != "pymvg":
            assert margin >= 1e-6                           # no decision hangs on rounding: nothing is excluded
        X, info = host_hook(lib, arrays, method=method, **RANDOM_KW)
        assert np.array_equal(info, info_r), method         # (pymvg: the step counts too -- the same subtraction and compare)
        assert np.isfinite(X).all()
        ok, worst = within_tolerance(X, Xr, truth)
        print("V=%d %s host hook vs restatement: worst err / bound %.3g" % (V, method, worst))
        assert ok, (method, worst)
        if method == "pymvg":
            steps = set((info_r >> restate.STEPS_SHIFT & 0x7f).ravel().tolist())
            # every kind of score is there (all-zero scores: 0.85 lowered to ~0 and once more, 17 or 18 steps)
            assert 0 in steps and 1 in steps and max(steps) >= 17 and len(steps) >= 5
        else:
            assert (info_r & restate.INFO_ZEROS).any() and not (info_r & restate.INFO_ZEROS).all()


def test_pymvg_with_one_view_or_nan_scores_writes_zeros(lib):
    (pts, conf, krt), _ = restate.random_scene(2, 1, 3, seed=3)
    nan_scene, _ = restate.random_scene(1, 4, 5, seed=4)
    nan_scene[1][0, :, 0] = np.nan                          # joint 0: no view can ever be selected
    nan_scene[1][0, 1:, 1] = np.nan                         # joint 1: one view can
    for arrays, flagged in (((pts, conf, krt), np.ones((2, 3), bool)), (nan_scene, np.array([[True, True, False, False, False]]))):
        X, info = host_hook(lib, arrays, method="pymvg", conf_thres=0.85)
        Xr, info_r, _ = restate.triangulate_views(*arrays, method="pymvg", conf_thres=0.85)
        assert np.array_equal(info, info_r)
        assert np.isfinite(X).all() and np.isfinite(Xr).all()
        assert np.array_equal((info & restate.INFO_ZEROS) != 0, flagged)
        assert (X[flagged] == 0).all() and (X[~flagged] != 0).all()
        assert ((info >> restate.STEPS_SHIFT & 0x7f)[flagged] >= 37).all()      # 0.85 lowered past -1


def test_header_ctypes_and_exports_agree_and_bad_arguments_are_errors(lib):
    text = open(os.path.join(ROOT, "include", "epipolar_amd.h")).read()
    for name in ("et_triangulate_views", "et_debug_host_triangulate_views"):
        assert ("int %s(" % name) in text and name in _lib.exported_symbols() and hasattr(lib, name)
    assert lib.et_abi_version() == 14 and _lib.ET_ABI_VERSION == 14      # additive: the version stays
    arrays, _ = restate.random_scene(1, 4, 2, seed=1)
    fp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros((1, 2, 3))
    ptrs = [fp(a) for a in arrays]
    null = ctypes.c_void_p(0)
    for entry, extra in ((lib.et_debug_host_triangulate_views, ()), (lib.et_triangulate_views, (null,))):
        # (the device entry point reports these before any launch: no GPU is touched)
        bad = lambda F, V, J, p, method, thres, o: entry(F, V, J, *p, method, thres, 35.0, o, None, *extra) != 0
        assert bad(1, 9, 2, ptrs, 0, 0.85, fp(out)) and b"V=9" in lib.et_last_error()
        assert bad(1, 4, 0, ptrs, 0, 0.85, fp(out)) and b"bad sizes" in lib.et_last_error()
        assert bad(1, 4, 2, ptrs, 3, 0.85, fp(out)) and b"method" in lib.et_last_error()
        assert bad(1, 4, 2, ptrs, 0, 2.5, fp(out)) and b"conf_thres" in lib.et_last_error()
        assert bad(1, 4, 2, ptrs, 0, float("nan"), fp(out)) and b"conf_thres" in lib.et_last_error()
        for k in range(3):
            p = list(ptrs)
            p[k] = null
            assert bad(1, 4, 2, p, 0, 0.85, fp(out)) and b"NULL" in lib.et_last_error()
        assert bad(1, 4, 2, ptrs, 0, 0.85, null) and b"NULL" in lib.et_last_error()
    for method in range(3):
        assert lib.et_debug_host_triangulate_views(1, 4, 2, *ptrs, method, 2.0, 35.0, fp(out), None) == 0     # info may be NULL
        assert np.isfinite(out).all()


def test_ops_wrapper_rejects_cpu_tensors_and_unknown_methods():
    arrays, _ = restate.random_scene(1, 4, 2, seed=1)
    with pytest.raises(_lib.EpipolarAmdError):
        ops.triangulate_views(*[torch.from_numpy(a) for a in arrays], method="pymvg", conf_thres=0.85)
    with pytest.raises(ValueError, match="pymvg, naive, refine"):
        ops.triangulate_views(*[torch.from_numpy(a) for a in arrays], method="epipolar", conf_thres=0.85)


def test_lift_dispatches_on_the_knob(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "triangulate_views", lambda *a, **k: calls.append(("views", a, k)) or "V")
    monkeypatch.setattr(ops, "triangulate_epipolar", lambda *a, **k: calls.append(("epipolar", a, k)) or "E")
    monkeypatch.setattr(model, "triangulate_dlt", lambda *a, **k: calls.append(("dlt", a, k)) or "D")
    F, V, J = 2, 4, 5
    locs, scos = torch.rand(F * V, J, 2), torch.rand(F * V, J)
    KRT, other = torch.rand(F * V, 3, 4, dtype=torch.float64), torch.rand(F * V, 3, 4)
    corr = torch.rand(F * V, 8, 8, 2)
    lift = lambda cfg, *extra: model.MultiViewPoseModel.lift(types.SimpleNamespace(cfg=cfg), locs, scos, KRT, V, *extra)
    # knob off (the default): exactly today's call
    assert _lift_cfg("pymvg").EPIPOLAR_AMD.LIFT_KERNELS is False
    for method in ("pymvg", "naive"):
        del calls[:]
        assert lift(_lift_cfg(method), corr, other) == "D"
        (kind, a, k), = calls
        assert kind == "dlt" and k == dict(conf_thres=0.85) and len(a) == 3
        assert torch.equal(a[0], (locs * 2.0).view(F, V, J, 2)) and torch.equal(a[1], KRT.view(F, V, 3, 4))
        assert torch.equal(a[2], scos.view(F, V, J))
    # knob on: the three methods go to their kernels, with and without corr_pos (EPIPOLAR.MULTITEST keeps none)
    on = {"EPIPOLAR_AMD.LIFT_KERNELS": True}
    for method, want in (("pymvg", "pymvg"), ("naive", "naive"), ("refine", "refine"), ("rpsm", "pymvg")):
        for extra in ((corr, other), ()):
            del calls[:]
            assert lift(_lift_cfg(method, **on), *extra) == "V"
            (kind, a, k), = calls
            assert kind == "views" and k == dict(method=want, conf_thres=0.85, ransac_thres=35.0)
            pts, conf, krt = a
            assert torch.equal(pts, (locs * 2.0).view(F, V, J, 2)) and pts.is_contiguous()
            assert torch.equal(conf, scos.view(F, V, J)) and conf.is_contiguous()
            assert krt.dtype == torch.float32 and tuple(krt.shape) == (F, V, 3, 4) and krt.is_contiguous()
            assert torch.equal(krt, KRT.float().view(F, V, 3, 4))
    # the epipolar methods are untouched by the knob
    del calls[:]
    assert lift(_lift_cfg("epipolar", **on), corr, other) == "E" and calls[0][0] == "epipolar"
    # RANSAC_THRES is read as the epipolar branch reads it: absent -> the reference's default
    del calls[:]
    cfg = _lift_cfg("naive", **on)
    del cfg.KEYPOINT["RANSAC_THRES"]
    lift(cfg)
    assert calls[0][2]["ransac_thres"] == 3.0
    # a YAML that leaves the key at the reference's default runs the reference's default method
    del calls[:]
    cfg = _lift_cfg("naive", **on)
    del cfg.KEYPOINT["TRIANGULATION"]
    lift(cfg)
    assert calls[0][2]["method"] == "naive"
    # an unknown name is an error that lists the valid ones, with the knob on
    del calls[:]
    with pytest.raises(ValueError, match="epipolar, epipolar_dlt, rpsm, pymvg, naive, refine"):
        lift(_lift_cfg("ransac", **on))
    assert not calls
