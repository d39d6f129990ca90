"""KEYPOINT.TRIANGULATION rpsm on the CPU: the NumPy restatement (tests/rpsm_restatement.py) and the library's host hook
(et_debug_host_rpsm: the kernels' own per-frame pieces in a serial loop) against what the reference's `rpsm` returned
(tests/golden/lifting/rpsm.npz, made by tests/golden/make_rpsm_golden.py), the hook against the restatement on random scenes, the
ABI's limits, pictorial.crop_transform, and the dispatch of MultiViewPoseModel.lift.

TOLERANCE_MM: with identical bins the poses differ only by the float32 rounding of grid positions; the fixture maker measured
8.53e-05 mm (restatement) and 3.05e-05 mm (host hook) against the reference over all cases, and the tests use 4 x the larger."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

import rpsm_restatement as restate
from epipolar_transformers_amd import _lib, build, model, ops, pictorial

TOLERANCE_MM = 3.42e-4
CASES = ["four_views_clean", "three_views_shifted_crop", "non_square_map", "first_nbins_6", "first_nbins_16",
         "first_limb_length_differs", "recur_nbins_3", "zero_heatmap_joint"]


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "lifting", "rpsm.npz"))


_RESTATED = {}


def case(golden, name):
    """(stacked one-frame scene, params, X_ref, the restatement's (pose, path, margins, band)) -- restated once per case."""
    g = lambda k: golden["%s.%s" % (name, k)]
    sc = {k: np.ascontiguousarray(g(k)[None]).astype(np.float32) for k in restate.ARRAYS}
    if "%s.first_limb_length" % name in golden.files:
        sc["first_limb_length"] = np.ascontiguousarray(g("first_limb_length")[None])
    params = dict(image_size=tuple(int(t) for t in g("image_size")), grid_size=int(g("grid_size")), first_nbins=int(g("first_nbins")),
                  recur_nbins=int(g("recur_nbins")), recur_depth=int(g("recur_depth")), tolerance=int(g("tolerance")))
    if name not in _RESTATED:
        _RESTATED[name] = restate.run(sc, params)
    return sc, params, g("X_ref"), _RESTATED[name]


def host_hook(lib, sc, params, parent=None):
    F, V, J, H, W = sc["heat"].shape
    out = np.full((F, J, 3), np.nan, np.float32)
    path = np.full((F, 1 + params["recur_depth"], J), -1, np.int32)
    fp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    parent = np.array(restate.H36M_PARENT[:J] if parent is None else parent, np.int32)
    rc = lib.et_debug_host_rpsm(F, V, J, H, W, fp(sc["heat"]), fp(sc["cams"]), fp(sc["trans"]), fp(sc["center"]), fp(sc["limb_length"]),
                                fp(sc.get("first_limb_length")), fp(parent), params["image_size"][0], params["image_size"][1],
                                params["grid_size"], params["first_nbins"], params["recur_nbins"], params["recur_depth"],
                                params["tolerance"], int(params.get("align_corners", False)), fp(out), fp(path))
    assert rc == 0, lib.et_last_error()
    return out, path


def test_fixture_holds_every_case_and_the_condition(golden):
    assert sorted({k.split(".")[0] for k in golden.files}) == sorted(CASES)
    seen = set()
    for name in CASES:
        sc, params, ref, (pose, path, margins, band) = case(golden, name)
        assert sc["heat"].shape[2] == 17 and max(sc["heat"].shape[3:]) <= 32 and params["recur_depth"] == 4
        assert restate.condition_holds(margins, band), (name, margins.min(), band.min())      # the maker's condition on the inputs
        seen |= {("V", sc["heat"].shape[1]), ("first", params["first_nbins"]), ("recur", params["recur_nbins"]),
                 ("square", sc["heat"].shape[3] == sc["heat"].shape[4]), ("first_limb", "first_limb_length" in sc)}
    assert {("V", 3), ("V", 4), ("first", 6), ("first", 16), ("recur", 3), ("square", False), ("first_limb", True)} <= seen
    heat = golden["zero_heatmap_joint.heat"]
    assert (heat[:, 16] == 0).all() and (heat[:, 15] != 0).any()
    # the shifted crop box: part of the first grid samples outside that view's map
    sc, params, _, _ = case(golden, "three_views_shifted_crop")
    axes = np.linspace(-params["grid_size"] / 2, params["grid_size"] / 2, params["first_nbins"])[None] + sc["center"][0].astype(np.float64)[:, None]
    ix, iy = restate.sample_pixel(restate.positions(axes), sc["cams"][0, 1].astype(np.float64), sc["trans"][0, 1].astype(np.float64),
                                  params["image_size"], 24, 24)
    outside = (ix <= -1) | (ix >= 24) | (iy <= -1) | (iy >= 24)
    assert outside.any() and not outside.all()


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference(golden, name):
    sc, params, ref, (pose, path, margins, band) = case(golden, name)
    err = np.abs(pose[0] - ref).max()
    print(name, "restatement vs reference: %.3g mm" % err)
    assert err <= TOLERANCE_MM, (name, err)
    if name == "zero_heatmap_joint":        # zero energy all the way to the root: the FIRST bin wins there at every level
        assert (path[0][:, 0] == 0).all() and (path[0][:, 16] == 0).all()


@pytest.mark.parametrize("name", CASES)
def test_host_hook_matches_the_reference_and_the_restatement(lib, golden, name):
    sc, params, ref, (pose, path, margins, band) = case(golden, name)
    got, got_path = host_hook(lib, sc, params)
    err = np.abs(got[0].astype(np.float64) - ref).max()
    print(name, "host hook vs reference: %.3g mm" % err)
    assert err <= TOLERANCE_MM, (name, err)
    assert np.array_equal(got_path, path)


@pytest.mark.parametrize("V,J,first_nbins,recur_nbins,grid_size,align", [(4, 17, 8, 2, 2000, False), (2, 5, 4, 3, 900, True),
                                                                        (8, 17, 6, 2, 1200, False)])
def test_host_hook_matches_the_restatement_on_random_scenes(lib, V, J, first_nbins, recur_nbins, grid_size, align):
    params = dict(image_size=(256, 256), grid_size=grid_size, first_nbins=first_nbins, recur_nbins=recur_nbins, recur_depth=4,
                  tolerance=150.0, align_corners=align)
    sc, (pose, path, margins, band) = restate.scene(40 + V, 3, V, J, 21, 19, params, log=print)
    assert restate.condition_holds(margins, band)
    got, got_path = host_hook(lib, sc, params)
    assert np.array_equal(got_path, path)
    err = np.abs(got - pose).max()
    print("V=%d J=%d host hook vs restatement: %.3g mm" % (V, J, err))
    assert err <= TOLERANCE_MM and np.isfinite(got).all()


def test_host_hook_takes_any_tree(lib):
    """A root that is not joint 0 and children listed before their parents: the same scene, relabelled, gives the same pose."""
    params = dict(image_size=(256, 256), grid_size=900, first_nbins=4, recur_nbins=2, recur_depth=3, tolerance=150.0)
    sc, (pose, path, _, _) = restate.scene(77, 1, 3, 5, 16, 16, params)
    perm = [4, 2, 0, 3, 1]                                   # new label of old joint j
    old_parent = restate.H36M_PARENT[:5]
    new_parent = [0] * 5
    for j, p in enumerate(old_parent):
        new_parent[perm[j]] = -1 if p < 0 else perm[p]
    inv = np.argsort(perm)                                   # old joint at each new label
    relabelled = dict(sc, heat=np.ascontiguousarray(sc["heat"][:, :, inv]))
    # limb e ends at the e-th non-root joint in ascending NEW order
    ends = [j for j in range(5) if new_parent[j] >= 0]
    relabelled["limb_length"] = np.ascontiguousarray(np.stack([sc["limb_length"][:, inv[j] - 1] for j in ends], 1))
    got, got_path = host_hook(lib, relabelled, params, parent=new_parent)
    base, base_path = host_hook(lib, sc, params)
    assert np.array_equal(got[:, perm], base) and np.array_equal(got_path[:, :, perm], base_path)
    assert np.array_equal(base_path, path)


def test_header_ctypes_and_exports_agree_and_limits_are_errors(lib):
    text = open(os.path.join(ROOT, "include", "epipolar_amd.h")).read()
    for name, ret in (("et_rpsm", "int"), ("et_debug_host_rpsm", "int"), ("et_rpsm_workspace_bytes", "size_t")):
        assert ("%s %s(" % (ret, name)) in text and name in _lib.exported_symbols() and hasattr(lib, name)
    assert lib.et_abi_version() == 14 and "#define ET_ABI_VERSION 14" in text.replace("  ", " ")     # additive: the version stays
    assert lib.et_rpsm_workspace_bytes(2, 17, 16, 2) >= 3 * 2 * 17 * 4096 * 4
    params = dict(image_size=(256, 256), grid_size=300, first_nbins=2, recur_nbins=2, recur_depth=1, tolerance=150.0)
    sc, _ = restate.scene(3, 1, 2, 3, 8, 8, params)
    fp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    parent = np.array([-1, 0, 1], np.int32)
    out, path = np.zeros((1, 3, 3), np.float32), np.zeros((1, 2, 3), np.int32)
    ws = np.zeros(lib.et_rpsm_workspace_bytes(1, 3, 2, 2), np.uint8)

    def call(entry, device, F=1, V=2, J=3, H=8, W=8, ptrs=None, parent=parent, image=(256.0, 256.0), grid=300.0, first=2, recur=2,
             depth=1, tol=150.0, out=fp(out), path=fp(path), ws_ptr=fp(ws), ws_bytes=ws.size, parent_ptr=None):
        ptrs = ptrs or [fp(sc[k]) for k in restate.ARRAYS] + [null]
        tail = (ws_ptr, ws_bytes, null) if device else ()
        return entry(F, V, J, H, W, *ptrs, fp(parent) if parent_ptr is None else parent_ptr, image[0], image[1], grid, first, recur, depth, tol, 0, out, path, *tail)

    for entry, device in ((lib.et_debug_host_rpsm, False), (lib.et_rpsm, True)):
        # (the device entry point reports these before any launch: no GPU is touched)
        bad = lambda msg, **kw: call(entry, device, **kw) != 0 and msg in lib.et_last_error()
        assert bad(b"V=0", V=0) and bad(b"V=9", V=9)
        assert bad(b"J=0", J=0) and bad(b"J=33", J=33)
        assert bad(b"first_nbins=1", first=1) and bad(b"first_nbins=17", first=17)
        assert bad(b"recur_nbins=1", recur=1) and bad(b"recur_nbins=4", recur=4)
        assert bad(b"recur_depth=-1", depth=-1) and bad(b"recur_depth=17", depth=17)
        assert bad(b"bad sizes", F=0) and bad(b"bad sizes", H=0) and bad(b"bad sizes", W=0)
        assert bad(b"must be positive", image=(0.0, 256.0)) and bad(b"must be positive", grid=0.0) and bad(b"must be positive", tol=0.0)
        for tree in ([-1, -1, 0], [1, 2, 0], [-1, 0, 3], [-1, 2, 1], [-1, 1, 0]):
            assert bad(b"not a tree with one root", parent=np.array(tree, np.int32)), tree
        for k in range(5):
            ptrs = [fp(sc[n]) for n in restate.ARRAYS] + [null]
            ptrs[k] = null
            assert bad(b"NULL", ptrs=ptrs)
        assert bad(b"NULL", out=null) and bad(b"NULL", parent_ptr=null)
    assert call(lib.et_rpsm, True, ws_ptr=null) != 0 and b"NULL" in lib.et_last_error()
    assert call(lib.et_rpsm, True, ws_bytes=ws.size - 1) != 0 and b"workspace" in lib.et_last_error()
    assert call(lib.et_debug_host_rpsm, False, path=null) == 0                                   # path may be NULL


def test_crop_transform_is_the_three_point_solve():
    rng = np.random.default_rng(5)
    for image_size in ((256, 256), (320, 256), (192, 256)):
        center = rng.uniform(100, 900, (6, 2)).astype(np.float32)
        scale = rng.uniform(0.8, 4.0, (6, 1)).astype(np.float32) * np.ones((1, 2), np.float32)
        got = pictorial.crop_transform(torch.from_numpy(center), torch.from_numpy(scale), image_size)
        assert got.shape == (6, 2, 3) and got.dtype == torch.float32
        want = np.stack([restate.crop_transform_three_point(c, s, image_size) for c, s in zip(center, scale)])
        # float32 closed form against a float64 solve of float32 points: entries up to ~1e3 px, a few float32 ulps
        assert np.abs(got.numpy() - want).max() <= 4 * 2.0 ** -23 * np.abs(want).max()
        one = pictorial.crop_transform(torch.from_numpy(center), torch.from_numpy(scale[:, 0]), image_size)
        assert torch.equal(one, got)
    pose = torch.from_numpy(rng.normal(0, 300, (2, 17, 3)).astype(np.float32))
    limbs = pictorial.limb_lengths(pose)
    assert limbs.shape == (2, 16) and pictorial.H36M_PARENT == restate.H36M_PARENT
    assert torch.allclose(limbs[1, 10], (pose[1, 11] - pose[1, 8]).norm())          # limb 10 ends at joint 11 (lsho), from 8 (neck)


def _lift_cfg(method, **over):
    from epipolar_transformers_amd import default_cfg

    cfg = default_cfg()
    cfg.merge_from_list(["KEYPOINT.TRIANGULATION", method, "KEYPOINT.CONF_THRES", 0.85, "DATASETS.IMAGE_RESIZE", 2.0,
                         "DATASETS.PREDICT_RESIZE", 1.0, "BACKBONE.DOWNSAMPLE", 4])
    for k, v in over.items():
        cfg.merge_from_list([k, v])
    return cfg


def test_config_defaults_are_the_references():
    from epipolar_transformers_amd import default_cfg

    cfg = default_cfg()
    ps = cfg.PICT_STRUCT
    assert (ps.FIRST_NBINS, ps.RECUR_NBINS, ps.RECUR_DEPTH, ps.LIMB_LENGTH_TOLERANCE, ps.GRID_SIZE) == (16, 2, 10, 150, 2000)
    assert cfg.KEYPOINT.ROOTIDX == 0


def test_lift_dispatches_rpsm(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "rpsm", lambda *a, **k: calls.append(("rpsm", a, k)) or "R")
    monkeypatch.setattr(model, "triangulate_dlt", lambda *a, **k: calls.append(("dlt", a, k)) or "D")
    F, V, J = 2, 4, 17
    locs, scos = torch.rand(F * V, J, 2), torch.rand(F * V, J)
    KRT = torch.rand(F * V, 3, 4)
    heat = torch.rand(F * V, J, 6, 5)
    extra = dict(cameras=torch.rand(F * V, 3, 4), crop_center=torch.rand(F * V, 2) * 500, crop_scale=torch.rand(F * V, 2) + 1,
                 center=torch.rand(F, 3), limb_length=torch.rand(F, J - 1), first_limb_length=torch.rand(J - 1))
    lift = lambda cfg, **kw: model.MultiViewPoseModel.lift(types.SimpleNamespace(cfg=cfg), locs, scos, KRT, V, **kw)
    cfg = _lift_cfg("rpsm", **{"PICT_STRUCT.FIRST_NBINS": 12, "PICT_STRUCT.RECUR_DEPTH": 7, "PICT_STRUCT.GRID_SIZE": 1800,
                               "DATASETS.IMAGE_SIZE": (320, 256)})
    assert lift(cfg, rpsm=extra, heatmaps=heat) == "R"
    (kind, a, k), = calls
    assert kind == "rpsm"
    first = k.pop("first_limb_length")
    assert k == dict(parent=None, image_size=(320, 256), grid_size=1800.0, first_nbins=12, recur_nbins=2, recur_depth=7,
                     tolerance=150.0, align_corners=False)
    hm, cams, trans, center, limb = a
    assert torch.equal(hm, heat.view(F, V, J, 6, 5)) and torch.equal(cams, extra["cameras"].view(F, V, 3, 4))
    assert torch.equal(trans, pictorial.crop_transform(extra["crop_center"], extra["crop_scale"], (320, 256)).view(F, V, 2, 3))
    assert torch.equal(center, extra["center"]) and torch.equal(limb, extra["limb_length"])
    assert torch.equal(first, extra["first_limb_length"])
    # EPIPOLAR.MULTITEST keeps no heat maps: an error that says so, not another method
    with pytest.raises(ValueError, match="MULTITEST"):
        lift(cfg, rpsm=extra)
    # without the dict: today's path, the thresholded DLT with today's arguments -- for rpsm and for every other method
    for method, kw in (("rpsm", {}), ("rpsm", dict(heatmaps=heat)), ("pymvg", dict(rpsm=extra, heatmaps=heat))):
        del calls[:]
        assert lift(_lift_cfg(method), **kw) == "D"
        (kind, a, k), = calls
        assert kind == "dlt" and k == dict(conf_thres=0.85) and torch.equal(a[0], (locs * 2.0).view(F, V, J, 2))
        assert torch.equal(a[1], KRT.view(F, V, 3, 4)) and torch.equal(a[2], scos.view(F, V, J))


def test_ops_wrapper_rejects_cpu_tensors():
    params = dict(image_size=(256, 256), grid_size=300, first_nbins=2, recur_nbins=2, recur_depth=1, tolerance=150.0)
    sc, _ = restate.scene(3, 1, 2, 3, 8, 8, params)
    with pytest.raises(_lib.EpipolarAmdError):
        ops.rpsm(*[torch.from_numpy(sc[k]) for k in restate.ARRAYS], parent=restate.H36M_PARENT[:3], **params)
