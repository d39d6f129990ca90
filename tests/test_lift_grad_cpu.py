"""The liftings' gradient on the CPU: the library's host hook (et_debug_host_triangulate_bwd: the kernel's own per-joint routine of
csrc/et_triangulate.h in a serial loop) against the float64 yardstick of tests/lift_grad_common.py -- torch autograd through
torch.linalg.svd on the DLT rows the RESTATEMENT's info word names -- for pymvg, naive, refine, epipolar and epipolar_dlt; exact
zeros, linearity, batch independence, the ABI's argument checks, and how ops and MultiViewPoseModel.lift pass `with_grad` on.

Tolerance per joint: 2^-23 x the joint's largest reference element (lift_grad_common).  Condition on the inputs: the two float64
yardsticks agree within 2^-30 = 9.3e-10 per joint.  Each test prints its figures (pytest -s): the condition's worst is 7.7e-12 (the
views' scenes) and 4.3e-11 (the epipolar ones); the hook's worst use of the bound is 0.44 in both families -- the float32 rounding
of the store and next to nothing else."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

import lift_grad_common as common
import triangulation_epipolar_restatement as epi
import triangulation_views_restatement as views
from epipolar_transformers_amd import _lib, build, model, ops

NULL = common.NULL
fp = common.fp
CASES = [(m, V) for m in common.METHODS for V in (4, 8)]
CASE_IDS = ["%s-V%d" % c for c in CASES]


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def forward_info(lib, sc):
    """The info word of the library's own forward (host hook): what its backward is given in production."""
    out, info = np.full((sc.F, sc.J, 3), np.nan), np.full((sc.F, sc.J), -1, np.int32)
    if sc.other is None:
        rc = lib.et_debug_host_triangulate_views(sc.F, sc.V, sc.J, fp(sc.pts), fp(sc.conf), fp(sc.krt), views.METHODS.index(sc.method),
                                                 0.85, 35.0, fp(out), fp(info))
    else:
        H, W = sc.corr.shape[2:4]
        rc = lib.et_debug_host_triangulate_epipolar(sc.F, sc.V, sc.J, H, W, fp(sc.pts), fp(sc.conf), fp(sc.krt), fp(sc.other),
                                                    fp(sc.corr), 64.0, 1.0, 0.85, 35.0, int(sc.method == "epipolar_dlt"), fp(out),
                                                    fp(info))
    assert rc == 0, lib.et_last_error()
    return info


def test_the_scenes_exercise_what_they_must():
    for family, flags in ((views.METHODS, ()), (("epipolar", "epipolar_dlt"), ("branches",))):
        counts, zeros, branches, clamped = set(), 0, set(), 0
        for method in family:
            for V in (4, 8):
                info = common.scene(method, V).info
                used = info >> 8 & 0xff
                counts |= {bin(int(u)).count("1") for u in used.ravel()}
                zeros += int(((used == 0) & (info & views.INFO_ZEROS != 0)).sum())
                branches |= set((info >> 16 & 3).ravel().tolist()) if flags else {0}
                clamped += int((info & epi.INFO_CLAMPED != 0).sum()) if flags else 0
        # solved joints, two-view and many-view solves
        assert 2 in counts and max(counts) >= 4, (family, counts)
        if flags:
            # (every joint of the epipolar scenes has a point: 35 mm admits an inlier everywhere)
            assert branches == {0, 1, 2} and clamped > 0 and 1 in counts
        else:
            assert zeros > 0 and 0 in counts         # flagged-zero joints: the views' scenes hold them


@pytest.mark.parametrize("method,V", CASES, ids=CASE_IDS)
def test_the_two_float64_yardsticks_agree(method, V):
    sc = common.scene(method, V)
    for k in range(2):
        worst = common.condition(sc, k)
        print("    %-12s V=%d grad_out %d: the yardsticks disagree by %.3e of a joint's largest element at the most" % (method, V, k, worst))
        assert worst <= common.CONDITION


@pytest.mark.parametrize("method,V", CASES, ids=CASE_IDS)
def test_host_hook_against_the_yardstick(lib, method, V):
    sc = common.scene(method, V)
    info = forward_info(lib, sc)
    assert np.array_equal(info, sc.info)                  # the library decides as the restatement does
    for k, gout in enumerate(common.grad_outs(sc.F, sc.J)):
        got = common.host_bwd(lib, sc, info, gout)
        assert np.isfinite(got).all()                     # every element written: the buffer started as NaN
        want = sc.reference(k)[0]
        ok, worst = common.use_of_bound(got, want)
        print("    %-12s V=%d grad_out %d: worst use of the bound %.3f" % (method, V, k, worst))
        assert ok, (method, V, k, worst)
        assert np.abs(want).max() > 0


@pytest.mark.parametrize("method,V", CASES, ids=CASE_IDS)
def test_flagged_joints_and_unused_views_are_exactly_zero(lib, method, V):
    sc = common.scene(method, V)
    got = common.host_bwd(lib, sc, sc.info, common.grad_outs(sc.F, sc.J)[1])
    used = sc.info >> 8 & 0xff
    seen = [0, 0]
    for f in range(sc.F):
        for j in range(sc.J):
            for v in range(V):
                if not used[f, j] >> v & 1:
                    assert (got[f, v, j] == 0).all() and not np.signbit(got[f, v, j]).any()
                    seen[0] += 1
                else:
                    assert (got[f, v, j] != 0).any()
                    seen[1] += 1
    assert seen[0] > 0 and seen[1] > 0


def test_one_view_gives_all_zeros(lib):
    full = common.scene("pymvg", 4)
    one = common.Scene(tuple(np.ascontiguousarray(a[:, :1]) for a in full.arrays), "pymvg")
    assert (one.info & views.INFO_ZEROS).all() and (one.info >> 8 & 0xff == 0).all()
    got = common.host_bwd(lib, one, forward_info(lib, one), common.grad_outs(one.F, one.J)[1])
    assert (got == 0).all()
    # a word that names the one view without branch bits is no DLT either (two rows): zeros, nothing divided by nothing
    got = common.host_bwd(lib, one, np.full_like(one.info, 1 | 1 << 8), common.grad_outs(one.F, one.J)[1])
    assert (got == 0).all()


@pytest.mark.parametrize("V", [4, 8])
def test_branch_bits_without_the_correspondences_give_zeros(lib, V):
    """An info word of the epipolar method handed to the backward of the views (NULL other_krt / corr_pos): the single-view
    branches are not followed -- zeros for those joints, the plain DLT for the others, no crash."""
    sc = common.scene("epipolar", V)
    gout = common.grad_outs(sc.F, sc.J)[1]
    got, full = common.host_bwd(lib, sc, sc.info, gout, other=None), common.host_bwd(lib, sc, sc.info, gout)
    single = (sc.info >> 16 & 3) != 0
    assert single.any() and not single.all() and np.isfinite(got).all()
    for f in range(sc.F):
        for j in range(sc.J):
            if single[f, j]:
                assert (got[f, :, j] == 0).all() and (full[f, :, j] != 0).any()
            else:
                assert same_bits(got[f, :, j], full[f, :, j])


@pytest.mark.parametrize("method,V", [("refine", 8), ("epipolar", 4)])
def test_doubled_grad_out_gives_doubled_bits(lib, method, V):
    sc = common.scene(method, V)
    gout = common.grad_outs(sc.F, sc.J)[1]
    once, twice = common.host_bwd(lib, sc, sc.info, gout), common.host_bwd(lib, sc, sc.info, 2.0 * gout)
    assert same_bits(once * np.float32(2), twice) and np.isfinite(twice).all()


@pytest.mark.parametrize("method,V", [("naive", 4), ("epipolar_dlt", 8)])
def test_a_frame_alone_gives_the_bits_it_has_in_the_batch(lib, method, V):
    sc = common.scene(method, V)
    gout = common.grad_outs(sc.F, sc.J)[1]
    batch = common.host_bwd(lib, sc, sc.info, gout)
    for f in range(sc.F):
        alone = common.Scene(tuple(np.ascontiguousarray(a[f:f + 1]) for a in sc.arrays), method)
        assert np.array_equal(alone.info, sc.info[f:f + 1])
        assert same_bits(common.host_bwd(lib, alone, alone.info, gout[f:f + 1])[0], batch[f])


def test_header_ctypes_and_exports_agree_and_bad_arguments_are_errors(lib):
    text = open(os.path.join(ROOT, "include", "epipolar_amd.h")).read()
    for name in ("et_triangulate_bwd", "et_debug_host_triangulate_bwd"):
        assert ("int %s(" % name) in text and name in _lib.exported_symbols() and hasattr(lib, name)
        assert ("`%s`" % name) in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert lib.et_abi_version() == 14 and _lib.ET_ABI_VERSION == 14      # additive: the version stays
    sc = common.Scene(epi.random_scene(1, 4, 2, seed=1)[0], "epipolar")
    gout, grad = np.ones((1, 2, 3)), np.zeros((1, 4, 2, 2), np.float32)
    err = lambda: lib.et_last_error()
    # (the device entry point reports these before any launch: no GPU is touched)
    for entry, extra in ((lib.et_debug_host_triangulate_bwd, ()), (lib.et_triangulate_bwd, (NULL,))):
        def bad(F=1, V=4, J=2, H=16, W=16, pts=fp(sc.pts), krt=fp(sc.krt), okrt=fp(sc.other), corr=fp(sc.corr), ds=64.0, resize=1.0,
                info=fp(sc.info), go=fp(gout), gp=fp(grad)):
            return entry(F, V, J, H, W, pts, krt, okrt, corr, ds, resize, info, go, gp, *extra) != 0
        assert bad(V=9) and b"V=9" in err()
        assert bad(V=0) and b"V=0" in err()
        assert bad(J=0) and b"bad sizes" in err()
        assert bad(F=0) and b"bad sizes" in err()
        for k in ("pts", "krt", "info", "go", "gp"):
            assert bad(**{k: NULL}) and b"NULL" in err(), k
        assert bad(okrt=NULL) and b"both" in err()
        assert bad(corr=NULL) and b"both" in err()
        assert bad(H=0) and b"map size" in err()
        assert bad(ds=0.0) and b"downsample" in err()
        assert bad(resize=float("nan")) and b"downsample" in err()
        if not extra:                                       # (valid arguments: only the host hook can run here)
            assert not bad()
            assert not bad(okrt=NULL, corr=NULL, H=0, W=0, ds=0.0, resize=0.0)     # the views' backward reads none of them


def test_ops_wrappers_reject_cpu_tensors_with_and_without_with_grad():
    arrays = [torch.from_numpy(a) for a in common.scene("epipolar", 4).arrays]
    for with_grad in (False, True):
        pts = arrays[0].clone().requires_grad_(with_grad)
        with pytest.raises(_lib.EpipolarAmdError):
            ops.triangulate_views(pts, arrays[1], arrays[2], method="pymvg", conf_thres=0.85, with_grad=with_grad)
        with pytest.raises(_lib.EpipolarAmdError):
            ops.triangulate_epipolar(pts, *arrays[1:], with_grad=with_grad, **common.EPIPOLAR_KW)


def _lift_cfg(method, **over):
    from epipolar_transformers_amd import default_cfg

    cfg = default_cfg()
    cfg.merge_from_list(["KEYPOINT.TRIANGULATION", method, "KEYPOINT.CONF_THRES", 0.85, "KEYPOINT.RANSAC_THRES", 35,
                         "DATASETS.IMAGE_RESIZE", 2.0, "DATASETS.PREDICT_RESIZE", 1.0, "BACKBONE.DOWNSAMPLE", 4])
    for k, v in over.items():
        cfg.merge_from_list([k, v])
    return cfg


def test_lift_passes_with_grad_exactly_when_peak_grad_is_set(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "triangulate_views", lambda *a, **k: calls.append(("views", a, k)) or "V")
    monkeypatch.setattr(ops, "triangulate_epipolar", lambda *a, **k: calls.append(("epipolar", a, k)) or "E")
    monkeypatch.setattr(model, "triangulate_dlt", lambda *a, **k: calls.append(("dlt", a, k)) or "D")
    F, V, J = 2, 4, 5
    locs, scos = torch.rand(F * V, J, 2), torch.rand(F * V, J)
    KRT, other, corr = torch.rand(F * V, 3, 4), torch.rand(F * V, 3, 4), torch.rand(F * V, 8, 8, 2)
    lift = lambda cfg: model.MultiViewPoseModel.lift(types.SimpleNamespace(cfg=cfg), locs, scos, KRT, V, corr, other)
    views_kw = lambda m: dict(method=m, conf_thres=0.85, ransac_thres=35.0)
    epi_kw = lambda m: dict(downsample=4.0, resize=2.0, conf_thres=0.85, ransac_thres=35.0, dlt=m == "epipolar_dlt")
    for peak_grad in (False, True):
        extra = {"with_grad": True} if peak_grad else {}             # off: today's keyword sets, no `with_grad` at all
        for method in views.METHODS:
            del calls[:]
            assert lift(_lift_cfg(method, **{"EPIPOLAR_AMD.LIFT_KERNELS": True, "EPIPOLAR_AMD.PEAK_GRAD": peak_grad})) == "V"
            (kind, a, k), = calls
            assert kind == "views" and k == dict(views_kw(method), **extra)
        for method in ("epipolar", "epipolar_dlt"):
            del calls[:]
            assert lift(_lift_cfg(method, **{"EPIPOLAR_AMD.PEAK_GRAD": peak_grad})) == "E"
            (kind, a, k), = calls
            assert kind == "epipolar" and k == dict(epi_kw(method), **extra)
        # the torch DLT takes no keyword of this kind: autograd follows it by itself
        del calls[:]
        assert lift(_lift_cfg("pymvg", **{"EPIPOLAR_AMD.PEAK_GRAD": peak_grad})) == "D"
        assert calls[0][2] == dict(conf_thres=0.85)
