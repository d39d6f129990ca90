"""The peak finder's gradient on the CPU: the library's host hook (et_debug_host_heatmap_peaks_bwd: the kernel's own per-cell routine
of csrc/et_peaks.h in a serial loop, the window's sums in the kernel's order) against what autograd through the reference's
find_tensor_peak_batch returned (tests/golden/lifting/peaks_grad.npz, made by tests/golden/make_peaks_grad_golden.py on the maps of
peaks.npz), the legacy division against the float64 autograd of the product's torch route, the non-finite maps, two structural
properties, and the ABI's argument checks.

The tolerance of a map is peaks_grad_common.bounds(): max(4 x ref_grad_err, 2^-20) x max |f64_grad|, ref_grad_err being the
REFERENCE's own distance from float64 on that map as the fixture records it -- never a figure of the code under test.  Each test
prints its figures (pytest -s): the hook's worst use of a bound is 0.72 (24 x 40, radius 3, downsample 8, corner00), legacy 0.52."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

import peaks_grad_common as common
import peaks_restatement as restate
from epipolar_transformers_amd import _lib, build
from oracle import ref_harness

NULL = ctypes.c_void_p(0)
RUN_IDS = [restate.run_name(*r) for r in restate.RUNS]
KINDS = restate.MAP_KINDS
NONFINITE_KINDS = ("nan_far", "nan_cell0", "all_nan", "plus_inf")
FIXTURE = os.path.join(GOLDEN_DIR, "lifting", "peaks_grad.npz")
same_bits = restate.same_bits


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "lifting", "peaks.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def grads():
    return np.load(FIXTURE, allow_pickle=False)


def fp(a):
    return NULL if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.skipif(not ref_harness.reference_available(), reason="the reference tree is not on this machine")
def test_fixture_regenerates_bit_for_bit():
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_peaks_grad_golden.py"), "--check"],
                          capture_output=True, text=True)
    assert done.returncode == 0 and "regenerated bit for bit" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


def test_fixture_holds_every_run_and_the_makers_conditions(golden, grads):
    want = set(RUN_IDS) | {"nonfinite_" + c for c in restate.NONFINITE_CASES}
    assert {k.rsplit(".", 1)[0] for k in grads.files} == want
    assert os.path.getsize(FIXTURE) < 1 << 20
    largest = 0.0
    for run in restate.RUNS:
        maps, radius, g = common.run_of(golden, grads, run)
        n = len(KINDS)
        assert g("g_locs").shape == (n, 2) and g("g_scores").shape == (n,) and g("g_locs").dtype == g("g_scores").dtype == np.float32
        for k, dt in (("ref_grad", np.float32), ("f64_grad", np.float64), ("ref_grad_locs", np.float32), ("ref_grad_scores", np.float32)):
            assert g(k).shape == maps.shape and g(k).dtype == dt and np.isfinite(g(k)).all()
        err = g("ref_grad_err")
        assert same_bits(err, common.worst(g("ref_grad"), g("f64_grad")) / np.abs(g("f64_grad")).reshape(n, -1).max(1))
        assert (err < 1e-2).all() and (err >= 1e-4).sum() <= 1
        largest = max(largest, float(np.sort(err)[-2]))
    assert largest < 1e-4
    for case in restate.NONFINITE_CASES:
        assert grads["nonfinite_%s.ref_grad" % case].shape == golden["nonfinite_%s.heat" % case][:4].shape


@pytest.mark.parametrize("run", restate.RUNS, ids=RUN_IDS)
def test_host_hook_within_the_references_own_error_of_float64(lib, golden, grads, run):
    maps, radius, g = common.run_of(golden, grads, run)
    _, downsample, threshold = run
    tol = common.bounds(g("ref_grad_err"), g("f64_grad"))
    both = common.host_bwd(lib, maps, radius, downsample, threshold, False, g("g_locs"), g("g_scores"))
    assert np.isfinite(both).all()                                       # every element written: the buffer started as NaN
    for name, want in (("reference", g("ref_grad")), ("float64", g("f64_grad"))):
        err = common.worst(both, want)
        k = int((err / tol).argmax())
        print("    %-24s against %-9s worst use of a bound %.3f (%s: %.3e of %.3e)" % (restate.run_name(*run), name, err[k] / tol[k], KINDS[k], err[k], tol[k]))
        assert (err <= tol).all(), (name, KINDS[k], err[k], tol[k])
    # the two NULL-pointer forms
    only_locs = common.host_bwd(lib, maps, radius, downsample, threshold, False, g("g_locs"), None)
    err = common.worst(only_locs, g("ref_grad_locs"))
    assert (err <= tol).all(), (KINDS[int((err / tol).argmax())], err.max())
    only_scores = common.host_bwd(lib, maps, radius, downsample, threshold, False, None, g("g_scores"))
    assert same_bits(only_scores, g("ref_grad_scores"))                 # one cell per map holds g_scores: nothing is rounded
    # ... and they add up to the whole: the arg-max cell is the only one both reach
    index = golden["%s.index" % restate.run_name(*run)]
    for m, i in enumerate(index):
        rest = np.ones(maps[m].size, bool)
        rest[i] = False
        assert same_bits(both[m].reshape(-1)[rest], only_locs[m].reshape(-1)[rest])
        assert both[m].reshape(-1)[i] == only_locs[m].reshape(-1)[i] + g("g_scores")[m]


@pytest.mark.parametrize("run", restate.RUNS, ids=RUN_IDS)
def test_legacy_division_against_the_float64_autograd_of_the_torch_route(lib, golden, grads, run):
    """Legacy floor division cannot be run through the reference under this torch: the expectation is the float64 autograd of
    backbones.soft_argmax_peaks(legacy_floor_division=True) -- after the non-legacy float64 form of that function has been pinned
    to the fixture's f64_grad: both are float64 runs of the same torch operations on the same values, so they may differ by float64
    rounding in another order at the most, 2^-40 of the largest element with room to spare."""
    maps, radius, g = common.run_of(golden, grads, run)
    _, downsample, threshold = run
    plain = common.torch_grad(maps, radius, downsample, threshold, False, g("g_locs"), g("g_scores"))
    size = np.abs(g("f64_grad")).reshape(len(maps), -1).max(1)
    pin = common.worst(plain, g("f64_grad")) / size
    print("    %-24s torch route, float64, against f64_grad: %.3e of the largest element" % (restate.run_name(*run), pin.max()))
    assert (pin <= 2.0 ** -40).all()
    want = common.torch_grad(maps, radius, downsample, threshold, True, g("g_locs"), g("g_scores"))
    tol = common.legacy_bounds(maps, radius, downsample, threshold, g("g_locs"), g("g_scores"), want)
    got = common.host_bwd(lib, maps, radius, downsample, threshold, True, g("g_locs"), g("g_scores"))
    err = common.worst(got, want)
    k = int((err / tol).argmax())
    print("    %-24s legacy: worst use of a bound %.3f (%s: %.3e of %.3e)" % (restate.run_name(*run), err[k] / tol[k], KINDS[k], err[k], tol[k]))
    assert np.isfinite(got).all() and (err <= tol).all(), (KINDS[k], err[k], tol[k])


@pytest.mark.parametrize("case", restate.NONFINITE_CASES)
def test_host_hook_on_the_nonfinite_maps(lib, golden, grads, case):
    """The gradient of locs.sum() + scores.sum() on nan_far, nan_cell0, all_nan and plus_inf: NaN exactly where the reference's is
    (the window's footprint), and on the finite cells -- all of them 0 in the reference, so the bound is 0 -- the same values."""
    H, W, radius = restate.CASES[case]
    maps, want = golden["nonfinite_%s.heat" % case][:4], grads["nonfinite_%s.ref_grad" % case]
    ones = np.ones((4, 2), np.float32)
    got = common.host_bwd(lib, maps, radius, 4.0, 1e-6, False, ones, ones[:, 0].copy())
    index = restate.peaks(maps, radius, 4.0, 1e-6)[2]
    for k, kind in enumerate(NONFINITE_KINDS):
        nan = np.isnan(want[k])
        print("    %s %-10s NaN cells %d of %d" % (case, kind, nan.sum(), H * W))
        assert np.array_equal(nan, common.footprint_mask(H, W, int(index[k]), radius)) and not np.isinf(got[k]).any()
        assert np.array_equal(np.isnan(got[k]), nan), kind
        assert (want[k][~nan] == 0).all() and (got[k][~nan] == 0).all()
    # scores alone: the window is not visited, so the one-hot gradient stays finite, as the reference's
    alone = common.host_bwd(lib, maps, radius, 4.0, 1e-6, False, None, ones[:, 0].copy())
    for k in range(4):
        hot = np.zeros(H * W, np.float32)
        hot[index[k]] = 1
        assert same_bits(alone[k].reshape(-1), hot)


@pytest.mark.parametrize("run", restate.RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("legacy", [False, True])
def test_nothing_outside_the_footprint_and_the_score_lands_on_the_first_maximum(lib, golden, grads, run, legacy):
    maps, radius, g = common.run_of(golden, grads, run)
    case, downsample, threshold = run
    H, W, _ = restate.CASES[case]
    index = golden["%s.index" % restate.run_name(*run)]
    got = common.host_bwd(lib, maps, radius, downsample, threshold, legacy, g("g_locs"), g("g_scores"))
    for m, i in enumerate(index):
        allowed = common.footprint_mask(H, W, int(i), radius, legacy)
        allowed.reshape(-1)[i] = True
        assert (got[m][~allowed] == 0).all(), KINDS[m]
    # the score's gradient alone: one cell, the forward's index -- the FIRST of the planted equal maxima
    alone = common.host_bwd(lib, maps, radius, downsample, threshold, legacy, None, g("g_scores"))
    spread, strided = restate.tie_indices(H, W)
    for kind, first in (("ties_spread", spread[0]), ("ties_strided", strided[0]), ("constant", 0)):
        m = KINDS.index(kind)
        hot = np.zeros(H * W, np.float32)
        hot[first] = g("g_scores")[m]
        assert index[m] == first and same_bits(alone[m].reshape(-1), hot), kind


def test_header_ctypes_and_exports_agree_and_bad_arguments_are_errors(lib):
    text = open(os.path.join(ROOT, "include", "epipolar_amd.h")).read()
    for name in ("et_heatmap_peaks_bwd", "et_debug_host_heatmap_peaks_bwd"):
        assert ("int %s(" % name) in text and name in _lib.exported_symbols() and hasattr(lib, name)
        assert ("`%s`" % name) in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert lib.et_abi_version() == 14 and _lib.ET_ABI_VERSION == 14      # additive: the version stays
    err = lambda: lib.et_last_error()
    maps, gl, gs, out = np.zeros((1, 4, 4), np.float32), np.zeros((1, 2), np.float32), np.zeros(1, np.float32), np.zeros((1, 4, 4), np.float32)
    # (the device entry point reports these before any launch: no GPU is touched)
    for entry, extra in ((lib.et_debug_host_heatmap_peaks_bwd, ()), (lib.et_heatmap_peaks_bwd, (NULL,))):
        bad = lambda n=1, h=4, w=4, r=2.0, m=fp(maps), l=fp(gl), s=fp(gs), o=fp(out): entry(n, h, w, m, r, 4.0, 1e-6, 0, l, s, o, *extra) != 0
        assert bad(h=1) and b"bad sizes" in err()
        assert bad(w=1) and b"bad sizes" in err()
        assert bad(n=0) and b"bad sizes" in err()
        assert bad(n=1 << 31) and b"bad sizes" in err()
        for r in (0.0, -1.0, float("nan"), 0.49, float("inf"), 5000.0):
            assert bad(r=r) and b"radius" in err(), r
        assert bad(m=NULL) and b"NULL" in err()
        assert bad(o=NULL) and b"NULL" in err()
        assert bad(l=NULL, s=NULL) and b"both NULL" in err()
        if not extra:                                       # (valid arguments: only the host hook can run here)
            assert not bad() and not bad(l=NULL) and not bad(s=NULL) and not bad(r=0.5)


def test_the_knob_is_off_by_default_and_the_cpu_route_is_untouched(golden):
    from epipolar_transformers_amd import backbones, default_cfg

    cfg = default_cfg()
    assert cfg.EPIPOLAR_AMD.PEAK_GRAD is False and backbones.peak_grad(cfg) is False
    cfg.merge_from_list(["EPIPOLAR_AMD.PEAK_GRAD", True])
    assert backbones.peak_grad(cfg) is True
    # find_peaks on a CPU tensor is plain torch with and without `grad`: the same bits, differentiable either way
    hm = torch.from_numpy(golden["24x40_r3.heat"])[None].requires_grad_(True)
    plain, with_grad = backbones.find_peaks(hm, 3.0, 4.0), backbones.find_peaks(hm, 3.0, 4.0, grad=True)
    for a, b in zip(plain, with_grad):
        assert a.requires_grad and b.requires_grad and same_bits(a.detach().numpy(), b.detach().numpy())
