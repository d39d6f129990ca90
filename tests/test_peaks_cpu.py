"""The head's peak finder on the CPU: the float64 restatement (tests/peaks_restatement.py), the product's CPU route
(backbones.soft_argmax_peaks) and the library's host hook (et_debug_host_heatmap_peaks: the kernel's own per-map routine of
csrc/et_peaks.h in a serial loop, its sums in the kernel's order) against what the reference's find_tensor_peak_batch returned
(tests/golden/lifting/peaks.npz, made by tests/golden/make_peaks_golden.py), the non-finite maps, and the ABI's argument checks.

The tolerance of a run is peaks_restatement.bound(): max(4 x ref_err, 2 ulp_float32(max |location|)), ref_err being the
REFERENCE's own distance from float64 as the fixture records it -- never a figure of the code under test."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

import peaks_restatement as restate
from epipolar_transformers_amd import _lib, backbones, build

NULL = ctypes.c_void_p(0)
RUN_IDS = [restate.run_name(*r) for r in restate.RUNS]


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "lifting", "peaks.npz"), allow_pickle=False)


def fp(a):
    return NULL if a is None else a.ctypes.data_as(ctypes.c_void_p)


same_bits, check_nonfinite = restate.same_bits, restate.check_nonfinite


host_peaks = restate.host_peaks


def run_of(golden, run):
    case, downsample, threshold = run
    name = restate.run_name(*run)
    g = lambda k: golden["%s.%s" % (name, k)]
    assert g("params").tolist() == [restate.CASES[case][2], downsample, threshold]
    return golden[case + ".heat"], g


def test_fixture_holds_every_case_and_the_makers_conditions(golden):
    want = set(restate.CASES) | set(RUN_IDS) | {"nonfinite_" + c for c in restate.NONFINITE_CASES}
    assert {k.rsplit(".", 1)[0] for k in golden.files} == want
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "lifting", "peaks.npz")) < 1 << 20
    for run in restate.RUNS:
        maps, g = run_of(golden, run)
        H, W, _ = restate.CASES[run[0]]
        assert maps.shape == (len(restate.MAP_KINDS), H, W) and maps.dtype == np.float32 and np.isfinite(maps).all()
        assert g("ref_locs").dtype == np.float32 and g("ref_scores").dtype == np.float32 and g("f64_locs").dtype == np.float64
        assert 0 < float(g("ref_err")) < 1e-4 and float(g("margin")) >= 1e-3
        assert float(g("ref_err")) == np.abs(g("ref_locs").astype(np.float64) - g("f64_locs")).max()
        assert restate.bound(g("ref_err"), g("ref_locs")) < 1e-4                # under 1e-4 px even at 500 px
    # both sides of the threshold are reached: the straddle maps lose some, not all, of their window
    maps, g = run_of(golden, ("64x64_r8", 4.0, 1e-6))
    for kind in ("straddle_inside", "straddle_corner"):
        m = maps[restate.MAP_KINDS.index(kind)]
        assert m.max() > 1e-6 and ((m > 0) & (m < 1e-6)).any()
    for case in restate.NONFINITE_CASES:
        assert golden["nonfinite_%s.heat" % case].shape[0] == len(restate.NONFINITE_MAPS)


@pytest.mark.parametrize("run", restate.RUNS, ids=RUN_IDS)
def test_restatement_matches_the_fixture(golden, run):
    maps, g = run_of(golden, run)
    _, downsample, threshold = run
    radius = restate.CASES[run[0]][2]
    for legacy, key in ((False, "f64_locs"), (True, "f64_locs_legacy")):
        locs, scores, index, margin = restate.peaks(maps, radius, downsample, threshold, legacy)
        assert same_bits(locs, g(key)) and same_bits(scores, g("ref_scores")) and same_bits(index, g("index"))
        assert margin.min() >= float(g("margin"))
    # the first maximum: the constant map, the planted ties
    H, W, _ = restate.CASES[run[0]]
    spread, strided = restate.tie_indices(H, W)
    kinds = restate.MAP_KINDS
    assert g("index")[kinds.index("constant")] == 0
    assert g("index")[kinds.index("ties_spread")] == spread[0] and g("index")[kinds.index("ties_strided")] == strided[0]
    assert same_bits(g("ref_scores"), maps.reshape(len(maps), -1).max(1))


@pytest.mark.parametrize("run", restate.RUNS, ids=RUN_IDS)
def test_cpu_route_equals_the_reference_bit_for_bit(golden, run):
    maps, g = run_of(golden, run)
    _, downsample, threshold = run
    locs, scores = backbones.soft_argmax_peaks(torch.from_numpy(maps)[None], restate.CASES[run[0]][2], downsample, threshold)
    assert same_bits(locs[0].numpy(), g("ref_locs")) and same_bits(scores[0].numpy(), g("ref_scores"))
    # find_peaks takes this route for a CPU tensor
    if threshold == 1e-6:
        again = backbones.find_peaks(torch.from_numpy(maps)[None], restate.CASES[run[0]][2], downsample)
        assert same_bits(again[0][0].numpy(), g("ref_locs")) and same_bits(again[1][0].numpy(), g("ref_scores"))


@pytest.mark.parametrize("run", restate.RUNS, ids=RUN_IDS)
def test_host_hook_within_the_references_own_error_of_float64(lib, golden, run):
    maps, g = run_of(golden, run)
    _, downsample, threshold = run
    radius = restate.CASES[run[0]][2]
    tol = restate.bound(g("ref_err"), g("ref_locs"))
    kinds = restate.MAP_KINDS
    for legacy, key in ((False, "f64_locs"), (True, "f64_locs_legacy")):
        locs, scores = host_peaks(lib, maps, radius, downsample, threshold, legacy)
        err = np.abs(locs.astype(np.float64) - g(key)).max(1)
        print("    %-24s legacy %d: worst %.3e px (%s)  bound %.3e" % (restate.run_name(*run), legacy, err.max(), kinds[err.argmax()], tol))
        assert same_bits(scores, g("ref_scores"))
        assert err.max() <= tol, (legacy, kinds[err.argmax()], err.max(), tol)
        # exact where the window sums to nothing or to a constant field around cell 0: the arg-max cell's own location
        if threshold > 1e-8:
            W = maps.shape[2]
            assert same_bits(locs[kinds.index("tiny")], restate.cell_location(0, W, downsample, legacy))


@pytest.mark.parametrize("case", restate.NONFINITE_CASES)
@pytest.mark.parametrize("legacy", [False, True])
def test_host_hook_on_the_nonfinite_maps(lib, golden, case, legacy):
    maps = golden["nonfinite_%s.heat" % case]
    ref_locs, ref_scores = golden["nonfinite_%s.ref_locs" % case], golden["nonfinite_%s.ref_scores" % case]
    H, W, radius = restate.CASES[case]
    locs, scores = host_peaks(lib, maps, radius, 4.0, 1e-6, legacy)
    check_nonfinite(locs, scores, ref_locs, ref_scores, W)
    # the restatement and the product's CPU route say the same
    r_locs, r_scores, r_index, _ = restate.peaks(maps, radius, 4.0, 1e-6, legacy)
    check_nonfinite(r_locs.astype(np.float32), r_scores, ref_locs, ref_scores, W)
    assert r_index.tolist() == [W - 1, 0, 0, (H - 1) * W + W - 2, 0]
    t_locs, t_scores = backbones.soft_argmax_peaks(torch.from_numpy(maps)[None], radius, 4.0, legacy_floor_division=legacy)
    check_nonfinite(t_locs[0].numpy(), t_scores[0].numpy(), ref_locs, ref_scores, W)


def test_header_ctypes_and_exports_agree_and_bad_arguments_are_errors(lib):
    text = open(os.path.join(ROOT, "include", "epipolar_amd.h")).read()
    for name in ("et_heatmap_peaks", "et_debug_host_heatmap_peaks"):
        assert ("int %s(" % name) in text and name in _lib.exported_symbols() and hasattr(lib, name)
    assert lib.et_abi_version() == 14 and _lib.ET_ABI_VERSION == 14      # additive: the version stays
    assert "NaN" in text[text.index("Peak finder of the pose head"):text.index("int et_heatmap_peaks(")]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "NaN" in integration[integration.index("`et_heatmap_peaks`"):][:2500]
    err = lambda: lib.et_last_error()
    maps, locs, scores = np.zeros((1, 4, 4), np.float32), np.zeros((1, 2), np.float32), np.zeros(1, np.float32)
    # (the device entry point reports these before any launch: no GPU is touched)
    for entry, extra in ((lib.et_debug_host_heatmap_peaks, ()), (lib.et_heatmap_peaks, (NULL,))):
        bad = lambda n=1, h=4, w=4, r=2.0, m=fp(maps), l=fp(locs), s=fp(scores): entry(n, h, w, m, r, 4.0, 1e-6, 0, l, s, *extra) != 0
        assert bad(h=1) and b"bad sizes" in err()
        assert bad(w=1) and b"bad sizes" in err()
        assert bad(n=0) and b"bad sizes" in err()
        assert bad(n=1 << 31) and b"bad sizes" in err()
        for r in (0.0, -1.0, float("nan"), 0.49, float("inf"), 5000.0):
            assert bad(r=r) and b"radius" in err(), r
        for k in ("m", "l", "s"):
            assert bad(**{k: NULL}) and b"NULL" in err()
        assert extra or not bad()                           # (valid arguments: only the host hook can run here)
        assert extra or not bad(r=0.5)                      # int(0.5 + 0.5) = 1: the smallest radius admitted
