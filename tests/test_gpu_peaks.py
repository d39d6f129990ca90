"""et_heatmap_peaks on the MI355X against float64 and the reference at its edges: every case of tests/golden/lifting/peaks.npz
(made from the real find_tensor_peak_batch by tests/golden/make_peaks_golden.py) with both forms of index / W, the non-finite
maps, the host hook (the kernel's own per-map routine on the CPU, sums in the kernel's order), repeated and side-stream calls, a
non-contiguous input, and the two routes of backbones.find_peaks.

The tolerance of a run is peaks_restatement.bound(): max(4 x ref_err, 2 ulp_float32(max |location|)) with ref_err the REFERENCE's
own distance from float64, read from the fixture (under 1e-4 px everywhere).  Measured on the MI355X (each test prints its
figures, pytest -s): the kernel's worst distance from float64 over all runs is 2.3e-5 px (96 x 96, radius 1.4, legacy division,
bound 6.1e-5 px); its worst use of a bound is 0.52 of it (64 x 64, radius 8: 1.9e-5 of 3.7e-5 px); it equals the host hook bit
for bit everywhere."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

import peaks_restatement as restate

pytestmark = pytest.mark.gpu

RUN_IDS = [restate.run_name(*r) for r in restate.RUNS]
same_bits, host_peaks = restate.same_bits, restate.host_peaks


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from epipolar_transformers_amd import _lib, ops

    assert ops.POISON_OUTPUTS                   # every output starts as NaN: nothing unwritten can pass for a result
    return _lib.load(), ops


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "lifting", "peaks.npz"), allow_pickle=False)


_kernel_cache = {}


def kernel(ops, golden, run, legacy):
    """The kernel's (locs (M, 2), scores (M)) float32 on a run's maps, computed once."""
    key = (run, legacy)
    if key not in _kernel_cache:
        case, downsample, threshold = run
        maps = torch.from_numpy(golden[case + ".heat"]).cuda()[None]
        locs, scores = ops.heatmap_peaks(maps, restate.CASES[case][2], downsample, threshold, legacy_floor_division=legacy)
        _kernel_cache[key] = (locs[0].cpu().numpy(), scores[0].cpu().numpy())
    return _kernel_cache[key]


@pytest.mark.parametrize("run", restate.RUNS, ids=RUN_IDS)
def test_kernel_within_the_references_own_error_of_float64(env, golden, run):
    lib, ops = env
    case, downsample, threshold = run
    name = restate.run_name(*run)
    g = lambda k: golden["%s.%s" % (name, k)]
    maps = golden[case + ".heat"]
    tol = restate.bound(g("ref_err"), g("ref_locs"))
    kinds = restate.MAP_KINDS
    for legacy, key in ((False, "f64_locs"), (True, "f64_locs_legacy")):
        locs, scores = kernel(ops, golden, run, legacy)
        err = np.abs(locs.astype(np.float64) - g(key)).max(1)
        print("    %-24s legacy %d: worst %.3e px (%s)  bound %.3e" % (name, legacy, err.max(), kinds[err.argmax()], tol))
        assert same_bits(scores, maps.reshape(len(maps), -1).max(1)) and same_bits(scores, g("ref_scores"))
        assert err.max() <= tol, (legacy, kinds[err.argmax()], err.max(), tol)
        if not legacy:
            to_ref = np.abs(locs.astype(np.float64) - g("ref_locs")).max()
            print("    %-24s            against the reference's float32: %.3e px" % ("", to_ref))
            assert to_ref <= tol + float(g("ref_err"))
        # the kernel and its routine on the host take every sum in the same order: equal bits
        h_locs, h_scores = host_peaks(lib, maps, restate.CASES[case][2], downsample, threshold, legacy)
        assert same_bits(locs, h_locs) and same_bits(scores, h_scores), np.abs(locs - h_locs).max()
        # everything below the threshold: exactly the arg-max cell's location, which pins the index
        if threshold > 1e-8:
            W = maps.shape[2]
            assert same_bits(locs[kinds.index("tiny")], restate.cell_location(0, W, downsample, legacy))


@pytest.mark.parametrize("case", list(restate.CASES))
def test_exact_locations_on_subthreshold_constant_and_single_cell_maps(env, case):
    """Maps whose window holds nothing above the threshold: a constant below it (every cell ties: index 0) and a single cell
    below it at each planted tie index -- the location is the arg-max cell's own, exactly, so a wrong index cannot hide."""
    lib, ops = env
    H, W, radius = restate.CASES[case]
    spread, strided = restate.tie_indices(H, W)
    cells = [0] + spread + strided + [H * W - 1]
    maps = np.zeros((len(cells) + 1, H, W), np.float32)
    maps[0] = 5e-7
    for m, c in zip(maps[1:], cells):
        m[:] = -1.0
        m.reshape(-1)[c] = 5e-7
    for legacy in (False, True):
        locs, scores = ops.heatmap_peaks(torch.from_numpy(maps).cuda()[None], radius, 4.0, legacy_floor_division=legacy)
        locs = locs[0].cpu().numpy()
        assert (scores[0].cpu().numpy() == np.float32(5e-7)).all()
        for got, c in zip(locs, [0] + cells):
            assert same_bits(got, restate.cell_location(c, W, 4.0, legacy)), (c, got)


@pytest.mark.parametrize("case", restate.NONFINITE_CASES)
@pytest.mark.parametrize("legacy", [False, True])
def test_nonfinite_maps_return_what_the_reference_returns(env, golden, case, legacy):
    lib, ops = env
    maps = golden["nonfinite_%s.heat" % case]
    H, W, radius = restate.CASES[case]
    locs, scores = ops.heatmap_peaks(torch.from_numpy(maps).cuda()[None], radius, 4.0, legacy_floor_division=legacy)
    locs, scores = locs[0].cpu().numpy(), scores[0].cpu().numpy()
    print("    %s legacy %d: all -inf -> %s score %s" % (case, legacy, locs[-1], scores[-1]))
    restate.check_nonfinite(locs, scores, golden["nonfinite_%s.ref_locs" % case], golden["nonfinite_%s.ref_scores" % case], W)
    h_locs, h_scores = host_peaks(lib, maps, radius, 4.0, 1e-6, legacy)
    assert same_bits(locs, h_locs) and same_bits(scores, h_scores)


def test_second_call_and_side_stream_give_equal_bits(env, golden):
    lib, ops = env
    run = ("64x64_r8", 4.0, 1e-6)
    maps = torch.from_numpy(golden["64x64_r8.heat"]).cuda()[None]
    first = kernel(ops, golden, run, False)
    again = ops.heatmap_peaks(maps, 8.0, 4.0)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        other = ops.heatmap_peaks(maps, 8.0, 4.0)
    torch.cuda.synchronize()
    for got in (again, other):
        assert same_bits(got[0][0].cpu().numpy(), first[0]) and same_bits(got[1][0].cpu().numpy(), first[1])


def test_channel_sliced_view_equals_its_contiguous_copy(env, golden):
    lib, ops = env
    maps = torch.from_numpy(golden["24x40_r3.heat"]).cuda()
    wide = torch.stack([maps, maps.flip(0), maps * 0.5], 0)              # (3, 16, 24, 40)
    view = wide[:, 3:12:2]                                              # a strided slice of the joints
    assert not view.is_contiguous()
    got, want = ops.heatmap_peaks(view, 3.0, 4.0), ops.heatmap_peaks(view.contiguous(), 3.0, 4.0)
    assert same_bits(got[0].cpu().numpy(), want[0].cpu().numpy()) and same_bits(got[1].cpu().numpy(), want[1].cpu().numpy())
    first = kernel(ops, golden, ("24x40_r3", 4.0, 1e-6), False)
    assert same_bits(got[0][0].cpu().numpy(), first[0][3:12:2]) and tuple(got[0].shape) == (3, 5, 2) and tuple(got[1].shape) == (3, 5)


@pytest.mark.parametrize("run", [r for r in restate.RUNS if r[2] == 1e-6], ids=[i for i, r in zip(RUN_IDS, restate.RUNS) if r[2] == 1e-6])
def test_find_peaks_agrees_between_its_gpu_and_cpu_routes(env, golden, run):
    from epipolar_transformers_amd import backbones

    case, downsample, _ = run
    g = lambda k: golden["%s.%s" % (restate.run_name(*run), k)]
    radius = restate.CASES[case][2]
    maps = torch.from_numpy(np.concatenate([golden[case + ".heat"]] + ([golden["nonfinite_%s.heat" % case]] if case in restate.NONFINITE_CASES else [])))[None]
    cpu_l, cpu_s = backbones.find_peaks(maps, radius, downsample)
    gpu_l, gpu_s = backbones.find_peaks(maps.cuda(), radius, downsample)
    assert gpu_l.is_cuda and not cpu_l.is_cuda
    cpu_l, cpu_s, gpu_l, gpu_s = cpu_l[0].numpy(), cpu_s[0].numpy(), gpu_l[0].cpu().numpy(), gpu_s[0].cpu().numpy()
    n = len(restate.MAP_KINDS)
    assert same_bits(cpu_l[:n], g("ref_locs")) and same_bits(cpu_s, gpu_s)
    diff = np.abs(cpu_l[:n].astype(np.float64) - gpu_l[:n]).max()
    print("    %-24s GPU route - CPU route: %.3e px (bound %.3e)" % (restate.run_name(*run), diff, restate.bound(g("ref_err"), g("ref_locs"))))
    assert diff <= restate.bound(g("ref_err"), g("ref_locs"))
    # ... and on NaN: the same maps report it on both routes (the map of -inf alone may differ: cell 0 or NaN, see check_nonfinite)
    assert np.array_equal(np.isnan(cpu_l[:n + 4]), np.isnan(gpu_l[:n + 4])) and np.array_equal(np.isnan(cpu_s), np.isnan(gpu_s))
    if len(cpu_l) > n:
        assert np.isnan(gpu_l[n:n + 4]).all() and np.isnan(gpu_s[n:n + 3]).all()
