"""et_heatmap_peaks_bwd on the MI355X, through the C ABI and through ops.heatmap_peaks(with_grad=True): every run of
tests/golden/lifting/peaks_grad.npz (autograd through the real find_tensor_peak_batch, made by tests/golden/make_peaks_grad_golden.py)
with both forms of index / W, the host hook (the kernel's own per-cell routine on the CPU, the window's sums in the kernel's
order), repeated calls and batches, guard bands, torch.autograd, and EPIPOLAR_AMD.PEAK_GRAD through a small PoseResNet.

The tolerance of a map is peaks_grad_common.bounds(): max(4 x ref_grad_err, 2^-20) x max |f64_grad| with ref_grad_err the
REFERENCE's own distance from float64 on that map, read from the fixture.  Each test prints its figures (pytest -s).  Measured on
the MI355X: the kernel equals the host hook bit for bit in every run and every form; its worst use of a bound is 0.72 (24 x 40,
radius 3, downsample 8, corner00: 3.9e-7 of 5.5e-7 against the reference's float32), through the PoseResNet 0.64."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

import abi_harness as hx
import peaks_grad_common as common
import peaks_restatement as restate

pytestmark = pytest.mark.gpu

RUN_IDS = [restate.run_name(*r) for r in restate.RUNS]
KINDS = restate.MAP_KINDS
same_bits = restate.same_bits


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from epipolar_transformers_amd import _lib, ops

    assert ops.POISON_OUTPUTS                   # every output starts as NaN: nothing unwritten can pass for a result
    return _lib.load(), ops


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "lifting", "peaks.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def grads():
    return np.load(os.path.join(GOLDEN_DIR, "lifting", "peaks_grad.npz"), allow_pickle=False)


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def kernel_bwd(maps, radius, downsample, threshold, legacy, g_locs, g_scores):
    """et_heatmap_peaks_bwd through the C ABI on (M, H, W) maps -> (M, H, W) float32 NumPy; the output starts as NaN."""
    maps = cuda(maps)
    m, h, w = maps.shape
    grad = torch.full_like(maps, float("nan"))
    hx.call("et_heatmap_peaks_bwd", m, h, w, maps, radius, downsample, threshold, int(legacy), cuda(g_locs), cuda(g_scores), grad)
    return grad.cpu().numpy()


_kernel_cache = {}


def kernel(golden, grads, run, legacy):
    """The kernel's gradient for both upstream gradients of a run, computed once."""
    if (run, legacy) not in _kernel_cache:
        maps, radius, g = common.run_of(golden, grads, run)
        _kernel_cache[run, legacy] = kernel_bwd(maps, radius, run[1], run[2], legacy, g("g_locs"), g("g_scores"))
    return _kernel_cache[run, legacy]


@pytest.mark.parametrize("run", restate.RUNS, ids=RUN_IDS)
def test_kernel_equals_the_host_hook_and_lies_within_the_references_own_error(env, golden, grads, run):
    lib, ops = env
    maps, radius, g = common.run_of(golden, grads, run)
    _, downsample, threshold = run
    tol = common.bounds(g("ref_grad_err"), g("f64_grad"))
    for legacy in (False, True):
        got = kernel(golden, grads, run, legacy)
        assert np.isfinite(got).all()                                    # every element written
        # the kernel and its routine on the host take every sum in the same order: equal bits
        assert same_bits(got, common.host_bwd(lib, maps, radius, downsample, threshold, legacy, g("g_locs"), g("g_scores")))
        for gl, gs in ((g("g_locs"), None), (None, g("g_scores"))):     # the two NULL-pointer forms
            assert same_bits(kernel_bwd(maps, radius, downsample, threshold, legacy, gl, gs),
                             common.host_bwd(lib, maps, radius, downsample, threshold, legacy, gl, gs))
    got = kernel(golden, grads, run, False)
    for name, want in (("reference", g("ref_grad")), ("float64", g("f64_grad"))):
        err = common.worst(got, want)
        k = int((err / tol).argmax())
        print("    %-24s against %-9s worst use of a bound %.3f (%s: %.3e of %.3e)" % (restate.run_name(*run), name, err[k] / tol[k], KINDS[k], err[k], tol[k]))
        assert (err <= tol).all(), (name, KINDS[k], err[k], tol[k])
    assert (common.worst(kernel_bwd(maps, radius, downsample, threshold, False, g("g_locs"), None), g("ref_grad_locs")) <= tol).all()
    assert same_bits(kernel_bwd(maps, radius, downsample, threshold, False, None, g("g_scores")), g("ref_grad_scores"))
    # legacy floor division: the float64 autograd of the torch route, its tolerance from that route's own float32 error
    want = common.torch_grad(maps, radius, downsample, threshold, True, g("g_locs"), g("g_scores"))
    err = common.worst(kernel(golden, grads, run, True), want)
    assert (err <= common.legacy_bounds(maps, radius, downsample, threshold, g("g_locs"), g("g_scores"), want)).all()


@pytest.mark.parametrize("case", restate.NONFINITE_CASES)
def test_nonfinite_maps_have_the_references_nan_mask(env, golden, grads, case):
    lib, ops = env
    H, W, radius = restate.CASES[case]
    maps, want = golden["nonfinite_%s.heat" % case][:4], grads["nonfinite_%s.ref_grad" % case]
    ones = np.ones((4, 2), np.float32)
    got = kernel_bwd(maps, radius, 4.0, 1e-6, False, ones, ones[:, 0].copy())
    assert same_bits(got, common.host_bwd(lib, maps, radius, 4.0, 1e-6, False, ones, ones[:, 0].copy()))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and (got[~nan] == 0).all() and (want[~nan] == 0).all()


def test_second_call_and_a_map_alone_give_the_bits_of_the_batch(env, golden, grads):
    run = ("64x64_r8", 4.0, 1e-6)
    maps, radius, g = common.run_of(golden, grads, run)
    first = kernel(golden, grads, run, False)
    assert same_bits(kernel_bwd(maps, radius, 4.0, 1e-6, False, g("g_locs"), g("g_scores")), first)
    for m in (0, KINDS.index("inside1"), KINDS.index("straddle_corner"), len(maps) - 1):
        alone = kernel_bwd(maps[m:m + 1], radius, 4.0, 1e-6, False, g("g_locs")[m:m + 1], g("g_scores")[m:m + 1])
        assert same_bits(alone[0], first[m]), KINDS[m]


@pytest.mark.parametrize("case", ["64x64_r8", "4x4_r8", "2x2_r1", "3x100_r2.5", "17x5_r0.6"])
def test_guard_bands_around_grad_heat_stay_untouched(env, golden, grads, case):
    run = (case, 4.0, 1e-6)
    maps, radius, g = common.run_of(golden, grads, run)
    m, h, w = maps.shape
    dev = {k: cuda(v) for k, v in (("maps", maps), ("g_locs", g("g_locs")), ("g_scores", g("g_scores")))}
    for gl, gs in ((dev["g_locs"], dev["g_scores"]), (dev["g_locs"], None), (None, dev["g_scores"])):
        a = hx.Arena().add("grad", (m, h, w)).build()
        snap = hx.frozen(**dev)
        hx.call("et_heatmap_peaks_bwd", m, h, w, dev["maps"], radius, 4.0, 1e-6, 0, gl, gs, a["grad"])
        a.check()
        hx.assert_unchanged(snap)
        assert torch.isfinite(a["grad"]).all()
        if gl is not None and gs is not None:
            assert same_bits(a["grad"].cpu().numpy(), kernel(golden, grads, run, False))


def test_autograd_through_the_operator_equals_the_direct_call(env, golden, grads):
    lib, ops = env
    run = ("24x40_r3", 4.0, 1e-6)
    maps, radius, g = common.run_of(golden, grads, run)
    direct = kernel(golden, grads, run, False)
    hm = cuda(maps)[None].requires_grad_(True)
    plain = ops.heatmap_peaks(hm.detach(), radius, 4.0)
    locs, scores = ops.heatmap_peaks(hm, radius, 4.0, with_grad=True)
    assert locs.grad_fn is not None and scores.grad_fn is not None
    assert hx.same_bits(locs.detach(), plain[0]) and hx.same_bits(scores.detach(), plain[1])
    both, = torch.autograd.grad([locs, scores], [hm], [cuda(g("g_locs"))[None], cuda(g("g_scores"))[None]], retain_graph=True)
    assert same_bits(both[0].cpu().numpy(), direct)
    # an output nobody differentiates reaches the library as NULL
    only_locs, = torch.autograd.grad([locs], [hm], [cuda(g("g_locs"))[None]], retain_graph=True)
    assert same_bits(only_locs[0].cpu().numpy(), kernel_bwd(maps, radius, 4.0, 1e-6, False, g("g_locs"), None))
    only_scores, = torch.autograd.grad([scores], [hm], [cuda(g("g_scores"))[None]])
    assert same_bits(only_scores[0].cpu().numpy(), g("ref_grad_scores"))
    # a non-contiguous (channel-sliced) input, a float64 upstream gradient
    wide = torch.stack([cuda(maps), cuda(maps).flip(0)], 0).requires_grad_(True)
    view = wide[:, 3:12:2]
    assert not view.is_contiguous()
    l2, _ = ops.heatmap_peaks(view, radius, 4.0, with_grad=True)
    (l2 * cuda(g("g_locs"))[None, 3:12:2].double()).sum().backward()
    assert same_bits(wide.grad[0, 3:12:2].cpu().numpy(), only_locs[0, 3:12:2].cpu().numpy())
    assert (wide.grad[:, 4:12:2] == 0).all() and (wide.grad[:, :3] == 0).all()


def test_without_with_grad_or_requires_grad_nothing_is_attached(env, golden):
    lib, ops = env
    maps = cuda(golden["24x40_r3.heat"])[None]
    for hm, with_grad in ((maps.clone().requires_grad_(True), False), (maps, True), (maps, False)):
        locs, scores = ops.heatmap_peaks(hm, 3.0, 4.0, with_grad=with_grad)
        assert locs.grad_fn is None and scores.grad_fn is None and not locs.requires_grad and not scores.requires_grad
    with torch.no_grad():
        locs, scores = ops.heatmap_peaks(maps.clone().requires_grad_(True), 3.0, 4.0, with_grad=True)
    assert locs.grad_fn is None and scores.grad_fn is None


def test_peak_grad_knob_through_a_small_pose_resnet(env):
    """forward_views of the smallest PoseResNet of tests/test_gpu_model.py.  Knob on: the detections require grad, the gradient of
    (locs * g).sum() reaches final_layer.weight, and what it leaves in the heat map equals the float64 autograd of
    backbones.soft_argmax_peaks on the same heat map -- within the bound rule, ref_grad_err being that torch route's float32
    distance from its float64 on these maps (the reference's operations).  Knob off: detached, and the same bits."""
    from epipolar_transformers_amd import synthetic as syn
    from epipolar_transformers_amd.model import ring_sources
    from test_gpu_model import _cfg, _model

    lib, ops = env
    cfg, size, hs = _cfg()
    m = _model(cfg)
    frames, V = 1, 4
    P = torch.from_numpy(syn.ring_cameras(V, size)).float().repeat(frames, 1, 1)
    img = torch.randn(frames * V, 3, size, size, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    src = ring_sources(frames, V, "cuda")
    sigma, ds = float(cfg.KEYPOINT.SIGMA), float(cfg.BACKBONE.DOWNSAMPLE)
    off = m.forward_views(img, P, src)
    assert not off[2].requires_grad and not off[3].requires_grad and off[1][0].requires_grad
    cfg.merge_from_list(["EPIPOLAR_AMD.PEAK_GRAD", True])
    on = m.forward_views(img, P, src)
    heat, locs, scos = on[1][0], on[2], on[3]
    assert locs.requires_grad and scos.requires_grad
    # the knob changes no value: each pass returns the detached operator's bits on its own heat map
    for out in (off, on):
        want = ops.heatmap_peaks(out[1][0].detach(), sigma, ds)
        assert hx.same_bits(out[2].detach(), want[0]) and hx.same_bits(out[3].detach(), want[1])
    g = torch.randn(locs.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    heat.retain_grad()
    (locs * g).sum().backward()
    wgrad = m.reference.final_layer.weight.grad
    assert wgrad is not None and torch.isfinite(wgrad).all() and wgrad.abs().max().item() > 0
    n, j, h, w = heat.shape
    maps = heat.detach().cpu().numpy().reshape(n * j, h, w)
    gl = g.cpu().numpy().reshape(n * j, 2)
    f64 = common.torch_grad(maps, sigma, ds, 1e-6, False, gl, None)
    f32 = common.torch_grad(maps, sigma, ds, 1e-6, False, gl, None, torch.float32)
    largest = np.abs(f64).reshape(n * j, -1).max(1)
    assert (largest > 0).any()
    # (a map with nothing above the threshold has no gradient at all: its bound is 0)
    tol = common.bounds(common.worst(f32, f64) / np.where(largest > 0, largest, 1.0), f64)
    err = common.worst(heat.grad.cpu().numpy().reshape(n * j, h, w), f64)
    k = int(np.divide(err, tol, out=np.zeros_like(err), where=tol > 0).argmax())
    print("    PoseResNet heat-map gradient, %d maps of %d with one: worst use of a bound %.3f (map %d: %.3e of %.3e)" % (
        (largest > 0).sum(), n * j, err[k] / tol[k], k, err[k], tol[k]))
    assert (err <= tol).all(), (k, err[k], tol[k])
