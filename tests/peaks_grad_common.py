"""What tests/test_peaks_grad_cpu.py, tests/test_gpu_peaks_grad.py and tests/golden/make_peaks_grad_golden.py share: the tolerance of
the peak finder's gradient, the window's footprint, the host hook's call and the float64 autograd of the product's torch route.

Tolerance of ONE map:  max(4 x ref_grad_err, 2^-20) x max |f64_grad|.  ref_grad_err is the REFERENCE's own distance from float64
on that map, relative to the map's largest gradient element, as tests/golden/lifting/peaks_grad.npz records it; the factor 4 is
the margin peaks_restatement.bound takes and for the same reason (another summation order); 2^-20 is eight float32 ulps of the
largest element, the floor for maps on which the reference happens to be exact.  Never a figure of the code under test."""
import ctypes

import numpy as np
import torch

import peaks_restatement as restate

FLOOR = 2.0 ** -20


def bounds(ref_grad_err, f64_grad):
    """Per-map absolute tolerances, (M,), for (M, H, W) gradients."""
    size = np.abs(np.asarray(f64_grad, np.float64)).reshape(len(f64_grad), -1).max(1)
    return np.maximum(4.0 * np.asarray(ref_grad_err, np.float64), FLOOR) * size


def worst(grad, want):
    """Per-map max |grad - want|, (M,)."""
    return np.abs(np.asarray(grad, np.float64) - np.asarray(want, np.float64)).reshape(len(grad), -1).max(1)


def footprint(H, W, index, radius, legacy=False):
    """The cells the window's bilinear taps touch, clipped to the map: (y0, y1, x0, x1), inclusive.  float32, operation by
    operation as find_tensor_peak_batch, F.affine_grid and F.grid_sample (align_corners False) place the first and last sample."""
    f = np.float32
    side = 2 * int(radius + 0.5) + 1

    def axis(centre, L):
        lo, hi = f(-1) + f(2) * (centre - f(radius)) / f(L - 1), f(-1) + f(2) * (centre + f(radius)) / f(L - 1)
        scale, offset = (hi - lo) / f(2), (hi + lo) / f(2)
        first, last = (((scale * (f(2 * i + 1) / f(side) - f(1)) + offset + f(1)) * f(L) - f(1)) / f(2) for i in (0, side - 1))
        return max(int(np.floor(first)), 0), min(int(np.floor(last)) + 1, L - 1)

    y0, y1 = axis(f(index // W) if legacy else f(index) / f(W), H)
    x0, x1 = axis(f(index % W), W)
    return y0, y1, x0, x1


def footprint_mask(H, W, index, radius, legacy=False):
    y0, y1, x0, x1 = footprint(H, W, index, radius, legacy)
    inside = np.zeros((H, W), bool)
    inside[y0:y1 + 1, x0:x1 + 1] = True
    return inside


def host_bwd(lib, maps, radius, downsample, threshold, legacy, g_locs, g_scores):
    """et_debug_host_heatmap_peaks_bwd on (M, H, W) maps -> (M, H, W) float32; the output starts as NaN; None is passed as NULL."""
    maps = np.ascontiguousarray(maps, np.float32)
    m, h, w = maps.shape
    grad = np.full((m, h, w), np.nan, np.float32)
    ptr = lambda a: ctypes.c_void_p(0) if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(ctypes.c_void_p)
    gl, gs = (None if g is None else np.ascontiguousarray(g, np.float32) for g in (g_locs, g_scores))
    rc = lib.et_debug_host_heatmap_peaks_bwd(m, h, w, ptr(maps), radius, downsample, threshold, int(legacy), ptr(gl), ptr(gs), ptr(grad))
    assert rc == 0, lib.et_last_error()
    return grad


def torch_grad(maps, radius, downsample, threshold, legacy, g_locs, g_scores, dtype=torch.float64):
    """Autograd of backbones.soft_argmax_peaks (the product's torch route, the reference's operations) on the `dtype` cast of (M, H, W)
    maps -> (M, H, W) NumPy."""
    from epipolar_transformers_amd import backbones

    hm = torch.from_numpy(np.asarray(maps)).to(dtype).requires_grad_(True)
    locs, scores = backbones.soft_argmax_peaks(hm[None], radius, downsample, threshold, legacy_floor_division=legacy)
    outs = [(o[0], torch.from_numpy(np.asarray(g)).to(dtype)) for o, g in ((locs, g_locs), (scores, g_scores)) if g is not None]
    grad, = torch.autograd.grad([o for o, _ in outs], [hm], [g for _, g in outs])
    return grad.numpy()


def legacy_bounds(maps, radius, downsample, threshold, g_locs, g_scores, f64_legacy):
    """bounds() for legacy floor division.  The window of a map moves with index // W, so the fixture's ref_grad_err (true division)
    says nothing about it, and the reference itself cannot be run in this form: its distance from float64 is taken from the torch
    route (the reference's operations; tests/test_peaks_cpu.py holds its forward to the reference bit for bit) in float32 against the
    same route in float64, per map."""
    f32 = torch_grad(maps, radius, downsample, threshold, True, g_locs, g_scores, torch.float32)
    size = np.abs(f64_legacy).reshape(len(maps), -1).max(1)
    return bounds(worst(f32, f64_legacy) / size, f64_legacy)


def run_of(golden, grads, run):
    """(maps, radius, g) of a run: g(name) reads the run's arrays of peaks_grad.npz."""
    case = run[0]
    name = restate.run_name(*run)
    return golden[case + ".heat"], restate.CASES[case][2], lambda k: grads["%s.%s" % (name, k)]
