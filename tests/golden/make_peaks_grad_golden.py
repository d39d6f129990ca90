"""Generate tests/golden/lifting/peaks_grad.npz: the gradient the REAL reference's find_tensor_peak_batch
(modeling/backbones/basic_batch.py:17-63) leaves in the heat map under torch autograd, on the CPU -- what et_heatmap_peaks_bwd
computes on the device.

Runs only where the reference tree is present (imported read-only through oracle/ref_harness.py).  What is executed is the
reference's own function; the maps are the ones tests/golden/lifting/peaks.npz already holds (made by make_peaks_golden.py: no
non-zero window sample within 1e-3 of the threshold), no new map is made.

    python tests/golden/make_peaks_grad_golden.py            # write the fixture
    python tests/golden/make_peaks_grad_golden.py --check    # regenerate and compare every array with the stored file, bit for bit

Stored (arrays only; keys "<run>.<name>", "nonfinite_<case>.<name>"; runs: peaks_restatement.RUNS, 16 maps each):
  <run>.g_locs (16, 2), <run>.g_scores (16) float32: the upstream gradients, standard_normal of default_rng(<run>.seed)
  <run>.ref_grad         (16, H, W) float32: the reference's autograd for both upstream gradients at once
  <run>.f64_grad         (16, H, W) float64: the same function on the float64 cast of the same maps and gradients
  <run>.ref_grad_err     (16) per map max |ref_grad - f64_grad| / max |f64_grad|: the REFERENCE's own distance from float64
  <run>.ref_grad_locs    (16, H, W) float32: the reference's gradient for g_locs alone (scores not differentiated)
  <run>.ref_grad_scores  (16, H, W) float32: ... for g_scores alone
  nonfinite_<case>.ref_grad (4, H, W) float32: the gradient of locs.sum() + scores.sum() on the first four maps of
                         peaks.npz's nonfinite_<case>.heat (peaks_restatement.NONFINITE_MAPS: nan_far, nan_cell0, all_nan, plus_inf)

The fifth non-finite map, all_minus_inf, is left out: there the reference's forward answer already hangs on rounding noise in its
bilinear weights (-inf times a weight that may or may not be zero: peaks_restatement.check_nonfinite), and so does its gradient.
It is the only map kind left out.

Legacy floor division (index / W as integer division, torch < 1.5) cannot be run through the reference under a current torch; its
expectation is the float64 autograd of backbones.soft_argmax_peaks(legacy_floor_division=True), taken in the tests, which first pin
the non-legacy float64 form of that function to f64_grad.

Conditions (asserted; caps, not measurements):
  * every map's ref_grad_err is below 1e-4 -- except at most one map per run, which stays below 1e-2.  (The exception is
    17x5_r0.6 / straddle_corner: the window hangs over a corner of the map and every sample that survives the threshold is a
    multiple of ONE cell, so the location does not depend on the map at all, the exact gradient of the location is 0 and float32
    returns the rounding noise of g / tot with tot near 1e-5; how large that reads against max |f64_grad| = |g_scores| is the luck
    of the draw.)  As in make_peaks_golden.py a seed that violates the condition is
    replaced by the next (seed + number of runs) -- the condition never changes, no run or map is dropped;
  * each non-finite gradient is NaN on the window's footprint (the cells its bilinear taps touch, clipped to the map) and nowhere
    else, and holds no +-inf.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]
from oracle import ref_harness as rh  # noqa: E402
import peaks_restatement as restate  # noqa: E402
from peaks_grad_common import footprint_mask  # noqa: E402

SEED = 5000
ERR_MAX = 1e-4              # per map ...
ERR_MAX_ONE = 1e-2          # ... but for at most one map of a run
NONFINITE_KINDS = ("nan_far", "nan_cell0", "all_nan", "plus_inf")
SRC = os.path.join(ROOT, "tests", "golden", "lifting", "peaks.npz")
OUT = os.path.join(ROOT, "tests", "golden", "lifting", "peaks_grad.npz")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def main(check=False):
    rh.install()
    rh.load_cfg(None)
    from modeling.backbones.basic_batch import find_tensor_peak_batch

    def reference(maps, radius, downsample, threshold, g_locs, g_scores, dtype=torch.float32):
        """The reference's autograd on (M, H, W) maps; an upstream gradient that is None is not differentiated."""
        hm = torch.from_numpy(maps).to(dtype).requires_grad_(True)
        locs, scores = find_tensor_peak_batch(hm, radius, downsample, threshold)
        assert locs.dtype == dtype and scores.dtype == dtype
        outs = [(o, torch.from_numpy(g).to(dtype)) for o, g in ((locs, g_locs), (scores, g_scores)) if g is not None]
        grad, = torch.autograd.grad([o for o, _ in outs], [hm], [g for _, g in outs])
        assert grad.dtype == dtype
        return grad.numpy()

    stored = np.load(SRC, allow_pickle=False)
    arrays = {}
    for number, (case, downsample, threshold) in enumerate(restate.RUNS):
        name = restate.run_name(case, downsample, threshold)
        maps, radius = stored[case + ".heat"], restate.CASES[case][2]
        assert stored[name + ".params"].tolist() == [radius, downsample, threshold]
        seed = SEED + number
        while True:
            rng = np.random.default_rng(seed)
            g_locs = rng.standard_normal((len(maps), 2)).astype(np.float32)
            g_scores = rng.standard_normal(len(maps)).astype(np.float32)
            ref = reference(maps, radius, downsample, threshold, g_locs, g_scores)
            f64 = reference(maps, radius, downsample, threshold, g_locs, g_scores, torch.float64)
            assert np.isfinite(ref).all() and np.isfinite(f64).all()
            size = np.abs(f64).reshape(len(maps), -1).max(1)
            assert (size > 0).all()
            err = np.abs(ref.astype(np.float64) - f64).reshape(len(maps), -1).max(1) / size
            if (err >= ERR_MAX).sum() <= 1 and (err < ERR_MAX_ONE).all():
                break
            print("%s: seed %d replaced (ref_grad_err up to %.3g)" % (name, seed, err.max()))
            seed += len(restate.RUNS)
        arrays[name + ".seed"] = np.int64(seed)
        arrays.update({name + ".g_locs": g_locs, name + ".g_scores": g_scores, name + ".ref_grad": ref, name + ".f64_grad": f64,
                       name + ".ref_grad_err": err,
                       name + ".ref_grad_locs": reference(maps, radius, downsample, threshold, g_locs, None),
                       name + ".ref_grad_scores": reference(maps, radius, downsample, threshold, None, g_scores)})
        worst = int(err.argmax())
        rest = np.delete(err, worst).max()
        print("%-22s ref_grad_err <= %.3g (%s), every other map <= %.3g; max |gradient| %.3g" % (
            name, err[worst], restate.MAP_KINDS[worst], rest, size.max()))

    for case in restate.NONFINITE_CASES:
        H, W, radius = restate.CASES[case]
        maps = stored["nonfinite_%s.heat" % case][:len(NONFINITE_KINDS)]
        assert restate.NONFINITE_MAPS[:len(NONFINITE_KINDS)] == NONFINITE_KINDS
        ones = np.ones((len(maps), 2), np.float32)
        grad = reference(maps, radius, 4.0, 1e-6, ones, ones[:, 0].copy())          # of locs.sum() + scores.sum()
        index = restate.peaks(maps, radius, 4.0, 1e-6)[2]
        counts = []
        for kind, g, i in zip(NONFINITE_KINDS, grad, index):
            inside = footprint_mask(H, W, int(i), radius)
            assert not np.isinf(g).any() and np.array_equal(np.isnan(g), inside), (case, kind)
            counts.append("%s %d" % (kind, inside.sum()))
        print("nonfinite %-10s NaN cells of %d: %s" % (case, H * W, ", ".join(counts)))
        arrays["nonfinite_%s.ref_grad" % case] = grad

    if check:
        old = np.load(OUT, allow_pickle=False)
        assert sorted(old.files) == sorted(arrays), "the stored fixture holds other arrays"
        for k, v in arrays.items():
            assert same_bits(old[k], np.asarray(v)), k
        print("every array of %s regenerated bit for bit" % OUT)
        return
    np.savez_compressed(OUT, **arrays)
    assert all(v.dtype != object for v in np.load(OUT, allow_pickle=False).values())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(check="--check" in sys.argv[1:])
