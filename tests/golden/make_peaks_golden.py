"""Generate tests/golden/lifting/peaks.npz from the REAL reference's find_tensor_peak_batch (modeling/backbones/basic_batch.py:17-63),
the peak finder et_heatmap_peaks computes on the device, run on the CPU.

Runs only where the reference tree is present (imported read-only through oracle/ref_harness.py).  What is executed is the
reference's own code; the maps come from tests/peaks_restatement.py's generators, and the float64 restatement's results are stored
next to the reference's float32 ones.

    python tests/golden/make_peaks_golden.py            # write the fixture
    python tests/golden/make_peaks_golden.py --check    # regenerate and compare every array with the stored file, bit for bit

Stored (arrays only; keys "<case>.heat", "<run>.<name>", "nonfinite_<case>.<name>"; cases and runs: peaks_restatement.CASES / RUNS):
  <case>.heat        (16, H, W) float32: the maps of peaks_restatement.MAP_KINDS
  <run>.params       [radius, downsample, threshold]
  <run>.ref_locs     (16, 2) float32, <run>.ref_scores (16) float32: what the reference returned
  <run>.f64_locs     (16, 2) float64: the restatement; <run>.f64_locs_legacy: with index // W (see below)
  <run>.index        (16) int64: the restatement's arg-max (the reference does not return its own)
  <run>.ref_err      max |reference - float64| over the case's maps, image pixels: the REFERENCE's distance from float64
  <run>.margin       the smallest relative distance of a non-zero window sample from the threshold, both forms of index / W
  nonfinite_<case>.heat (5, H, W), .ref_locs, .ref_scores: the maps of peaks_restatement.NONFINITE_MAPS, kept apart from ref_err

Legacy floor division (index / W as integer division, torch < 1.5) cannot be run through the reference under a current torch; the
legacy expectations rest on the restatement, which differs from the form pinned here only in `index // W`.

Conditions (asserted; a seed that violates one is replaced by the next -- the condition never changes, no case is dropped):
  * ref_err of every run is below 1e-4 px;
  * no non-zero window sample of any map lies within 1e-3 (relative) of the threshold.
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

REF_ERR_MAX = 1e-4
MARGIN_MIN = 1e-3
OUT = os.path.join(ROOT, "tests", "golden", "lifting", "peaks.npz")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def main(check=False):
    rh.install()
    rh.load_cfg(None)
    from modeling.backbones.basic_batch import find_tensor_peak_batch

    def reference(maps, radius, downsample, threshold):
        with torch.no_grad():
            locs, scores = find_tensor_peak_batch(torch.from_numpy(maps), radius, downsample, threshold)
        assert locs.dtype == torch.float32 and scores.dtype == torch.float32
        return locs.numpy(), scores.numpy()

    def evaluate(case, maps):
        """Every run of the case on these maps, or None when a condition fails."""
        radius = restate.CASES[case][2]
        runs = {}
        for c, downsample, threshold in restate.RUNS:
            if c != case:
                continue
            ref_locs, ref_scores = reference(maps, radius, downsample, threshold)
            f64, scores, index, margin = restate.peaks(maps, radius, downsample, threshold)
            legacy, scores_l, index_l, margin_l = restate.peaks(maps, radius, downsample, threshold, legacy_floor_division=True)
            assert same_bits(scores, ref_scores) and same_bits(scores_l, ref_scores) and (index == index_l).all()
            assert np.isfinite(ref_locs).all() and np.isfinite(f64).all() and np.isfinite(legacy).all()
            ref_err = np.abs(ref_locs.astype(np.float64) - f64).max()
            m = min(margin.min(), margin_l.min())
            if not (ref_err < REF_ERR_MAX and m >= MARGIN_MIN):
                print("%s: ref_err %.3g, margin %.3g" % (restate.run_name(c, downsample, threshold), ref_err, m))
                return None
            runs[restate.run_name(c, downsample, threshold)] = dict(
                params=np.array([radius, downsample, threshold]), ref_locs=ref_locs, ref_scores=ref_scores, f64_locs=f64,
                f64_locs_legacy=legacy, index=index, ref_err=np.float64(ref_err), margin=np.float64(m))
        return runs

    arrays = {}
    for ci, case in enumerate(restate.CASES):
        H, W, radius = restate.CASES[case]
        seed = 1000 * (ci + 1)
        while True:
            maps = restate.make_maps(case, seed)
            runs = evaluate(case, maps)
            if runs is not None:
                break
            print("%s: seed %d replaced" % (case, seed))
            seed += 1
        arrays[case + ".heat"] = maps
        kinds = restate.MAP_KINDS
        for name, run in runs.items():
            for k, v in run.items():
                arrays["%s.%s" % (name, k)] = v
            # what the maps were designed to reach
            idx, (ds, thr) = run["index"], run["params"][1:]
            spread, strided = restate.tie_indices(H, W)
            assert idx[kinds.index("constant")] == 0 and idx[kinds.index("ties_spread")] == spread[0] and idx[kinds.index("ties_strided")] == strided[0]
            assert run["ref_scores"][kinds.index("negative")] < 0
            if thr > 1e-8:
                t = kinds.index("tiny")
                assert same_bits(run["ref_locs"][t], restate.cell_location(0, W, ds)), run["ref_locs"][t]
            print("%-22s seed %d: ref_err %.3g px, margin %.3g, |loc| <= %.1f, bound %.3g" % (
                name, seed, run["ref_err"], run["margin"], np.abs(run["ref_locs"]).max(), restate.bound(run["ref_err"], run["ref_locs"])))
        for k, (y, x) in (("corner00", (0, 0)), ("corner01", (0, W - 1)), ("corner10", (H - 1, 0)), ("corner11", (H - 1, W - 1))):
            c = int(maps[kinds.index(k)].argmax())                    # the maximum lies in the corner cell or next to it
            assert abs(c // W - y) <= 1 and abs(c % W - x) <= 1, (case, k, c)

    for case in restate.NONFINITE_CASES:
        H, W, radius = restate.CASES[case]
        maps = restate.make_nonfinite_maps(case, 77)
        ref_locs, ref_scores = reference(maps, radius, 4.0, 1e-6)
        by = dict(zip(restate.NONFINITE_MAPS, zip(ref_locs, ref_scores)))
        for k in ("nan_far", "nan_cell0", "all_nan"):
            assert np.isnan(by[k][0]).all() and np.isnan(by[k][1]), (case, k, by[k])
        assert np.isnan(by["plus_inf"][0]).all() and by["plus_inf"][1] == np.inf
        assert by["all_minus_inf"][1] == -np.inf
        print("nonfinite %-12s all -inf: the reference's location %s" % (case, by["all_minus_inf"][0]))
        arrays["nonfinite_%s.heat" % case], arrays["nonfinite_%s.ref_locs" % case] = maps, ref_locs
        arrays["nonfinite_%s.ref_scores" % case] = ref_scores

    if check:
        stored = np.load(OUT, allow_pickle=False)
        assert sorted(stored.files) == sorted(arrays), "the stored fixture holds other arrays"
        for k, v in arrays.items():
            assert same_bits(stored[k], np.asarray(v)), k
        print("every array of %s regenerated bit for bit" % OUT)
        return
    np.savez_compressed(OUT, **arrays)
    assert all(v.dtype != object for v in np.load(OUT, allow_pickle=False).values())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(check="--check" in sys.argv[1:])
