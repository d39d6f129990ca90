"""Generate tests/golden/lifting/eval_metrics.npz from the REAL reference's JDR, calculate_err, calc_pck
(modeling/metrics/metrics2d.py:294-324, 199-235, 238-265, with get_max_preds of modeling/backbones/basic_batch.py:67-95 and
calc_dists / dist_acc) and EPEmean (modeling/metrics/metrics3d.py:5-46): the metrics of Modelbuilder.forward's test-time branch
that et_eval_jdr / et_eval_pck / et_eval_epe compute on the device.

Runs only where the reference tree is present (imported read-only through oracle/ref_harness.py).  What is executed is the
reference's own code; the inputs come from tests/eval_metrics_restatement.py's generators, and the restatement's results are
compared with the reference's here, bit for bit, before anything is written.

    python tests/golden/make_eval_metrics_golden.py

Legacy hazard.  Modelbuilder casts `visibility` to float32 (modeling/model.py:181) before it calls EPEmean.  Under a current torch
EPEmean then raises on BOTH of its branches: `~` on a float tensor, then -- in its `except` -- a uint8 tensor as an index mask.
This script calls it with a BOOLEAN visibility, which is what the first branch means.  It affects `perjointerr` only; the mean
never reads visibility.  EPEmean returns row 0 of `perjointerr`; to pin every row the batch is rolled so that each frame comes
first once (the mean is taken from the unrolled call).

Stored (arrays only, keys "<case>.<name>"):
  jdr_main (7,17,64,64), jdr_nonsquare (5,3,10,12), jdr_exact_half (4,2,20,20):
      pred, target float32 maps; thr; dists (J,N), acc (J+1) from JDR / calc_dists; pred_xy, target_xy from get_max_preds.
      jdr_nonsquare also holds acc_thr09 (thr 0.9 lies between one pixel along x, 1 / (10/10), and one along y, 1 / (12/10) --
      the reference divides x by the HEIGHT term, and only that order gives these values).  jdr_exact_half: every counted pair is
      one pixel apart or identical, so the distances are exactly 0.5 (NOT below the threshold) or 0.
  pck_main (7,17): locs float32, gt float64, vis float32 (one sample wholly invisible), thresholds, curve
      (np.linspace(0, MAX_TH, int(MAX_TH))), pck, err_joints, total_joints from calculate_err; calc_pck's values are asserted equal.
  epe_main (8,17): pred, gt float64, vis float32, unit 2.5, max_dist 150; mean, per_joint.

Cases the reference cannot produce are not here (tests pin them to the restatement): no joint that counts at all and no visible
item -- the reference divides zero by zero and raises.

Conditions on the inputs (asserted; a seed that violates one is replaced by the next, no case is dropped): every JDR distance
other than the designed exact 0.5 is at least 1e-6 from thr; every PCK error is at least 1e-6 from every threshold and curve
point, in float64.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]
from oracle import ref_harness as rh  # noqa: E402
import eval_metrics_restatement as restate  # noqa: E402

MARGIN = 1e-6
DEAD_JOINT = 5          # jdr_main: no sample counts for it (every target at x = 1)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def jdr_inputs(name, seed):
    rng = np.random.default_rng(seed)
    if name == "jdr_main":
        pred, target = restate.random_maps(7, 17, 64, 64, seed)
        xy = np.stack([np.ones(7, int), rng.integers(0, 64, 7)], -1)[:, None]
        target[:, DEAD_JOINT:DEAD_JOINT + 1] = restate.blob_maps(rng, xy, 64, 64)
    elif name == "jdr_nonsquare":
        # targets inside, predictions one pixel off along x, along y, along both, or on the spot
        t_xy = np.stack([rng.integers(2, 11, (5, 3)), rng.integers(2, 9, (5, 3))], -1)
        step = np.array([[1, 0], [0, 1], [1, 1], [0, 0], [-1, 0], [0, -1]])[rng.integers(0, 6, (5, 3))]
        step[0, 0], step[0, 1], step[0, 2] = (1, 0), (0, 1), (0, 0)
        pred, target = restate.blob_maps(rng, t_xy + step, 10, 12, 0.8), restate.blob_maps(rng, t_xy, 10, 12)
    else:
        t_xy = rng.integers(2, 18, (4, 2, 2))
        step = np.array([[1, 0], [0, 1], [-1, 0], [0, -1], [0, 0]])[rng.integers(0, 5, (4, 2))]
        step[0, 0], step[1, 0], step[0, 1] = (1, 0), (0, 0), (0, -1)
        pred, target = restate.blob_maps(rng, t_xy + step, 20, 20, 0.8), restate.blob_maps(rng, t_xy, 20, 20)
    return pred, target


def main():
    rh.install()
    rh.load_cfg(None, ["TEST.EPEMEAN_MAX_DIST", 150])
    from modeling.backbones.basic_batch import get_max_preds
    from modeling.metrics import metrics2d, metrics3d

    cases = {}

    def put(case, **arrays):
        for k, v in arrays.items():
            cases["%s.%s" % (case, k)] = np.asarray(v)

    # ---- JDR -----------------------------------------------------------------------------------------------------------------
    for ci, name in enumerate(("jdr_main", "jdr_nonsquare", "jdr_exact_half")):
        seed = 100 * (ci + 1)
        while True:
            pred, target = jdr_inputs(name, seed)
            dists, acc, pxy, txy = restate.jdr(pred, target)
            if restate.jdr_margin(dists) >= MARGIN and restate.jdr_margin(dists, 0.9) >= MARGIN:
                break
            print("%s: seed %d replaced" % (name, seed))
            seed += 1
        n, j, h, w = pred.shape
        ref_acc, ref_avg, ref_cnt, ref_pxy = metrics2d.JDR(pred, target)
        ref_txy, _ = get_max_preds(target)
        ref_dists = metrics2d.calc_dists(ref_pxy, ref_txy, np.ones((n, 2)) * np.array([h, w]) / 10)
        assert ref_acc[0] == ref_avg and ref_pxy.dtype == np.float32 and ref_dists.shape == (j, n)
        for what, ours, theirs in (("dists", dists, ref_dists), ("acc", acc, ref_acc), ("pred_xy", pxy, ref_pxy), ("target_xy", txy, ref_txy)):
            assert same_bits(ours, theirs), (name, what)
        put(name, pred=pred, target=target, thr=np.float64(0.5), dists=ref_dists, acc=ref_acc, pred_xy=ref_pxy, target_xy=ref_txy)
        counted = ref_dists != -1
        flat_p, flat_t = pred.reshape(n * j, -1), target.reshape(n * j, -1)
        twice = lambda f: int((((f == f.max(1, keepdims=True)).sum(1) > 1) & (f.max(1) > 0)).sum())
        print("%-15s seed %d: %d of %d items count, acc[0] %.4f, %d joints without a counted sample; maps without a positive value: "
              "pred %d target %d; maximum twice: pred %d target %d; exact 0.5: %d" % (
                  name, seed, counted.sum(), counted.size, ref_acc[0], (ref_acc[1:] == -1).sum(), (flat_p.max(1) <= 0).sum(),
                  (flat_t.max(1) <= 0).sum(), twice(flat_p), twice(flat_t), (ref_dists == 0.5).sum()))
        if name == "jdr_main":
            assert ref_acc[1 + DEAD_JOINT] == -1 and (flat_p.max(1) <= 0).any() and (flat_t.max(1) <= 0).any()
            assert twice(flat_p) and twice(flat_t) and ((ref_txy <= 1).any(-1) & (flat_t.max(1) > 0).reshape(n, j)).any()
            assert 0 < ref_acc[0] < 1 and not counted.all() and (ref_dists == 0.5).sum() == 0
        if name == "jdr_nonsquare":
            acc09 = metrics2d.JDR(pred, target, thr=0.9)[0]
            assert same_bits(acc09, restate.jdr(pred, target, 0.9)[1]) and not same_bits(acc09, ref_acc)
            assert ref_dists[0, 0] == 1.0 and abs(ref_dists[1, 0] - 1 / 1.2) < 1e-12 and ref_dists[2, 0] == 0.0     # x / (H/10), y / (W/10)
            put(name, acc_thr09=acc09)
        if name == "jdr_exact_half":
            assert counted.all() and set(np.unique(ref_dists)) == {0.0, 0.5} and ref_dists[0, 0] == 0.5 and ref_dists[0, 1] == 0.0
            assert ref_acc[1] == (ref_dists[0] == 0).mean()                     # 0.5 is not below 0.5

    # ---- PCK -----------------------------------------------------------------------------------------------------------------
    seed = 400
    while True:
        locs, gt, vis = restate.random_points2d(7, 17, seed)
        vis[3] = 0                                                              # a sample with nothing visible
        if restate.pck_margin(locs, gt, vis) >= MARGIN:
            break
        print("pck_main: seed %d replaced" % seed)
        seed += 1
    as_ref = lambda a: np.ascontiguousarray(a).transpose(0, 2, 1)               # N x 2 x J, as model.py:386-387 hands them over
    pcks, err_joints, total_joints = metrics2d.calculate_err(as_ref(locs), as_ref(gt), vis, restate.THRESHOLDS, restate.MAX_TH)
    only = metrics2d.calc_pck(as_ref(locs), as_ref(gt), vis, restate.THRESHOLDS)
    ref_pck = np.array([pcks["PCK@" + str(th)] for th in restate.THRESHOLDS], np.float64)
    assert same_bits(ref_pck, np.array([only["PCK@" + str(th)] for th in restate.THRESHOLDS], np.float64))
    hit, ej, tj = restate.pck(locs, gt, vis)
    assert same_bits(hit, ref_pck) and same_bits(ej, err_joints) and same_bits(tj, total_joints[:, 0])
    assert total_joints[3, 0] == 0 and (err_joints[3] == 0).all() and 0 < ref_pck[0] < ref_pck[-1] <= 100
    put("pck_main", locs=locs, gt=gt, vis=vis, thresholds=np.asarray(restate.THRESHOLDS, np.float64), curve=restate.curve_points(),
        pck=ref_pck, err_joints=err_joints, total_joints=total_joints[:, 0])
    print("pck_main        seed %d: PCK %s, %d of %d items visible" % (seed, np.round(ref_pck, 2).tolist(), (vis != 0).sum(), vis.size))

    # ---- EPEmean -------------------------------------------------------------------------------------------------------------
    pred, gt3, vis3 = restate.random_points3d(8, 17, 500)
    unit, max_dist = 2.5, 150.0
    tp, tg, tv = torch.from_numpy(pred), torch.from_numpy(gt3), torch.from_numpy(vis3 != 0)[..., None]
    mean, _ = metrics3d.EPEmean(tp, tg, tv, unit=unit)
    rows = [metrics3d.EPEmean(tp.roll(-f, 0), tg.roll(-f, 0), tv.roll(-f, 0), unit=unit)[1].numpy() for f in range(8)]
    ref_mean, ref_rows = np.float64(mean.item()), np.stack(rows)
    our_mean, our_rows = restate.epe(pred, gt3, vis3, unit, max_dist)
    errors = restate.epe_errors(pred, gt3, unit, max_dist)
    assert same_bits(our_rows, ref_rows) and abs(our_mean - ref_mean) <= restate.mean_bound(errors)
    assert (errors == max_dist).any() and (errors < max_dist).any() and (ref_rows == 0).any()
    put("epe_main", pred=pred, gt=gt3, vis=vis3, unit=np.float64(unit), max_dist=np.float64(max_dist), mean=ref_mean, per_joint=ref_rows)
    print("epe_main        mean %.6f (restatement differs by %.3g, bound %.3g), %d of %d items clamped" % (
        ref_mean, abs(our_mean - ref_mean), restate.mean_bound(errors), (errors == max_dist).sum(), errors.size))

    out = os.path.join(ROOT, "tests", "golden", "lifting", "eval_metrics.npz")
    np.savez_compressed(out, **cases)
    assert all(v.dtype != object for v in np.load(out, allow_pickle=False).values())
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
