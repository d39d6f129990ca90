"""Generate tests/golden/training/heatmap_loss.npz from the REAL reference's Heatmapcreator (data/transforms/keypoints2d.py:3-36) and
its three criteria -- JointsMSELoss, KeypointsMSESmoothLoss, MaskedMSELoss through compute_stage_loss
(modeling/metrics/metrics2d.py:18-90) -- with their gradients for the prediction by autograd on the CPU: what et_heatmap_targets,
et_heatmap_loss and et_heatmap_loss_bwd compute on the device.

Runs only where the reference tree is present (imported read-only through oracle/ref_harness.py).  What is executed is the
reference's own code; the inputs come from tests/heatmap_loss_restatement.py's generator, and the restatement's results are compared
with the reference's here before anything is written.

    python tests/golden/make_heatmap_loss_golden.py

Hazards.  JointsMSELoss needs weights of shape (N,J,1), KeypointsMSESmoothLoss (N,J) -- with (N,J,1) its `target_weight[..., None]`
broadcasts to four dimensions and raises; each is called with the shape it accepts.  With LOSS mse the reference's H36M branch
calls a two-argument lambda with three arguments and raises; mse is pinned to the other call, criterion(scoremap, batch_heatmaps)
(modeling/model.py:256-258), which is compute_stage_loss on a one-map list with masks=None.

Stored (arrays only, keys "<case>.<name>"), for the cases of heatmap_loss_restatement.CASES:
  pred (N,J,H,W) float32, points (N,J,2) float64, weight (N,J) float32, sigma, downsample;
  targets (N,J,H,W) float32: Heatmapcreator.get's float64 maps cast as Modelbuilder's .to(torch.float32) casts them;
  loss.joint, loss.joint_per_joint, loss.smoothmse, loss.mse: float32 scalars;
  grad.joint, grad.smoothmse, grad.mse (N,J,H,W) float32 -- for every case but `main` (the file stays small);
  smooth_hot.grad_ulps: the measured maximum, in float32 ulps, between the reference's and the restatement's smoothmse gradient
  above the threshold; smooth_hot.hot: how many terms lie above it.

Conditions (asserted; a seed that violates one is replaced by the next, no case is dropped):
  1  the restatement's float64 targets equal the reference's, bit for bit;
  2  no target value lies within relative 2**-45 of a float32 rounding midpoint (so any exp within about 100 ulp of float64, and
     a contracted r*r + c*c, rounds to the same float32);
  3  each reference loss lies within relative (M + J + 1) * 2**-24 of the restatement, M the number of terms of one mean;
  4  each reference gradient element lies within 2 ulp of float32 of the restatement for joint, mse and smoothmse below the
     threshold (the reference makes three float32 roundings), and is an exact zero where w = 0;
  5  above the smoothmse threshold, where torch's float32 pow is in the chain, within 8 ulp (a measured figure);
  and on the inputs: a weight of 0 and a fractional one in every case of more than one map, blobs cut by every edge and a map
  that is all background in the cases of six maps and more, 2-3 % of smooth_hot's smoothmse terms above 400."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]
from oracle import ref_harness as rh  # noqa: E402
import heatmap_loss_restatement as restate  # noqa: E402

MIDPOINT = 2.0 ** -45


class Retry(Exception):
    pass


def need(ok, why):
    if not ok:
        raise Retry(why)


def reference_results(metrics2d, cfg, creator, name, pred, points, weight):
    n, j, h, w, sigma, downsample = restate.CASES[name]
    maker = creator((h, w), sigma, downsample)
    maps = np.stack([maker.get(points[i]) for i in range(n)])
    assert maps.dtype == np.float64 and maps.shape == (n, j, h, w)
    tgt = torch.from_numpy(maps).to(torch.float32)

    def run(criterion, *args):
        p = torch.from_numpy(pred).clone().requires_grad_(True)
        value = criterion(p, *args)
        value.backward()
        return np.float32(value.item()), p.grad.numpy().copy()

    wt = torch.from_numpy(weight)
    out = {}
    cfg.defrost()
    cfg.KEYPOINT.LOSS_PER_JOINT = False
    out["joint"] = run(metrics2d.JointsMSELoss(), tgt, wt.reshape(n, j, 1))
    cfg.KEYPOINT.LOSS_PER_JOINT = True
    out["joint_per_joint"] = run(metrics2d.JointsMSELoss(), tgt, wt.reshape(n, j, 1))
    cfg.KEYPOINT.LOSS_PER_JOINT = False
    out["smoothmse"] = run(metrics2d.KeypointsMSESmoothLoss(), tgt, wt.reshape(n, j))
    out["mse"] = run(lambda p, t: metrics2d.compute_stage_loss(metrics2d.MaskedMSELoss(), t, [p])[0], tgt)
    return maps, tgt.numpy(), out


def check_case(name, pred, points, weight, maps, tgt, ref):
    n, j, h, w, sigma, downsample = restate.CASES[name]
    shape = (n, j, h, w)
    # inputs
    if n * j > 1:
        need((weight == 0).any() and ((weight > 0) & (weight < 1)).any(), "weights")
    if n * j >= 6:
        background = np.float32(np.exp(-restate.CLIP))
        need((tgt.reshape(n * j, -1) == background).all(1).any(), "no all-background map")
        blob = tgt > background
        need(all(e.any() for e in (blob[..., 0, :], blob[..., -1, :], blob[..., :, 0], blob[..., :, -1])), "an edge cuts no blob")
    # 1, 2
    ours = restate.targets(points, h, w, sigma, downsample)
    need(ours.tobytes() == maps.tobytes(), "condition 1: targets differ")
    need(restate.midpoint_distance(maps) >= MIDPOINT, "condition 2: a target next to a float32 midpoint")
    report = {}
    for kind in restate.KINDS:
        wk = None if kind == "mse" else weight
        for per_joint in ((False, True) if kind == "joint" else (False,)):
            key = kind + ("_per_joint" if per_joint else "")
            value, g = ref[key]
            mine = restate.loss(kind, pred, tgt, wk, per_joint)
            need(abs(float(value) - float(mine)) <= restate.loss_bound(kind, shape, mine), "condition 3: %s" % key)
            report["loss " + key] = abs(float(value) - float(mine)) / abs(float(mine)) * 2.0 ** 24
            gm = restate.grad(kind, pred, tgt, wk, per_joint)
            apart = restate.ulps_apart(g, gm)
            if kind == "smoothmse":
                hot = restate.smooth_raw(*restate.difference(kind, pred, tgt, wk)) > np.float32(restate.THRESHOLD)
                if name == "smooth_hot":
                    share = hot.mean()
                    need(0.02 <= share <= 0.03, "%.4f of the smoothmse terms above the threshold" % share)
                    need(apart[hot].max() <= 8, "condition 5: %.2f ulp" % apart[hot].max())
                    report["hot"], report["grad_ulps"] = int(hot.sum()), float(apart[hot].max())
                else:
                    need(not hot.any(), "a term above the smoothmse threshold outside smooth_hot")
                apart = apart[~hot]
            need(apart.max() <= 2, "condition 4: %s %.2f ulp" % (key, apart.max()))
            report["grad " + key] = float(apart.max())
            if wk is not None:
                zero = np.broadcast_to((weight == 0)[..., None, None], shape)
                need((g[zero] == 0).all() and (gm[zero] == 0).all(), "w = 0 without an exact zero gradient")
    return report


def main():
    rh.install()
    cfg = rh.load_cfg(None)
    from data.transforms.keypoints2d import Heatmapcreator
    from modeling.metrics import metrics2d

    cases = {}
    for ci, name in enumerate(restate.CASES):
        seed = 1000 * (ci + 1)
        while True:
            pred, points, weight = restate.case_inputs(name, seed)
            maps, tgt, ref = reference_results(metrics2d, cfg, Heatmapcreator, name, pred, points, weight)
            try:
                report = check_case(name, pred, points, weight, maps, tgt, ref)
                break
            except Retry as why:
                print("%s: seed %d replaced (%s)" % (name, seed, why))
                seed += 1
        n, j, h, w, sigma, downsample = restate.CASES[name]
        put = lambda k, v: cases.__setitem__("%s.%s" % (name, k), np.asarray(v))
        put("pred", pred), put("points", points), put("weight", weight), put("targets", tgt)
        put("sigma", np.float64(sigma)), put("downsample", np.float64(downsample))
        for key, (value, g) in ref.items():
            put("loss." + key, np.float32(value))
            if name != "main" and key != "joint_per_joint":
                put("grad." + key, g.astype(np.float32))
        if name == "smooth_hot":
            put("grad_ulps", np.float64(report["grad_ulps"])), put("hot", np.int64(report["hot"]))
        print("%-10s seed %d: nearest float32 midpoint 2^%.1f; %s" % (
            name, seed, np.log2(restate.midpoint_distance(maps)), ", ".join("%s %.3g" % kv for kv in sorted(report.items()))))

    out = os.path.join(ROOT, "tests", "golden", "training", "heatmap_loss.npz")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **cases)
    assert all(v.dtype != object for v in np.load(out, allow_pickle=False).values())
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
