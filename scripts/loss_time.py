"""Time the training loss, forward + backward, per KEYPOINT.LOSS kind: the HIP kernels with a dense target, the HIP kernels with the
target made on the fly from the points (ops.heatmap_loss), and the torch JointsMSELoss the model runs with EPIPOLAR_AMD.LOSS_KERNELS
off -- in one process on one GPU.

    python scripts/loss_time.py [--views 128] [--joints 17] [--size 64] [--out profiles/heatmap_loss.txt]

Host wall clock around a synchronised call, min / max of 12 after 5 warm-up calls (how README's other figures of this kind are
taken), and, third column, the time per call of 20 calls enqueued back to back between two device events.  A call is
loss = criterion(pred, ...) followed by loss.backward(); pred is a leaf that requires gradient.  The last line times
ops.heatmap_targets alone, the map stack the on-the-fly form never stores."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epipolar_transformers_amd import ops  # noqa: E402
from epipolar_transformers_amd.model import JointsMSELoss  # noqa: E402


def timed(step):
    times = []
    for _ in range(17):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    assert torch.isfinite(out).all()
    # ... and the same call 20 times back to back between two device events: the host runs ahead, as in a training loop
    first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    first.record()
    for _ in range(20):
        step()
    last.record()
    torch.cuda.synchronize()
    return min(times[5:]), max(times[5:]), first.elapsed_time(last) / 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=128)
    ap.add_argument("--joints", type=int, default=17)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--sigma", type=float, default=8.0)
    ap.add_argument("--downsample", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, J, S = a.views, a.joints, a.size
    rng = np.random.default_rng(0)
    pred = torch.tensor(rng.uniform(0, 1, (N, J, S, S)), dtype=torch.float32).cuda().requires_grad_(True)
    points = torch.tensor(rng.uniform(0, S * a.downsample, (N, J, 2)), dtype=torch.float64).cuda()
    vis = torch.tensor(rng.uniform(0, 1, (N, J)) < 0.9, dtype=torch.float32).cuda()
    target = ops.heatmap_targets(points, S, S, a.sigma, a.downsample)
    lines = ["training loss, forward + backward, N=%d J=%d %dx%d (%.1f MB per stack), sigma %g, downsample %g, %s, torch %s" % (
        N, J, S, S, pred.numel() * 4 / 1e6, a.sigma, a.downsample, torch.cuda.get_device_name(0), torch.__version__),
        "host wall clock around a synchronised call, min / max of 12 after 5 warm-up calls; per call of 20 back to back (device events); ms"]

    def step(criterion):
        def run():
            pred.grad = None
            loss = criterion()
            loss.backward()
            return loss
        return run

    fly = dict(points=points, sigma=a.sigma, downsample=a.downsample)
    torch_loss = JointsMSELoss()
    rows = [("joint", "torch JointsMSELoss (LOSS_KERNELS False)", lambda: torch_loss(pred, target, vis.view(N, J, 1)))]
    for kind in ("joint", "smoothmse", "mse"):
        w = None if kind == "mse" else vis
        rows.append((kind, "HIP kernels, dense target", lambda kind=kind, w=w: ops.heatmap_loss(pred, target, w, kind=kind)))
        rows.append((kind, "HIP kernels, target on the fly", lambda kind=kind, w=w: ops.heatmap_loss(pred, None, w, kind=kind, **fly)))
    for kind, what, criterion in rows:
        lines.append("%-9s %-42s %8.3f / %8.3f %8.3f" % ((kind, what) + timed(step(criterion))))
    lines.append("%-9s %-42s %8.3f / %8.3f %8.3f" % (("targets", "ops.heatmap_targets alone") +
                                                     timed(lambda: ops.heatmap_targets(points, S, S, a.sigma, a.downsample))))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
