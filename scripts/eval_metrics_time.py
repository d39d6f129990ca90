"""Time the test-time metrics of Modelbuilder.forward: the three HIP calls (ops.eval_jdr + ops.eval_pck + ops.eval_epe) against the
route a user had without them -- copy both heat-map stacks to the host and run the NumPy restatement of JDR, calculate_err and
EPEmean (tests/eval_metrics_restatement.py, vectorised: the reference's own Python loops over N * J items are slower still).

    python scripts/eval_metrics_time.py [--views 128] [--joints 17] [--size 64] [--frames 32] [--out profiles/eval_metrics.txt]

Host wall clock around a synchronised call, min / max of 12 after 5 warm-up calls, one process on one GPU."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import eval_metrics_restatement as restate  # noqa: E402
from epipolar_transformers_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=128)
    ap.add_argument("--joints", type=int, default=17)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, J, S, F = a.views, a.joints, a.size, a.frames
    gpu = lambda x: None if x is None else torch.from_numpy(x).cuda()
    pred, target = [gpu(x) for x in restate.random_maps(N, J, S, S, seed=0)]
    locs, gt2, vis = [gpu(x) for x in restate.random_points2d(N, J, seed=0)]
    pred3, gt3, vis3 = [gpu(x) for x in restate.random_points3d(F, J, seed=0)]

    def kernels():
        return ops.eval_jdr(pred, target), ops.eval_pck(locs, gt2, vis), ops.eval_epe(pred3, gt3, vis3, unit=1.0, max_dist=150.0)

    def host_route():
        host = lambda t: t.cpu().numpy()
        return (restate.jdr(host(pred), host(target)), restate.pck(host(locs), host(gt2), host(vis)),
                restate.epe(host(pred3), host(gt3), host(vis3), 1.0, 150.0))

    lines = ["metrics of N=%d views x J=%d joints, %dx%d maps (%.1f MB for both stacks), F=%d frames, %s, torch %s" % (
        N, J, S, S, 2 * pred.numel() * 4 / 1e6, F, torch.cuda.get_device_name(0), torch.__version__),
        "host wall clock around a synchronised call, min / max of 12 after 5 warm-up calls, ms"]
    for name, fn in (("ops.eval_jdr + eval_pck + eval_epe (HIP kernels)", kernels), ("D2H copy of both stacks + NumPy restatement", host_route)):
        times = []
        for _ in range(17):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        times = times[5:]
        lines.append("%-52s %9.3f / %9.3f" % (name, min(times), max(times)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
