"""Time one MultiViewPoseModel.lift per KEYPOINT.TRIANGULATION method: pymvg / naive / refine through their HIP kernels
(EPIPOLAR_AMD.LIFT_KERNELS True) and the batched torch DLT they replace (knob off), in one process on one GPU.

    python scripts/lift_time.py [--frames 32] [--views 4] [--joints 17] [--out profiles/lift_views.txt]

Host wall clock around a synchronised call, min / max of 12 after 5 warm-up calls (how README's other lifting figures are taken).
Detections: planted joints seen by jittered ring cameras with 1.5 px noise; scores uniform in [0.5, 1) against CONF_THRES 0.85, so
joints differ in how many views they select and some need the threshold lowered."""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epipolar_transformers_amd import default_cfg, synthetic as syn  # noqa: E402
from epipolar_transformers_amd.model import MultiViewPoseModel  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--joints", type=int, default=17)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F, V, J = a.frames, a.views, a.joints
    rng = np.random.default_rng(0)
    krt = np.stack([syn.ring_cameras(V, 1024.0, jitter=(0.02, 5.0), rng=rng) for _ in range(F)])
    X = np.array([0, 0, 900.0]) + rng.normal(0, 300, (F, J, 3))
    xh = np.einsum("fvik,fnk->fvni", krt, np.concatenate([X, np.ones((F, J, 1))], 2))
    locs = torch.tensor(xh[..., :2] / xh[..., 2:] + rng.normal(0, 1.5, (F, V, J, 2)), dtype=torch.float32).cuda().view(F * V, J, 2)
    scos = torch.tensor(rng.uniform(0.5, 1.0, (F * V, J)), dtype=torch.float32).cuda()
    KRT = torch.tensor(krt, dtype=torch.float32).cuda().view(F * V, 3, 4)
    lines = ["one lift, F=%d V=%d J=%d, CONF_THRES 0.85, RANSAC_THRES 35, %s, torch %s" % (
        F, V, J, torch.cuda.get_device_name(0), torch.__version__),
        "host wall clock around a synchronised call, min / max of 12 after 5 warm-up calls, ms"]
    for method, knob in (("pymvg", False), ("pymvg", True), ("naive", True), ("refine", True)):
        cfg = default_cfg()
        cfg.merge_from_list(["KEYPOINT.TRIANGULATION", method, "KEYPOINT.CONF_THRES", 0.85, "KEYPOINT.RANSAC_THRES", 35,
                             "EPIPOLAR_AMD.LIFT_KERNELS", knob])
        lift = lambda: MultiViewPoseModel.lift(types.SimpleNamespace(cfg=cfg), locs, scos, KRT, V)
        times = []
        for i in range(17):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = lift()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        assert torch.isfinite(out).all()
        times = times[5:]
        lines.append("%-7s %-34s %8.3f / %8.3f" % (method, "HIP kernel (LIFT_KERNELS True)" if knob else "torch DLT (LIFT_KERNELS False)",
                                                    min(times), max(times)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
