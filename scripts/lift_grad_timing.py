"""Time forward + backward of one differentiable lift: the HIP liftings with with_grad=True (et_triangulate_views or
et_triangulate_epipolar, then et_triangulate_bwd) for pymvg, naive, refine, epipolar and epipolar_dlt, against the route a loss on
lifted points had before them -- triangulate.triangulate_dlt under torch autograd (torch.linalg.svd) -- in one process.

Shape: 32 frames x 4 views x 17 joints (profiles/lift_views.txt's), planted joints seen by jittered ring cameras with 1.5 px
noise, scores uniform in [0.5, 1) against CONF_THRES 0.85, RANSAC_THRES 35; corr_pos random on a 64 x 64 map.  One call = the lift,
then backward of (X * g).sum() into the detections; host wall clock around a synchronised call; min / max of 12 calls after 3
warm-up calls, the routes alternating.  A report, not a bar: writes profiles/lift_grad.txt (--out elsewhere).

    python scripts/lift_grad_timing.py [--out PATH]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, VIEWS, JOINTS, MAP, CALLS, WARMUP = 32, 4, 17, 64, 12, 3
CONF_THRES, RANSAC_THRES, DOWNSAMPLE = 0.85, 35.0, 16.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lift_grad.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU")
    from epipolar_transformers_amd import ops, synthetic as syn
    from epipolar_transformers_amd.triangulate import triangulate_dlt

    F, V, J = FRAMES, VIEWS, JOINTS
    rng = np.random.default_rng(0)
    krt = np.stack([syn.ring_cameras(V, MAP * DOWNSAMPLE, jitter=(0.02, 5.0), rng=rng) for _ in range(F)])
    X = np.array([0, 0, 900.0]) + rng.normal(0, 300, (F, J, 3))
    xh = np.einsum("fvik,fnk->fvni", krt, np.concatenate([X, np.ones((F, J, 1))], 2))
    cuda = lambda a: torch.tensor(a, dtype=torch.float32).cuda().contiguous()
    pts = cuda(xh[..., :2] / xh[..., 2:] + rng.normal(0, 1.5, (F, V, J, 2)))
    conf = cuda(rng.uniform(0.5, 1.0, (F, V, J)))
    KRT = cuda(krt)
    other = cuda(krt[:, np.roll(np.arange(V), -1)])
    corr = cuda(rng.uniform(0, MAP - 1, (F, V, MAP, MAP, 2)))
    g = torch.randn(F, J, 3, device="cuda", dtype=torch.float64, generator=torch.Generator(device="cuda").manual_seed(0))

    views = lambda m: lambda p: ops.triangulate_views(p, conf, KRT, method=m, conf_thres=CONF_THRES, ransac_thres=RANSAC_THRES, with_grad=True)
    epipolar = lambda dlt: lambda p: ops.triangulate_epipolar(p, conf, KRT, other, corr, downsample=DOWNSAMPLE, resize=1.0, conf_thres=CONF_THRES,
                                                              ransac_thres=RANSAC_THRES, dlt=dlt, with_grad=True)
    routes = {"torch autograd (triangulate.triangulate_dlt)": lambda p: triangulate_dlt(p, KRT, conf, conf_thres=CONF_THRES),
              "hip kernels, pymvg": views("pymvg"), "hip kernels, naive": views("naive"), "hip kernels, refine": views("refine"),
              "hip kernels, epipolar": epipolar(False), "hip kernels, epipolar_dlt": epipolar(True)}

    def step(route):
        p = pts.detach().requires_grad_(True)
        (route(p) * g).sum().backward()
        return p.grad

    times = {k: [] for k in routes}
    for i in range(WARMUP + CALLS):
        for name, route in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(route)
            torch.cuda.synchronize()
            if i >= WARMUP:
                times[name].append((time.perf_counter() - t0) * 1e3)
    lines = ["one lift, forward + backward into the detections: F=%d V=%d J=%d, CONF_THRES %g, RANSAC_THRES %g" % (F, V, J, CONF_THRES, RANSAC_THRES),
             "%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "host wall clock around a synchronised call, ms: min / max of %d calls after %d warm-up calls, routes alternating" % (CALLS, WARMUP)]
    for name, t in times.items():
        lines.append("  %-48s %8.3f / %8.3f" % (name, min(t), max(t)))
    names = list(routes)
    torch_min = min(times[names[0]])
    for name in names[1:]:
        k = min(times[name])
        lines.append("%s is %s: torch min over its min %.2f" % (name, "the faster route" if k < torch_min else "NOT the faster route", torch_min / k))
    # pymvg and the torch DLT are the same method: the two gradients side by side, and the kernel route twice
    a, b = step(routes["hip kernels, pymvg"]), step(routes[names[0]])
    lines.append("pymvg against the torch DLT: largest |difference| of the two gradients %.3e, largest |gradient| %.3e; the kernel route "
                 "twice: %s" % ((a - b).abs().max().item(), b.abs().max().item(),
                                "equal bits" if torch.equal(a, step(routes["hip kernels, pymvg"])) else "DIFFERENT bits"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
