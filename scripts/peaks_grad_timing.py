"""Time forward + backward of the differentiable peak finder, ops.heatmap_peaks(with_grad=True) (et_heatmap_peaks and
et_heatmap_peaks_bwd), against torch autograd through backbones.soft_argmax_peaks on the same tensor, in one process.

Shape: 128 views x 17 joints of 64 x 64, radius = KEYPOINT.SIGMA and downsample = BACKBONE.DOWNSAMPLE of the default config.
One call = forward, then backward of (locs * g).sum() + (scores * h).sum() into the maps; host wall clock around a synchronised
call; min / max of 12 calls after 3 warm-up calls, the two routes alternating.  A report, not a bar: writes
profiles/peaks_grad.txt (--out elsewhere).

    python scripts/peaks_grad_timing.py [--out PATH]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWS, JOINTS, SIZE, CALLS, WARMUP = 128, 17, 64, 12, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peaks_grad.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU")
    from epipolar_transformers_amd import backbones, default_cfg, ops

    cfg = default_cfg()
    radius, downsample = float(cfg.KEYPOINT.SIGMA), float(cfg.BACKBONE.DOWNSAMPLE)
    gen = torch.Generator(device="cuda").manual_seed(0)
    # a bump per map on a noise floor, as a trained head leaves it
    yy, xx = torch.meshgrid(torch.arange(SIZE, device="cuda"), torch.arange(SIZE, device="cuda"), indexing="ij")
    centre = torch.rand(VIEWS, JOINTS, 2, device="cuda", generator=gen) * (SIZE - 1)
    d2 = (yy - centre[..., 1, None, None]) ** 2 + (xx - centre[..., 0, None, None]) ** 2
    maps = (0.8 * torch.exp(-d2 / (2 * radius)) + 0.005 * torch.rand(VIEWS, JOINTS, SIZE, SIZE, device="cuda", generator=gen)).contiguous()
    g = torch.randn(VIEWS, JOINTS, 2, device="cuda", generator=gen)
    h = torch.randn(VIEWS, JOINTS, device="cuda", generator=gen)

    def step(route):
        hm = maps.detach().requires_grad_(True)
        locs, scores = route(hm)
        ((locs * g).sum() + (scores * h).sum()).backward()
        return hm.grad

    routes = {"hip kernels (ops.heatmap_peaks, with_grad=True)": lambda hm: ops.heatmap_peaks(hm, radius, downsample, with_grad=True),
              "torch autograd (backbones.soft_argmax_peaks)": lambda hm: backbones.soft_argmax_peaks(hm, radius, downsample)}
    times = {k: [] for k in routes}
    for i in range(WARMUP + CALLS):
        for name, route in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            grad = step(route)
            torch.cuda.synchronize()
            if i >= WARMUP:
                times[name].append((time.perf_counter() - t0) * 1e3)
    a, b = (step(r) for r in routes.values())
    lines = ["peak finder, forward + backward: %d x %d maps of %d x %d, radius %g, downsample %g, float32" % (VIEWS, JOINTS, SIZE, SIZE, radius, downsample),
             "%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "host wall clock around a synchronised call, ms: min / max of %d calls after %d warm-up calls, routes alternating" % (CALLS, WARMUP)]
    for name, t in times.items():
        lines.append("  %-52s %8.3f / %8.3f" % (name, min(t), max(t)))
    k, t = (min(times[n]) for n in routes)
    lines.append("the kernel pair is %s: min over min %.2f" % ("the faster one" if k < t else "NOT the faster one", t / k))
    lines.append("largest |difference| of the two gradients %.3e, largest |gradient| %.3e; the kernel route twice: %s" % (
        (a - b).abs().max().item(), b.abs().max().item(), "equal bits" if torch.equal(a, step(list(routes.values())[0])) else "DIFFERENT bits"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
