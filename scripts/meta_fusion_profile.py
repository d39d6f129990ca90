"""The Meta fusion layer's data pass, `ops.meta_fuse` (et_meta_pack + et_meta_gemm; backward et_meta_gemm on the transposed packs +
et_meta_wgrad), against the same operation in stock torch -- torch.bmm with the per-pair weights + the shared 1x1 convolution + the
adds, what the reference's loop of conv2d calls amounts to -- measured, both routes on one visit.

Shape: N = 128 pairs of 64 x 64 x 256 maps, channels last.  Forward alone, and forward + backward of (x * g).sum() into src, the
per-pair weights, the shared weight and bias, and feat.  Host wall clock around a synchronised call, min / max of 12 calls after 3
warm-up calls, the routes alternating, in a child process under a time limit (a step that faults or hangs ends the run).  A report,
not a bar: writes profiles/meta_fusion.txt (--out elsewhere); --append FILE adds the lines of FILE (the errors tests/test_gpu_meta.py
prints, made on the same visit) behind them.

    python scripts/meta_fusion_profile.py [--out PATH] [--append FILE]
"""
import argparse
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, HW, C, CALLS, WARMUP, LIMIT = 128, 64, 256, 12, 3, 300


def _time(routes):
    times = {k: [] for k in routes}
    for i in range(WARMUP + CALLS):
        for name, route in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = route()
            torch.cuda.synchronize()
            if i >= WARMUP:
                times[name].append((time.perf_counter() - t0) * 1e3)
            del out
    return times


def run():
    from epipolar_transformers_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)
    src, feat, g = rnd(N, HW * HW, C).relu_(), rnd(N, HW * HW, C), rnd(N, HW * HW, C)
    weight, share, bias = rnd(N, C, C) * 0.05, rnd(C, C, 1, 1) / 16, rnd(C) * 0.05

    def torch_fwd(s, w, sw, sb, f):
        # ret_n = W_n . other_n (bmm) + share(other) (the 1x1 convolution as one matmul) + b_share, then + feat
        return torch.bmm(s, w.transpose(1, 2)) + torch.matmul(s, sw.view(C, C).t()) + sb + f

    def step(fn):
        leaves = [t.detach().requires_grad_() for t in (src, weight, share, bias, feat)]
        (fn(*leaves) * g).sum().backward()
        return [t.grad for t in leaves]

    with torch.no_grad():
        fwd = _time({"torch": lambda: torch_fwd(src, weight, share, bias, feat), "meta_fuse": lambda: ops.meta_fuse(src, weight, share, bias, feat)})
        a, b = torch_fwd(src, weight, share, bias, feat), ops.meta_fuse(src, weight, share, bias, feat)
    both = _time({"torch": lambda: step(torch_fwd), "meta_fuse": lambda: step(ops.meta_fuse)})
    ga, gb = step(torch_fwd), step(ops.meta_fuse)
    for title, t in (("forward", fwd), ("forward + backward", both)):
        print("%s:" % title)
        for name, v in t.items():
            print("  %-10s %8.3f / %8.3f ms" % (name, min(v), max(v)))
        print("  torch min over meta_fuse min %.3f" % (min(t["torch"]) / min(t["meta_fuse"])))
    print("x of the two routes: largest |difference| %.3e, largest |x| %.3e" % ((a - b).abs().max().item(), a.abs().max().item()))
    for name, p, q in zip(("src", "weight", "share_weight", "share_bias", "feat"), ga, gb):
        print("d %-13s largest |difference| %.3e, largest |gradient| %.3e" % (name + ":", (p - q).abs().max().item(), p.abs().max().item()))
    print("touching every map once, the forward moves %.2f GB and multiplies %.1f GFLOP" %
          ((3 * src.numel() * 4 + weight.numel() * 4) / 1e9, 2.0 * N * HW * HW * C * C / 1e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meta_fusion.txt"))
    ap.add_argument("--append", default=None)
    ap.add_argument("--child", action="store_true", help="(internal) run the measurement in this process")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU")
    if args.child:
        return run()
    text = ["ops.meta_fuse against torch (bmm + shared 1x1 convolution + adds): N=%d pairs, %d x %d x %d maps, channels last" % (N, HW, HW, C),
            "%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
            "host wall clock around a synchronised call, ms: min / max of %d calls after %d warm-up calls, routes alternating, one visit" % (CALLS, WARMUP)]
    try:
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True, timeout=LIMIT)
        text.append(proc.stdout.rstrip())
        if proc.returncode != 0:
            text.append("exit status %d\n%s" % (proc.returncode, proc.stderr.rstrip()[-2000:]))
    except subprocess.TimeoutExpired:
        text.append("no result within %d s" % LIMIT)
    if args.append and os.path.exists(args.append):
        text.append(open(args.append).read().rstrip())
    out = "\n".join(text) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(out)
    print(out, end="")


if __name__ == "__main__":
    main()
