"""Gathered against indexed: what naming the pairs by index into the trunk's stack of maps (EPIPOLAR_AMD.PAIR_INDEX, the *_ix entry
points) saves over gathering a private copy of every pair's maps with torch first -- measured, both routes on one visit.

Shape: 32 frames x 4 views, 64 x 64 x 256 maps, K = 64, the ring rig (every view's source is its ring neighbour); one stack of
128 maps, channels last, as the trunk leaves it.  Three workloads, each in a process of its own under its own time limit (a step that
faults or hangs ends the run: nothing is started on the device behind it):

  views-eval      the eval layer of MultiViewPoseModel.forward_views: feature[source_index] + Epipolar.forward_fused, against
                  forward_fused(feature, feature, src_index=source_index) (et_epipolar_forward_fused_ix)
  views-train     forward + tile backward of the same pairs: ops.EpipolarAttend on (feature, feature[source_index]) against
                  ops.EpipolarAttendIndexed on the stack, then backward of (out * g).sum() into the stack
  multitest       forward_multitest's layer call: all 32 x 4 x 3 (reference, source) pairs, both operands gathered, against both
                  named by index; with torch.cuda.max_memory_allocated over the call

Host wall clock around a synchronised call, min / max of 12 calls after 3 warm-up calls, the routes alternating.  A report, not a
bar: writes profiles/pair_index.txt (--out elsewhere); --append FILE adds the lines of FILE (the bench.py comparison of the existing
path against the parent commit, made on the same visit) behind them.

    python scripts/pair_index_profile.py [--out PATH] [--append FILE]
"""
import argparse
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, VIEWS, HW, C, K, CALLS, WARMUP = 32, 4, 64, 256, 64, 12, 3
CASES = {"views-eval": 240, "views-train": 240, "multitest": 300}        # case -> its time limit, seconds


def _layer():
    from epipolar_transformers_amd import default_cfg
    from epipolar_transformers_amd.epipolar import Epipolar

    cfg = default_cfg()
    cfg.merge_from_list(["KEYPOINT.HEATMAP_SIZE", (HW, HW), "KEYPOINT.NFEATS", C, "EPIPOLAR.SAMPLESIZE", K, "EPIPOLAR.ATTENTION", "avg",
                         "EPIPOLAR.PARAMETERIZED", ("z",), "EPIPOLAR.ZRESIDUAL", True, "EPIPOLAR.USE_CORRECT_NORMALIZE", True])
    torch.manual_seed(0)
    mod = Epipolar(cfg=cfg).cuda().eval()
    with torch.no_grad():
        mod.bn.weight.normal_(1, 0.1)
        mod.bn.bias.normal_(0, 0.1)
    return mod


def _time(routes):
    """{name: [ms]} (and {name: peak bytes above what was allocated before the call}) of the alternating routes."""
    times, peaks = {k: [] for k in routes}, {k: 0 for k in routes}
    for i in range(WARMUP + CALLS):
        for name, route in routes.items():
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            out = route()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                times[name].append(ms)
                peaks[name] = max(peaks[name], torch.cuda.max_memory_allocated() - before)
            del out
    return times, peaks


def run_case(case):
    from epipolar_transformers_amd import camera, ops, synthetic as syn
    from epipolar_transformers_amd.model import ring_sources

    m = FRAMES * VIEWS
    gen = torch.Generator(device="cuda").manual_seed(1)
    feature = torch.randn(m, C, HW, HW, device="cuda", generator=gen).relu_().contiguous(memory_format=torch.channels_last)
    P_ref, P_src = syn.make_pairs(FRAMES, VIEWS, HW * 4, seed=0, jitter=(0.05, 8.0))
    src = ring_sources(FRAMES, VIEWS)                               # host index: what forward_views is handed
    mod = _layer()
    lines, same = [], None
    if case == "views-eval":
        with torch.no_grad():
            routes = {"gathered": lambda: mod.forward_fused(feature, feature[src], P_ref, P_src)[0],
                      "indexed": lambda: mod.forward_fused(feature, feature, P_ref, P_src, src_index=src)[0]}
            times, peaks = _time(routes)
            same = torch.equal(routes["gathered"](), routes["indexed"]())
    elif case == "views-train":
        spec = mod.layer_spec()
        cam = camera.pair_algebra(P_ref, P_src).cuda()
        g = torch.randn(m, C, HW, HW, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)

        def step(indexed):
            pool = feature.detach().requires_grad_(True)
            if indexed:
                out = ops.EpipolarAttendIndexed.apply(pool, pool, cam, spec, None, src)[0]
            else:
                out = ops.EpipolarAttend.apply(pool, pool[src], cam, spec)[0]
            (out * g).sum().backward()
            return pool.grad

        routes = {"gathered": lambda: step(False), "indexed": lambda: step(True)}
        times, peaks = _time(routes)
        a, b = routes["gathered"](), routes["indexed"]()
        lines.append("  the two gradients of the stack: largest |difference| %.3e, largest |gradient| %.3e" %
                     ((a - b).abs().max().item(), a.abs().max().item()))
    else:
        base = torch.arange(m).view(FRAMES, VIEWS)
        ref_idx = torch.cat([base.reshape(-1) for _ in range(1, VIEWS)])
        src_idx = torch.cat([base.roll(-shift, 1).reshape(-1) for shift in range(1, VIEWS)])
        P = syn.ring_cameras(VIEWS, HW * 4)
        P = torch.from_numpy(P).float().repeat(FRAMES, 1, 1)
        Pr, Ps = P[ref_idx], P[src_idx]
        rd, sd = ref_idx.cuda(), src_idx.cuda()
        with torch.no_grad():
            routes = {"gathered": lambda: mod.forward_fused(feature[rd], feature[sd], Pr, Ps)[0],
                      "indexed": lambda: mod.forward_fused(feature, feature, Pr, Ps, ref_index=ref_idx, src_index=src_idx)[0]}
            times, peaks = _time(routes)
            same = torch.equal(routes["gathered"](), routes["indexed"]())
    pairs = len(src) if case != "multitest" else m * (VIEWS - 1)
    print("%s: %d pairs from a stack of %d maps" % (case, pairs, m))
    for name, t in times.items():
        print("  %-10s %8.3f / %8.3f ms        peak above the call's start %8.1f MB" % (name, min(t), max(t), peaks[name] / 1e6))
    g_min, i_min = min(times["gathered"]), min(times["indexed"])
    print("  indexed is %s: gathered min over indexed min %.3f; peak %.1f MB lower" %
          ("not slower" if i_min <= g_min else "SLOWER", g_min / i_min, (peaks["gathered"] - peaks["indexed"]) / 1e6))
    if same is not None:
        print("  x of the two routes: %s" % ("equal bits" if same else "DIFFERENT bits"))
    for line in lines:
        print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_index.txt"))
    ap.add_argument("--append", default=None)
    ap.add_argument("--case", choices=list(CASES), default=None, help="(internal) run one workload in this process")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU")
    if args.case:
        return run_case(args.case)
    text = ["gathered against indexed pairs: F=%d V=%d, %d x %d x %d maps, K=%d, ring sources" % (FRAMES, VIEWS, HW, HW, C, K),
            "%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
            "host wall clock around a synchronised call, ms: min / max of %d calls after %d warm-up calls, routes alternating, one visit" % (CALLS, WARMUP)]
    for case, limit in CASES.items():
        try:
            proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case], stdout=subprocess.PIPE,
                                  stderr=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            text.append("%s: no result within %d s; nothing further was run" % (case, limit))
            break
        text.append(proc.stdout.rstrip())
        if proc.returncode != 0:
            text.append("%s: exit status %d; nothing further was run\n%s" % (case, proc.returncode, proc.stderr.rstrip()[-2000:]))
            break
    if args.append and os.path.exists(args.append):
        text.append(open(args.append).read().rstrip())
    out = "\n".join(text) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(out)
    print(out, end="")


if __name__ == "__main__":
    main()
