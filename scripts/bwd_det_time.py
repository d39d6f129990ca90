#!/usr/bin/env python
"""Time the three backward forms that matter for reproducible training, in ONE process:

    tile      MFMA tiles, float atomics (the default; reproducible to rounding only)
    tile_det  the same tiles, 64-bit fixed-point sums with integer atomics (bit-reproducible)
    gather    coefficient entries + ordered per-row sums (bit-reproducible; the yardstick)

at Config 2 (128 pairs, 64 x 64, K 64) and Config 4 (96 x 96) on the ring, and on the rigs ring / epipole_inside / h36m_room at
64 x 64 -- there also tile_det with ET_VARIANT_BWD_SPLIT_IN_PLACE (every over-capacity tile split in place instead of deferred:
the other input-only partition rule).  Device events around every call, warm-up, >= 12 timed calls, min / p50 / max.

    python scripts/bwd_det_time.py [--reps 12] [--pairs 128]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epipolar_transformers_amd import _lib, camera, ops, synthetic as syn  # noqa: E402

C = 256


def call_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[0], t[len(t) // 2], t[-1]


def case(rig, n, h, k, reps, split_too):
    dev = torch.device("cuda:0")
    per = 4 if rig in ("ring", "h36m_room") else 2
    P1, P2 = syn.rig_pairs(rig, (n + per - 1) // per, 4 * h, seed=1000, jitter=(0.05, 8.0))
    cam = camera.pair_algebra(P1[:n], P2[:n]).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    ref = torch.randn(n, h, h, C, device=dev, generator=g).relu_()
    src = torch.randn(n, h, h, C, device=dev, generator=g).relu_()
    go = torch.randn(n, h, h, C, device=dev, generator=g)
    spec = ops.LayerSpec(H=h, W=h, K=k)
    attn = ops.forward_nhwc(spec, ref, src, cam)[1]
    forms = [("tile", spec, "tile"), ("tile_det", spec, "tile_det"), ("gather", spec, "gather")]
    if split_too:
        forms.insert(2, ("tile_det split-in-place", ops.LayerSpec(H=h, W=h, K=k, variant=_lib.ET_VARIANT_BWD_SPLIT_IN_PLACE), "tile_det"))
    res = {}
    for name, sp, form in forms:
        res[name] = call_ms(lambda: ops.backward_nhwc(sp, ref, src, cam, go, form=form, attn=attn), reps)
        extra = ""
        if form == "tile_det":
            hdr = ops.backward_deferred_tiles(dev, header=True)
            extra = "   (second launch: %d tiles whole, %d shared by eight blocks)" % (hdr[0], hdr[2])
        print("%-15s %3d pairs %3dx%-3d K %-3d  %-24s min %7.3f  p50 %7.3f  max %7.3f ms%s" % ((rig, n, h, h, k, name) + res[name] + (extra,)), flush=True)
    ops.check_tile_errors()
    ops.release_workspaces()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--pairs", type=int, default=128)
    a = ap.parse_args()
    assert a.reps >= 12
    print("backward forms, %s, %d timed calls each after 3 warm-up calls (device events)" % (torch.cuda.get_device_name(0), a.reps))
    c2 = case("ring", a.pairs, 64, 64, a.reps, True)
    for rig in ("epipole_inside", "h36m_room"):
        case(rig, a.pairs, 64, 64, a.reps, True)
    case("ring", a.pairs, 96, 64, a.reps, False)
    ratio = c2["tile_det"][1] / c2["gather"][1]
    print("Config 2: tile_det p50 / gather p50 = %.3f (accepted: <= 0.5)   tile p50 %.3f ms" % (ratio, c2["tile"][1]))
