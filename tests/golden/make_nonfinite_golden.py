"""Golden vectors for NON-FINITE feature maps and incoming gradients, from the REAL reference.

    python tests/golden/make_nonfinite_golden.py [case names]

Writes tests/golden/nonfinite/<name>.npz (a subdirectory: the suite's conftest takes every npz directly in tests/golden/ as a
layer fixture).  Needs the reference tree (oracle/ref_harness.py), so it runs where the other makers run.

What a file holds (tests/nonfinite_fixture.py reads it back):
  * the FINITE base inputs of three pairs -- feat1, feat2, grad_out (N,C,H,W), P1, P2, the reference's own per-pair algebra `cam`
    (and the z / bn parameters of the 256-channel cases; the prior table of the prior modes) -- quantised to a few mantissa bits so
    that the file compresses: the features are post-ReLU multiples of 1/32, grad_out multiples of 1/16;
  * the reference's base outputs of PAIR 1, once: out1, attn1, corr_pos1, grad_feat1_1, grad_feat2_1 (and finalout1);
  * per case `<c>`: `<c>.site` rows of (tensor, y, x, channel) -- tensor 0 feat2 (the source map), 1 feat1 (the reference map),
    2 grad_out, 3 the prior table (y = k, x = pixel index, channel unused); channel -1 = every channel --, `<c>.kind` (0 NaN, 1 +Inf,
    2 -Inf), `<c>.corr_pos` of pair 1, and for every output `<c>.<out>.mask` = the bit-packed NaN | +Inf | -Inf masks (3, bytes)
    over pair 1's array, `<c>.<out>.idx` / `.val` = the flat indices and values of the FINITE entries that differ from the base run
    (a -Inf logit leaves the soft-max finite and takes its weight away: the other weights of that pixel change).
The sites always sit in pair 1 of 3.

What the maker ASSERTS on the reference itself, case by case:
  * pairs 0 and 2 of the poisoned run equal the base run bit for bit, in every output: the reference confines a non-finite value
    to its pair;
  * every entry of pair 1 that is finite and belongs to a pixel the base run and the poisoned run agree on is bit-equal -- i.e. the
    entries stored as idx / val all lie in pixels that also hold a changed weight or a non-finite value (so `touched` below is
    the whole effect);
  * the set of touched pixels (non-finite or changed, any channel) of every output -- out, attn, finalout, grad_feat1 over
    reference pixels, grad_feat2 over source pixels -- holds at most half of the pair's pixels, and is non-empty for the outputs
    the site must reach (the corner sites must reach nothing: see below).
The sites: src_one / src_all (one / every channel of a source pixel), ref_one (one channel of a reference pixel), ref_zero (the
same where a sample reads an exact post-ReLU zero in that channel; another (pixel, channel) than ref_one), gout_one, prior_one,
src_stale (a tap the next sample of the line replaces by an out-of-image tap), src_corner_one / src_corner_all (source pixel
(0, 0): the tile kernels pad their row lists, and a pad must not read a real row -- the reference changes only where a line
really taps the corner, possibly nowhere) and src_grid (a sample exactly on a source grid point: an in-image tap of weight 0,
which the reference multiplies).  src_grid needs such a sample among the pair's lines: only the K = 101 lines hold one, so the
C = 8 per-pixel kernels, the K = 16 heads and the general-kernel modes are NOT exercised on a zero-weight in-image tap.
Sites are chosen by a fixed rule (nearest to the map centre among the candidates whose tap coverage admits the bound) and then
checked by these asserts on the real runs; nothing is relaxed to make a site pass.
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as orc  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402
from epipolar_transformers_amd import synthetic as syn  # noqa: E402

KINDS = (("nan", float("nan")), ("pinf", float("inf")), ("ninf", float("-inf")))
SRC, REF, GOUT, PRIOR = 0, 1, 2, 3
NPAIRS, POISONED = 3, 1

HEAD = [
    # the smallest shapes at which each route still runs its real code
    dict(name="head_10x10_c256_k16", H=10, C=256, K=16, image=40, softmax=True, z=True),      # persistent / fused / tiled backward
    dict(name="head_10x10_c256_k101", H=10, C=256, K=101, image=40, softmax=True, z=False),   # both halves of the two-pass soft-max
    # (K = 100 itself cannot be run: the reference's torch.range(0, 1, 1 / 99) yields 99 samples and its view fails; 101 is the nearest K it takes)
    # 16 x 16 (the shape tests/test_gpu_fused.py overflows with): under ET_VARIANT_TILE_SPLIT's row-set capacity of 64 the tiles
    # also overflow for capacity reasons.  Forward outputs only, no z branch: with the gradients the file would exceed 1 MiB.
    dict(name="cap_16x16_c256_k16", H=16, C=256, K=16, image=64, softmax=True, z=False, fwd_only=True),
    dict(name="head_nosoftmax_10x10_c256_k16", H=10, C=256, K=16, image=40, softmax=False, z=False),   # partly-NaN arg-max on the tile routes
    dict(name="pixel_16x16_c8_k8", H=16, C=8, K=8, image=64, softmax=True, z=False),          # per-pixel kernels
    dict(name="pixel_nosoftmax_16x16_c8_k8", H=16, C=8, K=8, image=64, softmax=False, z=False),
]
MODES = [
    # the c8_k8 / c16_k16 mode cases of make_golden_modes.py that run a maximum, a cosine or a prior over the data
    dict(name="mode_param_pool_c16_k16", C=16, K=16, ov=["EPIPOLAR.PARAMETERIZED", "('z', 'theta', 'phi', 'g')", "EPIPOLAR.POOLING", "True",
                                                        "EPIPOLAR.BOTTLENECK", "2", "EPIPOLAR.ZRESIDUAL", "False"]),
    dict(name="mode_attention_max_c8_k8", C=8, K=8, ov=["EPIPOLAR.ATTENTION", "max", "EPIPOLAR.PARAMETERIZED", "('z',)",
                                                        "EPIPOLAR.ZRESIDUAL", "True"]),
    dict(name="mode_cosine_c8_k8", C=8, K=8, ov=["EPIPOLAR.SIMILARITY", "cos", "EPIPOLAR.PARAMETERIZED", "('z',)", "EPIPOLAR.ZRESIDUAL", "True"]),
    dict(name="mode_prior_add_c8_k8", C=8, K=8, prior=True, ov=["EPIPOLAR.PRIOR", "True", "DATASETS.CAMERAS", "(1, 2, 3, 4)",
                                                                "EPIPOLAR.PARAMETERIZED", "()"]),
    dict(name="mode_prior_mul_c8_k8", C=8, K=8, prior=True, ov=["EPIPOLAR.PRIOR", "True", "EPIPOLAR.PRIORMUL", "True",
                                                                "DATASETS.CAMERAS", "(1, 2, 3, 4)", "EPIPOLAR.PARAMETERIZED", "()"]),
]
MODE_H, MODE_IMAGE = 16, 64

npf = lambda t: np.ascontiguousarray(t.detach().numpy().astype(np.float32))


def quantised(t, step):
    return (t / step).round() * step


def inputs_of(name, N, C, H):
    seed = sum(map(ord, name)) % 1000
    f1, f2 = syn.make_features(N, C, H, H, seed=seed, relu=True)
    f1, f2 = quantised(f1, 1 / 32), quantised(f2, 1 / 32)
    f1[POISONED, :, 3, 5] = 0.0                     # the exact-zero mask (epipolar.py:298): one all-zero reference pixel
    g = torch.Generator().manual_seed(seed + 1)
    grad_out = quantised(torch.randn(N, C, H, H, generator=g), 1 / 16)
    return seed, f1.contiguous(), f2.contiguous(), grad_out.contiguous(), g


def tap_coverage(locs, H, W, align_corners=False):
    """(HW_ref, HW_src) bool: reference pixel p has an IN-BOUNDS bilinear tap on source pixel s (a zero weight counts: grid_sample
    multiplies it), and `exact` (K,HW_ref) bool: the sample falls exactly on a source grid point in x or in y."""
    K = locs.shape[0]
    # the float32 coordinates grid_sample itself computes
    xf = ((locs[..., 0] + 1) * W - 1) / 2
    yf = ((locs[..., 1] + 1) * H - 1) / 2
    x0, y0 = xf.floor().long().view(K, -1), yf.floor().long().view(K, -1)
    cov = torch.zeros(H * W, H * W, dtype=torch.bool)
    pix = torch.arange(H * W).view(1, -1).expand(K, -1)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            cov[pix[ok], (yy * W + xx)[ok]] = True
    exact = ((xf == xf.floor()) | (yf == yf.floor())).view(K, -1)
    return cov, exact, (x0, y0, xf.view(K, -1), yf.view(K, -1))


def centre_order(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    d = (yy - (H - 1) / 2) ** 2 + (xx - (W - 1) / 2) ** 2
    return [int(i) for i in np.argsort(d.ravel(), kind="stable")]


def choose_sites(locs1, f1, f2, H, W, C):
    """The sites of pair 1 (fixed rule, see the module text).  locs1: (K,H,W,2) of pair 1; f1, f2: (C,H,W) of pair 1."""
    cov, exact, (x0, y0, xf, yf) = tap_coverage(locs1, H, W)
    K = locs1.shape[0]
    nref = cov.sum(0)                                # reference pixels that tap source pixel s
    order = centre_order(H, W)
    lim = (H * W) // 2
    src = next(s for s in order if 1 <= int(nref[s]) <= lim)
    sy, sx = divmod(src, W)
    # a channel whose reference partner is non-zero in some tapping pixel: the similarity itself becomes non-finite
    taps = torch.nonzero(cov[:, src]).view(-1)
    ch = next(c for c in range(C) if (f1[c].view(-1)[taps] != 0).any())
    sites = {"src_one": [(SRC, sy, sx, ch)], "src_all": [(SRC, sy, sx, -1)]}
    # one channel of one reference pixel (not the all-zero one), a non-zero channel
    rp = next(p for p in order if (f1.view(C, -1)[:, p] != 0).any())
    ry, rx = divmod(rp, W)
    rc = next(c for c in range(C) if f1[c, ry, rx] != 0)
    sites["ref_one"] = [(REF, ry, rx, rc)]
    # ... and once where that channel's partner is an exact post-ReLU zero: some sample of the pixel reads exactly 0 in that
    # channel from all its in-bounds taps, so Inf x 0 = NaN enters the similarity
    s2 = torch.nn.functional.grid_sample(f2.view(1, C, H, W).expand(K, -1, -1, -1), locs1, mode="bilinear", padding_mode="zeros",
                                         align_corners=False)               # (K,C,H,W)
    inb = ((x0 >= 0) & (x0 + 1 < W) & (y0 >= 0) & (y0 + 1 < H)).view(K, H, W)       # (all four taps inside)
    zero = (s2 == 0) & inb.unsqueeze(1)
    found = None
    for p in order:
        py, px = divmod(p, W)
        cs = [int(c) for c in torch.nonzero(zero[:, :, py, px].any(0)).view(-1) if (py, px, int(c)) != (ry, rx, rc)]
        if len(cs) and (f1[:, py, px] != 0).any():
            found = (REF, py, px, cs[0])
            break
    assert found is not None, "no reference pixel samples an exact zero"
    sites["ref_zero"] = [found]
    sites["gout_one"] = [(GOUT, ry, rx, rc)]
    # a sample that falls exactly on a source grid point: two (or three) of its four taps carry the weight 0 and the reference
    # still multiplies them.  The site is such a zero-weight in-bounds tap.
    grid = None
    for p in order:
        for k in range(K):
            if not exact[k, p]:
                continue
            X, Y, fx, fy = int(x0[k, p]), int(y0[k, p]), float(xf[k, p]), float(yf[k, p])
            for dy in (0, 1):
                for dx in (0, 1):
                    wx = (1 - (fx - X)) if dx == 0 else (fx - X)
                    wy = (1 - (fy - Y)) if dy == 0 else (fy - Y)
                    xx, yy = X + dx, Y + dy
                    if wx * wy == 0 and 0 <= xx < W and 0 <= yy < H and 1 <= int(nref[yy * W + xx]) <= lim:
                        grid = (SRC, yy, xx, ch if (f1[ch].view(-1)[torch.nonzero(cov[:, yy * W + xx]).view(-1)] != 0).any() else -1)
                        break
                if grid:
                    break
            if grid:
                break
        if grid:
            break
    if grid is not None:
        sites["src_grid"] = [grid]
    # a tap that the NEXT sample of the same line replaces by a tap outside the image (zero padding: the reference adds
    # nothing for it).  Kernels that keep tap rows in registers by coordinate parity must not multiply the stale row with the
    # absent tap's weight 0.  The site: an in-bounds tap (y, x) of sample k - 1 of pixel p such that sample k has the out-of-image
    # tap of the same parity in x and in y, and does not itself tap (y, x).
    stale = None
    for p in order:
        for k in range(1, K):
            Xp, Yp, Xk, Yk = int(x0[k - 1, p]), int(y0[k - 1, p]), int(x0[k, p]), int(y0[k, p])
            prev = {(Yp + dy, Xp + dx) for dy in (0, 1) for dx in (0, 1) if 0 <= Xp + dx < W and 0 <= Yp + dy < H}
            cur = {(Yk + dy, Xk + dx) for dy in (0, 1) for dx in (0, 1)}
            for (yy, xx) in sorted(cur):
                if 0 <= xx < W and 0 <= yy < H:
                    continue
                for (py, px) in sorted(prev - cur):
                    if (py & 1, px & 1) == (yy & 1, xx & 1) and 1 <= int(nref[py * W + px]) <= lim:
                        stale = (SRC, py, px, ch if (f1[ch].view(-1)[torch.nonzero(cov[:, py * W + px]).view(-1)] != 0).any() else -1)
                        break
                if stale:
                    break
            if stale:
                break
        if stale:
            break
    if stale is not None:
        sites["src_stale"] = [stale]
    sites["src_corner_one"] = [(SRC, 0, 0, ch)]
    sites["src_corner_all"] = [(SRC, 0, 0, -1)]
    return sites


def poison(tensors, site_rows, value):
    """Copies of (f2, f1, grad_out[, prior]) with `value` at the sites of pair 1."""
    out = [t.clone() for t in tensors]
    for tid, y, x, c in site_rows:
        if tid == PRIOR:
            out[PRIOR].view(out[PRIOR].shape[0], -1)[y, x] = value
        elif c < 0:
            out[tid][POISONED, :, y, x] = value
        else:
            out[tid][POISONED, c, y, x] = value
    return out


def record(case, base, run, data, reach, H, W):
    """Compare a poisoned run with the base run, assert the confinement on the reference, store the masks.  `reach`: the outputs
    the site must reach (non-empty touched set)."""
    for o, b in base.items():
        r = run[o]
        if o == "corr_pos":
            assert np.array_equal(r[0], b[0]) and np.array_equal(r[2], b[2]), (case, o, "pairs 0 / 2 changed")
            data[case + ".corr_pos"] = r[POISONED]
            continue
        for n in (0, 2):
            assert np.array_equal(r[n].view(np.uint32), b[n].view(np.uint32)), (case, o, "pair %d is not bit-equal to the base run" % n)
        r1, b1 = r[POISONED], b[POISONED]
        nan, pinf, ninf = np.isnan(r1), np.isposinf(r1), np.isneginf(r1)
        changed = np.isfinite(r1) & (r1.view(np.uint32) != b1.view(np.uint32))
        touched = (nan | pinf | ninf | changed).any(0)              # (H,W)
        if o in reach:
            assert touched.any(), (case, o, "the site does not reach this output")
        assert touched.sum() <= (H * W) // 2, (case, o, "touches %d of %d pixels" % (touched.sum(), H * W))
        data["%s.%s.mask" % (case, o)] = np.stack([np.packbits(m.ravel()) for m in (nan, pinf, ninf)])
        idx = np.nonzero(changed.ravel())[0].astype(np.int32)
        data["%s.%s.idx" % (case, o)] = idx
        data["%s.%s.val" % (case, o)] = r1.ravel()[idx]
        data["%s.%s.touched" % (case, o)] = np.packbits(touched.ravel())


def run_cases(name, sites, tensors, runner, base, data, H, W):
    stats = []
    for sname, rows in sites.items():
        for kname, val in KINDS:
            case = "%s.%s" % (sname, kname)
            run = runner(*poison(tensors, rows, val))
            tid = rows[0][0]
            # (what a site must reach: the forward outputs -- a gradient need not depend on it, e.g. d(feat_ref) with the soft-max
            #  off does not read feat_ref --; an incoming gradient reaches d(feat_src))
            reach = ("grad_feat2",) if tid == GOUT else tuple(o for o in ("out", "finalout", "attn") if o in base)
            if sname.startswith("src_corner"):
                reach = ()          # (only the lines that really tap the corner change, possibly none)
            record(case, base, run, data, reach, H, W)
            data[case + ".site"] = np.asarray(rows, np.int64)
            data[case + ".kind"] = np.int64([k for k, _ in KINDS].index(kname))
            stats.append(case)
    data["cases"] = np.array(stats)


def run_head(c):
    H, C, K = c["H"], c["C"], c["K"]
    ov = ["KEYPOINT.HEATMAP_SIZE", "(%d, %d)" % (H, H), "KEYPOINT.NFEATS", str(C), "EPIPOLAR.SAMPLESIZE", str(K),
          "DATASETS.IMAGE_SIZE", "(%d, %d)" % (c["image"], c["image"]), "EPIPOLAR.USE_CORRECT_NORMALIZE", "True",
          "EPIPOLAR.SOFTMAX_ENABLED", str(c["softmax"]), "VIS.EPIPOLAR_LINE", "True",
          "DATASETS.IMAGE_RESIZE", "1.0", "DATASETS.PREDICT_RESIZE", "1.0"]
    mod, cfg = rh.reference_epipolar(overrides=ov)
    seed, f1, f2, grad_out, g = inputs_of(c["name"], NPAIRS, C, H)
    P1, P2 = syn.make_pairs(1, 4, c["image"], seed=seed, jitter=(0.05, 3.0))
    P1, P2 = P1[:NPAIRS], P2[:NPAIRS]
    with torch.no_grad():
        mod.z.weight.copy_(torch.randn(mod.z.weight.shape, generator=g).mul_(0.05).bfloat16().float())
        mod.z.bias.copy_(quantised(torch.randn(mod.z.bias.shape, generator=g) * 0.1, 1 / 256))
        mod.bn.weight.copy_(quantised(1 + 0.1 * torch.randn(C, generator=g), 1 / 256))
        mod.bn.bias.copy_(quantised(0.1 * torch.randn(C, generator=g), 1 / 256))
        mod.bn.running_mean.copy_(quantised(0.1 * torch.randn(C, generator=g), 1 / 256))
        mod.bn.running_var.copy_(quantised(0.5 + torch.rand(C, generator=g), 1 / 256))
    mod.eval()
    saved = cfg.EPIPOLAR.PARAMETERIZED
    state = {}

    def runner(a2, a1, go):
        a1, a2 = a1.clone().requires_grad_(True), a2.clone().requires_grad_(True)
        dict.__setitem__(cfg.EPIPOLAR, "PARAMETERIZED", ())                 # pre-z output: the z branch switched off
        out, corr_pos, attn, locs = mod(a1, a2, P1, P2)
        if not c.get("fwd_only"):
            (out * go).sum().backward()
        dict.__setitem__(cfg.EPIPOLAR, "PARAMETERIZED", saved)
        r = dict(out=npf(out), attn=npf(attn), corr_pos=npf(corr_pos))
        if not c.get("fwd_only"):
            r.update(grad_feat1=npf(a1.grad), grad_feat2=npf(a2.grad))
        if c["z"]:
            with torch.no_grad():
                r["finalout"] = npf(mod(a1.detach(), a2.detach(), P1, P2)[0])
        state["locs"] = locs.detach()
        return r

    base = runner(f2, f1, grad_out)
    for o, v in base.items():
        assert np.isfinite(v).all(), o
    locs = state["locs"]                                    # (N,K,H,W,2)
    a, b, e = orc.camera_algebra(P1, P2)
    cam = np.concatenate([a.reshape(NPAIRS, 12), b.reshape(NPAIRS, 12), e.reshape(NPAIRS, 3)], 1).astype(np.float32)
    data = dict(feat1=npf(f1), feat2=npf(f2), grad_out=npf(grad_out), P1=npf(P1), P2=npf(P2), cam=cam,
                sample_locs1=npf(locs[POISONED]),
                meta=np.array([H, H, C, K, NPAIRS, c["image"], 1, int(c["softmax"]), 0], np.int64),
                softmax_scale=np.float32(cfg.EPIPOLAR.SOFTMAXSCALE), downsample=np.float32(cfg.BACKBONE.DOWNSAMPLE),
                torch_version=np.array(torch.__version__))
    if c["z"]:
        data.update(z_weight=npf(mod.z.weight), z_bias=npf(mod.z.bias), bn_weight=npf(mod.bn.weight), bn_bias=npf(mod.bn.bias),
                    bn_running_mean=npf(mod.bn.running_mean), bn_running_var=npf(mod.bn.running_var))
    for o, v in base.items():
        data[o + "1"] = v[POISONED]
    sites = choose_sites(locs[POISONED], f1[POISONED], f2[POISONED], H, H, C)
    if c.get("fwd_only"):
        sites.pop("gout_one")
    run_cases(c["name"], sites, (f2, f1, grad_out), runner, base, data, H, H)
    return data


def run_mode(c):
    H, C, K = MODE_H, c["C"], c["K"]
    ov = ["KEYPOINT.HEATMAP_SIZE", "(%d, %d)" % (H, H), "KEYPOINT.NFEATS", str(C), "EPIPOLAR.SAMPLESIZE", str(K),
          "DATASETS.IMAGE_SIZE", "(%d, %d)" % (MODE_IMAGE, MODE_IMAGE), "EPIPOLAR.USE_CORRECT_NORMALIZE", "True",
          "VIS.EPIPOLAR_LINE", "True"] + c["ov"]
    seed = sum(map(ord, c["name"])) % 1000
    torch.manual_seed(seed)            # (the reference draws its prior tables from the global generator, epipolar.py:79-80)
    mod, cfg = rh.reference_epipolar(overrides=ov)
    _, f1, f2, _, g = inputs_of(c["name"], NPAIRS, C, H)
    P1, P2 = syn.make_pairs(1, 4, MODE_IMAGE, seed=seed, jitter=(0.05, 3.0))
    P1, P2 = P1[:NPAIRS], P2[:NPAIRS]
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(quantised(0.2 * torch.randn(p.shape, generator=g), 1 / 256))
        if hasattr(mod, "bn"):
            mod.bn.weight.copy_(quantised(1 + 0.1 * torch.randn(C, generator=g), 1 / 256))
            mod.bn.running_mean.copy_(quantised(0.1 * torch.randn(C, generator=g), 1 / 256))
            mod.bn.running_var.copy_(quantised(0.5 + torch.rand(C, generator=g), 1 / 256))
        for v in getattr(mod, "prior", {}).values():
            v.copy_(quantised(v, 1 / 1024))
    # pair 1 is (camera 2, other camera 3): its table is poisoned in the prior cases
    camera, other_camera = torch.tensor([1, 2, 3]), torch.tensor([2, 3, 4])
    kw = dict(camera=camera, other_camera=other_camera)
    mod.eval()
    state = {}
    grad_out = quantised(torch.randn(NPAIRS, C, H, H, generator=g), 1 / 16)
    table = mod.prior[(2, 3)] if c.get("prior") else None
    table0 = table.detach().clone() if table is not None else None

    def runner(a2, a1, go, pr=None):
        a1, a2 = a1.clone().requires_grad_(True), a2.clone().requires_grad_(True)
        if table is not None:
            with torch.no_grad():
                table.copy_(pr if pr is not None else table0)
        fin, corr_pos, attn, locs = mod(a1, a2, P1, P2, **kw)
        (fin * go).sum().backward()
        state["locs"] = locs.detach()
        zeros = lambda t: torch.zeros_like(t)
        return dict(finalout=npf(fin), attn=npf(attn), corr_pos=npf(corr_pos),
                    grad_feat1=npf(a1.grad if a1.grad is not None else zeros(a1)),
                    grad_feat2=npf(a2.grad if a2.grad is not None else zeros(a2)))

    base = runner(f2, f1, grad_out)
    for o, v in base.items():
        assert np.isfinite(v).all(), o
    locs = state["locs"]
    a, b, e = orc.camera_algebra(P1, P2)
    cam = np.concatenate([a.reshape(NPAIRS, 12), b.reshape(NPAIRS, 12), e.reshape(NPAIRS, 3)], 1).astype(np.float32)
    data = dict(feat1=npf(f1), feat2=npf(f2), grad_out=npf(grad_out), P1=npf(P1), P2=npf(P2), cam=cam,
                camera=camera.numpy(), other_camera=other_camera.numpy(), sample_locs1=npf(locs[POISONED]),
                overrides=np.array(c["ov"]), meta=np.array([H, C, K, NPAIRS, MODE_IMAGE], np.int64),
                torch_version=np.array(torch.__version__))
    for k, v in mod.state_dict().items():
        data["sd." + k] = npf(v) if v.dtype.is_floating_point else v.numpy()
    for (i, j), v in getattr(mod, "prior", {}).items():
        data["prior.%d.%d" % (i, j)] = npf(v if (i, j) != (2, 3) else table0)
    for o, v in base.items():
        data[o + "1"] = v[POISONED]
    sites = choose_sites(locs[POISONED], f1[POISONED], f2[POISONED], H, H, C)
    tensors = [f2, f1, grad_out]
    if table is not None:
        tensors.append(table0)
        # one element of the prior: sample 2 of the pixel the reference sites use
        (_, ry, rx, _), = sites["ref_one"]
        sites = dict(sites, prior_one=[(PRIOR, 2, ry * H + rx, 0)])
    run_cases(c["name"], sites, tuple(tensors), runner, base, data, H, H)
    if table is not None:
        with torch.no_grad():
            table.copy_(table0)
    return data


def main():
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    outdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nonfinite")
    os.makedirs(outdir, exist_ok=True)
    only = set(sys.argv[1:])
    for c in HEAD + MODES:
        if only and c["name"] not in only:
            continue
        data = run_head(c) if c in HEAD else run_mode(c)
        path = os.path.join(outdir, c["name"] + ".npz")
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        assert size <= 1 << 20, (c["name"], size)
        print("%-34s %7.1f KiB  %d cases" % (c["name"], size / 1024, len(data["cases"])))


if __name__ == "__main__":
    main()
