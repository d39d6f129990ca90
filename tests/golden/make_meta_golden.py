"""Golden vectors for the Meta fusion layer and the `metaHG*` hourglass callers, from the REAL reference (modeling/layers/meta.py,
vision/multiview.py findFundamentalMat, modeling/backbones/ProHG.py behind registry names metaHG / metaHG1 / metaHG11).

    python tests/golden/make_meta_golden.py [layer | <hourglass case> ...]

The layer alone -> tests/golden/meta/layer_<case>.npz (+ `_y`, `_gin`: the two map-sized tensors, a file each so that every file
stays below 1 MiB); four cases at C = 256:
    n3_5x7    N = 3, HW = 35    less than one 64-row tile, not a multiple of the weight gradient's 16-row step
    n2_5x13   N = 2, HW = 65    a second tile of one row
    n2_16x16  N = 2, HW = 256   exact tiles
    n1_5x7    N = 1, HW = 35    a single pair
Stored: P_ref / P_src, the reference's float32 F and F64 (the same formulas in float64), the reference's y = meta(...) + feat and its
autograd gradients (input, share.*, fc0.*; of fc1.weight -- 26 MB -- every 257th row and the float64 sum of magnitudes; fc1.bias,
which is the per-pair weight gradient summed over the pairs), and how far the reference's own float32 results lie from a float64
evaluation of the same formulas on the same float32 inputs and F (`ref_dist_*`, relative to each tensor's largest magnitude; strided
samples of the float64 results are kept as `*_64s`).  NOT stored, but rebuilt from seeded torch CPU generators on both sides, as the
26 MB fc1.weight has to be: the weights (`meta_weights`) and the maps (`meta_inputs`).

The whole net -> tests/golden/hourglass_meta_<case>.npz: metaHG1 / MERGE late, metaHG (three stacks) / MERGE early, metaHG11 / MERGE
late at the sizes of make_hourglass_golden.py, eval mode.

The maker asserts, and records, per layer case: max|y| within [0.5, 20]; the hyper part W_n . input at least a quarter of
max|y - feat| (a kernel that read only `share` fails) and what every pair n > 0 would lose under pair 0's weight at least 5 % of it
(`pair_contrast`); the reference within 1e-5 of the float64
evaluation.  Runs only in the build container."""
import contextlib
import io
import os
import sys
import warnings
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

C = 256
LAYER_DIR = os.path.join(HERE, "meta")
LAYER_CASES = [dict(name="n3_5x7", N=3, H=5, W=7), dict(name="n2_5x13", N=2, H=5, W=13), dict(name="n2_16x16", N=2, H=16, W=16),
               dict(name="n1_5x7", N=1, H=5, W=7)]
SIZE, HS, J, N_HG = 64, 16, 7, 2
HG_CASES = [dict(name="hg1_late", body="metaHG1", merge="late"), dict(name="hg3_early", body="metaHG", merge="early"),
            dict(name="hg11_late", body="metaHG11", merge="late")]
# (MERGE both cannot run with a metaHG* body in the reference: it has one Meta layer per STACK and indexes them by fusion point, two
#  per stack under `both` -- ProHG.py:185-187, 220, 263-271 raise IndexError at the stack's second point.  So the depth-1 factory is
#  covered under MERGE late.)
FC1_ROW_STEP = 257


def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()) & 0x7FFFFFFF)


def meta_weights(prefix, f_scale):
    """State-dict entries `prefix + fc0.* | fc1.* | share.*` of one Meta layer, every tensor from its own torch CPU generator
    seeded by the CRC of its key (model_weights.py's scheme).  Centred draws -- deterministic_state_dict would give every fc weight
    a positive value near 1.  fc0.weight is scaled by `f_scale` = 1 / max|F| of the fixture, so that the hidden units and the hyper
    weights are O(1): F itself is 1e5 - 1e6."""
    draw = lambda name, shape, std: torch.randn(shape, generator=_gen(prefix + name)) * std
    return {prefix + "fc0.weight": draw("fc0.weight", (100, 9), 1.0) * float(f_scale),
            prefix + "fc0.bias": draw("fc0.bias", (100,), 0.1),
            prefix + "fc1.weight": draw("fc1.weight", (C * C, 100), 0.04),
            prefix + "fc1.bias": draw("fc1.bias", (C * C,), 0.02),
            prefix + "share.weight": draw("share.weight", (C, C, 1, 1), 1.0 / 16.0),
            prefix + "share.bias": draw("share.bias", (C,), 0.05)}


def meta_inputs(case):
    """input (post-ReLU), feat, grad_out of a layer case, (N, C, H, W) float32, from seeded CPU generators."""
    c = next(k for k in LAYER_CASES if k["name"] == case)
    shape = (c["N"], C, c["H"], c["W"])
    draw = lambda what: torch.randn(shape, generator=_gen("meta_layer/%s/%s" % (case, what)))
    return draw("input").relu_(), draw("feat"), draw("grad_out")


def layer_pairs(c):
    from epipolar_transformers_amd import synthetic as syn

    P_ref, _ = syn.make_pairs(1, 4, SIZE, seed=41 + c["N"] * 7 + c["W"], jitter=(0.03, 2.0))
    P_src = P_ref[[1, 3, 0, 2]]                                       # (not the ring's neighbour: the pairs' geometries differ more)
    return P_ref[:c["N"]].contiguous(), P_src[:c["N"]].contiguous()


def fundamental64(P1, P2):
    """findFundamentalMat's formulas (vision/multiview.py:85-124, camera_center :16-21) in float64."""
    P1, P2 = P1.double(), P2.double()
    p2p1inv = P2 @ torch.linalg.pinv(P1)
    centre = -torch.inverse(P1[..., :3]) @ P1[..., 3, None]
    hom = torch.ones(P1.shape[0], 4, 1, dtype=torch.float64)
    hom[:, :3] = centre
    e2 = (P2 @ hom).view(-1, 3)
    cross = torch.zeros_like(p2p1inv)
    cross[:, 0, 1], cross[:, 0, 2], cross[:, 1, 2] = -e2[:, 2], e2[:, 1], -e2[:, 0]
    cross[:, 1, 0], cross[:, 2, 0], cross[:, 2, 1] = e2[:, 2], -e2[:, 1], e2[:, 0]
    return cross @ p2p1inv


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():       # (findFundamentalMat prints its operands)
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


GRAD_KEYS = ("input", "share.weight", "share.bias", "fc0.weight", "fc0.bias", "fc1.weight", "fc1.bias")


def _float64_layer(sd, F32, inp, feat, gout):
    """y and the gradients of GRAD_KEYS from the layer's formulas (meta.py:27-50, + feat) in float64 on the float32 inputs and F."""
    p = {k: v.double().requires_grad_() for k, v in sd.items()}
    x = inp.double().requires_grad_()
    n = x.shape[0]
    hidden = torch.relu(F32.double().reshape(n, 9) @ p["fc0.weight"].t() + p["fc0.bias"])
    w = (hidden @ p["fc1.weight"].t() + p["fc1.bias"]).view(n, C, C)
    hyper = torch.einsum("noc,nchw->nohw", w, x)
    y = hyper + torch.einsum("oc,nchw->nohw", p["share.weight"].view(C, C), x) + p["share.bias"].view(1, C, 1, 1) + feat.double()
    y.backward(gout.double())
    grads = {"input": x.grad}
    grads.update({k: p[k].grad for k in GRAD_KEYS[1:]})
    # what pair n's rows would lose if the kernel took pair 0's weight for them, relative to max|y - feat|
    swap = torch.einsum("noc,nchw->nohw", (w - w[:1]).detach(), x.detach()).abs().amax((1, 2, 3))
    contrast = float(swap[1:].min() / (y.detach() - feat.double()).abs().max()) if n > 1 else float("nan")
    return y.detach(), grads, hyper.detach(), contrast


def run_layer_case(c):
    from oracle import ref_harness as rh

    rh.load_cfg("configs/epipolar/keypoint_h36m_zresidual_fixed.yaml", ["DEVICE", "cpu"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from modeling.layers.meta import Meta
        from vision.multiview import findFundamentalMat
    P_ref, P_src = layer_pairs(c)
    n = c["N"]
    F32 = _quiet(findFundamentalMat, P_ref, P_src).reshape(n, 3, 3)
    F64 = fundamental64(P_ref, P_src)
    f_scale = 1.0 / float(F32.abs().max())
    sd = meta_weights("", f_scale)
    ref = Meta(C)
    ref.load_state_dict(sd)
    inp, feat, gout = meta_inputs(c["name"])
    x = inp.clone().requires_grad_()
    y = _quiet(ref, P_ref, P_src, x) + feat
    y.backward(gout)
    grads = {"input": x.grad}
    grads.update({k: dict(ref.named_parameters())[k].grad for k in GRAD_KEYS[1:]})
    y64, grads64, hyper64, contrast = _float64_layer(sd, F32, inp, feat, gout)

    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())
    rec = dict(max_abs_y=float(y.detach().abs().max()), pair_contrast=contrast, hyper_share=float(hyper64.abs().max() / (y64 - feat.double()).abs().max()),
               ref_dist_y=rel(y.detach(), y64), ref_dist_F=np.array([rel(F32[i], F64[i]) for i in range(n)]))
    for k in GRAD_KEYS:
        rec["ref_dist_grad_" + k] = rel(grads[k], grads64[k])
    assert 0.5 <= rec["max_abs_y"] <= 20.0, rec
    assert rec["hyper_share"] >= 0.25, rec
    assert rec["ref_dist_y"] < 1e-5 and all(rec["ref_dist_grad_" + k] < 1e-5 for k in GRAD_KEYS), rec
    assert n == 1 or rec["pair_contrast"] >= 0.05, rec          # (the gates are 1e-4: pair 0's weight for every pair is far outside)

    npf = lambda t: t.detach().numpy().astype(np.float32)
    main = dict(dims=np.array([n, C, c["H"], c["W"]]), P_ref=npf(P_ref), P_src=npf(P_src), F=npf(F32), F64=F64.numpy(),
                f_scale=np.array(f_scale, np.float64), fc1_row_step=np.array(FC1_ROW_STEP))
    main.update({k: np.array(v, np.float64) for k, v in rec.items()})
    for k in GRAD_KEYS[1:]:
        g = grads[k]
        if k == "fc1.weight":
            main["grad_fc1.weight_rows"] = npf(g[::FC1_ROW_STEP])
            main["grad_fc1.weight_abs_sum"] = np.array(float(g.double().abs().sum()), np.float64)
            main["grad_fc1.weight_max"] = np.array(float(g.abs().max()), np.float64)
            main["grad_fc1.weight_rows_64"] = grads64[k][::FC1_ROW_STEP].numpy()
        else:
            main["grad_" + k] = npf(g)
            main["grad_%s_64s" % k] = grads64[k].reshape(-1)[::17].numpy()
    main["y_64s"] = y64.reshape(-1)[::17].numpy()
    main["grad_input_64s"] = grads64["input"].reshape(-1)[::17].numpy()
    print("%-9s max|y| %.2f  hyper share %.2f  pair contrast %.2f  reference vs float64: y %.1e  F %.1e  grads %s" % (
        c["name"], rec["max_abs_y"], rec["hyper_share"], rec["pair_contrast"], rec["ref_dist_y"], rec["ref_dist_F"].max(),
        " ".join("%.1e" % rec["ref_dist_grad_" + k] for k in GRAD_KEYS)))
    return {"": main, "_y": dict(y=npf(y)), "_gin": dict(grad_input=npf(grads["input"]))}


def run_hourglass_case(c):
    from model_weights import deterministic_state_dict
    from make_hourglass_golden import calm
    from oracle import ref_harness as rh
    from epipolar_transformers_amd import synthetic as syn

    ov = ["BACKBONE.BODY", c["body"], "BACKBONE.PRETRAINED", "False", "EPIPOLAR.PRETRAINED", "False", "EPIPOLAR.MERGE", c["merge"],
          "KEYPOINT.HEATMAP_SIZE", "(%d, %d)" % (HS, HS), "KEYPOINT.NUM_PTS", str(J), "KEYPOINT.SIGMA", "2.0", "KEYPOINT.NFEATS", "256",
          "DATASETS.IMAGE_SIZE", "(%d, %d)" % (SIZE, SIZE), "DEVICE", "cpu"]
    cfg = rh.load_cfg("configs/epipolar/keypoint_h36m_zresidual_fixed.yaml", ov)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from modeling import registry
        import modeling.backbones.ProHG  # noqa: F401  (registers the hourglass names)
        from vision.multiview import findFundamentalMat

        net = registry.BACKBONES[cfg.BACKBONE.BODY](cfg)
    src = torch.arange(N_HG).roll(-1)
    P_ref, P_src = syn.make_pairs(1, N_HG, SIZE, seed=31, jitter=(0.03, 2.0))
    assert torch.equal(P_src, P_ref[src])
    F32 = _quiet(findFundamentalMat, P_ref, P_src).reshape(N_HG, 3, 3)
    f_scale = 1.0 / float(F32.abs().max())
    sd = deterministic_state_dict(net.state_dict())
    metas = sorted({k.rsplit(".", 2)[0] + "." for k in sd if k.startswith(("meta.", "testmeta."))})
    for prefix in metas:
        sd.update(meta_weights(prefix, f_scale))
    net.load_state_dict(sd)
    net.eval()
    g = torch.Generator().manual_seed(sum(map(ord, "meta_" + c["name"])))
    img = torch.randn(N_HG, 3, SIZE, SIZE, generator=g)
    scales = calm(net, img)                                                  # (in place: state_dict() tensors alias the parameters)
    with torch.no_grad():
        own = _quiet(net, img)[0]                                            # per-stack maps of every view (no fusion)
        other_features = [f[src] for f in own]
        out = _quiet(net, img, other_inputs=[other_features, P_src, None, P_ref, None, None, img[src]])
    features, heatmaps, locs, scos, corr_pos, depth, _, warped = out
    assert corr_pos is None and depth is None and warped is None
    npf = lambda t: t.detach().numpy().astype(np.float32)
    data = dict(meta=np.array([SIZE, HS, J, N_HG]), body=np.array(c["body"]), merge=np.array(c["merge"]), img=npf(img), src=src.numpy(),
                KRT=npf(P_ref), F=npf(F32), f_scale=np.array(f_scale, np.float64), weight_scales=np.array(scales, np.float64),
                locs=npf(locs), scos=npf(scos), n_features=np.array(len(features)), n_heatmaps=np.array(len(heatmaps)),
                n_own=np.array(len(own)), feature_last=npf(features[-1]),
                feature_checksum=np.array([float(f.double().abs().sum()) for f in features]),
                state_dict_keys=np.array(sorted(net.state_dict())))
    for i, h in enumerate(heatmaps):
        data["heatmap%d" % i] = npf(h)
    # the fusion must matter: the same net without the other view gives different heat maps
    with torch.no_grad():
        alone = _quiet(net, img)[1][-1]
    data["fusion_effect"] = np.array(float((alone - heatmaps[-1]).abs().max() / heatmaps[-1].abs().max()))
    assert float(data["fusion_effect"]) > 0.05, float(data["fusion_effect"])
    print("%-10s %d state-dict keys, feature scale %.2f, heat-map scale %.3f, fusion effect %.2f" %
          (c["name"], len(net.state_dict()), float(features[-1].abs().max()), float(heatmaps[-1].abs().max()), float(data["fusion_effect"])))
    return data


def main():
    torch.set_num_threads(4)
    only = set(sys.argv[1:])
    os.makedirs(LAYER_DIR, exist_ok=True)
    if not only or "layer" in only:
        for c in LAYER_CASES:
            for suffix, data in run_layer_case(c).items():
                path = os.path.join(LAYER_DIR, "layer_%s%s.npz" % (c["name"], suffix))
                np.savez_compressed(path, **data)
                print("  -> %s %.0f KiB" % (os.path.relpath(path, HERE), os.path.getsize(path) / 1024))
    for c in HG_CASES:
        if only and c["name"] not in only:
            continue
        path = os.path.join(HERE, "hourglass_meta_%s.npz" % c["name"])
        np.savez_compressed(path, **run_hourglass_case(c))
        print("  -> %s %.0f KiB" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
