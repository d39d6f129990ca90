"""Generate tests/golden/*.npz from the REAL reference implementation.

Runs only in the build container (needs /root/reference, imported read-only
through oracle/ref_harness.py).  The fixtures are what pins the oracle: the
upstream repository has no tests or golden vectors of its own.

    python tests/golden/make_golden.py

Each case stores its inputs (so tests never depend on RNG reproducibility),
`cam` = the reference's own per-pair float32 algebra on the generating machine
(P1inv | P2 | epipole; the SVD behind it is not bit-reproducible across CPUs,
and the layer is discontinuous in it), and the reference's outputs:
  sample_locs (K,N,H,W,2) | attn (N,K,H,W) | out (N,C,H,W) pre-z | corr_pos
    (for the larger cases sample_locs / attn keep only the rows listed in
    `rows`, i.e. sample_locs[:, :, rows] and attn[:, :, rows])
  finalout_eval  : bn(z(out))+out, BN in eval mode   (epipolar.py:249-253)
  finalout_train : same with BN batch statistics (+ running stats after)
  The residual fusion `ret + feat` (resnet.py:388) is a single float32 add of
  finalout and feat1, so it is not stored separately.
  grad_feat1 / grad_feat2     : autograd of sum(out * grad_out)
Semantics recorded in each file: align_corners=False (default of the torch in
this image, 2.10), USE_CORRECT_NORMALIZE as per case.
Optional per case: `image_resize` / `predict_resize` (DATASETS.IMAGE_RESIZE /
PREDICT_RESIZE; stored as the keys of the same names, a file without them means
1.0; the synthetic cameras project into the scaled image of image x image_resize
x predict_resize pixels, DATASETS.IMAGE_SIZE stays 4H) and `softmax_scale`
(EPIPOLAR.SOFTMAXSCALE; always stored as `softmax_scale`).
The cases added for the geometry settings stay within 1 MiB each: one pair at
10 x 10 for the 256-channel head, a three-row subset at 64 x 64.
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

CASES = [
    # name, H(=W), C, K, frames, image, jitter, relu, correct_normalize, softmax_enabled, views
    dict(name="tiny_16x16_c8_k8", H=16, C=8, K=8, frames=1, image=64, jitter=None, relu=True, correct=True, softmax=True),
    dict(name="mid_24x24_c8_k16_jitter", H=24, C=8, K=16, frames=1, image=96, jitter=(0.05, 5.0), relu=True, correct=True, softmax=True),
    dict(name="legacy_normalize_16x16_c8_k10", H=16, C=8, K=10, frames=1, image=64, jitter=(0.03, 3.0), relu=False, correct=False, softmax=True),
    dict(name="nosoftmax_16x16_c8_k12", H=16, C=8, K=12, frames=1, image=64, jitter=None, relu=True, correct=True, softmax=False),
    dict(name="h36m_64x64_c8_k64", H=64, C=8, K=64, frames=1, image=256, jitter=(0.05, 8.0), relu=True, correct=True, softmax=True, pairs=1, rows=(0, 13, 31, 50, 63)),
    dict(name="k128_32x32_c8", H=32, C=8, K=128, frames=1, image=128, jitter=(0.02, 2.0), relu=True, correct=True, softmax=True, pairs=1, rows=(0, 9, 17, 31)),
    dict(name="views8_16x16_c8_k16", H=16, C=8, K=16, frames=1, image=64, jitter=None, relu=True, correct=True, softmax=True, views=8),
    # the 256-channel head: these go through the MFMA tile kernels (forward and backward), so those are pinned to
    # outputs of the real reference directly and not only through the C oracle
    dict(name="head_16x16_c256_k16", H=16, C=256, K=16, frames=1, image=64, jitter=(0.05, 3.0), relu=True, correct=True, softmax=True, pairs=2),
    dict(name="head_24x24_c256_k33", H=24, C=256, K=33, frames=1, image=96, jitter=(0.05, 5.0), relu=True, correct=True, softmax=True, pairs=1),
    # ---- camera geometries beyond the look-at ring (synthetic.rig_pairs): at the 256-channel head, so that the MFMA tile
    # kernels (persistent, one block per tile, fused, all three backward forms) are pinned to the real reference on them, and
    # at 64 x 64 with 8 channels (selected rows) so that the oracle is pinned at the headline map size on every rig
    dict(name="rig_inside_16x16_c256_k16", rig="epipole_inside", H=16, C=256, K=16, frames=1, image=64, jitter=(0.05, 3.0), relu=True, correct=True, softmax=True),
    dict(name="rig_border_16x16_c256_k16", rig="epipole_border", H=16, C=256, K=16, frames=1, image=64, jitter=None, relu=True, correct=True, softmax=True),
    dict(name="rig_nearrect_x_16x16_c256_k16", rig="near_rectified_x", H=16, C=256, K=16, frames=1, image=64, jitter=None, relu=True, correct=True, softmax=True, pairs=1),
    dict(name="rig_nearrect_y_16x16_c256_k16", rig="near_rectified_y", H=16, C=256, K=16, frames=1, image=64, jitter=None, relu=True, correct=True, softmax=True, pairs=1),
    dict(name="rig_rectified_16x16_c256_k16", rig="rectified_x", H=16, C=256, K=16, frames=1, image=64, jitter=None, relu=True, correct=True, softmax=True, pairs=1),
    dict(name="rig_identical_16x16_c256_k16", rig="identical", H=16, C=256, K=16, frames=1, image=64, jitter=None, relu=True, correct=True, softmax=True, pairs=1),
    dict(name="rig_h36m_16x16_c256_k16", rig="h36m_room", H=16, C=256, K=16, frames=1, image=64, jitter=(0.05, 3.0), relu=True, correct=True, softmax=True, pair_index=(1, 2)),
    dict(name="rig_inside_64x64_c8_k64", rig="epipole_inside", H=64, C=8, K=64, frames=1, image=256, jitter=(0.05, 8.0), relu=True, correct=True, softmax=True, rows=(0, 13, 28, 29, 31, 50, 63)),
    dict(name="rig_border_64x64_c8_k64", rig="epipole_border", H=64, C=8, K=64, frames=1, image=256, jitter=None, relu=True, correct=True, softmax=True, rows=(0, 13, 30, 31, 50, 63)),
    dict(name="rig_nearrect_x_64x64_c8_k64", rig="near_rectified_x", H=64, C=8, K=64, frames=1, image=256, jitter=None, relu=True, correct=True, softmax=True, pairs=1, rows=(0, 13, 31, 32, 33, 50, 63)),
    dict(name="rig_nearrect_y_64x64_c8_k64", rig="near_rectified_y", H=64, C=8, K=64, frames=1, image=256, jitter=None, relu=True, correct=True, softmax=True, pairs=1, rows=(0, 13, 31, 50, 63)),
    dict(name="rig_h36m_64x64_c8_k64", rig="h36m_room", H=64, C=8, K=64, frames=1, image=256, jitter=(0.05, 8.0), relu=True, correct=True, softmax=True, rows=(0, 13, 31, 50, 63)),
    # ---- the geometry settings real configs use besides the headline one: legacy normalize (the default of core/config.py:118
    # and of five epipolar YAMLs), resize factors that are not powers of two (IMAGE_RESIZE 1000/256) and the built-in defaults
    # (IMAGE_RESIZE 2, PREDICT_RESIZE 4), a soft-max scale of 1/sqrt(K); 256 channels, so that the tile kernels run on them
    dict(name="legacy_10x10_c256_k16", H=10, C=256, K=16, frames=1, image=40, jitter=(0.05, 3.0), relu=True, correct=False, softmax=True, pairs=1),
    dict(name="legacy_inside_10x10_c256_k16", rig="epipole_inside", H=10, C=256, K=16, frames=1, image=40, jitter=(0.05, 3.0), relu=True, correct=False, softmax=True, pairs=1),
    dict(name="legacy_64x64_c8_k64", H=64, C=8, K=64, frames=1, image=256, jitter=(0.05, 8.0), relu=True, correct=False, softmax=True, pairs=1, rows=(0, 31, 63)),
    dict(name="resize3p9_10x10_c256_k16", H=10, C=256, K=16, frames=1, image=40, jitter=(0.05, 3.0), relu=True, correct=True, softmax=True, pairs=1, image_resize=3.90625),
    dict(name="resize2x4_legacy_10x10_c256_k16", H=10, C=256, K=16, frames=1, image=40, jitter=(0.05, 3.0), relu=True, correct=False, softmax=True, pairs=1, image_resize=2.0, predict_resize=4.0),
    dict(name="scale_10x10_c256_k33", H=10, C=256, K=33, frames=1, image=40, jitter=(0.05, 3.0), relu=True, correct=True, softmax=True, pairs=1, softmax_scale=33 ** -0.5),
]


def run_case(c):
    H = c["H"]
    ov = ["KEYPOINT.HEATMAP_SIZE", "(%d, %d)" % (H, H), "KEYPOINT.NFEATS", str(c["C"]),
          "EPIPOLAR.SAMPLESIZE", str(c["K"]), "DATASETS.IMAGE_SIZE", "(%d, %d)" % (c["image"], c["image"]),
          "EPIPOLAR.USE_CORRECT_NORMALIZE", str(c["correct"]), "EPIPOLAR.SOFTMAX_ENABLED", str(c["softmax"]),
          "VIS.EPIPOLAR_LINE", "True"]
    ir, pr = float(c.get("image_resize", 1.0)), float(c.get("predict_resize", 1.0))
    ov += ["DATASETS.IMAGE_RESIZE", repr(ir), "DATASETS.PREDICT_RESIZE", repr(pr)]
    if "softmax_scale" in c:
        ov += ["EPIPOLAR.SOFTMAXSCALE", repr(float(c["softmax_scale"]))]
    mod, cfg = rh.reference_epipolar(overrides=ov)
    seed = abs(hash(c["name"])) % 1000 if False else sum(map(ord, c["name"])) % 1000
    cam_image = c["image"] * ir * pr            # the cameras project into the image the resize factors scale the grid to
    if "rig" in c:
        P1, P2 = syn.rig_pairs(c["rig"], c["frames"], cam_image, seed=seed, jitter=c["jitter"])
    else:
        P1, P2 = syn.make_pairs(c["frames"], c.get("views", 4), cam_image, seed=seed, jitter=c["jitter"])
    if "pairs" in c:
        P1, P2 = P1[: c["pairs"]], P2[: c["pairs"]]
    if "pair_index" in c:
        P1, P2 = P1[list(c["pair_index"])], P2[list(c["pair_index"])]
    N = P1.shape[0]
    f1, f2 = syn.make_features(N, c["C"], H, H, seed=seed, relu=c["relu"])
    if c["relu"]:
        # exercise the exact-zero mask (epipolar.py:298): one all-zero reference pixel
        f1[0, :, 3, 5] = 0.0
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        mod.z.weight.normal_(0, 0.05, generator=g)
        mod.z.bias.normal_(0, 0.1, generator=g)
        mod.bn.weight.normal_(1, 0.1, generator=g)
        mod.bn.bias.normal_(0, 0.1, generator=g)
        mod.bn.running_mean.normal_(0, 0.1, generator=g)
        mod.bn.running_var.uniform_(0.5, 1.5, generator=g)
    grad_out = torch.randn(N, c["C"], H, H, generator=g)

    # ---- eval mode -------------------------------------------------------
    mod.eval()
    a1 = f1.clone().requires_grad_(True)
    a2 = f2.clone().requires_grad_(True)
    # pre-z output: run the reference with the z branch switched off
    cfg.defrost() if hasattr(cfg, "defrost") else None
    saved = cfg.EPIPOLAR.PARAMETERIZED
    dict.__setitem__(cfg.EPIPOLAR, "PARAMETERIZED", ())
    out, corr_pos, attn, locs = mod(a1, a2, P1, P2)
    (out * grad_out).sum().backward()
    dict.__setitem__(cfg.EPIPOLAR, "PARAMETERIZED", saved)
    with torch.no_grad():
        finalout_eval, _, _, _ = mod(f1, f2, P1, P2)
        rm, rv = mod.bn.running_mean.clone(), mod.bn.running_var.clone()
        mod.train()
        finalout_train, _, _, _ = mod(f1, f2, P1, P2)
        rm_after, rv_after = mod.bn.running_mean.clone(), mod.bn.running_var.clone()
    npf = lambda t: t.detach().numpy().astype(np.float32)
    # the per-pair float32 algebra exactly as the reference computed it ON THIS MACHINE (pinverse loop,
    # inverse, epipole: epipolar.py:336,344-348); LAPACK results differ in the last bits across CPUs
    a, b, e = orc.camera_algebra(P1, P2)
    cam = np.concatenate([a.reshape(N, 12), b.reshape(N, 12), e.reshape(N, 3)], 1).astype(np.float32)
    rows = list(c.get("rows", range(H)))
    data = dict(
        feat1=npf(f1), feat2=npf(f2), P1=npf(P1), P2=npf(P2), grad_out=npf(grad_out), cam=cam,
        z_weight=npf(mod.z.weight), z_bias=npf(mod.z.bias), bn_weight=npf(mod.bn.weight),
        bn_bias=npf(mod.bn.bias), bn_running_mean=npf(rm), bn_running_var=npf(rv),
        bn_running_mean_after=npf(rm_after), bn_running_var_after=npf(rv_after),
        sample_locs=npf(locs.transpose(0, 1))[:, :, rows],   # VIS.EPIPOLAR_LINE returns (N,K,H,W,2); store (K,N,rows,W,2)
        attn=npf(attn)[:, :, rows], out=npf(out), corr_pos=npf(corr_pos), rows=np.asarray(rows, np.int64),
        finalout_eval=npf(finalout_eval), finalout_train=npf(finalout_train),
        grad_feat1=npf(a1.grad), grad_feat2=npf(a2.grad),
        meta=np.array([H, H, c["C"], c["K"], N, c["image"], int(c["correct"]), int(c["softmax"]), 0], np.int64),
        softmax_scale=np.float32(cfg.EPIPOLAR.SOFTMAXSCALE),
        downsample=np.float32(cfg.BACKBONE.DOWNSAMPLE),
        torch_version=np.array(torch.__version__),
    )
    if "image_resize" in c or "predict_resize" in c:
        data.update(image_resize=np.float32(ir), predict_resize=np.float32(pr))
    return data


def main():
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    outdir = os.path.dirname(os.path.abspath(__file__))
    only = set(sys.argv[1:])          # optional: names of the cases to (re)generate; default all
    for c in CASES:
        if only and c["name"] not in only:
            continue
        data = run_case(c)
        path = os.path.join(outdir, c["name"] + ".npz")
        np.savez_compressed(path, **data)
        print("%-36s %7.1f KiB" % (c["name"], os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
