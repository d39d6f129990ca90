"""Parity of the HIP path (called through the C ABI) against
  (1) the golden vectors produced by the real reference, and
  (2) the CPU oracle on seeded inputs, up to BASELINE.json's full shape.

Tolerances (BASELINE.json north_star / SURVEY.md section 8c, float32):
  sample_locs <= 1e-5 (normalised units; measured 0), attn <= 1e-5,
  out / fused x <= 1e-4 absolute, corr_pos exact except at float ties,
  gradients <= 1e-4 relative to the tensor's max magnitude.
"""
import numpy as np
import pytest
import torch

from conftest import assert_corr_pos, golden_cases, load_golden

pytestmark = pytest.mark.gpu

TOL_LOCS, TOL_ATTN, TOL_OUT, TOL_GRAD_REL = 1e-5, 1e-5, 1e-4, 1e-4


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from epipolar_transformers_amd import _lib, camera, ops

    _lib.load()
    return _lib, camera, ops


def _resize(d):
    """DATASETS.IMAGE_RESIZE / PREDICT_RESIZE of a fixture (keys absent: 1.0, tests/golden/make_golden.py)"""
    return dict(image_resize=float(d.get("image_resize", 1.0)), predict_resize=float(d.get("predict_resize", 1.0)))


def _spec(ops, d, **kw):
    m = d["dims"]
    return ops.LayerSpec(H=m["H"], W=m["W"], K=m["K"], downsample=float(d["downsample"]),
                         correct_normalize=m["correct"], softmax_scale=float(d["softmax_scale"]),
                         softmax_enabled=m["softmax"], **_resize(d), **kw)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_forward(env, d, variant=0):
    _lib, camera, ops = env
    spec = _spec(ops, d, variant=variant)
    cam = _dev(d["cam"])
    ref = ops.to_nhwc(_dev(d["feat1"]))
    src = ops.to_nhwc(_dev(d["feat2"]))
    out, attn, corr = ops.forward_nhwc(spec, ref, src, cam)
    torch.cuda.synchronize()
    return spec, cam, ref, src, out.permute(0, 3, 1, 2).cpu().numpy(), attn.cpu().numpy(), corr.cpu().numpy()


def _assert_corr_pos(ops, spec, cam, corr, want_corr, attn, tie=2e-6, max_frac=2e-2):
    """conftest.assert_corr_pos with the sample locations of the HIP geometry kernel (bit-equal to the reference's):
    every pixel whose corr_pos differs from the reference's must be a proven arg-max tie."""
    corr, want_corr = np.asarray(corr), np.asarray(want_corr)
    if not (corr != want_corr).any():
        return 0.0
    locs = ops.sample_locs(spec, cam).cpu().numpy()                    # (K,N,H,W,2)
    return float(assert_corr_pos(locs, corr, want_corr, attn, spec.correct_normalize, tie, max_frac).mean())


def _close(got, want, atol, rtol=2e-6):
    err = np.abs(got - want) - rtol * np.abs(want)
    assert err.max() <= atol, "max|d|=%g (scale %g)" % (np.abs(got - want).max(), np.abs(want).max())


@pytest.mark.parametrize("case", golden_cases())
def test_sample_locs_vs_reference(env, case):
    _lib, camera, ops = env
    d = load_golden(case)
    spec = _spec(ops, d)
    cam = _dev(d["cam"])
    locs = ops.sample_locs(spec, cam).cpu().numpy()[:, :, d["rows"]]
    assert np.abs(locs - d["sample_locs"]).max() <= TOL_LOCS
    # the device evaluates the same IEEE float32 expression tree: expect bit equality
    assert np.array_equal(locs, d["sample_locs"])


# (1, 2, 3 select nothing in the library; like any bit outside the tile path's own they make the binding leave it)
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("case", golden_cases())
def test_forward_vs_reference(env, case, variant):
    _lib, camera, ops = env
    d = load_golden(case)
    spec, cam, ref, _, out, attn, corr = _run_forward(env, d, variant)
    if d["dims"]["C"] == 256 and variant == 0:
        # the 256-channel fixtures must really exercise the MFMA tile kernels
        import ctypes
        assert int(_lib.load().et_epipolar_forward_workspace_bytes(ctypes.byref(spec.desc(ref.shape[0], 256)))) > 0
    _close(attn[:, :, d["rows"]], d["attn"], TOL_ATTN)
    _close(out, d["out"], TOL_OUT)
    _assert_corr_pos(ops, spec, cam, corr, d["corr_pos"], attn)


@pytest.mark.parametrize("case", golden_cases())
def test_forward_vs_oracle_full_tensors(env, oracle_mod, case):
    d = load_golden(case)
    m = d["dims"]
    spec_o = oracle_mod.LayerSpec(m["H"], m["W"], m["K"], downsample=float(d["downsample"]),
                                  correct_normalize=m["correct"], softmax_scale=float(d["softmax_scale"]),
                                  softmax_enabled=m["softmax"], **_resize(d))
    want = oracle_mod.forward(spec_o, d["feat1"], d["feat2"], None, None, cam=d["cam"])
    spec, cam, _, _, out, attn, corr = _run_forward(env, d)
    _close(attn, want["attn"], TOL_ATTN)
    _close(out, want["out"], TOL_OUT)
    _assert_corr_pos(env[2], spec, cam, corr, want["corr_pos"], attn)


@pytest.mark.parametrize("case", golden_cases())
def test_zero_feature_pixel_uniform_attention(env, case):
    d = load_golden(case)
    if not (d["feat1"][0, :, 3, 5] == 0).all() or not d["dims"]["softmax"]:
        pytest.skip("no all-zero reference pixel in this case")
    _, _, _, _, out, attn, _ = _run_forward(env, d)
    assert np.allclose(attn[0, :, 3, 5], 1.0 / d["dims"]["K"], atol=1e-7)       # epipolar.py:298 (H3)


@pytest.mark.parametrize("gather", [True, False])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("case", golden_cases())
def test_backward_vs_reference_autograd(env, case, variant, gather):
    """gather=True: atomic-free gather-form d(feat_src) (workspace); False: float-atomic scatter."""
    _lib, camera, ops = env
    d = load_golden(case)
    spec, cam, ref, src, _, _, _ = _run_forward(env, d, variant)
    g = ops.to_nhwc(_dev(d["grad_out"]))
    forms = ["gather" if gather else "atomic"]
    if d["dims"]["C"] == 256 and variant == 0 and gather:
        forms.append("tile")            # the MFMA tile backward against the reference's autograd, directly
    for form in forms:
        g_ref, g_src = ops.backward_nhwc(spec, ref, src, cam, g, form=form)
        torch.cuda.synchronize()
        if form == "gather":            # no float atomics: bit-reproducible
            g_ref2, g_src2 = ops.backward_nhwc(spec, ref, src, cam, g, form="gather")
            assert torch.equal(g_src, g_src2) and torch.equal(g_ref, g_ref2)
        for got, want in ((g_ref, d["grad_feat1"]), (g_src, d["grad_feat2"])):
            got = got.permute(0, 3, 1, 2).cpu().numpy()
            scale = np.abs(want).max()
            assert np.abs(got - want).max() <= TOL_GRAD_REL * scale, (form, np.abs(got - want).max(), scale)


@pytest.mark.parametrize("case", golden_cases())
def test_backward_other_grad_masks_sum_to_full(env, case):
    """OTHER_GRAD (epipolar.py:141-153): the similarity-path and value-path
    gradients of feat_src add up to the full one."""
    _lib, camera, ops = env
    d = load_golden(case)
    spec, cam, ref, src, _, _, _ = _run_forward(env, d)
    g = ops.to_nhwc(_dev(d["grad_out"]))
    parts = []
    for mask in (3, 1, 2, 0):
        spec.src_grad_mask = mask
        g_ref, g_src = ops.backward_nhwc(spec, ref, src, cam, g)
        parts.append((g_ref.cpu().numpy(), g_src.cpu().numpy()))
    full, sim_only, val_only, none = parts
    scale = np.abs(full[1]).max()
    assert np.abs(sim_only[1] + val_only[1] - full[1]).max() <= 1e-5 * scale
    assert np.abs(none[1]).max() == 0
    for p in parts[1:]:
        assert np.abs(p[0] - full[0]).max() <= 1e-6 * max(1.0, np.abs(full[0]).max())   # d(feat_ref) never masked


@pytest.mark.parametrize("case", golden_cases())
def test_module_dropin_eval_and_train(env, case):
    """The nn.Module boundary: same ctor/forward/returns/state_dict keys as the
    reference operator; eval mode uses the fused epilogue kernel, train mode
    batch statistics."""
    from epipolar_transformers_amd import default_cfg
    from epipolar_transformers_amd.epipolar import Epipolar

    _lib, camera, ops = env
    d = load_golden(case)
    m = d["dims"]
    cfg = default_cfg()
    cfg.merge_from_list(["KEYPOINT.HEATMAP_SIZE", (m["H"], m["W"]), "KEYPOINT.NFEATS", m["C"],
                         "EPIPOLAR.SAMPLESIZE", m["K"], "EPIPOLAR.ATTENTION", "avg",
                         "EPIPOLAR.PARAMETERIZED", ("z",), "EPIPOLAR.ZRESIDUAL", True,
                         "EPIPOLAR.USE_CORRECT_NORMALIZE", m["correct"], "EPIPOLAR.SOFTMAX_ENABLED", m["softmax"],
                         "EPIPOLAR.SOFTMAXSCALE", float(d["softmax_scale"]), "VIS.EPIPOLAR_LINE", True,
                         "DATASETS.IMAGE_RESIZE", _resize(d)["image_resize"], "DATASETS.PREDICT_RESIZE", _resize(d)["predict_resize"]])
    mod = Epipolar(cfg=cfg).cuda()
    assert sorted(mod.state_dict()) == sorted(["z.weight", "z.bias", "bn.weight", "bn.bias", "bn.running_mean",
                                               "bn.running_var", "bn.num_batches_tracked"])
    sd = {"z.weight": d["z_weight"], "z.bias": d["z_bias"], "bn.weight": d["bn_weight"], "bn.bias": d["bn_bias"],
          "bn.running_mean": d["bn_running_mean"], "bn.running_var": d["bn_running_var"]}
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    f1, f2 = _dev(d["feat1"]), _dev(d["feat2"])
    P1, P2 = torch.from_numpy(d["P1"]), torch.from_numpy(d["P2"])       # host-resident, as the loader yields them
    mod.eval()
    with torch.no_grad():
        fin, corr, depth, locs = mod(f1, f2, P1, P2)
        x, _, _, _ = mod.forward_fused(f1, f2, P1.cuda(), P2.cuda())   # device-resident P also accepted
    assert tuple(fin.shape) == d["finalout_eval"].shape and tuple(depth.shape) == (m["N"], m["K"], m["H"], m["W"])
    assert tuple(corr.shape) == (m["N"], m["H"], m["W"], 2) and tuple(locs.shape) == (m["N"], m["K"], m["H"], m["W"], 2)
    if not np.array_equal(camera.pair_algebra(P1, P2).numpy(), d["cam"]):
        # LAPACK on this host rounds the SVD differently from the machine that made the fixture: the
        # module (which runs the algebra itself) can then only be held to the fixture away from the
        # layer's discontinuities -- compare against the oracle fed with THIS host's algebra instead.
        from oracle import oracle as orc

        so = orc.LayerSpec(m["H"], m["W"], m["K"], downsample=float(d["downsample"]), correct_normalize=m["correct"],
                           softmax_scale=float(d["softmax_scale"]), softmax_enabled=m["softmax"], **_resize(d))
        w = orc.forward(so, d["feat1"], d["feat2"], P1, P2)
        for key, tr in (("finalout_eval", False), ("finalout_train", True)):
            fin_o, _, rm_o, rv_o = orc.epilogue(w["out"], d["feat1"], d["z_weight"], d["z_bias"], d["bn_weight"], d["bn_bias"],
                                                d["bn_running_mean"], d["bn_running_var"], training=tr, return_stats=True)
            d[key] = fin_o.numpy()
        d["bn_running_mean_after"], d["bn_running_var_after"] = rm_o.numpy(), rv_o.numpy()      # (of the training-mode call)
        d["out"] = w["out"]
        d["sample_locs"] = w["sample_locs"][:, :, d["rows"]]
        d["grad_feat1"], d["grad_feat2"] = orc.backward(so, d["feat1"], d["feat2"], w["sample_locs"], d["grad_out"])
    # with the soft-max off a masked sample keeps its -1e10/K weight: |out| reaches 1e9 and the z/BN
    # epilogue cancels it by orders of magnitude -- hold that case to float32 noise of the operands
    tol_fin = TOL_OUT if m["softmax"] else 2e-6 * float(np.abs(d["out"]).max())
    _close(fin.cpu().numpy(), d["finalout_eval"], tol_fin)
    _close(x.cpu().numpy(), d["finalout_eval"] + d["feat1"], tol_fin)      # resnet.py:388
    assert np.array_equal(locs.cpu().numpy().transpose(1, 0, 2, 3, 4)[:, :, d["rows"]], d["sample_locs"])
    mod.train()
    with torch.no_grad():
        fin_t, _, _, _ = mod(f1, f2, P1, P2)
    # train mode divides z(out) by the BATCH standard deviation (stock torch ops here, as in the reference).  A channel of
    # z(out) that hardly varies over the batch -- the 8-channel fixtures have channels with variance 3e-5 around a mean of 0.2
    # -- is ill-conditioned: float32-level differences in `out` (tolerance 1e-4, held above) move that variance by 1e-4
    # relative and are then multiplied by |gamma| / sqrt(var + eps), up to 150.  The 256-channel fixtures sit at 10-15.
    y_ref = torch.nn.functional.conv2d(torch.from_numpy(d["out"]), torch.from_numpy(d["z_weight"]), torch.from_numpy(d["z_bias"]))
    amp = float((np.abs(d["bn_weight"]) / np.sqrt(y_ref.var((0, 2, 3), unbiased=False).numpy() + 1e-5)).max())
    _close(fin_t.cpu().numpy(), d["finalout_train"], tol_fin * max(1.0, amp / 10.0), rtol=1e-5)
    # batch statistics are sums over N*H*W values; with the soft-max off a masked sample keeps its
    # -1e10/K weight, the sums cancel by ~3 orders of magnitude and carry that much float32 noise
    _close(mod.bn.running_mean.cpu().numpy(), d["bn_running_mean_after"], 1e-5, rtol=1e-5 if m["softmax"] else 2e-3)
    _close(mod.bn.running_var.cpu().numpy(), d["bn_running_var_after"], 1e-5, rtol=1e-5 if m["softmax"] else 2e-3)
    # autograd through the module (train mode), gradients of sum(out * grad_out) w.r.t. both maps
    a1, a2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    out, _, _ = mod.attend(a1, a2, P1, P2)
    (out * _dev(d["grad_out"])).sum().backward()
    for got, want in ((a1.grad, d["grad_feat1"]), (a2.grad, d["grad_feat2"])):
        scale = np.abs(want).max()
        assert np.abs(got.cpu().numpy() - want).max() <= TOL_GRAD_REL * scale


def test_layout_converters_roundtrip(env):
    _lib, camera, ops = env
    x = torch.randn(3, 20, 7, 9, device="cuda")
    nhwc = ops.to_nhwc(x)
    assert torch.equal(nhwc, x.permute(0, 2, 3, 1).contiguous())
    assert torch.equal(ops.to_nchw_contiguous(nhwc), x)
    cl = x.contiguous(memory_format=torch.channels_last)
    assert ops.to_nhwc(cl).data_ptr() == cl.data_ptr()          # zero-copy for channels_last producers


# ---------------------------------------------------------------------------------------
# BASELINE.json shapes
# ---------------------------------------------------------------------------------------
def _full_inputs(frames, views, H, C, image, seed):
    from epipolar_transformers_amd import synthetic as syn

    P1, P2 = syn.make_pairs(frames, views, image, seed=seed, jitter=(0.05, 8.0))
    f1, f2 = syn.make_features(P1.shape[0], C, H, H, seed=seed)
    return P1, P2, f1, f2


@pytest.mark.parametrize("shape", [dict(H=64, C=256, K=64, image=256, views=4, name="config2 R50 256x256"),
                                   dict(H=96, C=256, K=64, image=384, views=4, name="config4 R152 384x384"),
                                   dict(H=128, C=256, K=128, image=512, views=8, name="config5 stress")])
@pytest.mark.parametrize("variant", [0, 16384])
def test_full_shape_pairs_vs_oracle(env, oracle_mod, shape, variant):
    """BASELINE.json configs 2/4/5 at their real C, HxW and K, on a few pairs the
    oracle finishes in seconds (full tensors compared)."""
    _lib, camera, ops = env
    H, C, K = shape["H"], shape["C"], shape["K"]
    P1, P2, f1, f2 = _full_inputs(1, shape["views"], H, C, shape["image"], seed=11)
    P1, P2, f1, f2 = P1[:2], P2[:2], f1[:2], f2[:2]
    f1[0, :, 5, 7] = 0
    # 0: default (MFMA tiles where eligible: configs 2 and 4), 16384: the per-pixel kernels (4 pixels/wave at
    # C=256, K<=64; 1 pixel/wave at K=128)
    spec = ops.LayerSpec(H=H, W=H, K=K, variant=variant)
    cam = camera.pair_algebra(P1, P2).cuda()
    ref, src = ops.to_nhwc(f1.cuda()), ops.to_nhwc(f2.cuda())
    bias = torch.linspace(-1, 1, C, device="cuda")
    out, attn, corr, base = ops.forward_nhwc(spec, ref, src, cam, res_bias=bias, want_res_base=True)
    assert torch.equal(base, ref + bias)                     # additive term of the residual fusion
    want = oracle_mod.forward(oracle_mod.LayerSpec(H, H, K), f1, f2, None, None, cam=cam.cpu().numpy())
    _close(attn.cpu().numpy(), want["attn"], TOL_ATTN)
    _close(out.permute(0, 3, 1, 2).cpu().numpy(), want["out"], TOL_OUT)
    _assert_corr_pos(ops, spec, cam, corr.cpu().numpy(), want["corr_pos"], attn.cpu().numpy())
    locs = ops.sample_locs(spec, cam).cpu().numpy()
    assert np.array_equal(locs, want["sample_locs"])
    # gradients at full C on one pair
    g = torch.randn(1, C, H, H, generator=torch.Generator().manual_seed(5))
    g1, g2 = oracle_mod.backward(oracle_mod.LayerSpec(H, H, K), f1[:1].numpy(), f2[:1].numpy(),
                                 want["sample_locs"][:, :1], g.numpy())
    spec1 = ops.LayerSpec(H=H, W=H, K=K)
    for form in ("tile", "gather", "atomic"):
        gr, gs = ops.backward_nhwc(spec1, ref[:1].contiguous(), src[:1].contiguous(), cam[:1].contiguous(),
                                   ops.to_nhwc(g.cuda()), form=form)
        for got, wantg in ((gr, g1), (gs, g2)):
            scale = np.abs(wantg).max()
            assert np.abs(got.permute(0, 3, 1, 2).cpu().numpy() - wantg).max() <= TOL_GRAD_REL * scale


def test_config2_full_batch_properties(env):
    """Config 2 at its full size (N=128, C=256, 64x64, K=64): size-independent
    properties instead of an oracle run."""
    _lib, camera, ops = env
    P1, P2, f1, f2 = _full_inputs(32, 4, 64, 256, 256, seed=0)
    spec = ops.LayerSpec(H=64, W=64, K=64)
    cam = camera.pair_algebra(P1, P2).cuda()
    ref, src = ops.to_nhwc(f1.cuda()), ops.to_nhwc(f2.cuda())
    out, attn, corr = ops.forward_nhwc(spec, ref, src, cam)
    # (1) soft-max rows sum to one
    assert (attn.sum(1) - 1).abs().max().item() < 1e-5
    # (2) determinism: the forward has no atomics, a second launch is bit-identical
    out2, attn2, corr2 = ops.forward_nhwc(spec, ref, src, cam)
    assert torch.equal(out, out2) and torch.equal(attn, attn2) and torch.equal(corr, corr2)
    # (3) all variants agree
    for v in (65536, 16384):
        spec_v = ops.LayerSpec(H=64, W=64, K=64, variant=v)
        out_v, attn_v, _ = ops.forward_nhwc(spec_v, ref, src, cam)
        assert (out_v - out).abs().max().item() <= 1e-5 and (attn_v - attn).abs().max().item() <= 3e-6   # (spec: 1e-4 / 1e-5 vs the reference)
    # (4) a constant source map: every channel sees the same weights, so all channels of a pixel
    #     are equal, and zero padding can only remove mass: 0 <= out <= 1
    ones = torch.ones_like(src)
    out1, attn1, _ = ops.forward_nhwc(spec, ref, ones, cam)
    assert out1.max().item() <= 1 + 1e-5 and out1.min().item() >= 0
    assert (out1.amax(-1) - out1.amin(-1)).max().item() <= 1e-6
    assert out1.mean().item() > 0.5
    # (5) out is linear in the VALUE role of feat_src for fixed attention: scaling the source by 2
    #     with logits compensated (feat_ref / 2) doubles the output exactly (power of two)
    out_s, attn_s, _ = ops.forward_nhwc(spec, (ref * 0.5).contiguous(), (src * 2).contiguous(), cam)
    assert torch.equal(attn_s, attn) and torch.equal(out_s, out * 2)
    # (6) checksum of checksums vs the per-pair launches (batching must not change a pair's result)
    sub = slice(40, 44)
    out_p, attn_p, _ = ops.forward_nhwc(spec, ref[sub].contiguous(), src[sub].contiguous(), cam[sub].contiguous())
    assert torch.equal(out_p, out[sub]) and torch.equal(attn_p, attn[sub])


def test_pose_backbone_multiview_forward(env, oracle_mod):
    """Row (b) of the boundary on the GPU: `epipolarposeR-18` called the way Modelbuilder does
    (model.py:241-247): a source pass with other_inputs=None, then the reference pass with the
    source features; the fused layer inside must equal trunk features -> oracle -> epilogue."""
    _lib, camera, ops = env
    from epipolar_transformers_amd import backbones, default_cfg, synthetic as syn

    size, hs = 64, 16
    cfg = default_cfg()
    cfg.merge_from_list(["BACKBONE.BODY", "epipolarposeR-18", "BACKBONE.PRETRAINED", False,
                         "KEYPOINT.HEATMAP_SIZE", (hs, hs), "KEYPOINT.NUM_PTS", 17, "KEYPOINT.SIGMA", 2.0,
                         "DATASETS.IMAGE_SIZE", (size, size), "EPIPOLAR.MERGE", "late", "EPIPOLAR.ATTENTION", "avg",
                         "EPIPOLAR.PARAMETERIZED", ("z",), "EPIPOLAR.ZRESIDUAL", True,
                         "EPIPOLAR.USE_CORRECT_NORMALIZE", True, "EPIPOLAR.SAMPLESIZE", 16])
    torch.manual_seed(3)
    net = backbones.build_backbone(cfg).cuda().eval()
    with torch.no_grad():
        net.epipolar_sampler.bn.weight.normal_(1, 0.1)
        net.epipolar_sampler.bn.bias.normal_(0, 0.1)
    P1, P2 = syn.make_pairs(1, 4, size, seed=2, jitter=(0.03, 2.0))
    img = torch.randn(4, 3, size, size, device="cuda")
    other = img.roll(-1, 0)                                        # view v+1 is the source of view v
    with torch.no_grad():
        src_feat = net(other)[0]                                   # model.py:244
        feat, heat, locs, scos, corr, depth, sl, _ = net(img, [src_feat, P2, None, P1, None, None, other])
    assert tuple(heat[0].shape) == (4, 17, hs, hs) and tuple(depth.shape) == (4, 16, hs, hs)
    f1, f2 = feat.float().cpu(), src_feat.float().cpu()
    so = oracle_mod.LayerSpec(hs, hs, 16)
    cam = camera.pair_algebra(P1, P2).numpy()
    want = oracle_mod.forward(so, f1.numpy(), f2.numpy(), None, None, cam=cam)
    s = net.epipolar_sampler
    fin, fused = oracle_mod.epilogue(want["out"], f1.numpy(), s.z.weight.detach().cpu().numpy(),
                                     s.z.bias.detach().cpu().numpy(), s.bn.weight.detach().cpu().numpy(),
                                     s.bn.bias.detach().cpu().numpy(), s.bn.running_mean.cpu().numpy(),
                                     s.bn.running_var.cpu().numpy(), training=False)
    with torch.no_grad():
        want_heat = net.final_layer(fused.cuda()).cpu().numpy()
    scale = max(1.0, float(np.abs(want_heat).max()))
    assert np.abs(heat[0].cpu().numpy() - want_heat).max() <= 1e-4 * scale
    _close(depth.cpu().numpy(), want["attn"], TOL_ATTN)


def test_mpjpe_delta_vs_reference_pipeline(env):
    """BASELINE.json: 'MPJPE within 0.1 mm of reference'.  The frozen scene holds the REAL reference's 2-D
    detections (reference Epipolar.forward + `ret + feat` + 1x1 head + its own peak finder, CPU).  The same
    feature maps go through the MI355X path; both sets of detections are triangulated by the same batched DLT."""
    import os

    from conftest import GOLDEN_DIR
    from epipolar_transformers_amd import default_cfg
    from epipolar_transformers_amd.backbones import find_peaks as soft_argmax_peaks     # the HIP peak kernel on the GPU
    from epipolar_transformers_amd.epipolar import Epipolar
    from epipolar_transformers_amd.triangulate import mpjpe, triangulate_dlt

    _lib, camera, ops = env
    d = np.load(os.path.join(GOLDEN_DIR, "mpjpe_scene.npz"))
    V, J, C, HS, IMG, K = [int(v) for v in d["meta"]]
    cfg = default_cfg()
    cfg.merge_from_list(["KEYPOINT.HEATMAP_SIZE", (HS, HS), "KEYPOINT.NFEATS", C, "EPIPOLAR.SAMPLESIZE", K,
                         "EPIPOLAR.ATTENTION", "avg", "EPIPOLAR.PARAMETERIZED", ("z",), "EPIPOLAR.ZRESIDUAL", True,
                         "EPIPOLAR.USE_CORRECT_NORMALIZE", True, "DATASETS.IMAGE_SIZE", (IMG, IMG)])
    mod = Epipolar(cfg=cfg).cuda().eval()
    mod.load_state_dict({k: torch.from_numpy(d[v]) for k, v in
                         (("z.weight", "z_weight"), ("z.bias", "z_bias"), ("bn.weight", "bn_weight"),
                          ("bn.bias", "bn_bias"), ("bn.running_mean", "bn_mean"), ("bn.running_var", "bn_var"))},
                        strict=False)
    feat = _dev(d["feat"])
    P = torch.from_numpy(d["P"])
    # the reference's own per-pair algebra travels with the fixture (LAPACK differs across hosts)
    mod._cams.get = lambda *a, **k: _dev(d["cam"])
    with torch.no_grad():
        x, corr, depth, _ = mod.forward_fused(feat, feat.roll(-1, 0).contiguous(), P, P.roll(-1, 0))
        heat = torch.nn.functional.conv2d(x, _dev(d["final_w"]), _dev(d["final_b"]))
        locs, scos = soft_argmax_peaks(heat, float(d["sigma"]), 4)
    ref_locs = torch.from_numpy(d["ref_locs"]).double()
    assert (locs.cpu().double() - ref_locs).abs().max().item() < 1e-2        # image pixels
    Pd = P.double()[None]
    X_ref = triangulate_dlt(ref_locs[None], Pd, torch.from_numpy(d["ref_scores"])[None])
    X_new = triangulate_dlt(locs.cpu().double()[None], Pd, scos.cpu()[None])
    delta = mpjpe(X_new, X_ref).item()
    print("MPJPE delta vs reference pipeline: %.5f mm; vs ground truth: ref %.2f mm, ours %.2f mm" %
          (delta, mpjpe(X_ref[0], torch.from_numpy(d["joints"])).item(),
           mpjpe(X_new[0], torch.from_numpy(d["joints"])).item()))
    assert delta < 0.1                                                       # mm


@pytest.mark.parametrize("shape", [dict(H=10, W=10, C=256, K=16), dict(H=9, W=7, C=256, K=20), dict(H=12, W=20, C=32, K=9),
                                   dict(H=7, W=13, C=12, K=70), dict(H=5, W=6, C=260, K=8),
                                   dict(H=32, W=32, C=256, K=128), dict(H=20, W=24, C=256, K=200),
                                   dict(H=128, W=128, C=256, K=48),
                                   # the one-pixel-per-wave forward at two float4 groups per lane: one sample per lane with
                                   # a short last batch, two per lane with K a multiple of 8 and not
                                   dict(H=9, W=7, C=260, K=12), dict(H=9, W=7, C=260, K=72), dict(H=9, W=7, C=260, K=76),
                                   # ... and four samples per lane in all four slots: K a multiple of 8 and not, and one
                                   # float4 group per lane with a short last batch
                                   dict(H=9, W=7, C=260, K=200), dict(H=9, W=7, C=260, K=204), dict(H=9, W=7, C=32, K=204)])
@pytest.mark.parametrize("variant", [0, 32768, 16384, 28])
def test_ragged_shapes_vs_oracle(env, oracle_mod, shape, variant):
    """Non-square maps, H*W not a multiple of the 16-pixel block / 32-pixel tile (partial blocks, padded tiles),
    K not a multiple of the batch, K > 64 on the tile path, C below/above one wave of float4 -- forward,
    residual base and both backward forms.  Variant 0 takes the MFMA tile kernel for the C=256 shapes, 32768
    the same with 64-row tiles (tiles overflow and are split into pixel groups), 16384 the per-pixel kernels.
    The bits that were the per-pixel kernels' round-1 switches (28 among them) are accepted and select nothing."""
    _lib, camera, ops = env
    from epipolar_transformers_amd import synthetic as syn

    H, W, C, K = shape["H"], shape["W"], shape["C"], shape["K"]
    if variant == 32768 and (C != 256 or 4 * min(K, max(H, W)) > 64):
        pytest.skip("64-row tile splitting applies to C=256 with 4*min(K, max(H,W)) <= 64")
    if H * W >= 16384 and variant not in (0, 16384):
        pytest.skip("the largest map (bitonic ordering of 16384 pixels, 384-row tiles) is checked on the two defaults")
    P1, P2 = syn.make_pairs(1, 4, 64, seed=21, jitter=(0.05, 2.0))
    P1, P2 = P1[:3], P2[:3]
    g = torch.Generator().manual_seed(H * 100 + W)
    f1 = torch.randn(3, C, H, W, generator=g).relu()
    f2 = torch.randn(3, C, H, W, generator=g).relu()
    go = torch.randn(3, C, H, W, generator=g)
    # a non-square grid in the reference means HEATMAP_SIZE=(H,W) with image (4H,4W): xs from W, ys from H
    spec = ops.LayerSpec(H=H, W=W, K=K, variant=variant)
    so = oracle_mod.LayerSpec(H, W, K)
    cam = camera.pair_algebra(P1, P2)
    want = oracle_mod.forward(so, f1, f2, None, None, cam=cam.numpy())
    ref, src = ops.to_nhwc(f1.cuda()), ops.to_nhwc(f2.cuda())
    out, attn, corr, base = ops.forward_nhwc(spec, ref, src, cam.cuda(), want_res_base=True)
    assert torch.equal(base, ref)
    _close(attn.cpu().numpy(), want["attn"], TOL_ATTN)
    _close(out.permute(0, 3, 1, 2).cpu().numpy(), want["out"], TOL_OUT)
    _assert_corr_pos(ops, spec, cam.cuda(), corr.cpu().numpy(), want["corr_pos"], attn.cpu().numpy(), max_frac=5e-2)
    assert np.array_equal(ops.sample_locs(spec, cam.cuda()).cpu().numpy(), want["sample_locs"])
    g1, g2 = oracle_mod.backward(so, f1.numpy(), f2.numpy(), want["sample_locs"], go.numpy())
    forms = ["gather", "atomic"] + (["tile"] if C == 256 and variant in (0, 32768) else [])
    for form in forms:
        gr, gs = ops.backward_nhwc(spec, ref, src, cam.cuda(), ops.to_nhwc(go.cuda()), form=form)
        for got, wantg in ((gr, g1), (gs, g2)):
            scale = max(np.abs(wantg).max(), 1e-6)
            assert np.abs(got.permute(0, 3, 1, 2).cpu().numpy() - wantg).max() <= TOL_GRAD_REL * scale
    if variant == 16384 and (H, W, C, K) == (10, 10, 256, 16):
        retired = ops.LayerSpec(H=H, W=W, K=K, variant=16384 | 28 | 256 | 1024 | 2048 | 512 | 3)
        for got, same in zip(ops.forward_nhwc(retired, ref, src, cam.cuda(), want_res_base=True), (out, attn, corr, base)):
            assert torch.equal(got, same)
        for got, same in zip(ops.backward_nhwc(retired, ref, src, cam.cuda(), ops.to_nhwc(go.cuda()), form="gather"),
                             ops.backward_nhwc(spec, ref, src, cam.cuda(), ops.to_nhwc(go.cuda()), form="gather")):
            assert torch.equal(got, same)


def test_tile_path_statistics_and_split(env):
    """The MFMA tile path: epipolar-line ordering keeps the row set of a 32-pixel tile small (no tile of the
    headline geometry overflows 256 rows), and the 64-row test variant really exercises the group splitting
    while giving the same results."""
    _lib, camera, ops = env
    P1, P2, f1, f2 = _full_inputs(1, 4, 64, 256, 256, seed=13)
    cam = camera.pair_algebra(P1, P2).cuda()
    ref, src = ops.to_nhwc(f1.cuda()), ops.to_nhwc(f2.cuda())
    n = P1.shape[0]
    for variant in (0, _lib.ET_VARIANT_TILE_CLASSIC):        # warp-specialised persistent kernel, one block per tile
        spec = ops.LayerSpec(H=64, W=64, K=64, variant=variant)
        ws = ops.tile_workspace(spec, n, 256, "cuda")
        out, attn, corr = ops.forward_nhwc(spec, ref, src, cam, workspace=ws)
        torch.cuda.synchronize()
        st = ops.tile_stats(spec, n, 256, ws).cpu().numpy()
        rows, groups = st & 0xFFFF, st >> 16
        assert groups.min() == 1 and groups.max() == 1 and rows.max() <= 256
        assert rows[rows > 0].mean() < 200            # a pixel alone touches ~130 rows: the tiles are tight
    # small map, 64-row tiles: most tiles must split
    H = W = 16
    P1, P2 = _full_inputs(1, 4, H, 256, 64, seed=14)[:2]
    g = torch.Generator().manual_seed(3)
    r16 = torch.randn(4, H, W, 256, generator=g).relu().cuda()
    s16 = torch.randn(4, H, W, 256, generator=g).relu().cuda()
    cam16 = camera.pair_algebra(P1, P2).cuda()
    o_pp, a_pp, _ = ops.forward_nhwc(ops.LayerSpec(H=H, W=W, K=16, variant=16384), r16, s16, cam16)
    o_full, a_full, _ = ops.forward_nhwc(ops.LayerSpec(H=H, W=W, K=16), r16, s16, cam16)
    assert (o_full - o_pp).abs().max().item() <= TOL_OUT and (a_full - a_pp).abs().max().item() <= TOL_ATTN
    # 32768: the persistent kernel hands every overflowing tile to the list kernel, which splits it;
    # 32768 | classic: the one-block-per-tile kernel splits in place
    for variant in (_lib.ET_VARIANT_TILE_SPLIT, _lib.ET_VARIANT_TILE_SPLIT | _lib.ET_VARIANT_TILE_CLASSIC):
        spec = ops.LayerSpec(H=H, W=W, K=16, variant=variant)
        ws = ops.tile_workspace(spec, 4, 256, "cuda")
        o_split, a_split, _ = ops.forward_nhwc(spec, r16, s16, cam16, workspace=ws)
        torch.cuda.synchronize()
        st = ops.tile_stats(spec, 4, 256, ws).cpu().numpy()
        assert (st >> 16).min() >= 1 and (st >> 16).max() > 1, "no tile was split: the test does not cover the group loop"
        assert (o_split - o_pp).abs().max().item() <= TOL_OUT and (a_split - a_pp).abs().max().item() <= TOL_ATTN


def test_tiled_backward_masks_and_split(env):
    """The MFMA tile backward (C=256): equals the bit-reproducible gather form to rounding for every OTHER_GRAD mask,
    in its merged form (Bs and B at once, one round of atomics per tile) and as the one-array kernel, also when 64-row
    tiles force the pixel-group splitting (no group may run twice: d(feat_src) is accumulated with atomics)."""
    _lib, camera, ops = env
    # variant 0: the merged form (two arrays, one round of atomics); 65536: the one-array kernel; 32768: 64-row tiles
    for (H, K, variant) in ((16, 16, 0), (16, 16, 65536), (16, 16, 32768), (24, 33, 0), (24, 33, 65536)):
        P1, P2 = _full_inputs(1, 4, H, 256, H * 4, seed=31)[:2]
        g = torch.Generator().manual_seed(H + K)
        ref = torch.randn(4, H, H, 256, generator=g).relu().cuda()
        src = torch.randn(4, H, H, 256, generator=g).relu().cuda()
        go = torch.randn(4, H, H, 256, generator=g).cuda()
        ref[0, 3, 5] = 0                                     # an all-masked pixel
        cam = camera.pair_algebra(P1, P2).cuda()
        for mask in (3, 1, 2, 0):
            spec = ops.LayerSpec(H=H, W=H, K=K, variant=variant, src_grad_mask=mask)
            gr_t, gs_t = ops.backward_nhwc(spec, ref, src, cam, go, form="tile")
            gr_g, gs_g = ops.backward_nhwc(spec, ref, src, cam, go, form="gather")
            # the same with the attention the forward returned (no soft-max recomputation; the all-masked pixel is
            # recognised by its uniform attention) -- from the default forward and from the exact-fp32 per-pixel one
            attn_w = ops.forward_nhwc(ops.LayerSpec(H=H, W=H, K=K), ref, src, cam)[1]
            attn_p = ops.forward_nhwc(ops.LayerSpec(H=H, W=H, K=K, variant=_lib.ET_VARIANT_NO_TILE), ref, src, cam)[1]
            gr_a, gs_a = ops.backward_nhwc(spec, ref, src, cam, go, form="tile", attn=attn_w)
            gr_b, gs_b = ops.backward_nhwc(spec, ref, src, cam, go, form="tile", attn=attn_p)
            for got, want in ((gr_t, gr_g), (gs_t, gs_g), (gr_a, gr_g), (gs_a, gs_g), (gr_b, gr_g), (gs_b, gs_g)):
                scale = max(want.abs().max().item(), 1e-6)
                assert (got - want).abs().max().item() <= TOL_GRAD_REL * scale, (H, K, variant, mask)
            assert gr_a[0, 3, 5].abs().max().item() == 0 and gr_g[0, 3, 5].abs().max().item() == 0   # masked: no gradient
            if mask == 0:
                assert gs_t.abs().max().item() == 0 and gs_a.abs().max().item() == 0
    with pytest.raises(_lib.EpipolarAmdError):               # outside the tile path: loud, no silent fallback
        ops.backward_nhwc(ops.LayerSpec(H=8, W=8, K=8), torch.zeros(1, 8, 8, 32, device="cuda"),
                          torch.zeros(1, 8, 8, 32, device="cuda"), torch.zeros(1, 27, device="cuda"),
                          torch.zeros(1, 8, 8, 32, device="cuda"), form="tile")


def test_tiled_backward_split_gemm_guard_redoes_overflowing_tiles_in_fp32(env):
    """The merged tile backward runs its D-type GEMMs as split-fp16 products under a per-pair scale ESTIMATED from
    sampled pixels (every fourth pixel at 16 x 16); a source value outside the sample that the scale pushes beyond fp16
    makes the block redo the tile's GEMM in exact fp32 -- gradients still equal the gather form, never inf / NaN."""
    _lib, camera, ops = env
    H, K = 16, 16
    P1, P2 = _full_inputs(1, 4, H, 256, H * 4, seed=37)[:2]
    g = torch.Generator().manual_seed(5)
    ref = torch.randn(4, H, H, 256, generator=g).relu().cuda()
    src = torch.randn(4, H, H, 256, generator=g).relu().cuda()
    go = torch.randn(4, H, H, 256, generator=g).cuda()
    src[1, 5, 6, 100] = 4e4                                  # pixel 86: not a multiple of four, i.e. outside the sample
    src[2, 9, 3, 7] = -6e4
    cam = camera.pair_algebra(P1, P2).cuda()
    spec = ops.LayerSpec(H=H, W=H, K=K)
    attn = ops.forward_nhwc(ops.LayerSpec(H=H, W=H, K=K, variant=_lib.ET_VARIANT_NO_TILE), ref, src, cam)[1]
    gr_g, gs_g = ops.backward_nhwc(spec, ref, src, cam, go, form="gather")
    for kw in (dict(), dict(attn=attn)):
        gr_t, gs_t = ops.backward_nhwc(spec, ref, src, cam, go, form="tile", **kw)
        for got, want in ((gr_t, gr_g), (gs_t, gs_g)):
            assert torch.isfinite(got).all()
            assert ((got - want).abs() - 1e-5 * want.abs()).max().item() <= TOL_GRAD_REL * max(want.abs().median().item() * 50, 1e-6)


# ---------------------------------------------------------------------------------------
# exported surface that had no test: et_residual_epilogue, the un-parameterised layer, MERGE early / both
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [256, 12])
def test_residual_epilogue_abi(env, C):
    """et_residual_epilogue: finalout = out + y*scale + shift (epipolar.py:250-253), x = feat + finalout
    (resnet.py:388); y/scale/shift nullable (un-parameterised layer), finalout / x individually nullable."""
    _lib, camera, ops = env
    g = torch.Generator(device="cuda").manual_seed(C)
    shape = (3, 7, 9, C)
    feat, out, y = (torch.randn(shape, device="cuda", generator=g) for _ in range(3))
    scale = torch.randn(C, device="cuda", generator=g)
    shift = torch.randn(C, device="cuda", generator=g)
    want_fin = torch.addcmul(shift, y, scale) + out          # fmaf(y, scale, shift) + out, as the kernel rounds it
    fin, x = ops.residual_epilogue(feat, out, y, scale, shift)
    assert (fin - want_fin).abs().max().item() <= 1e-6 and (x - (want_fin + feat)).abs().max().item() <= 1e-6
    fin_only, none_x = ops.residual_epilogue(feat, out, y, scale, shift, want_finalout=True, want_x=False)
    assert none_x is None and torch.equal(fin_only, fin)
    none_fin, x_only = ops.residual_epilogue(feat, out, y, scale, shift, want_finalout=False, want_x=True)
    assert none_fin is None and torch.equal(x_only, x)
    fin0, x0 = ops.residual_epilogue(feat, out)              # no z branch: finalout = out, x = feat + out
    assert torch.equal(fin0, out) and torch.equal(x0, feat + out)
    with pytest.raises(_lib.EpipolarAmdError):               # y without its affine: loud
        ops.residual_epilogue(feat, out, y, None, None)
    with pytest.raises(_lib.EpipolarAmdError):               # nothing to write
        ops.residual_epilogue(feat, out, want_finalout=False, want_x=False)


@pytest.mark.parametrize("case", ["tiny_16x16_c8_k8", "head_16x16_c256_k16"])
def test_unparameterized_layer_vs_reference(env, case):
    """EPIPOLAR.PARAMETERIZED = () (keypoint_h36m.yaml, ...resnet152_320.yaml, ...resnet152_384.yaml): no z / bn,
    forward returns the attended features themselves (epipolar.py:249-255), the backbone adds feat (resnet.py:388)
    -- forward_fused takes the et_residual_epilogue kernel for it."""
    from epipolar_transformers_amd import default_cfg
    from epipolar_transformers_amd.epipolar import Epipolar

    d = load_golden(case)
    m = d["dims"]
    cfg = default_cfg()
    cfg.merge_from_list(["KEYPOINT.HEATMAP_SIZE", (m["H"], m["W"]), "KEYPOINT.NFEATS", m["C"],
                         "EPIPOLAR.SAMPLESIZE", m["K"], "EPIPOLAR.ATTENTION", "avg", "EPIPOLAR.PARAMETERIZED", (),
                         "EPIPOLAR.USE_CORRECT_NORMALIZE", m["correct"], "EPIPOLAR.SOFTMAX_ENABLED", m["softmax"],
                         "EPIPOLAR.SOFTMAXSCALE", float(d["softmax_scale"])])
    mod = Epipolar(cfg=cfg).cuda().eval()
    assert list(mod.state_dict()) == []
    mod._cams.get = lambda *a, **k: _dev(d["cam"])           # the algebra the fixture was generated with
    f1, f2 = _dev(d["feat1"]), _dev(d["feat2"])
    P1, P2 = torch.from_numpy(d["P1"]), torch.from_numpy(d["P2"])
    with torch.no_grad():
        fin, corr, depth, locs = mod(f1, f2, P1, P2)
        x, corr2, depth2, _ = mod.forward_fused(f1, f2, P1, P2)
    assert locs is None
    _close(fin.cpu().numpy(), d["out"], TOL_OUT)
    _close(x.cpu().numpy(), d["out"] + d["feat1"], TOL_OUT)
    _close(depth.cpu().numpy()[:, :, d["rows"]], d["attn"], TOL_ATTN)
    assert torch.equal(corr, corr2) and torch.equal(depth, depth2)
    # train mode / autograd takes the torch epilogue: same numbers
    a1 = f1.clone().requires_grad_(True)
    xt, _, _, _ = mod.forward_fused(a1, f2, P1, P2)
    _close(xt.detach().cpu().numpy(), d["out"] + d["feat1"], TOL_OUT)


@pytest.mark.parametrize("merge", ["early", "both"])
def test_pose_backbone_merge_early_and_both(env, oracle_mod, merge):
    """MERGE early / both (resnet.py:390-416): the layer fuses the reference view's layer1 features (early) -- and
    again its deconvolution features through `epipolar_sampler1` (both) -- with the source view's features.  Checked
    through hooks: what enters layer2 / final_layer must be   feat + bn(z(attend(feat, src)))+attend   per the oracle."""
    _lib, camera, ops = env
    from epipolar_transformers_amd import backbones, default_cfg, synthetic as syn

    size, hs = 64, 16
    cfg = default_cfg()
    cfg.merge_from_list(["BACKBONE.BODY", "epipolarposeR-50", "BACKBONE.PRETRAINED", False,
                         "KEYPOINT.HEATMAP_SIZE", (hs, hs), "KEYPOINT.NUM_PTS", 17, "KEYPOINT.SIGMA", 2.0,
                         "DATASETS.IMAGE_SIZE", (size, size), "EPIPOLAR.MERGE", merge, "EPIPOLAR.ATTENTION", "avg",
                         "EPIPOLAR.PARAMETERIZED", ("z",), "EPIPOLAR.ZRESIDUAL", True,
                         "EPIPOLAR.USE_CORRECT_NORMALIZE", True, "EPIPOLAR.SAMPLESIZE", 16])
    torch.manual_seed(5)
    net = backbones.build_backbone(cfg).cuda().eval()
    assert (getattr(net, "epipolar_sampler1", None) is not None) == (merge == "both")
    samplers = [net.epipolar_sampler] + ([net.epipolar_sampler1] if merge == "both" else [])
    with torch.no_grad():
        for s in samplers:
            s.bn.weight.normal_(1, 0.1)
            s.bn.bias.normal_(0, 0.1)
            s.bn.running_mean.normal_(0, 0.1)
            s.bn.running_var.uniform_(0.5, 1.5)
    seen = {}
    hooks = [net.layer1.register_forward_hook(lambda m, i, o: seen.__setitem__("layer1_out", o.detach().clone())),
             net.layer2.register_forward_pre_hook(lambda m, i: seen.__setitem__("layer2_in", i[0].detach().clone())),
             net.deconv_layers.register_forward_hook(lambda m, i, o: seen.__setitem__("deconv_out", o.detach().clone())),
             net.final_layer.register_forward_pre_hook(lambda m, i: seen.__setitem__("final_in", i[0].detach().clone()))]
    P1, P2 = syn.make_pairs(1, 4, size, seed=4, jitter=(0.03, 2.0))
    img = torch.randn(4, 3, size, size, device="cuda")
    other = img.roll(-1, 0)
    with torch.no_grad():
        src_feat = net(other)[0]
        feat, heat, locs, scos, corr, depth, sl, _ = net(img, [src_feat, P2, None, P1, None, None, other])
    for h in hooks:
        h.remove()
    assert tuple(depth.shape) == (4, 16, hs, hs) and tuple(corr.shape) == (4, hs, hs, 2)
    so = oracle_mod.LayerSpec(hs, hs, 16)
    cam = camera.pair_algebra(P1, P2).numpy()
    f2 = src_feat.float().cpu().numpy()

    def fused(sampler, f1):
        want = oracle_mod.forward(so, f1, f2, None, None, cam=cam)
        _, x = oracle_mod.epilogue(want["out"], f1, sampler.z.weight.detach().cpu().numpy(),
                                   sampler.z.bias.detach().cpu().numpy(), sampler.bn.weight.detach().cpu().numpy(),
                                   sampler.bn.bias.detach().cpu().numpy(), sampler.bn.running_mean.cpu().numpy(),
                                   sampler.bn.running_var.cpu().numpy(), training=False)
        return want, x.numpy()

    want1, x1 = fused(net.epipolar_sampler, seen["layer1_out"].float().cpu().numpy())
    scale = max(1.0, float(np.abs(x1).max()))
    assert np.abs(seen["layer2_in"].float().cpu().numpy() - x1).max() <= 1e-4 * scale
    if merge == "early":
        _close(depth.cpu().numpy(), want1["attn"], TOL_ATTN)
        assert torch.equal(seen["final_in"], seen["deconv_out"])          # nothing fused after the deconvolutions
    else:
        want2, x2 = fused(net.epipolar_sampler1, seen["deconv_out"].float().cpu().numpy())
        scale = max(1.0, float(np.abs(x2).max()))
        assert np.abs(seen["final_in"].float().cpu().numpy() - x2).max() <= 1e-4 * scale
        _close(depth.cpu().numpy(), want2["attn"], TOL_ATTN)


@pytest.mark.parametrize("legacy", [False, True])
@pytest.mark.parametrize("shape,radius", [((5, 17, 64, 64), 8.0), ((3, 20, 16, 16), 2.0), ((2, 4, 24, 40), 3.0)])
def test_heatmap_peaks_kernel(env, shape, radius, legacy):
    """et_heatmap_peaks (row N2: the head's peak finder as ONE kernel) against the float64 restatement of find_tensor_peak_batch
    (tests/peaks_restatement.py).  The bound is the one of tests/test_gpu_peaks.py, max(4 x ref_err, 2 ulp_float32(max |location|)),
    with ref_err measured on THESE maps: the distance from float64 of the batched torch restatement run on the CPU, which
    tests/test_peaks_cpu.py holds bit-equal to the real reference."""
    _lib, camera, ops = env
    import peaks_restatement as restate
    from epipolar_transformers_amd.backbones import soft_argmax_peaks

    g = torch.Generator(device="cuda").manual_seed(shape[1])
    n, j, h, w = shape
    hm = torch.randn(shape, device="cuda", generator=g) * 0.05
    # a Gaussian bump per map (what a trained head produces), some near the border, one map all below the threshold
    cy = torch.randint(0, h, (n, j), device="cuda", generator=g).float()
    cx = torch.randint(0, w, (n, j), device="cuda", generator=g).float()
    yy = torch.arange(h, device="cuda").view(1, 1, h, 1).float()
    xx = torch.arange(w, device="cuda").view(1, 1, 1, w).float()
    hm = hm.abs() * 0.1 + torch.exp(-((yy - cy[..., None, None]) ** 2 + (xx - cx[..., None, None]) ** 2) / (2 * radius))
    hm[0, 0] = 1e-8
    maps = hm.cpu().numpy().reshape(n * j, h, w)
    ref_l, want_s = soft_argmax_peaks(hm.cpu(), radius, 4)
    f64, _, _, margin = restate.peaks(maps, radius, 4.0)
    want_l, _, _, margin_l = restate.peaks(maps, radius, 4.0, legacy_floor_division=legacy)
    assert min(margin.min(), margin_l.min()) >= 1e-3             # no sample so near the threshold that float32 may decide otherwise
    ref_err = np.abs(ref_l.numpy().reshape(-1, 2).astype(np.float64) - f64).max()
    bound = restate.bound(ref_err, ref_l.numpy())
    got_l, got_s = ops.heatmap_peaks(hm, radius, 4, legacy_floor_division=legacy)
    assert torch.equal(got_s.cpu(), want_s)
    err = np.abs(got_l.cpu().numpy().reshape(-1, 2).astype(np.float64) - want_l).max()          # image pixels
    print("    %s r %g legacy %d: worst %.3e px, the reference's own %.3e, bound %.3e" % (shape, radius, legacy, err, ref_err, bound))
    assert ref_err < 1e-4 and err <= bound, (err, bound)


def test_split_fp16_guard_outliers_fall_back_to_exact_fp32(env):
    """The warp-specialised forward computes its two GEMMs as split-fp16 products under per-pair power-of-two scales
    ESTIMATED from 64 sampled pixel rows (column 0 of every image row at 64x64).  A value outside the sample that the
    scale would push beyond fp16's range must send its tiles to the exact-fp32 kernel -- in the reference rows
    (checked where the A stage is written) and in the source rows (checked by GEMM 1) -- never produce inf / NaN."""
    _lib, camera, ops = env
    P1, P2, f1, f2 = _full_inputs(1, 4, 64, 256, 256, seed=3)
    cam = camera.pair_algebra(P1, P2).cuda()
    ref, src = ops.to_nhwc(f1.cuda()).contiguous(), ops.to_nhwc(f2.cuda()).contiguous()
    ref[0, 10, 11, 5] = 4e4            # ~2^18 x the sampled maximum after scaling: beyond fp16
    src[1, 40, 3, 100] = 4e4
    src[2, 17, 29, 7] = -6e4
    bias = torch.randn(256, device="cuda")
    got = ops.forward_nhwc(ops.LayerSpec(H=64, W=64, K=64), ref, src, cam, res_bias=bias, want_res_base=True)
    want = ops.forward_nhwc(ops.LayerSpec(H=64, W=64, K=64, variant=_lib.ET_VARIANT_NO_TILE), ref, src, cam,
                            res_bias=bias, want_res_base=True)
    for g, w, atol in zip(got, want, (1e-4, 1e-5, 0.0, 0.0)):
        g, w = g.float(), w.float()
        assert torch.isfinite(g).all()
        assert ((g - w).abs() - 1e-5 * w.abs()).max().item() <= atol


@pytest.mark.parametrize("rows", [64, 77, 1000, 4 * 64 * 64 + 13])
@pytest.mark.parametrize("with_feat", [True, False])
def test_residual_gemm_abi(env, rows, with_feat):
    """et_residual_gemm (eval-mode bn(z(out)) + out [+ feat] folded into x = [feat +] bias + out . Wf^T, split-fp16 MFMA with
    one power-of-two scale per row) against float64: fp32-GEMM-level error on every row, whatever its magnitude --
    ragged row counts, an all-zero row, rows of 1e-6 and 3e4 times the typical size."""
    _lib, camera, ops = env
    g = torch.Generator(device="cuda").manual_seed(rows)
    out = torch.randn(rows, 256, device="cuda", generator=g).relu_() * 2.5
    out[3] *= 1e-6
    out[5] *= 3e4
    out[min(rows - 1, 70)] = 0
    feat = torch.randn(rows, 256, device="cuda", generator=g) if with_feat else None
    wf = torch.randn(256, 256, device="cuda", generator=g) * 0.05 + torch.eye(256, device="cuda")
    bias = torch.randn(256, device="cuda", generator=g)
    packed = ops.residual_gemm_pack(wf)
    x = ops.residual_gemm(out, packed, bias, feat)
    prod = out.double() @ wf.double().t()
    want = prod + bias.double() + (feat.double() if with_feat else 0)
    # the error of a product row scales with the magnitudes that went into it, the additive terms add one rounding each
    bound = 4e-6 * (out.double().abs() @ wf.double().abs().t()) + 3e-7 * (want.abs() + 1)
    assert torch.isfinite(x).all()
    assert ((x.double() - want).abs() <= bound).all(), ((x.double() - want).abs() / bound).max().item()
    # same error class as the fp32 library GEMM it replaces
    lib32 = torch.addmm(bias, out, wf.t()) + (feat if with_feat else 0)
    scale = prod.abs().amax(1, keepdim=True).clamp_min(1e-30)
    assert ((x.double() - want).abs() / scale).max().item() <= 4 * ((lib32.double() - want).abs() / scale).max().item() + 1e-6
