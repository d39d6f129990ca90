"""The 256-channel kernels under the geometry settings real configs use besides the headline one, against the C oracle.

Every other GPU test runs the layer at one setting (USE_CORRECT_NORMALIZE True, IMAGE_RESIZE = PREDICT_RESIZE = 1,
align_corners False, soft-max scale 1/8).  Real use differs:
  legacy       USE_CORRECT_NORMALIZE False: the default (core/config.py:118) and that of keypoint_h36m.yaml,
               keypoint_h36m_param.yaml, keypoint_h36m_resnet152_{320,384,384_strong}.yaml: normalize divides by the map size
               and shifts by half a pixel (multiview.py:30-35)
  align        EPIPOLAR_AMD.ALIGN_CORNERS: grid_sample's older semantics, a different `unnormalize` for every tap, row mask and
               band line of the tile kernels
  resize3p9    IMAGE_RESIZE 1000/256 (commented out in the YAMLs): not a power of two, so every kernel takes its
               sample_location<false> instantiation (csrc/epipolar_geometry.h, Pow2Recips.ok false)
               (with legacy normalize too: the reference's default normalize)
  resize2x4    IMAGE_RESIZE 2 x PREDICT_RESIZE 4 with legacy normalize: the reference's built-in defaults
  scale        EPIPOLAR.SOFTMAXSCALE = 1/sqrt(K) at a K other than 64
The tile kernels find the source rows a tile touches (band line, column masks, row lists) apart from the arithmetic that samples
them: a half-pixel or W / (W - 1) disagreement between the two would fetch taps from rows that were never loaded, or send whole
tiles through the overflow list.  The oracle is pinned to the real reference on the normalize, resize and scale settings by
tests/golden/{legacy,resize,scale}_*.npz (tests/test_oracle_golden.py); align_corners against the oracle only.
Bounds are the suite's: sample_locs bit-equal, attention 1e-5, out / x 1e-4, gradients 1e-4 of each tensor's scale.
"""
import numpy as np
import pytest
import torch

from conftest import assert_corr_pos

pytestmark = pytest.mark.gpu

C = 256
TOL_ATTN, TOL_OUT, TOL_GRAD_REL = 1e-5, 1e-4, 1e-4
WS_BAND, TILE_CLASSIC, NO_TILE = 1048576, 65536, 16384

SETTINGS = {
    "legacy": dict(correct_normalize=False),
    "align": dict(align_corners=True),
    "legacy-align": dict(correct_normalize=False, align_corners=True),
    "resize3p9": dict(image_resize=3.90625),
    "resize3p9-legacy": dict(image_resize=3.90625, correct_normalize=False),
    "resize2x4-legacy": dict(image_resize=2.0, predict_resize=4.0, correct_normalize=False),
    "scale": dict(softmax_scale=None),          # 1 / sqrt(K) of the case
}

# (h, w, k, rig, pairs): Config 2 and Config 4 maps, a non-square map (div_w != div_h), the two-pass kernel (K > 64) at
# Config 5's shape and at K = 85 (keypoint_h36m_resnet50_384_strong_fixed.yaml)
FWD_SHAPES = [(64, 64, 64, "ring", 2), (64, 64, 64, "epipole_inside", 2), (96, 96, 64, "h36m_room", 2),
              (96, 96, 64, "near_rectified_x", 2), (48, 80, 40, "ring", 2), (128, 128, 128, "ring", 1),
              (96, 96, 85, "epipole_inside", 1)]
BWD_SHAPES = [(64, 64, 64, "ring", 2), (64, 64, 64, "epipole_inside", 2), (96, 96, 64, "h36m_room", 2), (128, 128, 128, "ring", 1)]
# (the oracle's backward at 128 x 128, K = 128 takes ~20 CPU-seconds: there, the settings that move the sample arithmetic of
# every tap -- legacy normalize with align_corners, and the two resize settings under legacy normalize)
BWD_CASES = [(st, sh) for sh in BWD_SHAPES for st in SETTINGS
             if sh[2] <= 64 or st in ("legacy-align", "resize3p9-legacy", "resize2x4-legacy")]
FUSED_SHAPES = [(64, 64, 64, "ring", 2), (96, 96, 64, "h36m_room", 2)]
_ids = lambda shapes: ["%dx%d-K%d-%s" % s[:4] for s in shapes]

_cache = {}


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from epipolar_transformers_amd import _lib, camera, ops

    _lib.load()
    return _lib, camera, ops


def _settings(setting, k):
    kw = dict(SETTINGS[setting])
    if "softmax_scale" in kw:
        kw["softmax_scale"] = float(np.float32(k ** -0.5))
    return kw


def _case(oracle_mod, camera, setting, h, w, k, rig, n, backward=False):
    """`n` pairs of the rig, the cameras projecting into the image the resize factors scale the grid to, and the oracle's
    forward (+ backward) at the setting (cached per setting, shape and rig: several tests share a case)."""
    key = (setting, h, w, k, rig, n)
    if key not in _cache:
        from epipolar_transformers_amd import synthetic as syn

        kw = _settings(setting, k)
        seed = 800 + h + w + k + len(rig)
        image = 4 * max(h, w) * kw.get("image_resize", 1.0) * kw.get("predict_resize", 1.0)
        P1, P2 = syn.rig_pairs(rig, 1, image, seed=seed, jitter=(0.05, 8.0))
        pick = [1, 2] if rig == "h36m_room" else [0, 1]          # (the two pairs of the room rig with invalid pixels)
        P1, P2 = P1[pick[:n]], P2[pick[:n]]
        f1, f2 = syn.make_features(n, C, h, w, seed=seed)
        f1[0, :, 5, 7] = 0                                       # an all-zero reference pixel: every sample masked
        cam = camera.pair_algebra(P1, P2)
        so = oracle_mod.LayerSpec(h, w, k, **kw)
        with np.errstate(all="ignore"):
            want = oracle_mod.forward(so, f1, f2, None, None, cam=cam.numpy())
        _cache[key] = dict(f1=f1, f2=f2, cam=cam, want=want, so=so, kw=kw, seed=seed)
    case = _cache[key]
    if backward and "g1" not in case:
        g = torch.randn(n, C, h, w, generator=torch.Generator().manual_seed(case["seed"] + 1))
        with np.errstate(all="ignore"):
            case["g1"], case["g2"] = oracle_mod.backward(case["so"], case["f1"].numpy(), case["f2"].numpy(),
                                                         case["want"]["sample_locs"], g.numpy())
        case["g"] = g
    return case


def _overflow(ws):
    base = (-ws.data_ptr()) % 256
    return int(ws[base:base + 4].view(torch.int32).item())


def _overflow_limit(rig, h, w, k, n):
    """The bounds tests/test_gpu_rigs.py (K <= 64) and tests/test_gpu_two_pass.py (K > 64) hold the rig to."""
    tiles = n * ((h * w + 31) // 32)
    if k > 64 and h * w <= 96 * 96:
        return 0 if rig in ("ring", "epipole_border", "h36m_room") else tiles // 2
    # (above 96 x 96 the ring leaves the odd tile to the list kernels at the headline setting too: Config 5's left-over tiles)
    return {"near_rectified_x": tiles // 20, "near_rectified_y": tiles // 20, "epipole_inside": tiles // 20,
            "rectified_x": tiles // 4, "identical": tiles // 4}.get(rig, max(2, tiles // 50))


def _check_forward(case, out, attn, corr, correct):
    want = case["want"]
    attn_h, out_h, corr_h = attn.cpu().numpy(), out.permute(0, 3, 1, 2).cpu().numpy(), corr.cpu().numpy()
    assert np.isfinite(attn_h).all() and np.isfinite(out_h).all()
    assert np.abs(attn_h - want["attn"]).max() <= TOL_ATTN, float(np.abs(attn_h - want["attn"]).max())
    assert np.abs(out_h - want["out"]).max() <= TOL_OUT, float(np.abs(out_h - want["out"]).max())
    if (corr_h != want["corr_pos"]).any():
        assert_corr_pos(want["sample_locs"], corr_h, want["corr_pos"], attn_h, correct, 2e-6, 2e-2)


@pytest.mark.parametrize("h,w,k,rig,n", FWD_SHAPES, ids=_ids(FWD_SHAPES))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_forward_kernels_vs_oracle(env, oracle_mod, setting, h, w, k, rig, n):
    """The persistent kernel (its band instance too), the one-block-per-tile kernel and the per-pixel kernels."""
    _lib, camera, ops = env
    case = _case(oracle_mod, camera, setting, h, w, k, rig, n)
    kw = case["kw"]
    correct = kw.get("correct_normalize", True)
    ref, src, cam = ops.to_nhwc(case["f1"].cuda()), ops.to_nhwc(case["f2"].cuda()), case["cam"].cuda()
    spec0 = ops.LayerSpec(H=h, W=w, K=k, **kw)
    assert np.array_equal(ops.sample_locs(spec0, cam).cpu().numpy(), case["want"]["sample_locs"], equal_nan=True)
    res = {}
    variants = [0, TILE_CLASSIC, NO_TILE] + ([WS_BAND] if h * w <= 64 * 64 and k <= 64 else [])
    for variant in variants:
        spec = ops.LayerSpec(H=h, W=w, K=k, variant=variant, **kw)
        ws = ops.tile_workspace(spec, n, C, ref.device) if variant != NO_TILE else None
        out, attn, corr = ops.forward_nhwc(spec, ref, src, cam, workspace=ws)
        torch.cuda.synchronize()
        if ws is not None:
            assert ws.numel() > 0, "the 256-channel shape was meant to take the tile kernels"
            ops.check_tile_errors(workspace=ws)
        _check_forward(case, out, attn, corr, correct)
        if variant in (0, WS_BAND):
            ovf = _overflow(ws)
            assert ovf <= _overflow_limit(rig, h, w, k, n), (variant, ovf)
            res[variant] = (out, attn, corr, ops.tile_stats(spec, n, C, ws), ovf)
    if WS_BAND in res:
        # the band instance forced onto a small map: the same row sets and the same arithmetic as the default instance
        a, b = res[0], res[WS_BAND]
        assert a[4] == b[4]
        assert torch.equal(a[3], b[3])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def _bound(out, wf, want):
    """tests/test_gpu_fused.py's bound of the one-kernel layer against float64"""
    return 4e-6 * (out.double().abs() @ wf.double().abs().t()) + 3e-7 * (want.abs() + 1)


@pytest.mark.parametrize("h,w,k,rig,n", FUSED_SHAPES, ids=_ids(FUSED_SHAPES))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_fused_layer_vs_oracle(env, oracle_mod, setting, h, w, k, rig, n):
    """et_epipolar_forward_fused: x = feat + bias + out @ Wf^T against float64 of that epilogue applied to the oracle's `out`."""
    _lib, camera, ops = env
    case = _case(oracle_mod, camera, setting, h, w, k, rig, n)
    g = torch.Generator().manual_seed(case["seed"] + 2)
    wf = torch.randn(C, C, generator=g) * 0.05 + torch.eye(C)
    bias = torch.randn(C, generator=g)
    spec = ops.LayerSpec(H=h, W=w, K=k, **case["kw"])
    assert ops.fused_layer_applies(spec, C, n)
    ref, src, cam = ops.to_nhwc(case["f1"].cuda()), ops.to_nhwc(case["f2"].cuda()), case["cam"].cuda()
    wf_d, bias_d = wf.cuda(), bias.cuda()
    ws = ops.tile_workspace(spec, n, C, ref.device)
    x, attn, corr, out = ops.forward_fused_nhwc(spec, ref, src, cam, ops.residual_gemm_pack(wf_d), bias_d, want_out=True, workspace=ws)
    torch.cuda.synchronize()
    ops.check_tile_errors(workspace=ws)
    assert torch.isfinite(x).all()
    _check_forward(case, out, attn, corr, case["kw"].get("correct_normalize", True))
    # against float64 of the epilogue of the kernel's own `out` (tests/test_gpu_fused.py's bound) ...
    want = out.double().reshape(-1, C) @ wf_d.double().t() + bias_d.double() + ref.double().reshape(-1, C)
    err = (x.double().reshape(-1, C) - want).abs()
    assert (err <= _bound(out.reshape(-1, C), wf_d, want)).all()
    # ... and of the oracle's `out`
    out_o = torch.from_numpy(case["want"]["out"]).permute(0, 2, 3, 1).reshape(-1, C).double()
    want_o = out_o @ wf.double().t() + bias.double() + case["f1"].permute(0, 2, 3, 1).reshape(-1, C).double()
    assert (x.double().reshape(-1, C).cpu() - want_o).abs().max().item() <= TOL_OUT


@pytest.mark.parametrize("setting,shape", BWD_CASES, ids=["%s-%s" % (st, _ids([sh])[0]) for st, sh in BWD_CASES])
def test_backward_forms_vs_oracle(env, oracle_mod, setting, shape):
    """The tiled backward (merged kernel, the deferred list on the epipole-inside rig, kpl = 2 at K = 128), the same re-using the
    forward's attention, the gather form and the float-atomic form."""
    _lib, camera, ops = env
    h, w, k, rig, n = shape
    case = _case(oracle_mod, camera, setting, h, w, k, rig, n, backward=True)
    spec = ops.LayerSpec(H=h, W=w, K=k, **case["kw"])
    ref, src, cam = ops.to_nhwc(case["f1"].cuda()), ops.to_nhwc(case["f2"].cuda()), case["cam"].cuda()
    g = ops.to_nhwc(case["g"].cuda())
    for form in ("tile", "tile-attn", "gather", "atomic"):
        attn = ops.forward_nhwc(spec, ref, src, cam)[1] if form == "tile-attn" else None
        gr, gs = ops.backward_nhwc(spec, ref, src, cam, g, form=form.split("-")[0], attn=attn)
        torch.cuda.synchronize()
        if form == "tile" and rig == "epipole_inside" and h == 64:
            assert ops.backward_deferred_tiles(ref.device) > 0, "the case was meant to reach the deferred list"
        for got, want in ((gr, case["g1"]), (gs, case["g2"])):
            got = got.permute(0, 3, 1, 2).cpu().numpy()
            assert np.isfinite(got).all()
            scale = max(float(np.abs(want).max()), 1e-30)
            assert np.abs(got - want).max() <= TOL_GRAD_REL * scale, (form, float(np.abs(got - want).max()), scale)


@pytest.mark.parametrize("setting", ["legacy", "legacy-align", "resize3p9"])
def test_general_kernel_vs_torch_restatement_at_param_yaml_head(env, setting):
    """keypoint_h36m_param.yaml's head (64 x 64, C = 256, K = 64, theta / phi / g with BOTTLENECK 2, POOLING; it keeps legacy
    normalize): the general kernel's forward and every gradient against the torch restatement run in float64."""
    from epipolar_transformers_amd import default_cfg, synthetic as syn
    from epipolar_transformers_amd.epipolar import Epipolar

    H, K, N = 64, 64, 2
    kw = _settings(setting, K)
    par = ("z", "theta", "phi", "g")
    cfg = default_cfg()
    cfg.merge_from_list(["KEYPOINT.HEATMAP_SIZE", (H, H), "KEYPOINT.NFEATS", C, "EPIPOLAR.SAMPLESIZE", K,
                         "DATASETS.IMAGE_SIZE", (4 * H, 4 * H), "EPIPOLAR.USE_CORRECT_NORMALIZE", kw.get("correct_normalize", True),
                         "EPIPOLAR_AMD.ALIGN_CORNERS", kw.get("align_corners", False),
                         "DATASETS.IMAGE_RESIZE", kw.get("image_resize", 1.0), "DATASETS.PREDICT_RESIZE", kw.get("predict_resize", 1.0),
                         "EPIPOLAR.ATTENTION", "avg", "EPIPOLAR.PARAMETERIZED", par, "EPIPOLAR.BOTTLENECK", 2,
                         "EPIPOLAR.ZRESIDUAL", False, "EPIPOLAR.POOLING", True])
    torch.manual_seed(9)
    mod = Epipolar(cfg=cfg).cuda().eval()
    with torch.no_grad():
        for nm in ("theta", "phi", "g"):
            getattr(mod, nm).weight.normal_(0, 0.1)
            getattr(mod, nm).bias.normal_(0, 0.1)
    image = 4 * H * kw.get("image_resize", 1.0) * kw.get("predict_resize", 1.0)
    P1, P2 = syn.make_pairs(1, 4, image, seed=41, jitter=(0.05, 8.0))
    P1, P2 = P1[:N], P2[:N]
    f1, f2 = syn.make_features(N, C, H, H, seed=42)
    gout = torch.randn(N, C // 2, H, H, generator=torch.Generator().manual_seed(43)).cuda()
    a, b = f1.cuda().requires_grad_(True), f2.cuda().requires_grad_(True)
    assert mod._general_kernel_applies(a, b)
    out_h, attn_h, corr_h = mod._attend_general(a, b, P1, P2)
    (out_h * gout).sum().backward()
    grads_h = [a.grad.clone(), b.grad.clone()] + [q.grad.clone() for nm in ("theta", "phi", "g") for q in getattr(mod, nm).parameters()]
    # the restatement in float64: a double copy of the module and of the maps; it samples at the (float32, bit-exact) locations
    # of the geometry kernel, widened for grid_sample
    from epipolar_transformers_amd import ops
    mod64 = Epipolar(cfg=cfg).cuda().eval()
    mod64.load_state_dict(mod.state_dict())
    mod64.double()
    a64, b64 = f1.cuda().double().requires_grad_(True), f2.cuda().double().requires_grad_(True)
    real = ops.sample_locs
    ops.sample_locs = lambda *a_, **k_: real(*a_, **k_).double()
    try:
        out_t, attn_t, corr_t = mod64._attend_general_chunk(a64, b64, P1, P2)
    finally:
        ops.sample_locs = real
    (out_t * gout.double()).sum().backward()
    grads_t = [a64.grad, b64.grad] + [q.grad for nm in ("theta", "phi", "g") for q in getattr(mod64, nm).parameters()]
    assert (attn_h.double() - attn_t).abs().max().item() <= 1e-5 * max(1.0, attn_t.abs().max().item())
    assert (out_h.double() - out_t).abs().max().item() <= 1e-4 * max(1.0, out_t.abs().max().item())
    locs = ops.sample_locs(mod.layer_spec(), mod._cam(P1, P2, a.device)).cpu().numpy()
    assert_corr_pos(locs, corr_h.cpu().numpy(), corr_t.float().cpu().numpy(), attn_h.detach().cpu().numpy(),
                    kw.get("correct_normalize", True), tie=2e-6, max_frac=2e-2)
    # the gradients against autograd through the restatement in float32 (tests/test_gpu_modes.py's standard for the general
    # kernel's gradients; feat1 and theta, which no pooling decision separates from the loss, against float64 too).  POOLING
    # keeps the larger of samples k and k + K/2 and sends the gradient to it alone; at this shape (4 million pooled pairs per
    # map) a few dozen pairs are equal to the rounding of the sampling arithmetic and the kernel may keep the other sample (seen
    # at the headline setting as well): d feat2 may differ there -- a few entries --, the phi / g weights, sums over all pixels,
    # by their share; phi.b's gradient cancels to zero analytically (a constant shift of phi(feat2) moves every similarity of a
    # pixel alike) and is judged on the scale of phi.w's
    a32, b32 = f1.cuda().requires_grad_(True), f2.cuda().requires_grad_(True)
    mod.zero_grad()
    out_32, _, _ = mod._attend_general_chunk(a32, b32, P1, P2)
    (out_32 * gout).sum().backward()
    grads_32 = [a32.grad, b32.grad] + [q.grad for nm in ("theta", "phi", "g") for q in getattr(mod, nm).parameters()]
    names = ["feat1", "feat2", "theta.w", "theta.b", "phi.w", "phi.b", "g.w", "g.b"]
    for nm, gh, gt, g64 in zip(names, grads_h, grads_32, grads_t):
        scale = max((grads_32[4] if nm == "phi.b" else gt).abs().max().item(), 1e-6)
        err = (gh - gt).abs()
        if nm in ("feat1", "theta.w", "theta.b"):
            assert err.max().item() <= 2e-4 * scale, nm
            assert (gh.double() - g64).abs().max().item() <= 2e-4 * max(g64.abs().max().item(), 1e-6), nm
        elif nm == "feat2":
            assert (err > 2e-4 * scale).float().mean().item() <= 1e-4, (nm, int((err > 2e-4 * scale).sum()))
            assert err.max().item() <= 2e-2 * scale, (nm, err.max().item(), scale)
        else:
            assert err.max().item() <= 2e-3 * scale, (nm, err.max().item(), scale)


def test_module_at_resnet152_384_head_legacy(env):
    """Epipolar at keypoint_h36m_resnet152_384.yaml's layer settings (96 x 96, K = 64, legacy normalize) with the z / BN epilogue:
    the eval output of the one-kernel layer and one train step (output, running statistics, six gradients) against the same
    module on stock torch ops (EPIPOLAR_AMD.FUSED_EPILOGUE / FUSED_TRAIN_EPILOGUE False)."""
    from epipolar_transformers_amd import default_cfg, synthetic as syn
    from epipolar_transformers_amd.epipolar import Epipolar

    _lib, camera, ops = env
    n, h, k = 2, 96, 64
    P1, P2 = syn.make_pairs(1, 4, 4 * h, seed=15, jitter=(0.05, 8.0))
    P1, P2 = P1[:n], P2[:n]
    g0 = torch.Generator().manual_seed(16)
    f1, f2 = torch.randn(n, C, h, h, generator=g0).relu(), torch.randn(n, C, h, h, generator=g0).relu()
    gout = torch.randn(n, C, h, h, generator=g0).cuda()
    res, evals = [], []
    for fused in (True, False):
        cfg = default_cfg()
        cfg.merge_from_list(["KEYPOINT.HEATMAP_SIZE", (h, h), "KEYPOINT.NFEATS", C, "EPIPOLAR.SAMPLESIZE", k, "EPIPOLAR.ATTENTION", "avg",
                             "EPIPOLAR.PARAMETERIZED", ("z",), "EPIPOLAR.ZRESIDUAL", True, "EPIPOLAR.USE_CORRECT_NORMALIZE", False,
                             "DATASETS.IMAGE_SIZE", (4 * h, 4 * h), "EPIPOLAR_AMD.FUSED_EPILOGUE", fused,
                             "EPIPOLAR_AMD.FUSED_TRAIN_EPILOGUE", fused])
        torch.manual_seed(3)
        mod = Epipolar(cfg=cfg).cuda()
        with torch.no_grad():
            mod.bn.weight.normal_(1, 0.1)
            mod.bn.bias.normal_(0, 0.1)
            mod.bn.running_mean.normal_(0, 0.1)
            mod.bn.running_var.uniform_(0.5, 1.5)
        assert not mod.layer_spec().correct_normalize
        mod.eval()
        with torch.no_grad():
            evals.append(mod.forward_fused(f1.cuda(), f2.cuda(), P1, P2)[0])
        mod.train()
        a1, a2 = f1.cuda().requires_grad_(True), f2.cuda().requires_grad_(True)
        y = mod.forward_fused(a1, a2, P1, P2)[0]
        (y * gout).sum().backward()
        res.append([y.detach(), mod.bn.running_mean.clone(), mod.bn.running_var.clone(),
                    a1.grad.clone(), a2.grad.clone()] + [q.grad.clone() for q in (mod.z.weight, mod.z.bias, mod.bn.weight, mod.bn.bias)])
    assert (evals[0] - evals[1]).abs().max().item() <= 2e-4 * max(evals[1].abs().max().item(), 1e-6)
    names = ["y", "running_mean", "running_var", "d feat1", "d feat2", "d z.weight", "d z.bias", "d bn.weight", "d bn.bias"]
    for nm, a, b in zip(names, *res):
        scale = max(b.abs().max().item(), 1e-6)
        # (tests/test_gpu_fused.py::test_train_epilogue_kernels_vs_torch_ops: d z.bias cancels to zero analytically)
        tol = 2e-4 * (res[1][5].abs().max().item() if nm == "d z.bias" else scale)
        assert (a - b).abs().max().item() <= tol, (nm, (a - b).abs().max().item(), scale)
