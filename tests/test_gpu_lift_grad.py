"""et_triangulate_bwd on the MI355X, through the C ABI and through ops.triangulate_views / ops.triangulate_epipolar(with_grad=True):
the scenes of tests/test_lift_grad_cpu.py (F = 3, J = 17, V = 4 and 8, all five methods), one joint alone (F J = 1, V = 2) and
J = 257 (one lane in a second block), against the host hook (the kernel's own per-joint routine on the CPU) bit for bit and against
the float64 yardstick of tests/lift_grad_common.py; repeated calls, torch.autograd, and EPIPOLAR_AMD.PEAK_GRAD with
EPIPOLAR_AMD.LIFT_KERNELS through a small MultiViewPoseModel.

Tolerance per joint: 2^-23 x the joint's largest reference element; condition on the inputs: the two float64 yardsticks agree within
2^-30 per joint (lift_grad_common).  Each test prints its figures (pytest -s).  Measured on the MI355X: the kernel equals the host hook bit for bit in
every case and repeats its bits; the yardsticks are 8.1e-11 apart at the most; the worst use of the bound is 0.488 (pymvg, V = 2,
J = 257), on the F = 3 scenes 0.443 (epipolar, V = 4)."""
import copy

import numpy as np
import pytest
import torch

import abi_harness as hx
import lift_grad_common as common

pytestmark = pytest.mark.gpu

# (method, V, F, J): the CPU test's scenes, one joint alone, and 257 joints -- 256 lanes fill a block
CASES = [(m, V, 3, 17) for m in common.METHODS for V in (4, 8)] + \
        [(m, 2, 1, J) for m in ("pymvg", "epipolar") for J in (1, 257)]
CASE_IDS = ["%s-V%d-F%d-J%d" % c for c in CASES]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from epipolar_transformers_amd import _lib, ops

    assert ops.POISON_OUTPUTS                   # every output starts as NaN: nothing unwritten can pass for a result
    return _lib.load(), ops


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def kernel_bwd(sc, info, gout):
    """et_triangulate_bwd through the C ABI -> (F, V, J, 2) float32 NumPy; the output starts as NaN."""
    pts = cuda(sc.pts)
    H, W = sc.corr.shape[2:4] if sc.corr is not None else (0, 0)
    ds, resize = (common.EPIPOLAR_KW["downsample"], common.EPIPOLAR_KW["resize"]) if sc.corr is not None else (0.0, 0.0)
    grad = torch.full_like(pts, float("nan"))
    hx.call("et_triangulate_bwd", sc.F, sc.V, sc.J, H, W, pts, cuda(sc.krt), cuda(sc.other), cuda(sc.corr), ds, resize,
            cuda(np.ascontiguousarray(info, np.int32)), cuda(np.ascontiguousarray(gout, np.float64)), grad)
    return grad.cpu().numpy()


def lift(ops, sc, pts, **kw):
    """The scene's lifting through ops, on the tensor `pts`."""
    if sc.other is None:
        return ops.triangulate_views(pts, cuda(sc.conf), cuda(sc.krt), method=sc.method, **common.VIEWS_KW, **kw)
    return ops.triangulate_epipolar(pts, cuda(sc.conf), cuda(sc.krt), cuda(sc.other), cuda(sc.corr), dlt=sc.method == "epipolar_dlt",
                                    **common.EPIPOLAR_KW, **kw)


@pytest.mark.parametrize("method,V,F,J", CASES, ids=CASE_IDS)
def test_kernel_equals_the_host_hook_and_lies_within_the_bound(env, method, V, F, J):
    lib, ops = env
    sc = common.scene(method, V, F, J)
    _, info = lift(ops, sc, cuda(sc.pts), want_info=True)
    info = info.cpu().numpy()
    assert np.array_equal(info, sc.info)                  # the forward kernel decides as the restatement does
    for k, gout in enumerate(common.grad_outs(F, J)):
        worst = common.condition(sc, k)
        assert worst <= common.CONDITION, worst           # the condition on the inputs
        got = kernel_bwd(sc, info, gout)
        assert np.isfinite(got).all()                     # every element written
        # the kernel and its routine on the host take every operation in the same order: equal bits
        assert same_bits(got, common.host_bwd(lib, sc, info, gout))
        assert same_bits(got, kernel_bwd(sc, info, gout))             # ... and the same call again
        ok, use = common.use_of_bound(got, sc.reference(k)[0])
        print("    %-12s V=%d F=%d J=%-3d grad_out %d: yardsticks apart %.3e, worst use of the bound %.3f" % (method, V, F, J, k, worst, use))
        assert ok, (method, V, k, use)
        used = info >> 8 & 0xff
        for v in range(V):
            assert (got[:, v][(used >> v & 1) == 0] == 0).all()         # exact zeros for what was not used


@pytest.mark.parametrize("method", common.METHODS)
def test_autograd_through_the_operator_equals_the_direct_call(env, method):
    lib, ops = env
    sc = common.scene(method, 4)
    gout = common.grad_outs(sc.F, sc.J)[1]
    direct = kernel_bwd(sc, sc.info, gout)
    pts = cuda(sc.pts).requires_grad_()
    plain = lift(ops, sc, pts.detach())
    out, info = lift(ops, sc, pts, with_grad=True, want_info=True)
    assert out.grad_fn is not None and out.dtype == torch.float64 and hx.same_bits(out.detach(), plain)
    assert not info.requires_grad and np.array_equal(info.cpu().numpy(), sc.info)
    out.backward(cuda(gout))
    assert pts.grad.dtype == torch.float32 and same_bits(pts.grad.cpu().numpy(), direct)
    # without want_info, a float32 upstream gradient (cast to float64 by the operator), through a non-leaf
    leaf = cuda(sc.pts).requires_grad_()
    out = lift(ops, sc, leaf * 1.0, with_grad=True)
    g32 = cuda(gout.astype(np.float32))
    (out.float() * g32).sum().backward()
    assert same_bits(leaf.grad.cpu().numpy(), kernel_bwd(sc, sc.info, g32.double().cpu().numpy()))
    # nothing is attached without with_grad, without requires_grad, or under no_grad
    for p, with_grad in ((cuda(sc.pts).requires_grad_(), False), (cuda(sc.pts), True), (cuda(sc.pts), False)):
        out = lift(ops, sc, p, with_grad=with_grad)
        assert out.grad_fn is None and not out.requires_grad and hx.same_bits(out, plain)
    with torch.no_grad():
        out = lift(ops, sc, cuda(sc.pts).requires_grad_(), with_grad=True)
    assert out.grad_fn is None and not out.requires_grad and hx.same_bits(out, plain)


def test_peak_grad_with_lift_kernels_through_a_small_model(env):
    """2 frames x 4 views through the smallest PoseResNet of tests/test_gpu_model.py, KEYPOINT.TRIANGULATION pymvg, a squared-error
    loss on lift(...).  With PEAK_GRAD and LIFT_KERNELS the gradient on final_layer.weight is finite, non-zero and equals the one
    with LIFT_KERNELS off (the torch DLT under autograd).  The scores handed to lift are all 0.9 > CONF_THRES 0.85, so both routes
    use all four views of every joint (asserted through the info word).  Tolerance: 4 x the distance of the torch route from
    itself -- final_layer, backbones.soft_argmax_peaks, the torch DLT and the loss on the layer's input, in float64 against
    float32 -- relative to the largest element.  Measured on the MI355X: the torch route's float32 lies 1.1e-5 of the largest element
    from its float64, the kernels 3.3e-6 from the torch DLT (0.07 of the bound).  Both routes lift the detections of ONE forward
    pass.  lift is given a jittered ring per frame with the world in metres (see below).  With PEAK_GRAD off the lifted points
    carry no grad_fn."""
    from epipolar_transformers_amd import backbones, synthetic as syn
    from epipolar_transformers_amd.model import ring_sources
    from test_gpu_model import _cfg, _model

    lib, ops = env
    cfg, size, hs = _cfg(**{"KEYPOINT.TRIANGULATION": "pymvg", "KEYPOINT.CONF_THRES": 0.85})
    m = _model(cfg)
    frames, V = 2, 4
    P = torch.from_numpy(syn.ring_cameras(V, size)).float().repeat(frames, 1, 1)
    img = torch.randn(frames * V, 3, size, size, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    src = ring_sources(frames, V, "cuda")
    J = int(cfg.KEYPOINT.NUM_PTS)
    # The cameras handed to lift: a jittered ring per frame, the world in metres.  An untrained head detects the same cell in all
    # four views for some joints; under the exact four-fold symmetry of the plain ring that DLT has equal singular values, where
    # torch.linalg.svd's backward is NaN, and in millimetres the homogeneous DLT of inconsistent rays ends at infinity.
    rng = np.random.default_rng(3)
    P_lift = torch.from_numpy(np.concatenate([syn.ring_cameras(V, size, jitter=(0.02, 5.0 * size / 1024), rng=rng)
                                              for _ in range(frames)])).float()
    P_lift[:, :, 3] *= 1e-3
    target = torch.randn(frames, J, 3, device="cuda", dtype=torch.float64, generator=torch.Generator(device="cuda").manual_seed(7)) * 0.1
    seen = {}
    hook = m.reference.final_layer.register_forward_hook(lambda mod, args, out: seen.__setitem__("x", args[0].detach()))
    weight = m.reference.final_layer.weight

    def forward(peak_grad):
        cfg.merge_from_list(["EPIPOLAR_AMD.PEAK_GRAD", peak_grad])
        out = m.forward_views(img, P, src)
        return out[2], torch.full_like(out[3], 0.9)

    def lifted(locs, conf, lift_kernels):
        cfg.merge_from_list(["EPIPOLAR_AMD.LIFT_KERNELS", lift_kernels])
        X = m.lift(locs, conf, P_lift, V)
        assert torch.isfinite(X).all() and X.abs().max().item() < 1e3          # (the scene is well posed: points within a kilometre)
        return X

    X = lifted(*forward(False), True)
    assert X.grad_fn is None and not X.requires_grad         # PEAK_GRAD off: as before
    # ONE forward pass for both routes: the trunk's convolutions do not repeat their bits from call to call, and the liftings are
    # what is compared
    locs, conf = forward(True)
    hook.remove()
    scale = float(cfg.DATASETS.IMAGE_RESIZE) * float(cfg.DATASETS.PREDICT_RESIZE)
    _, info = ops.triangulate_views((locs.detach() * scale).view(frames, V, J, 2).contiguous(), conf.view(frames, V, J).contiguous(),
                                    P_lift.cuda().view(frames, V, 3, 4).contiguous(), method="pymvg", conf_thres=0.85, want_info=True)
    assert (info == (0xf | 0xf << 8)).all()                  # all four views selected and used, no threshold step, no zeros
    wgrad = lambda lift_kernels: torch.autograd.grad(((lifted(locs, conf, lift_kernels) - target) ** 2).sum(), weight, retain_graph=True)[0]
    kernels, torch_dlt = wgrad(True), wgrad(False)
    assert torch.isfinite(kernels).all() and kernels.abs().max().item() > 0

    def torch_route(dtype):
        final = copy.deepcopy(m.reference.final_layer).to(dtype)
        heat = final(seen["x"].to(dtype))
        found = backbones.soft_argmax_peaks(heat, float(cfg.KEYPOINT.SIGMA), float(cfg.BACKBONE.DOWNSAMPLE))[0]
        return torch.autograd.grad(((lifted(found, conf, False) - target) ** 2).sum(), final.weight)[0].double()

    f64 = torch_route(torch.float64)
    largest = f64.abs().max().item()
    own = (torch_route(torch.float32) - f64).abs().max().item() / largest
    apart = (kernels.double() - torch_dlt.double()).abs().max().item() / largest
    print("    final_layer.weight gradient: the torch route float32 against float64 %.3e of the largest element, "
          "kernels against the torch DLT %.3e (%.3f of 4 x)" % (own, apart, apart / (4 * own)))
    assert own > 0 and apart <= 4 * own, (apart, own)
