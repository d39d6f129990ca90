"""The training loss on the GPU: ops.heatmap_targets and ops.heatmap_loss (et_heatmap_targets / et_heatmap_loss / et_heatmap_loss_bwd)
against the reference's fixture (tests/golden/training/heatmap_loss.npz), the library's host hooks and the NumPy restatement, and
MultiViewPoseModel under EPIPOLAR_AMD.LOSS_KERNELS.

Shapes: the fixture's (9x7, 10x12, 17x19 with unaligned map bases, 64x64) and one 128x128 map, the library's limit.  Bounds: the CPU
file's (tests/test_heatmap_loss_cpu.py) -- equal bits for the targets, for the dense loss and gradient against the host hook (same
terms, same order, float64) and for on-the-fly against dense; the maker's conditions 3-5 plus one ulp against the reference."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

import heatmap_loss_restatement as restate

pytestmark = pytest.mark.gpu

LIMIT = (1, 1, 128, 128, 8.0, 4)                     # the largest map the library takes
LIMIT_POINT = np.array([[[250.3, 77.9]]])            # (its targets stay 2^-31 away from every float32 midpoint)
GRAD_CASES = [c for c in restate.CASES if c != "main"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "training", "heatmap_loss.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def hooks():
    import test_heatmap_loss_cpu as cpu
    from epipolar_transformers_amd import _lib

    return cpu, _lib.load()


def case(golden, name):
    return lambda k: golden["%s.%s" % (name, k)]


def dev(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.requires_grad_(True) if grad else t


def run(kind, pred, target=None, weight=None, per_joint=False, grad_out=None, **how):
    """ops.heatmap_loss on the device -> (loss float32 scalar, gradient) as NumPy."""
    from epipolar_transformers_amd import ops

    p = pred if isinstance(pred, torch.Tensor) else dev(pred, grad=True)
    loss = ops.heatmap_loss(p, None if target is None else dev(target), None if weight is None else dev(weight), kind=kind,
                            per_joint=per_joint, **{k: dev(v) if k == "points" else v for k, v in how.items()})
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    if grad_out is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(grad_out, device="cuda"))
    return loss.detach().cpu().numpy()[()], p.grad.cpu().numpy()


def limit_inputs():
    rng = np.random.default_rng(128)
    n, j, h, w, sigma, downsample = LIMIT
    pred = (rng.integers(-96, 160, (n, j, h, w)) / 128.0).astype(np.float32)
    return pred, LIMIT_POINT, np.array([[0.7]], np.float32)


@pytest.mark.parametrize("name", list(restate.CASES) + ["limit"])
def test_targets_equal_the_references_bits(golden, name):
    from epipolar_transformers_amd import ops

    if name == "limit":
        n, j, h, w, sigma, downsample = LIMIT
        points = LIMIT_POINT
        assert restate.midpoint_distance(restate.targets(points, h, w, sigma, downsample)) >= 2.0 ** -45
        want = restate.targets(points, h, w, sigma, downsample).astype(np.float32)
    else:
        n, j, h, w, sigma, downsample = restate.CASES[name]
        points, want = case(golden, name)("points"), case(golden, name)("targets")
    got = ops.heatmap_targets(dev(points), h, w, sigma, downsample)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, j, h, w)
    assert got.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("name", list(restate.CASES) + ["limit"])
def test_dense_loss_and_gradient_equal_the_host_hooks_bits(golden, hooks, name):
    cpu, lib = hooks
    if name == "limit":
        pred, points, weight = limit_inputs()
        tgt = restate.targets(points, *LIMIT[2:]).astype(np.float32)
    else:
        g = case(golden, name)
        pred, tgt, weight = g("pred"), g("targets"), g("weight")
    for kind, per_joint, _ in cpu.variants(name):
        wk = None if kind == "mse" else weight
        want_loss, want_grad = cpu.host_loss(lib, kind, pred, tgt, wk, per_joint, grad_out=1.0)
        loss, grad = run(kind, pred, tgt, wk, per_joint)
        assert loss == want_loss, (name, kind, per_joint, loss, want_loss)
        assert grad.tobytes() == want_grad.tobytes(), (name, kind, per_joint)
    # (N,J,1) weights, and none
    loss, grad = run("joint", pred, tgt, weight.reshape(*weight.shape, 1))
    assert loss == cpu.host_loss(lib, "joint", pred, tgt, weight)
    assert run("smoothmse", pred, tgt)[0] == cpu.host_loss(lib, "smoothmse", pred, tgt, None)


@pytest.mark.parametrize("name", list(restate.CASES) + ["limit"])
def test_on_the_fly_targets_equal_dense_targets_to_the_bit(golden, name):
    from epipolar_transformers_amd import ops

    if name == "limit":
        pred, points, weight = limit_inputs()
        n, j, h, w, sigma, downsample = LIMIT
    else:
        g = case(golden, name)
        pred, points, weight = g("pred"), g("points"), g("weight")
        n, j, h, w, sigma, downsample = restate.CASES[name]
    tgt = ops.heatmap_targets(dev(points), h, w, sigma, downsample).cpu().numpy()
    for kind in restate.KINDS:
        wk = None if kind == "mse" else weight
        dense = run(kind, pred, tgt, wk)
        fly = run(kind, pred, None, wk, points=points, sigma=sigma, downsample=downsample)
        assert fly[0] == dense[0] and fly[1].tobytes() == dense[1].tobytes(), (name, kind)


@pytest.mark.parametrize("name", list(restate.CASES))
def test_device_matches_the_reference_fixture(golden, hooks, name):
    cpu, _ = hooks
    g = case(golden, name)
    pred, tgt, weight = g("pred"), g("targets"), g("weight")
    n, j, h, w, sigma, downsample = restate.CASES[name]
    for kind, per_joint, key in cpu.variants(name):
        wk = None if kind == "mse" else weight
        loss, grad = run(kind, pred, None, wk, per_joint, points=g("points"), sigma=sigma, downsample=downsample)
        want = restate.loss(kind, pred, tgt, wk, per_joint)
        ref = g("loss." + key)
        print("%s %s: device %.9g restatement %.9g reference %.9g" % (name, key, loss, want, ref))
        assert restate.ulps_apart(loss, want) <= 1
        assert abs(float(loss) - float(ref)) <= restate.loss_bound(kind, pred.shape, want) + restate.ulp32(want)
        if name == "main" or per_joint:
            continue
        assert restate.ulps_apart(grad, restate.grad(kind, pred, tgt, wk)).max() <= 1
        apart = restate.ulps_apart(grad, g("grad." + kind))
        hot = np.zeros(pred.shape, bool)
        if kind == "smoothmse":
            hot = restate.smooth_raw(*restate.difference(kind, pred, tgt, wk)) > 400
        assert apart[~hot].max() <= 2 + 1, (name, kind, apart[~hot].max())
        if hot.any():
            assert name == "smooth_hot" and apart[hot].max() <= float(case(golden, "smooth_hot")("grad_ulps")) + 1
        if wk is not None and (weight == 0).any():
            assert (grad[np.broadcast_to((weight == 0)[..., None, None], pred.shape)] == 0).all()


def test_two_calls_give_the_same_bits_and_grad_output_scales_exactly(golden):
    g = case(golden, "smooth_hot")
    pred, tgt, weight = g("pred"), g("targets"), g("weight")
    for kind in restate.KINDS:
        wk = None if kind == "mse" else weight
        a, b = run(kind, pred, tgt, wk), run(kind, pred, tgt, wk)
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()
        half = run(kind, pred, tgt, wk, grad_out=0.5)
        assert half[0] == a[0] and (half[1] == a[1] * np.float32(0.5)).all() and (a[1] != 0).any()
    # the gradient reaches what the loss is combined with, without a synchronisation on the way: 3 * loss
    p = dev(pred, grad=True)
    from epipolar_transformers_amd import ops

    (ops.heatmap_loss(p, dev(tgt), dev(weight), kind="joint") * 3.0).backward()
    assert (p.grad.cpu().numpy() == run("joint", pred, tgt, weight, grad_out=3.0)[1]).all()


def test_a_channels_last_pred_is_copied_once_and_gives_the_same_bits(golden):
    """heat[0] comes from a channels-last trunk: ops.heatmap_loss takes it (one contiguous copy) instead of raising."""
    g = case(golden, "odd")
    pred, tgt, weight = g("pred"), g("targets"), g("weight")
    want = run("joint", pred, tgt, weight)
    p = dev(pred).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    assert not p.is_contiguous()
    got = run("joint", p, tgt, weight)
    assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and tuple(p.grad.shape) == pred.shape
    # the other operands must be contiguous: the usual ValueError
    from epipolar_transformers_amd import ops

    with pytest.raises(ValueError):
        ops.heatmap_loss(dev(pred), dev(tgt).contiguous(memory_format=torch.channels_last), kind="joint")
    with pytest.raises(ValueError):
        ops.heatmap_loss(dev(pred), dev(tgt)[:, :2], kind="joint")
    with pytest.raises(TypeError):
        ops.heatmap_loss(dev(pred), kind="joint", points=dev(g("points")).float(), sigma=12.0, downsample=4)


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def _model_and_batch(**over):
    """epipolarposeR-18 on 64x64 images, 2 frames x 4 views: the model, inputs and sizes of tests/test_gpu_model.py."""
    import test_gpu_model as tgm
    from epipolar_transformers_amd import synthetic as syn
    from epipolar_transformers_amd.model import ring_sources

    cfg, size, hs = tgm._cfg(**dict({"VIS.MULTIVIEW": False, "KEYPOINT.SIGMA": 8.0}, **over))
    m = tgm._model(cfg).train()
    frames, views = 2, 4
    g = torch.Generator(device="cuda").manual_seed(5)
    batch = {"img": torch.randn(frames * views, 3, size, size, device="cuda", generator=g),
             "KRT": torch.from_numpy(syn.ring_cameras(views, size)).float().repeat(frames, 1, 1),
             "other_index": ring_sources(frames, views, "cuda"), "num_views": views,
             "visibility": (torch.rand(frames * views, 17, 1, device="cuda", generator=g) < 0.8).float()}
    points = torch.rand(frames * views, 17, 3, device="cuda", generator=g, dtype=torch.float64) * size
    return m, cfg, batch, points, hs


def _freeze_forward(m, batch):
    """One real forward pass, then forward_views returns ITS result: every later m(...) sees the same heat maps to the bit."""
    with torch.no_grad():
        res = m.forward_views(batch["img"], batch["KRT"], batch["other_index"])
    m.forward_views = lambda *a, **k: res
    return res[1][0]


def test_model_knob_on_joint_equals_the_torch_loss_and_its_gradients():
    import test_gpu_model as tgm  # noqa: F401  (the tolerance below is its gradient tolerance)
    from epipolar_transformers_amd import ops

    m, cfg, batch, points, hs = _model_and_batch()
    batch["heatmap"] = ops.heatmap_targets(points[..., :2].contiguous(), hs, hs, 8.0, 4)
    shape = (8, 17, hs, hs)
    named = dict(m.reference.named_parameters())

    def elementwise(got, want, floor, k):
        # tests/test_gpu_model.py's elementwise tolerance for a whole-network gradient: relative L2 2e-2, maximum 5e-2 of the
        # largest element
        diff = got - want
        assert np.linalg.norm(diff) <= 2e-2 * max(np.linalg.norm(want), floor), k
        assert np.abs(diff).max() <= 5e-2 * max(float(np.abs(want).max()), floor), k

    # ---- two training steps, each with a forward pass of its own, as a training loop runs them.  Two passes of this network differ
    # by rounding (the loss below by ~1e-7 relative, knob or no knob), and that flips a few ReLU gates, each a discrete change of the
    # deep layers' gradients: tests/test_gpu_model.py therefore bounds three named tensors elementwise and every parameter's
    # gradient NORM, and so does this.
    results = {}
    for knob in (False, True):
        cfg.merge_from_list(["EPIPOLAR_AMD.LOSS_KERNELS", knob, "KEYPOINT.LOSS", "joint"])
        m.zero_grad()
        losses, _ = m(dict(batch), is_train=True)
        assert list(losses) == ["loss"]
        losses["loss"].backward()
        results[knob] = (losses["loss"].item(), {k: p.grad.detach().cpu().numpy().copy() for k, p in named.items() if p.grad is not None})
    (off, grads_off), (on, grads_on) = results[False], results[True]
    print("two passes: loss torch %.9g kernels %.9g" % (off, on))
    assert abs(on - off) <= restate.loss_bound("joint", shape, off) + restate.ulp32(off)
    assert sorted(grads_on) == sorted(grads_off) and "conv1.weight" in grads_on and "epipolar_sampler.z.weight" in grads_on
    for k in ("conv1.weight", "epipolar_sampler.z.weight", "final_layer.weight"):
        elementwise(grads_on[k], grads_off[k], 0.0, k)
    norms_off = {k: float(np.linalg.norm(v)) for k, v in grads_off.items()}
    floor = 1e-3 * max(norms_off.values())
    for k, want in norms_off.items():
        # (a bias in front of a batch norm in training mode has a mathematically zero gradient: rounding noise, hence the floor)
        assert abs(float(np.linalg.norm(grads_on[k])) - want) <= 2e-2 * max(want, floor), (k, float(np.linalg.norm(grads_on[k])), want)

    # ---- ONE forward pass, both losses on its heat maps, both backward passes through its graph: no gate can flip, so here EVERY
    # parameter's gradient is held to the elementwise tolerance (what is left is the backward's own summation order)
    m.zero_grad()
    res = m.forward_views(batch["img"], batch["KRT"], batch["other_index"])
    m.forward_views = lambda *a, **k: res
    params = [p for k, p in named.items() if k in grads_off]
    same = {}
    for knob in (False, True):
        cfg.merge_from_list(["EPIPOLAR_AMD.LOSS_KERNELS", knob])
        losses, _ = m(dict(batch), is_train=True)
        grads = torch.autograd.grad(losses["loss"], params, retain_graph=True)
        same[knob] = (losses["loss"].item(), [g.cpu().numpy() for g in grads])
    print("one pass:   loss torch %.9g kernels %.9g" % (same[False][0], same[True][0]))
    assert abs(same[True][0] - same[False][0]) <= restate.loss_bound("joint", shape, same[False][0]) + restate.ulp32(same[False][0])
    floor = 1e-3 * max(float(np.linalg.norm(g)) for g in same[False][1])
    for k, got, want in zip([k for k in named if k in grads_off], same[True][1], same[False][1]):
        elementwise(got, want, floor, k)


def test_model_targets_from_points_and_the_other_kinds():
    from epipolar_transformers_amd import ops

    m, cfg, batch, points, hs = _model_and_batch(**{"EPIPOLAR_AMD.LOSS_KERNELS": True})
    heat = _freeze_forward(m, batch)
    print("heat[0] contiguous:", heat.is_contiguous(), "strides", heat.stride())   # (channels-last when the trunk ran so)
    target = ops.heatmap_targets(points[..., :2].contiguous(), hs, hs, 8.0, 4)
    vis = batch["visibility"].reshape(8, 17)
    for kind in restate.KINDS:
        cfg.merge_from_list(["KEYPOINT.LOSS", kind])
        from_points, _ = m(dict(batch, **{"points-2d": points}), is_train=True)
        from_maps, _ = m(dict(batch, heatmap=target, **{"points-2d": points}), is_train=True)      # the heat map wins
        direct = ops.heatmap_loss(heat, target, None if kind == "mse" else vis.contiguous(), kind=kind)
        assert list(from_points) == ["loss"] and list(from_maps) == ["loss"]
        assert from_points["loss"].dtype == torch.float32 and from_points["loss"].is_cuda
        assert from_points["loss"].item() == from_maps["loss"].item() == direct.item() and direct.item() > 0, kind
    # neither heat map nor points: no loss
    assert m(dict(batch), is_train=True)[0] == {}
    cfg.merge_from_list(["KEYPOINT.LOSS", "l1"])
    with pytest.raises(ValueError, match="joint, smoothmse, mse"):
        m(dict(batch, heatmap=target), is_train=True)


def test_model_knob_off_computes_what_it_computed_before():
    """The knob off, or absent from the config altogether: `loss` is the torch JointsMSELoss of the heat maps, bit for bit, whatever
    KEYPOINT.LOSS says -- and the reference fixture's test of tests/test_gpu_model.py passes as it stands."""
    import test_gpu_model as tgm
    from epipolar_transformers_amd import ops
    from epipolar_transformers_amd.model import JointsMSELoss

    m, cfg, batch, points, hs = _model_and_batch(**{"KEYPOINT.LOSS": "smoothmse"})
    heat = _freeze_forward(m, batch)
    batch["heatmap"] = ops.heatmap_targets(points[..., :2].contiguous(), hs, hs, 8.0, 4)
    want = JointsMSELoss()(heat, batch["heatmap"], batch["visibility"])
    off, _ = m(dict(batch), is_train=True)
    dict.__delitem__(cfg.EPIPOLAR_AMD, "LOSS_KERNELS")
    absent, _ = m(dict(batch), is_train=True)
    assert list(off) == ["loss"] and torch.equal(off["loss"], want) and torch.equal(absent["loss"], want)
    tgm.test_model_equals_the_reference_modelbuilder_fixture()
