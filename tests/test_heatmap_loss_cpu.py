"""The training loss on the CPU: the library's host hooks (et_debug_host_heatmap_targets / _loss / _loss_bwd: the kernels' own
per-lane routines in serial loops, in the kernels' summation order) and the NumPy restatement against what the reference's
Heatmapcreator, JointsMSELoss, KeypointsMSESmoothLoss and MaskedMSELoss returned (tests/golden/training/heatmap_loss.npz, made by
make_heatmap_loss_golden.py), the ABI's argument checks, and the wiring of MultiViewPoseModel.forward under EPIPOLAR_AMD.LOSS_KERNELS.

Bounds.  Targets: equal bits (the maker's condition 2 keeps every value away from a float32 rounding midpoint).  Hook against
restatement: 1 ulp of float32 for the loss -- both sum the same non-negative float32 terms in float64, in error by M * 2^-53, so one
rounding decides -- and for every gradient element.  Against the reference: the maker's conditions 3 (loss), 4 and 5 (gradient: 2 ulp,
above the smoothmse threshold the recorded smooth_hot.grad_ulps) plus that one ulp."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

import heatmap_loss_restatement as restate
from epipolar_transformers_amd import _lib, build, default_cfg, model, ops

NEW_SYMBOLS = ("et_heatmap_targets", "et_heatmap_loss", "et_heatmap_loss_bwd", "et_debug_host_heatmap_targets",
               "et_debug_host_heatmap_loss", "et_debug_host_heatmap_loss_bwd")
KIND_CODES = {"joint": 0, "smoothmse": 1, "mse": 2}
GRAD_CASES = [c for c in restate.CASES if c != "main"]
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "training", "heatmap_loss.npz"), allow_pickle=False)


def case(golden, name):
    return lambda k: golden["%s.%s" % (name, k)]


def fp(a):
    return NULL if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_targets(lib, points, h, w, sigma, downsample):
    n, j, _ = points.shape
    out = np.full((n, j, h, w), np.nan, np.float32)
    rc = lib.et_debug_host_heatmap_targets(n, j, h, w, fp(points), sigma, downsample, fp(out))
    assert rc == 0, lib.et_last_error()
    return out


def host_loss(lib, kind, pred, target=None, weight=None, per_joint=False, points=None, sigma=0.0, downsample=0.0, grad_out=None):
    """-> loss (float32 scalar), and with `grad_out` also the gradient."""
    n, j, h, w = pred.shape
    partials, loss, den = np.full(n * j, np.nan), np.full(1, np.nan, np.float32), np.full(1, np.nan)
    rc = lib.et_debug_host_heatmap_loss(KIND_CODES[kind], n, j, h, w, fp(pred), fp(target), fp(points), sigma, downsample, fp(weight),
                                        int(per_joint), fp(partials), fp(loss), fp(den))
    assert rc == 0, lib.et_last_error()
    if grad_out is None:
        return loss[0]
    grad = np.full(pred.shape, np.nan, np.float32)
    go = np.array([grad_out], np.float32)
    rc = lib.et_debug_host_heatmap_loss_bwd(KIND_CODES[kind], n, j, h, w, fp(pred), fp(target), fp(points), sigma, downsample,
                                            fp(weight), fp(den), fp(go), fp(grad))
    assert rc == 0, lib.et_last_error()
    return loss[0], grad


def variants(name):
    """(kind, per_joint, key in the fixture) of every loss a case stores."""
    return [("joint", False, "joint"), ("joint", True, "joint_per_joint"), ("smoothmse", False, "smoothmse"), ("mse", False, "mse")]


def test_fixture_holds_every_case_and_the_makers_conditions(golden):
    assert sorted({k.split(".")[0] for k in golden.files}) == sorted(restate.CASES)
    background = np.float32(np.exp(-restate.CLIP))
    assert float(background) == 0.009999999776482582                   # prints as 0.01: the background is not zero
    for name, (n, j, h, w, sigma, downsample) in restate.CASES.items():
        g = case(golden, name)
        assert g("pred").shape == (n, j, h, w) and g("pred").dtype == np.float32 and g("targets").dtype == np.float32
        assert g("points").shape == (n, j, 2) and g("points").dtype == np.float64 and g("weight").shape == (n, j)
        assert float(g("sigma")) == sigma and float(g("downsample")) == downsample
        assert set(np.unique(g("weight"))) <= set(restate.WEIGHT_VALUES.tolist())
        assert g("targets").min() == background and g("targets").max() <= 1
        assert ("%s.grad.joint" % name in golden.files) == (name != "main")
        if n * j > 1:
            assert (g("weight") == 0).any() and ((g("weight") > 0) & (g("weight") < 1)).any()
        if n * j >= 6:
            assert (g("targets").reshape(n * j, -1) == background).all(1).any()           # a map that is all background
        assert restate.midpoint_distance(restate.targets(g("points"), h, w, sigma, downsample)) >= 2.0 ** -45
    g = case(golden, "smooth_hot")
    hot = restate.smooth_raw(*restate.difference("smoothmse", g("pred"), g("targets"), g("weight"))) > 400
    assert int(g("hot")) == hot.sum() and 0.02 <= hot.mean() <= 0.03 and 0 < float(g("grad_ulps")) <= 8


@pytest.mark.parametrize("name", list(restate.CASES))
def test_targets_equal_the_references_bits(lib, golden, name):
    g = case(golden, name)
    n, j, h, w, sigma, downsample = restate.CASES[name]
    assert restate.targets(g("points"), h, w, sigma, downsample).astype(np.float32).tobytes() == g("targets").tobytes()
    got = host_targets(lib, g("points"), h, w, sigma, downsample)
    assert got.tobytes() == g("targets").tobytes()


def test_targets_pair_v_with_the_rows_and_ignore_visibility(lib):
    # one point at (u, v) = (9.5, 21.5) on an 8 x 6 map, downsample 4: column 2 (4 * 2 + 1.5), row 5 (4 * 5 + 1.5)
    pts = np.array([[[9.5, 21.5]]])
    got = host_targets(lib, pts, 8, 6, 2.0, 4)
    assert got.shape == (1, 1, 8, 6) and np.unravel_index(got.argmax(), got.shape) == (0, 0, 5, 2) and got[0, 0, 5, 2] == 1.0
    assert got[0, 0, 0, 0] == np.float32(np.exp(-restate.CLIP))
    # a misaligned output base gives the same map (the scalar route)
    buf = np.full(1 + 48, np.nan, np.float32)
    assert lib.et_debug_host_heatmap_targets(1, 1, 8, 6, fp(pts), 2.0, 4.0, ctypes.c_void_p(buf.ctypes.data + 4)) == 0
    assert buf[1:].tobytes() == got.tobytes() and np.isnan(buf[0])


@pytest.mark.parametrize("name", list(restate.CASES))
def test_losses_match_the_restatement_and_the_reference(lib, golden, name):
    g = case(golden, name)
    pred, tgt, weight = g("pred"), g("targets"), g("weight")
    for kind, per_joint, key in variants(name):
        wk = None if kind == "mse" else weight
        want = restate.loss(kind, pred, tgt, wk, per_joint)
        got = host_loss(lib, kind, pred, tgt, wk, per_joint)
        ref = g("loss." + key)
        print("%s %s: hook %.9g restatement %.9g reference %.9g" % (name, key, got, want, ref))
        assert got.dtype == np.float32 and restate.ulps_apart(got, want) <= 1, (name, key)
        bound = restate.loss_bound(kind, pred.shape, want) + restate.ulp32(want)
        assert abs(float(got) - float(ref)) <= bound and abs(float(want) - float(ref)) <= bound, (name, key)
        # (N,J,1) weights are the same memory; on-the-fly targets are the same values
        if wk is not None:
            assert host_loss(lib, kind, pred, tgt, wk.reshape(*wk.shape, 1), per_joint) == got
        n, j, h, w, sigma, downsample = restate.CASES[name]
        assert host_loss(lib, kind, pred, None, wk, per_joint, points=g("points"), sigma=sigma, downsample=downsample) == got
    # no weight means ones
    ones = np.ones(weight.shape, np.float32)
    for kind in ("joint", "smoothmse"):
        assert host_loss(lib, kind, pred, tgt, None) == host_loss(lib, kind, pred, tgt, ones)


@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradients_match_the_restatement_and_the_reference(lib, golden, name):
    g = case(golden, name)
    pred, tgt, weight = g("pred"), g("targets"), g("weight")
    n, j, h, w, sigma, downsample = restate.CASES[name]
    for kind in restate.KINDS:
        wk = None if kind == "mse" else weight
        _, got = host_loss(lib, kind, pred, tgt, wk, grad_out=1.0)
        want = restate.grad(kind, pred, tgt, wk)
        ref = g("grad." + kind)
        assert got.dtype == np.float32 and not np.isnan(got).any()
        assert restate.ulps_apart(got, want).max() <= 1, (name, kind)
        apart = restate.ulps_apart(got, ref)
        hot = np.zeros(pred.shape, bool)
        if kind == "smoothmse":
            hot = restate.smooth_raw(*restate.difference(kind, pred, tgt, wk)) > 400
        print("%s %s: hook - reference %.2f ulp (hot: %.2f)" % (name, kind, apart[~hot].max(), apart[hot].max() if hot.any() else 0))
        assert apart[~hot].max() <= 2 + 1, (name, kind)
        if hot.any():
            assert name == "smooth_hot" and apart[hot].max() <= float(case(golden, "smooth_hot")("grad_ulps")) + 1
        if wk is not None:
            zero = np.broadcast_to((weight == 0)[..., None, None], pred.shape)
            assert zero.any() or n * j == 1
            assert (got[zero] == 0).all()
        # grad_output scales: 0.5 halves every element exactly; the target made on the fly gives the same bits
        _, half = host_loss(lib, kind, pred, tgt, wk, grad_out=0.5)
        assert (half == got * np.float32(0.5)).all()
        _, fly = host_loss(lib, kind, pred, None, wk, points=g("points"), sigma=sigma, downsample=downsample, grad_out=1.0)
        assert fly.tobytes() == got.tobytes()
    # per_joint multiplies the joint gradient by J (to rounding)
    _, pj = host_loss(lib, "joint", pred, tgt, weight, per_joint=True, grad_out=1.0)
    assert restate.ulps_apart(pj, restate.grad("joint", pred, tgt, weight, per_joint=True)).max() <= 1


def test_summation_order_does_not_depend_on_alignment(lib, golden):
    """Lanes own 16-byte quads of the flat tensor by INDEX: a base that is not 16-byte aligned takes the scalar route through
    the same order and gives the same bits."""
    g = case(golden, "odd")                                          # 323-element maps: partial first and last quads
    pred, tgt, weight = g("pred"), g("targets"), g("weight")

    def shifted(a):
        buf = np.empty(a.size + 1, np.float32)
        buf[1:] = a.reshape(-1)
        return buf[1:].reshape(a.shape)

    sp, st = shifted(pred), shifted(tgt)
    assert sp.ctypes.data % 16 == 4 or sp.ctypes.data % 16 != pred.ctypes.data % 16
    for kind in restate.KINDS:
        wk = None if kind == "mse" else weight
        a, ga = host_loss(lib, kind, pred, tgt, wk, grad_out=1.0)
        b, gb = host_loss(lib, kind, sp, st, wk, grad_out=1.0)
        assert a == b and ga.tobytes() == gb.tobytes()


def test_header_ctypes_and_exports_agree_and_bad_arguments_are_errors(lib):
    text = open(os.path.join(ROOT, "include", "epipolar_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert ("int %s(" % name) in text and name in _lib.exported_symbols() and hasattr(lib, name)
    assert lib.et_abi_version() == 14 and _lib.ET_ABI_VERSION == 14      # additive: the version stays
    for name, code in KIND_CODES.items():
        assert ops.LOSS_KINDS[name] == code and ("#define ET_LOSS_%s %d" % (name.upper(), code)) in text
    err = lambda: lib.et_last_error()
    # (the device entry points report these before any launch: no GPU is touched)
    pts, out = np.zeros((1, 1, 2)), np.zeros((1, 1, 4, 4), np.float32)
    for entry, extra in ((lib.et_debug_host_heatmap_targets, ()), (lib.et_heatmap_targets, (NULL,))):
        bad = lambda n, j, h, w, p=fp(pts), o=fp(out), sigma=2.0, ds=4.0: entry(n, j, h, w, p, sigma, ds, o, *extra) != 0
        assert bad(0, 1, 4, 4) and b"bad sizes" in err()
        assert bad(1, 0, 4, 4) and b"bad sizes" in err()
        assert bad(1, 1, 0, 4) and b"map 0 x 4" in err()
        assert bad(1, 1, 128, 129) and b"16384" in err()
        assert bad(1, 1, 4, 4, p=NULL) and b"NULL" in err()
        assert bad(1, 1, 4, 4, o=NULL) and b"NULL" in err()
        assert bad(1, 1, 4, 4, sigma=0.0) and b"sigma" in err()
        assert bad(1, 1, 4, 4, ds=-1.0) and b"downsample" in err()
        assert bad(1, 1, 4, 4, sigma=float("nan")) and b"sigma" in err()
        assert extra or not bad(1, 1, 4, 4)                 # (valid arguments: only the host hook can run here)
    pred, wt = np.zeros((1, 1, 4, 4), np.float32), np.ones((1, 1), np.float32)
    part, loss, den, go = np.zeros(1), np.zeros(1, np.float32), np.ones(1), np.ones(1, np.float32)

    def forward(entry, extra):
        return lambda kind=0, n=1, j=1, h=4, w=4, p=fp(pred), t=fp(out), pt=NULL, sigma=0.0, ds=0.0, wgt=NULL, a=fp(part), b=fp(loss), \
            c=fp(den): entry(kind, n, j, h, w, p, t, pt, sigma, ds, wgt, 0, a, b, c, *extra) != 0

    def backward(entry, extra):
        return lambda kind=0, n=1, j=1, h=4, w=4, p=fp(pred), t=fp(out), pt=NULL, sigma=0.0, ds=0.0, wgt=NULL, a=fp(den), b=fp(go), \
            c=fp(out.copy()): entry(kind, n, j, h, w, p, t, pt, sigma, ds, wgt, a, b, c, *extra) != 0

    for bad, runs in ((forward(lib.et_debug_host_heatmap_loss, ()), True), (forward(lib.et_heatmap_loss, (NULL,)), False),
                      (backward(lib.et_debug_host_heatmap_loss_bwd, ()), True), (backward(lib.et_heatmap_loss_bwd, (NULL,)), False)):
        assert bad(n=0) and b"bad sizes" in err()
        assert bad(j=-1) and b"bad sizes" in err()
        assert bad(h=0) and b"map 0 x 4" in err()
        assert bad(h=128, w=129) and b"16384" in err()
        assert bad(kind=3) and b"unknown kind 3" in err()
        assert bad(kind=-1) and b"unknown kind" in err()
        assert bad(kind=2, wgt=fp(wt)) and b"no weight" in err()
        for k in ("p", "a", "b", "c"):
            assert bad(**{k: NULL}) and b"NULL" in err()
        assert bad(t=NULL) and b"neither" in err()
        assert bad(pt=fp(pts), sigma=2.0, ds=4.0) and b"both" in err()
        assert bad(t=NULL, pt=fp(pts), sigma=0.0, ds=4.0) and b"sigma" in err()
        assert bad(t=NULL, pt=fp(pts), sigma=2.0, ds=0.0) and b"downsample" in err()
        if runs:
            assert not bad() and not bad(wgt=fp(wt)) and not bad(kind=2) and not bad(t=NULL, pt=fp(pts), sigma=2.0, ds=4.0)


def test_ops_wrappers_check_their_arguments_before_the_device():
    pred, tgt = torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4)
    pts = torch.zeros(1, 2, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="joint, smoothmse, mse"):
        ops.heatmap_loss(pred, tgt, kind="l1")
    with pytest.raises(ValueError, match="neither"):
        ops.heatmap_loss(pred, kind="joint")
    with pytest.raises(ValueError, match="both"):
        ops.heatmap_loss(pred, tgt, kind="joint", points=pts, sigma=2.0, downsample=4)
    with pytest.raises(ValueError, match="no weight"):
        ops.heatmap_loss(pred, tgt, torch.ones(1, 2), kind="mse")
    with pytest.raises(_lib.EpipolarAmdError):                       # no CPU fallback
        ops.heatmap_loss(pred, tgt, kind="joint")
    with pytest.raises(_lib.EpipolarAmdError):
        ops.heatmap_targets(pts, 4, 4, 2.0, 4)


# ---- the wiring of MultiViewPoseModel.forward, with the kernels and the network replaced by recorders ----------------------------
class _Stub(model.MultiViewPoseModel):
    """forward() with a canned backbone result: heat a list of (M,J,H,W) maps."""

    def __init__(self, cfg, maps=1, m=4, joints=5, hw=(6, 5)):
        torch.nn.Module.__init__(self)
        self.cfg, self.sharded = cfg, None
        self.criterion = model.JointsMSELoss(bool(getattr(cfg.KEYPOINT, "LOSS_PER_JOINT", False)))
        g = torch.Generator().manual_seed(0)
        heat = [torch.rand(m, joints, *hw, generator=g) for _ in range(maps)]
        self.canned = (None, heat, torch.rand(m, joints, 2, generator=g), torch.rand(m, joints, generator=g), None, None, None, None)

    def forward_views(self, *a, **k):
        return self.canned


def _cfg(knob, **keypoint):
    cfg = default_cfg()
    cfg.merge_from_list(["BACKBONE.BODY", "epipolarposeR-18", "BACKBONE.PRETRAINED", False, "KEYPOINT.NUM_PTS", 5, "KEYPOINT.SIGMA", 8.0,
                         "EPIPOLAR.MERGE", "late", "EPIPOLAR.SAMPLESIZE", 16, "VIS.MULTIVIEW", False, "EPIPOLAR_AMD.LOSS_KERNELS", knob])
    for k, v in keypoint.items():
        setattr(cfg.KEYPOINT, k, v)
    return cfg


def _batch(stub, heatmap=True, points=True, visibility=(4, 5, 1)):
    g = torch.Generator().manual_seed(1)
    heat = stub.canned[1][0]
    m, j = heat.shape[:2]
    batch = {"img": torch.zeros(m, 3, 8, 8), "KRT": torch.rand(m, 3, 4, generator=g), "other_index": torch.arange(m), "num_views": 2}
    if heatmap:
        batch["heatmap"] = torch.rand(heat.shape, generator=g)
    if points:
        batch["points-2d"] = torch.rand(m, j, 3, generator=g) * 20
    if visibility:
        batch["visibility"] = torch.rand(visibility, generator=g) < 0.7
    return batch


@pytest.fixture
def recorded(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "heatmap_loss", lambda *a, **k: calls.append((a, k)) or torch.tensor(float(len(calls))))
    return calls


def test_knob_defaults_to_off_and_off_is_todays_loss(recorded):
    assert default_cfg().EPIPOLAR_AMD.LOSS_KERNELS is False
    for keypoint in ({}, {"LOSS": "smoothmse"}, {"LOSS": "no such loss"}):      # KEYPOINT.LOSS belongs to the knob
        stub = _Stub(_cfg(False, **keypoint))
        assert type(stub.criterion) is model.JointsMSELoss and not stub.criterion.per_joint
        batch = _batch(stub)
        losses, metrics = stub(batch, is_train=True)
        assert not recorded and list(losses) == ["loss"] and metrics == {}
        want = model.JointsMSELoss()(stub.canned[1][0], batch["heatmap"], batch["visibility"].float())
        assert torch.equal(losses["loss"], want)
    # the real constructor builds the same criterion, and with the knob off never reads KEYPOINT.LOSS
    real = model.MultiViewPoseModel(_cfg(False, LOSS="no such loss", LOSS_PER_JOINT=True))
    assert type(real.criterion) is model.JointsMSELoss and real.criterion.per_joint
    # without a heat map there is no loss, as before
    assert stub(_batch(stub, heatmap=False), is_train=True) == ({}, {})


def test_knob_on_an_unknown_loss_is_a_value_error(recorded):
    with pytest.raises(ValueError, match="joint, smoothmse, mse"):
        model.MultiViewPoseModel(_cfg(True, LOSS="l1"))
    stub = _Stub(_cfg(True, LOSS="l1"))
    with pytest.raises(ValueError, match="KEYPOINT.LOSS 'l1' is none of joint, smoothmse, mse"):
        stub(_batch(stub), is_train=True)
    assert not recorded
    # evaluation never reads it
    stub(_batch(stub), is_train=False)


@pytest.mark.parametrize("visibility", [(4, 5), (4, 5, 1), None], ids=str)
def test_knob_on_hands_the_kernels_the_batch(recorded, visibility):
    for keypoint, kind in (({}, "joint"), ({"LOSS": "joint", "LOSS_PER_JOINT": True}, "joint"), ({"LOSS": "smoothmse"}, "smoothmse")):
        del recorded[:]
        stub = _Stub(_cfg(True, **keypoint), maps=2)
        batch = _batch(stub, visibility=visibility)
        losses, _ = stub(batch, is_train=True)
        assert len(recorded) == 1 and list(losses) == ["loss"] and float(losses["loss"]) == 1.0      # stage_loss0, renamed
        (pred, target, weight), how = recorded[0]
        assert torch.equal(pred, stub.canned[1][0]) and torch.equal(target, batch["heatmap"]) and target.is_contiguous()
        assert how == dict(kind=kind, per_joint=bool(keypoint.get("LOSS_PER_JOINT", False)))
        if visibility is None:
            assert weight is None
        else:
            assert weight.dtype == torch.float32 and tuple(weight.shape) == (4, 5)
            assert torch.equal(weight, batch["visibility"].reshape(4, 5).float())


def test_knob_on_mse_writes_every_stage_and_ignores_visibility(recorded):
    stub = _Stub(_cfg(True, LOSS="mse"), maps=3)
    batch = _batch(stub)
    losses, _ = stub(batch, is_train=True)
    assert list(losses) == ["stage_loss0", "stage_loss1", "stage_loss2", "loss"] and float(losses["loss"]) == 6.0
    for i, ((pred, target, weight), how) in enumerate(recorded):
        assert torch.equal(pred, stub.canned[1][i]) and weight is None and how == dict(kind="mse", per_joint=False)
    del recorded[:]
    stub = _Stub(_cfg(True, LOSS="mse"), maps=1)
    losses, _ = stub(_batch(stub), is_train=True)
    assert list(losses) == ["loss"] and len(recorded) == 1                # `loss` from stage_loss0


def test_knob_on_without_a_heatmap_the_target_comes_from_the_points(recorded):
    stub = _Stub(_cfg(True, LOSS="smoothmse"))
    batch = _batch(stub, heatmap=False)
    losses, _ = stub(batch, is_train=True)
    (pred, target, weight), how = recorded[0]
    assert target is None and list(losses) == ["loss"]
    assert how["points"].dtype == torch.float64 and torch.equal(how["points"], batch["points-2d"][..., :2].double())
    assert how["points"].is_contiguous() and how["sigma"] == 8.0 and how["downsample"] == 4.0 and how["kind"] == "smoothmse"
    # neither: no loss, as today
    del recorded[:]
    assert stub(_batch(stub, heatmap=False, points=False), is_train=True) == ({}, {}) and not recorded
    # evaluation is untouched by the knob
    assert stub(_batch(stub), is_train=False)[0] == {} and not recorded
