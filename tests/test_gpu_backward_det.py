"""The deterministic tiled backward (ABI 14: et_epipolar_backward_tiled_det, ops.backward_nhwc(form="tile_det"),
EPIPOLAR_AMD.DETERMINISTIC): d(feat_src) summed as 64-bit fixed point with integer atomics under a per-pair quantum, a tile
partition that depends on the inputs only.

  1. parity with the oracle on every rig, with the metric and tolerance of tests/test_gpu_rigs.py (max|got - want| <= 1e-4 max|want|);
  2. bit-reproducibility: five calls, two streams, dirty workspaces, NaN-poisoned outputs;
  3. batch independence: a pair alone, elsewhere in the batch, among 128;
  4. range: inputs and grad_out scaled by 1e-3 .. 1e3, grad_out down to 1e-6, all-zero grad_out; the error word stays 0
     (no test trips the guard on the GPU: the bound is tested on the CPU, tests/test_det_abi_cpu.py);
  5. workspace contracts: guard bands, a 16-byte-aligned base, one workspace for three kinds of call, a workspace too small;
  6. the module with EPIPOLAR_AMD.DETERMINISTIC; 7. twenty poisoned runs at two shapes.
"""
import ctypes

import numpy as np
import pytest
import torch

import abi_harness as hx
from abi_harness import C, Arena, call

pytestmark = pytest.mark.gpu

TOL_GRAD_REL = 1e-4                   # tests/test_gpu_rigs.py::test_backward_forms_vs_oracle_on_rig
RIGS = ["ring", "epipole_inside", "epipole_border", "near_rectified_x", "near_rectified_y", "rectified_x", "identical", "h36m_room"]
_cache = {}


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from epipolar_transformers_amd import _lib, camera, ops

    _lib.load()
    assert ops.POISON_OUTPUTS
    return _lib, camera, ops


def _case(oracle_mod, camera, rig, h, k):
    """Two pairs of the rig + the oracle's gradients (the cases of tests/test_gpu_rigs.py)."""
    key = (rig, h, k)
    if key in _cache:
        return _cache[key]
    from epipolar_transformers_amd import synthetic as syn

    seed = 700 + h + len(rig)
    jitter = None if rig in ("epipole_border",) else (0.05, 8.0)
    P1, P2 = syn.rig_pairs(rig, 1, 4 * h, seed=seed, jitter=jitter)
    pick = [1, 2] if rig == "h36m_room" else [0, 1]
    P1, P2 = P1[pick], P2[pick]
    f1, f2 = syn.make_features(2, C, h, h, seed=seed)
    f1[0, :, 5, 7] = 0
    cam = camera.pair_algebra(P1, P2)
    so = oracle_mod.LayerSpec(h, h, k)
    with np.errstate(all="ignore"):
        want = oracle_mod.forward(so, f1, f2, None, None, cam=cam.numpy())
        g = torch.randn(2, C, h, h, generator=torch.Generator().manual_seed(seed + 1))
        g1, g2 = oracle_mod.backward(so, f1.numpy(), f2.numpy(), want["sample_locs"], g.numpy())
    _cache[key] = dict(f1=f1, f2=f2, cam=cam, g=g, g1=g1, g2=g2)
    return _cache[key]


def _assert_close(what, got, want):
    got = got.permute(0, 3, 1, 2).cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert np.isfinite(got).all(), what
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max())
    print("%s: max error %.3g of %.3g (bound %.3g)" % (what, err, scale, TOL_GRAD_REL * scale))
    assert err <= TOL_GRAD_REL * scale, (what, err, scale)


def _err_word(ws):
    return int(hx.ws_header(ws)[1].item())


def _parity(env, oracle_mod, rig, h, k):
    _lib, camera, ops = env
    case = _case(oracle_mod, camera, rig, h, k)
    ref, src, cam = ops.to_nhwc(case["f1"].cuda()), ops.to_nhwc(case["f2"].cuda()), case["cam"].cuda()
    g = ops.to_nhwc(case["g"].cuda())
    spec = ops.LayerSpec(H=h, W=h, K=k)
    attn = ops.forward_nhwc(spec, ref, src, cam)[1]
    ws = ops.det_tile_workspace(spec, 2, C, ref.device)
    res = {}
    for a in (None, attn):
        gr, gs = ops.backward_nhwc(spec, ref, src, cam, g, form="tile_det", attn=a, workspace=ws)
        torch.cuda.synchronize()
        assert _err_word(ws) == 0
        tag = "%s %dx%d K%d %s" % (rig, h, h, k, "attn" if a is not None else "recompute")
        _assert_close(tag + " grad_ref", gr, case["g1"])
        _assert_close(tag + " grad_src", gs, case["g2"])
        res[a is not None] = (gr, gs)
    # one source role at a time: masks 1 + 2 give mask 3, grad_ref is the same
    parts = []
    for mask in (1, 2):
        gr, gs = ops.backward_nhwc(ops.LayerSpec(H=h, W=h, K=k, src_grad_mask=mask), ref, src, cam, g, form="tile_det", attn=attn, workspace=ws)
        torch.cuda.synchronize()
        assert _err_word(ws) == 0
        _assert_close("%s mask %d grad_ref" % (rig, mask), gr, case["g1"])
        parts.append(gs)
    _assert_close("%s masks 1 + 2 grad_src" % rig, parts[0] + parts[1], case["g2"])
    _assert_close("%s masks 1 + 2 against mask 3" % rig, (parts[0] + parts[1]).permute(0, 3, 1, 2).cpu().numpy(),
                  res[True][1].permute(0, 3, 1, 2).cpu().numpy())


@pytest.mark.parametrize("h,k", [(64, 64), (96, 64)], ids=["64x64-K64", "96x96-K64"])
@pytest.mark.parametrize("rig", RIGS)
def test_parity_vs_oracle_on_rig(env, oracle_mod, rig, h, k):
    _parity(env, oracle_mod, rig, h, k)


@pytest.mark.parametrize("rig,h,k", [("ring", 64, 128), ("epipole_inside", 64, 128), ("h36m_room", 128, 64)],
                         ids=["ring-64x64-K128", "epipole-inside-64x64-K128", "room-128x128-K64"])
def test_parity_vs_oracle_two_samples_per_lane_and_large_map(env, oracle_mod, rig, h, k):
    _parity(env, oracle_mod, rig, h, k)


def _batch(camera, rig, n, h, seed, scale=1.0, gscale=1.0):
    from epipolar_transformers_amd import synthetic as syn

    per = 4 if rig in ("ring", "h36m_room") else 2
    P1, P2 = syn.rig_pairs(rig, (n + per - 1) // per, 4 * h, seed=seed, jitter=(0.05, 8.0))
    cam = camera.pair_algebra(P1[:n], P2[:n]).cuda()
    g0 = torch.Generator(device="cuda").manual_seed(seed)
    ref = torch.randn(n, h, h, C, device="cuda", generator=g0).relu_() * scale
    src = torch.randn(n, h, h, C, device="cuda", generator=g0).relu_() * scale
    gout = torch.randn(n, h, h, C, device="cuda", generator=g0) * gscale
    return ref, src, cam, gout


@pytest.mark.parametrize("rig,n", [("h36m_room", 128), ("epipole_inside", 16), ("ring", 16)])
def test_five_calls_two_streams_dirty_workspace_same_bits(env, rig, n):
    """Five calls on identical inputs: torch.equal gradients -- on the room rig at the headline batch (every branch of the
    default over-capacity policy), the epipole-inside rig and the ring; with and without the forward's attention; on two
    streams with a workspace each; on a workspace with garbage behind the header; outputs NaN-poisoned (ops.POISON_OUTPUTS)."""
    _lib, camera, ops = env
    h, k = 64, 64
    ref, src, cam, gout = _batch(camera, rig, n, h, 1000)
    spec = ops.LayerSpec(H=h, W=h, K=k)
    attn = ops.forward_nhwc(spec, ref, src, cam)[1]
    for a in (attn, None):
        ws = ops.det_tile_workspace(spec, n, C, ref.device)
        first = ops.backward_nhwc(spec, ref, src, cam, gout, form="tile_det", attn=a, workspace=ws)
        assert torch.isfinite(first[0]).all() and torch.isfinite(first[1]).all()
        for rep in range(4):
            again = ops.backward_nhwc(spec, ref, src, cam, gout, form="tile_det", attn=a, workspace=ws)
            assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]), "call %d differs" % (rep + 2)
        if a is None and n > 16:
            continue
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        wss = [ops.det_tile_workspace(spec, n, C, ref.device),
               hx.dirty_tile_workspace(ops.det_tile_workspace(spec, n, C, ref.device), "random", -123456789)]
        out = []
        for st, w in zip(streams, wss):
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                out.append(ops.backward_nhwc(spec, ref, src, cam, gout, form="tile_det", attn=a, workspace=w))
        torch.cuda.synchronize()
        for got, w in zip(out, wss):
            assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])
            assert _err_word(w) == 0
        w = hx.dirty_tile_workspace(ops.det_tile_workspace(spec, n, C, ref.device), "ff", 0x7FFFFF00)
        got = ops.backward_nhwc(spec, ref, src, cam, gout, form="tile_det", attn=a, workspace=w)
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])
        assert not hx.ws_header(w)[10:].any()


@pytest.mark.parametrize("rig", ["h36m_room", "epipole_inside"])
def test_a_pair_has_the_same_gradients_alone_and_in_any_batch(env, rig):
    """The quantum is per pair and the partition per tile: pair i alone (N = 1), at another position, among 128."""
    _lib, camera, ops = env
    h, k, n = 64, 64, 128
    ref, src, cam, gout = _batch(camera, rig, n, h, 2000)
    spec = ops.LayerSpec(H=h, W=h, K=k)
    gr, gs = ops.backward_nhwc(spec, ref, src, cam, gout, form="tile_det")
    for i in (0, 1, 2, 77, 127):
        sl = slice(i, i + 1)
        one = ops.backward_nhwc(spec, ref[sl].contiguous(), src[sl].contiguous(), cam[sl].contiguous(), gout[sl].contiguous(), form="tile_det")
        assert torch.equal(one[0][0], gr[i]) and torch.equal(one[1][0], gs[i]), "pair %d alone differs from the batch" % i
    idx = torch.tensor([5, 127, 1, 77, 0, 2], device="cuda")                 # other positions, another batch size
    sub = ops.backward_nhwc(spec, ref[idx].contiguous(), src[idx].contiguous(), cam[idx].contiguous(), gout[idx].contiguous(), form="tile_det")
    assert torch.equal(sub[0], gr[idx]) and torch.equal(sub[1], gs[idx])


@pytest.mark.parametrize("scale,gscale", [(1e-3, 1e-3), (1e3, 1e3), (1.0, 1e-6), (1e-3, 1e3), (1e3, 1e-6)])
def test_range_of_inputs(env, scale, gscale):
    """Scaled inputs against the bit-reproducible gather form (itself pinned to the oracle) at the parity tolerance; the soft-max
    scale shrinks with scale^2 so that the attention stays a soft-max and not an arg-max."""
    _lib, camera, ops = env
    h, k, n = 64, 64, 4
    ref, src, cam, gout = _batch(camera, "epipole_inside", n, h, 3000, scale, gscale)
    spec = ops.LayerSpec(H=h, W=h, K=k, softmax_scale=0.125 / (scale * scale))
    ws = ops.det_tile_workspace(spec, n, C, ref.device)
    gr, gs = ops.backward_nhwc(spec, ref, src, cam, gout, form="tile_det", workspace=ws)
    torch.cuda.synchronize()
    assert _err_word(ws) == 0
    g_ref, g_src = ops.backward_nhwc(spec, ref, src, cam, gout, form="gather")
    for what, got, want in (("grad_ref", gr, g_ref), ("grad_src", gs, g_src)):
        _assert_close("scale %g / %g %s" % (scale, gscale, what), got.cpu().numpy(), want.cpu().numpy())


def test_zero_grad_out_gives_exact_zeros(env):
    _lib, camera, ops = env
    ref, src, cam, gout = _batch(camera, "ring", 4, 64, 3001)
    spec = ops.LayerSpec(H=64, W=64, K=64)
    ws = ops.det_tile_workspace(spec, 4, C, ref.device)
    gr, gs = ops.backward_nhwc(spec, ref, src, cam, torch.zeros_like(gout), form="tile_det", workspace=ws)
    assert not gr.any() and not gs.any() and _err_word(ws) == 0


def test_form_selection_and_softmax_off(env):
    _lib, camera, ops = env
    ref, src, cam, gout = _batch(camera, "ring", 2, 16, 3002)
    bit = _lib.ET_VARIANT_BWD_DETERMINISTIC
    called = []
    keep = _lib.load().et_epipolar_backward_tiled_det
    want = ops.backward_nhwc(ops.LayerSpec(H=16, W=16, K=16), ref, src, cam, gout, form="tile_det")
    got = ops.backward_nhwc(ops.LayerSpec(H=16, W=16, K=16, variant=bit), ref, src, cam, gout)          # form=None: the bit decides
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    gather = ops.backward_nhwc(ops.LayerSpec(H=16, W=16, K=16), ref, src, cam, gout, form="gather")
    # no tile path (C = 64) and soft-max off: the choice stays the bit-reproducible gather form
    r64, s64, g64 = ref[..., :64].contiguous(), src[..., :64].contiguous(), gout[..., :64].contiguous()
    a = ops.backward_nhwc(ops.LayerSpec(H=16, W=16, K=16, variant=bit), r64, s64, cam, g64)
    b = ops.backward_nhwc(ops.LayerSpec(H=16, W=16, K=16), r64, s64, cam, g64, form="gather")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    off = ops.LayerSpec(H=16, W=16, K=16, softmax_enabled=False, variant=bit)
    a = ops.backward_nhwc(off, ref * 0.25, src * 0.25, cam, gout)
    b = ops.backward_nhwc(ops.LayerSpec(H=16, W=16, K=16, softmax_enabled=False), ref * 0.25, src * 0.25, cam, gout, form="gather")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(_lib.EpipolarAmdError, match="soft-max"):
        ops.backward_nhwc(off, ref, src, cam, gout, form="tile_det")
    for x, y in zip(want, gather):
        assert (x - y).abs().max().item() <= TOL_GRAD_REL * y.abs().max().item()


@pytest.mark.parametrize("rig,n,h,w,k,shift", [("ring", 3, 16, 16, 16, 0), ("epipole_inside", 2, 64, 64, 64, 16), ("ring", 2, 40, 96, 33, 16),
                                               ("ring", 2, 20, 60, 128, 0)])
def test_guard_bands_and_a_16_byte_aligned_base(env, rig, n, h, w, k, shift):
    _lib, camera, ops = env
    lib = _lib.load()
    ref, src, cam = hx.pair_inputs(n, h, w, 50 + h, rig)
    gout = torch.randn(n, h, w, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    spec = ops.LayerSpec(H=h, W=w, K=k)
    xs, ys, steps = spec.constants(torch.device("cuda", torch.cuda.current_device()))
    d = spec.desc(n, C)
    nbytes = int(lib.et_epipolar_backward_tiled_det_workspace_bytes(ctypes.byref(d)))
    a = Arena().add("gref", (n, h, w, C)).add("gsrc", (n, h, w, C)).add("ws", nbytes, torch.uint8, fill=0, shift=shift).build()
    snap = hx.frozen(xs=xs, ys=ys, steps=steps, cam=cam, ref=ref, src=src, gout=gout)
    call("et_epipolar_backward_tiled_det", d, xs, ys, steps, cam, ref, src, None, gout, a["gref"], a["gsrc"], a["ws"], ctypes.c_size_t(nbytes))
    a.check()
    hx.assert_unchanged(snap)
    assert _err_word(a["ws"]) == 0
    g_ref, g_src = ops.backward_nhwc(spec, ref, src, cam, gout, form="gather")
    for got, want in ((a["gref"], g_ref), (a["gsrc"], g_src)):
        assert torch.isfinite(got).all()
        assert (got - want).abs().max().item() <= TOL_GRAD_REL * max(want.abs().max().item(), 1e-30)
    with pytest.raises(_lib.EpipolarAmdError, match="smaller than"):
        call("et_epipolar_backward_tiled_det", d, xs, ys, steps, cam, ref, src, None, gout, a["gref"], a["gsrc"], a["ws"], ctypes.c_size_t(nbytes - 1))
    a.check()


def test_one_workspace_for_forward_backward_and_deterministic_backward(env):
    """forward_tiled, backward_tiled and backward_tiled_det in turn on one workspace, one stream, two shapes: what each returns on
    a fresh workspace (the forward and the deterministic backward bit for bit)."""
    _lib, camera, ops = env
    shapes = [("epipole_inside", 4, 64, 64), ("ring", 3, 16, 16), ("epipole_inside", 4, 64, 64)]
    big = ops.det_tile_workspace(ops.LayerSpec(H=64, W=64, K=64), 4, C, "cuda")
    for rig, n, h, k in shapes:
        ref, src, cam, gout = _batch(camera, rig, n, h, 60 + h)
        spec = ops.LayerSpec(H=h, W=h, K=k)
        for ws in (big, None):
            fresh = (lambda: ops.det_tile_workspace(spec, n, C, "cuda")) if ws is None else (lambda: big)
            fw = ops.forward_nhwc(spec, ref, src, cam, workspace=fresh())
            bt = ops.backward_nhwc(spec, ref, src, cam, gout, form="tile", attn=fw[1], workspace=fresh())
            bd = ops.backward_nhwc(spec, ref, src, cam, gout, form="tile_det", attn=fw[1], workspace=fresh())
            torch.cuda.synchronize()
            if ws is big:
                got = (fw, bt, bd)
                assert _err_word(big) == 0
        for a, b in zip(got[0], fw):
            assert hx.same_bits(a, b)
        for a, b in zip(got[2], bd):
            assert torch.equal(a, b)
        for a, b in zip(got[1], bd):
            assert (a - b).abs().max().item() <= TOL_GRAD_REL * b.abs().max().item()


def _module(det, h=32, k=16, extra=()):
    from epipolar_transformers_amd import default_cfg
    from epipolar_transformers_amd.epipolar import Epipolar

    cfg = default_cfg()
    cfg.merge_from_list(["KEYPOINT.HEATMAP_SIZE", (h, h), "KEYPOINT.NFEATS", C, "EPIPOLAR.SAMPLESIZE", k, "EPIPOLAR.ATTENTION", "avg",
                         "EPIPOLAR.PARAMETERIZED", ("z",), "EPIPOLAR.ZRESIDUAL", True, "EPIPOLAR.USE_CORRECT_NORMALIZE", True,
                         "DATASETS.IMAGE_SIZE", (4 * h, 4 * h), "EPIPOLAR_AMD.DETERMINISTIC", det] + list(extra))
    torch.manual_seed(3)
    mod = Epipolar(cfg=cfg).cuda().train()
    if hasattr(mod, "bn"):
        with torch.no_grad():
            mod.bn.weight.normal_(1, 0.1)
            mod.bn.bias.normal_(0, 0.1)
    return mod


def _train_pass(mod, f1, f2, P1, P2, gout):
    a1, a2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    y = mod(a1, a2, P1, P2)[0]
    (y * gout).sum().backward()
    torch.cuda.synchronize()
    return [y.detach().clone(), a1.grad.clone(), a2.grad.clone()] + [q.grad.clone() for q in (mod.z.weight, mod.z.bias, mod.bn.weight, mod.bn.bias)] + \
           [mod.bn.running_mean.clone(), mod.bn.running_var.clone()]


def test_module_with_the_deterministic_knob(env, monkeypatch):
    """Two training-mode forward + backward passes from the same state: the six gradients and the running statistics bit for bit.
    With the knob off the module takes the float-atomic tile form as before and returns the same outputs; an option-branch
    configuration raises on backward with the knob on."""
    from epipolar_transformers_amd import synthetic as syn

    _lib, camera, ops = env
    n, h = 8, 32
    P1, P2 = syn.make_pairs(n // 4, 4, 4 * h, seed=5, jitter=(0.05, 4.0))
    g0 = torch.Generator().manual_seed(11)
    f1, f2 = torch.randn(n, C, h, h, generator=g0).relu().cuda(), torch.randn(n, C, h, h, generator=g0).relu().cuda()
    gout = torch.randn(n, C, h, h, generator=g0).cuda()
    forms = []
    keep = ops.backward_nhwc

    def spy(spec, *a, **kw):
        forms.append(bool(spec.variant & _lib.ET_VARIANT_BWD_DETERMINISTIC))
        return keep(spec, *a, **kw)

    monkeypatch.setattr(ops, "backward_nhwc", spy)
    runs = [_train_pass(_module(True), f1, f2, P1, P2, gout) for _ in range(2)]
    assert forms == [True, True]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    off = _train_pass(_module(False), f1, f2, P1, P2, gout)
    assert forms == [True, True, False]
    assert torch.equal(off[0], runs[0][0]) and torch.equal(off[7], runs[0][7]) and torch.equal(off[8], runs[0][8])     # same forward
    for a, b in zip(off[1:7], runs[0][1:7]):
        assert (a - b).abs().max().item() <= 2e-4 * max(b.abs().max().item(), 1e-6)
    mod = _module(True, extra=["EPIPOLAR.PARAMETERIZED", ("z", "theta", "phi", "g")])
    a1, a2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    y = mod(a1, a2, P1, P2)[0]
    with pytest.raises(RuntimeError, match="DETERMINISTIC"):
        (y * gout).sum().backward()


@pytest.mark.parametrize("rig,n,h,k", [("epipole_inside", 32, 64, 64), ("ring", 4, 96, 64)], ids=["64x64-K64-N32-epipole-inside", "96x96-K64-N4"])
def test_twenty_poisoned_runs_are_finite_and_bit_equal(env, rig, n, h, k):
    _lib, camera, ops = env
    ref, src, cam, gout = _batch(camera, rig, n, h, 11 + n)
    spec = ops.LayerSpec(H=h, W=h, K=k)
    attn = ops.forward_nhwc(spec, ref, src, cam)[1]
    first = {}
    for rep in range(20):
        a = attn if rep % 2 else None
        gr, gs = ops.backward_nhwc(spec, ref, src, cam, gout, form="tile_det", attn=a)
        assert torch.isfinite(gr).all() and torch.isfinite(gs).all(), "run %d" % rep
        if rep % 2 not in first:
            first[rep % 2] = (gr, gs)
        else:
            assert torch.equal(gr, first[rep % 2][0]) and torch.equal(gs, first[rep % 2][1]), "run %d differs from the first" % rep
    g_ref, g_src = ops.backward_nhwc(spec, ref, src, cam, gout, form="gather")
    for got, want in ((first[0][0], g_ref), (first[0][1], g_src)):
        assert (got - want).abs().max().item() <= TOL_GRAD_REL * want.abs().max().item()
