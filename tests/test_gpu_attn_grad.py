"""The gradient through the returned attention (ET_HAS_ATTN_GRAD: the *_ga entry points, ops.backward_nhwc(grad_attn=...),
ops.backward_general_nhwc(grad_attn=...), EPIPOLAR_AMD.ATTN_GRAD) in every backward kernel family.

Reference: float64 torch autograd through oracle.torch_ref_path.forward (the op-sequence port pinned to the real reference's
fixtures) on the sample locations of oracle.sample_locs, loss (out . G).sum() + (attn . GA).sum(); for the option branches the
module's own torch restatement (EPIPOLAR_AMD.GENERAL_KERNEL False) in float64.  Tolerance: TOL_GRAD_REL = 1e-4 times the
largest magnitude of the reference gradient (tests/test_gpu_rigs.py).  The gradient is linear in (G, GA), so one float64
backward per term and shape serves the three losses: (G, GA), (0, GA) and (G, 1e4 GA)."""
import copy
import os
import warnings

import numpy as np
import pytest
import torch

import abi_harness as hx
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

TOL_GRAD_REL = 1e-4                   # tests/test_gpu_rigs.py::test_backward_forms_vs_oracle_on_rig
N = 2
LOSSES = {"out+attn": (1.0, 1.0), "attn-only": (0.0, 1.0), "attn-1e4": (1.0, 1e4)}      # multiples of (G, GA)
_cache = {}


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from epipolar_transformers_amd import _lib, camera, ops

    _lib.load()
    assert ops.POISON_OUTPUTS
    return _lib, camera, ops


def _inputs(camera, rig, h, w, c, k, seed):
    """Two pairs of the rig (the room rig: the two with pixels that have no segment), seeded post-ReLU features with an all-zero
    reference row (an all-masked pixel) and an all-zero source patch (partly masked pixels), G and GA."""
    from epipolar_transformers_amd import synthetic as syn

    P1, P2 = syn.rig_pairs(rig, 1, 4 * max(h, w), seed=seed, jitter=(0.05, 8.0))
    pick = [1, 2] if rig == "h36m_room" else [0, 1]
    cam = camera.pair_algebra(P1[pick], P2[pick])
    f1, f2 = syn.make_features(N, c, h, w, seed=seed)
    f1[0, :, h // 2, w // 3] = 0
    f2[:, :, h // 3:h // 3 + 3, w // 2:w // 2 + 3] = 0
    gen = torch.Generator().manual_seed(seed + 1)
    G = torch.randn(N, c, h, w, generator=gen)
    GA = torch.randn(N, k, h, w, generator=gen)
    return f1, f2, cam, G, GA


def _case(oracle_mod, camera, h, w, c, k, softmax):
    """Inputs + the float64 reference gradients of the two terms, computed once per shape and shared (never modified)."""
    key = (h, w, c, k, softmax)
    if key in _cache:
        return _cache[key]
    from oracle import torch_ref_path as trp

    f1, f2, cam, G, GA = _inputs(camera, "h36m_room", h, w, c, k, 4100 + h + k)
    so = oracle_mod.LayerSpec(h, w, k, softmax_enabled=softmax)
    with np.errstate(all="ignore"):
        locs = oracle_mod.sample_locs(so, None, None, cam=cam.numpy())
    a, b = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    out, attn, _ = trp.forward(a, b, torch.from_numpy(locs).double(), softmax_scale=0.125, softmax_enabled=softmax)
    d_out = torch.autograd.grad((out * G.double()).sum(), (a, b), retain_graph=True)
    d_att = torch.autograd.grad((attn * GA.double()).sum(), (a, b))
    assert all(float(t.abs().max()) > 0 for t in d_att), "the attention term must carry a gradient"
    _cache[key] = dict(f1=f1, f2=f2, cam=cam, G=G, GA=GA, d_out=[t.numpy() for t in d_out], d_att=[t.numpy() for t in d_att],
                       attn=attn.detach().numpy())
    return _cache[key]


def _assert_close(what, got, want, tol=TOL_GRAD_REL):
    got = got.permute(0, 3, 1, 2).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), what
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max())
    print("%s: max error %.3g of %.3g (bound %.3g)" % (what, err, scale, tol * scale))
    assert err <= tol * scale, (what, err, scale)


def _backward(ops, spec, case, form, loss, c):
    """One HIP backward of `form` ("gather", "atomic", "tile", "tile-attn", "tile_det", "tile_det-attn") under `loss`."""
    sg, sa = LOSSES[loss]
    ref, src, cam = ops.to_nhwc(case["f1"].cuda()), ops.to_nhwc(case["f2"].cuda()), case["cam"].cuda()
    g, ga = ops.to_nhwc((case["G"] * sg).cuda()), (case["GA"] * sa).cuda()
    base = form.split("-")[0]
    attn = ops.forward_nhwc(spec, ref, src, cam)[1] if form.endswith("-attn") else None
    ws = ops.det_tile_workspace(spec, N, c, ref.device) if base == "tile_det" else None
    gr, gs = ops.backward_nhwc(spec, ref, src, cam, g, form=base, attn=attn, workspace=ws, grad_attn=ga)
    torch.cuda.synchronize()
    if ws is not None:
        assert int(hx.ws_header(ws)[1].item()) == 0, "the sticky error word"
    want = [sg * o + sa * t for o, t in zip(case["d_out"], case["d_att"])]
    tag = "%s %s %dx%d C%d K%d" % (form, loss, spec.H, spec.W, c, spec.K)
    _assert_close(tag + " grad_ref", gr, want[0])
    _assert_close(tag + " grad_src", gs, want[1])


# ---- per-pixel forms ----------------------------------------------------------------------------------------------------
PIXEL_SHAPES = [(10, 10, 8, 16, True), (9, 7, 36, 5, True), (16, 16, 8, 12, False)]


@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("form", ["gather", "atomic"])
@pytest.mark.parametrize("h,w,c,k,softmax", PIXEL_SHAPES, ids=["10x10-C8-K16", "9x7-C36-K5", "16x16-C8-K12-softmax-off"])
def test_per_pixel_forms_vs_float64_autograd(env, oracle_mod, h, w, c, k, softmax, form, loss):
    _lib, camera, ops = env
    case = _case(oracle_mod, camera, h, w, c, k, softmax)
    _backward(ops, ops.LayerSpec(H=h, W=w, K=k, softmax_enabled=softmax), case, form, loss, c)


def test_the_forward_attention_is_the_references(env, oracle_mod):
    """(what GA multiplies: the attention the kernels return against the float64 reference's, on the rig with invalid pixels)"""
    _lib, camera, ops = env
    case = _case(oracle_mod, camera, 10, 10, 8, 16, True)
    spec = ops.LayerSpec(H=10, W=10, K=16)
    attn = ops.forward_nhwc(spec, ops.to_nhwc(case["f1"].cuda()), ops.to_nhwc(case["f2"].cuda()), case["cam"].cuda())[1]
    assert np.abs(attn.cpu().numpy() - case["attn"]).max() <= 1e-5


# ---- tile forms (C = 256) -----------------------------------------------------------------------------------------------
TILE_SHAPES = [(16, 16, 16), (33, 20, 20), (24, 24, 100)]            # one tile row set; a ragged last tile; two samples per lane


@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("form", ["tile", "tile-attn", "tile_det", "tile_det-attn"])
@pytest.mark.parametrize("h,w,k", TILE_SHAPES, ids=["16x16-K16", "33x20-K20", "24x24-K100"])
def test_tile_forms_vs_float64_autograd(env, oracle_mod, h, w, k, form, loss):
    _lib, camera, ops = env
    case = _case(oracle_mod, camera, h, w, 256, k, True)
    _backward(ops, ops.LayerSpec(H=h, W=w, K=k), case, form, loss, 256)


@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("form", ["tile", "tile-attn"])
def test_tile_forms_softmax_off_vs_float64_autograd(env, oracle_mod, form, loss):
    """(the deterministic form refuses the soft-max off)"""
    _lib, camera, ops = env
    case = _case(oracle_mod, camera, 16, 16, 256, 16, False)
    _backward(ops, ops.LayerSpec(H=16, W=16, K=16, softmax_enabled=False), case, form, loss, 256)


@pytest.mark.parametrize("form", ["tile", "tile-attn", "tile_det"])
def test_deferred_tiles_vs_the_gather_form(env, form):
    """The second launch of a merged call (the list kernel): the epipole-inside rig at 64 x 64, K = 64, where
    tests/test_gpu_rigs.py asserts deferred tiles.  A float64 op-sequence reference costs several GB there; the gather form with the
    same grad_attn is within one tolerance of the truth by the small shapes above, and so is the tile form: 2 x TOL_GRAD_REL."""
    _lib, camera, ops = env
    h = k = 64
    f1, f2, cam, G, GA = _inputs(camera, "epipole_inside", h, h, 256, k, 764)
    ref, src, cam = ops.to_nhwc(f1.cuda()), ops.to_nhwc(f2.cuda()), cam.cuda()
    g, ga = ops.to_nhwc(G.cuda()), GA.cuda()
    spec = ops.LayerSpec(H=h, W=h, K=k)
    key = ("gather", h)
    if key not in _cache:
        _cache[key] = [t.permute(0, 3, 1, 2).cpu().numpy().astype(np.float64)
                       for t in ops.backward_nhwc(spec, ref, src, cam, g, form="gather", grad_attn=ga)]
        plain = ops.backward_nhwc(spec, ref, src, cam, g, form="gather")
        # (the attention term is not lost in the noise of the comparison below)
        assert float((plain[0].permute(0, 3, 1, 2).cpu() - torch.from_numpy(_cache[key][0])).abs().max()) > 10 * TOL_GRAD_REL * np.abs(_cache[key][0]).max()
    want = _cache[key]
    base = form.split("-")[0]
    attn = ops.forward_nhwc(spec, ref, src, cam)[1] if form.endswith("-attn") else None
    ws = ops.det_tile_workspace(spec, N, 256, ref.device) if base == "tile_det" else ops.tile_workspace(spec, N, 256, ref.device)
    gr, gs = ops.backward_nhwc(spec, ref, src, cam, g, form=base, attn=attn, workspace=ws, grad_attn=ga)
    torch.cuda.synchronize()
    hdr = ops.backward_deferred_tiles(ref.device, header=True, workspace=ws)
    # (the deterministic merged launch lists the tiles beyond the second launch's own capacity from the back, counted in word 2)
    assert hdr[0] + (hdr[2] if base == "tile_det" else 0) > 0, hdr
    assert int(hx.ws_header(ws)[1].item()) == 0
    _assert_close(form + " deferred grad_ref", gr, want[0], 2 * TOL_GRAD_REL)
    _assert_close(form + " deferred grad_src", gs, want[1], 2 * TOL_GRAD_REL)


# ---- the deterministic form: bits ---------------------------------------------------------------------------------------
def test_tile_det_same_bits_twice_on_a_second_stream_and_alone(env, oracle_mod):
    _lib, camera, ops = env
    h, w, k = 33, 20, 20
    case = _case(oracle_mod, camera, h, w, 256, k, True)
    ref, src, cam = ops.to_nhwc(case["f1"].cuda()), ops.to_nhwc(case["f2"].cuda()), case["cam"].cuda()
    g, ga = ops.to_nhwc(case["G"].cuda()), case["GA"].cuda()
    spec = ops.LayerSpec(H=h, W=w, K=k)
    ws = ops.det_tile_workspace(spec, N, 256, ref.device)
    first = ops.backward_nhwc(spec, ref, src, cam, g, form="tile_det", workspace=ws, grad_attn=ga)
    again = ops.backward_nhwc(spec, ref, src, cam, g, form="tile_det", workspace=ws, grad_attn=ga)
    assert hx.same_bits(first[0], again[0]) and hx.same_bits(first[1], again[1])
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    ws2 = ops.det_tile_workspace(spec, N, 256, ref.device)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        other = ops.backward_nhwc(spec, ref, src, cam, g, form="tile_det", workspace=ws2, grad_attn=ga)
    torch.cuda.synchronize()
    assert hx.same_bits(first[0], other[0]) and hx.same_bits(first[1], other[1])
    # pair 0 alone and inside the batch of two: the quantum (M_ga included) is per pair
    one = lambda t: t[:1].contiguous()
    alone = ops.backward_nhwc(spec, one(ref), one(src), one(cam), one(g), form="tile_det", grad_attn=one(ga))
    assert hx.same_bits(alone[0][0], first[0][0]) and hx.same_bits(alone[1][0], first[1][0])
    assert int(hx.ws_header(ws)[1].item()) == 0 and int(hx.ws_header(ws2)[1].item()) == 0


@pytest.mark.parametrize("with_attn", [False, True], ids=["recompute", "attn"])
def test_tile_det_without_grad_attn_is_the_old_entry_point_bit_for_bit(env, oracle_mod, with_attn):
    """The binding's path (et_epipolar_backward_tiled_det_ga with NULL) and a direct call of et_epipolar_backward_tiled_det give the
    same bits.  The old entry point forwards to the new one, so this pins the two exports to each other and the Python path to
    the C one; that the bits are those of the library before grad_attn existed was checked once, on one GPU, with both
    libraries side by side (profiles/attn_grad_bwd.txt, section 3)."""
    _lib, camera, ops = env
    h, w, k = 33, 20, 20
    case = _case(oracle_mod, camera, h, w, 256, k, True)
    ref, src, cam = ops.to_nhwc(case["f1"].cuda()), ops.to_nhwc(case["f2"].cuda()), case["cam"].cuda()
    g = ops.to_nhwc(case["G"].cuda())
    spec = ops.LayerSpec(H=h, W=w, K=k)
    attn = ops.forward_nhwc(spec, ref, src, cam)[1] if with_attn else None
    ws = ops.det_tile_workspace(spec, N, 256, ref.device)
    new = ops.backward_nhwc(spec, ref, src, cam, g, form="tile_det", attn=attn, workspace=ws, grad_attn=None)
    xs, ys, steps = spec.constants(ref.device)
    gr, gs = torch.full_like(ref, float("nan")), torch.full_like(src, float("nan"))
    import ctypes
    hx.call("et_epipolar_backward_tiled_det", spec.desc(N, 256), xs, ys, steps, cam, ref, src, attn, g, gr, gs, ws, ctypes.c_size_t(ws.numel()))
    torch.cuda.synchronize()
    assert hx.same_bits(new[0], gr) and hx.same_bits(new[1], gs)


# ---- the general op (option branches) against the module's torch restatement in float64 -----------------------------------
GENERAL = ["prior_add_c8_k8", "prior_mul_c8_k8", "cosine_c8_k8", "param_pool_c16_k16", "similarity_prior_c8_k8", "attention_max_c8_k8"]


def _mode_module(d):
    """The module of a mode fixture (tests/golden/modes): its configuration, the reference's weights and prior tables, and the
    camera algebra the reference computed for it."""
    from epipolar_transformers_amd import default_cfg
    from epipolar_transformers_amd.epipolar import Epipolar

    H, C, K, _, image = [int(v) for v in d["meta"]]
    cfg = default_cfg()
    cfg.merge_from_list(["KEYPOINT.HEATMAP_SIZE", (H, H), "KEYPOINT.NFEATS", C, "EPIPOLAR.SAMPLESIZE", K,
                         "DATASETS.IMAGE_SIZE", (image, image), "EPIPOLAR.USE_CORRECT_NORMALIZE", True,
                         "EPIPOLAR.ATTENTION", "avg", "EPIPOLAR.PARAMETERIZED", ("z",), "EPIPOLAR.ZRESIDUAL", True,
                         "EPIPOLAR.MERGE", "late", "EPIPOLAR.SHARE_WEIGHTS", True] +
                        [str(v) for v in d["overrides"]])     # (the case's own overrides last: they win)
    mod = Epipolar(cfg=cfg).cuda().eval()
    sd = {k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd.")}
    assert sorted(mod.state_dict()) == sorted(sd)
    mod.load_state_dict(sd)
    for k in d.files:
        if k.startswith("prior."):
            _, i, j = k.split(".")
            with torch.no_grad():
                mod.prior[(int(i), int(j))] = torch.nn.Parameter(torch.from_numpy(d[k]).cuda())
    cam = torch.from_numpy(d["cam"]).cuda()
    mod._cams.get = lambda *a, **kw: cam
    return mod


def _all_masked_pixels(mod, d):
    """(N,H,W) mask of the pixels whose similarities are all masked, found with the restatement itself, prior off: soft-max of
    equal logits = 1 / K'; and the fixture's camera pairs, the keys of the prior tables."""
    from epipolar_transformers_amd.epipolar import EpipolarSlowPathWarning

    P1, P2 = torch.from_numpy(d["P1"]), torch.from_numpy(d["P2"])
    cams = torch.from_numpy(d["camera"]), torch.from_numpy(d["other_camera"])
    probe = copy.deepcopy(mod).double()
    probe.cfg.merge_from_list(["EPIPOLAR_AMD.GENERAL_KERNEL", False, "EPIPOLAR.PRIOR", False])
    probe_sample = probe._sample_torch
    probe._sample_torch = lambda src, locs: probe_sample(src, locs.to(src.dtype))
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore", EpipolarSlowPathWarning)
        a0 = probe._attend_general(torch.from_numpy(d["feat1"]).cuda().double(), torch.from_numpy(d["feat2"]).cuda().double(),
                                   P1, P2, *cams)[1]
    all_masked = (a0 == 1.0 / a0.shape[1]).all(1)                                  # (N,H,W)
    zero_rows = torch.from_numpy((d["feat1"] == 0).all(1)).cuda()
    pairs = [(int(a), int(b)) for a, b in zip(d["camera"], d["other_camera"])]
    assert zero_rows.any() and (all_masked | ~zero_rows).all() and len(set(pairs)) == len(pairs)
    return all_masked, pairs


@pytest.mark.parametrize("name", GENERAL)
def test_general_op_vs_the_float64_restatement(name):
    from epipolar_transformers_amd.epipolar import EpipolarSlowPathWarning

    d = np.load(os.path.join(GOLDEN_DIR, "modes", name + ".npz"))
    mod = _mode_module(d)
    P1, P2 = torch.from_numpy(d["P1"]), torch.from_numpy(d["P2"])
    cams = torch.from_numpy(d["camera"]), torch.from_numpy(d["other_camera"])
    if name.startswith("prior_add"):
        # A pixel whose similarities are ALL masked (an all-zero reference row, or no sample inside the image) has the logits
        # -1e10 + prior.  In float32 -- the arithmetic of the reference and of the kernel -- that sum IS -1e10 (uniform attention);
        # in float64 it keeps the prior, and the restatement would not be the reference there (measured: its own float32 run
        # differs from its float64 run by 8.6e-4 in the attention of those pixels, 4.8e-4 of the largest d feat2, 1.6e-3 of the
        # largest d prior).  With prior 0 at those pixels both sums are -1e10 exactly; the pixels stay all-masked and their prior
        # entries keep their gradient.  (The prior as the fixture has it at those pixels: the test below.)
        all_masked, pairs = _all_masked_pixels(mod, d)
        with torch.no_grad():
            for n, key in enumerate(pairs):
                mod.prior[key][:, all_masked[n]] = 0
    want_mod = copy.deepcopy(mod).double()
    for m, extra in ((mod, ["EPIPOLAR_AMD.ATTN_GRAD", True]), (want_mod, ["EPIPOLAR_AMD.GENERAL_KERNEL", False])):
        m.cfg.defrost() if hasattr(m.cfg, "defrost") else None
        m.cfg.merge_from_list(extra)
    sample = want_mod._sample_torch
    want_mod._sample_torch = lambda src, locs: sample(src, locs.to(src.dtype))      # (grid_sample wants one dtype)
    is_max = name.startswith("attention_max")
    res = []
    for m, dt in ((mod, torch.float32), (want_mod, torch.float64)):
        f1 = torch.from_numpy(d["feat1"]).cuda().to(dt).requires_grad_(True)
        f2 = torch.from_numpy(d["feat2"]).cuda().to(dt).requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", EpipolarSlowPathWarning)
            assert m._general_kernel_applies(f1, f2, None, None, *cams) == (m is mod)
            out, attn, _ = m._attend_general(f1, f2, P1, P2, *cams)
        assert attn.requires_grad
        if m is mod:
            gen = torch.Generator().manual_seed(31)
            G, GA = torch.randn(out.shape, generator=gen).cuda(), torch.randn(attn.shape, generator=gen).cuda()
        # ATTENTION max: `out` is the arg-max sample (ties are test_gpu_modes' business) -- the attention term alone, which
        # must reach q and the similarity map through the cosine
        loss = (attn * GA.to(dt)).sum() if is_max else (out * G.to(dt)).sum() + (attn * GA.to(dt)).sum()
        loss.backward()
        grads = {"feat1": f1.grad, "feat2": f2.grad}
        grads.update({"prior%s" % (key,): p.grad for key, p in m.prior.items()})
        res.append({k: (None if v is None else v.detach().double().cpu().numpy()) for k, v in grads.items()})
    got, want = res
    checked = 0
    for key, w_ in want.items():
        if w_ is None:
            assert got[key] is None or not np.abs(got[key]).max() > 0, key
            continue
        g_ = np.zeros_like(w_) if got[key] is None else got[key]
        scale = max(float(np.abs(w_).max()), 1e-30)
        err = float(np.abs(g_ - w_).max())
        print("%s %s: max error %.3g of %.3g" % (name, key, err, scale))
        assert np.isfinite(g_).all() and err <= TOL_GRAD_REL * scale, (name, key, err, scale)
        checked += scale > 1e-20
    assert checked >= (2 if not name.startswith("similarity_prior") else 1)
    if is_max:
        assert np.abs(got["feat1"]).max() > 0 and np.abs(got["feat2"]).max() > 0       # grad_q and grad_map_sim from GA alone
    if "prior" in name:
        assert any(k.startswith("prior") and v is not None and np.abs(v).max() > 0 for k, v in got.items()), "grad_prior"


def test_prior_add_with_the_fixtures_prior_at_all_masked_pixels():
    """PRIOR add with the prior as the fixture has it, non-zero at the all-masked pixels too, which the float64 comparison above
    cannot have.  There every logit is -1e10 + prior in float32, and that IS -1e10 while |prior| < 512 (half a unit in the last
    place of 1e10, which is 1024): each float32 operation of the kernel sees the operands it sees with prior 0 at those pixels,
    so all gradients of (out . G).sum() + (attn . GA).sum() agree between the two priors up to the order of the float sums --
    bounded with the project's gradient tolerance -- and the prior entries of those pixels get their gradient from GA."""
    name = "prior_add_c8_k8"
    d = np.load(os.path.join(GOLDEN_DIR, "modes", name + ".npz"))
    P1, P2 = torch.from_numpy(d["P1"]), torch.from_numpy(d["P2"])
    cams = torch.from_numpy(d["camera"]), torch.from_numpy(d["other_camera"])
    res = []
    for zeroed in (False, True):
        mod = _mode_module(d)
        all_masked, pairs = _all_masked_pixels(mod, d)
        at_masked = torch.cat([mod.prior[key][:, all_masked[n]].detach().abs().flatten() for n, key in enumerate(pairs)])
        assert at_masked.numel() > 0 and 0 < float(at_masked.max()) < 512
        if zeroed:
            with torch.no_grad():
                for n, key in enumerate(pairs):
                    mod.prior[key][:, all_masked[n]] = 0
        mod.cfg.merge_from_list(["EPIPOLAR_AMD.ATTN_GRAD", True])
        f1 = torch.from_numpy(d["feat1"]).cuda().requires_grad_(True)
        f2 = torch.from_numpy(d["feat2"]).cuda().requires_grad_(True)
        assert mod._general_kernel_applies(f1, f2, None, None, *cams)
        out, attn, _ = mod._attend_general(f1, f2, P1, P2, *cams)
        gen = torch.Generator().manual_seed(31)
        G, GA = torch.randn(out.shape, generator=gen).cuda(), torch.randn(attn.shape, generator=gen).cuda()
        ((out * G).sum() + (attn * GA).sum()).backward()
        grads = {"feat1": f1.grad, "feat2": f2.grad}
        grads.update({"prior%s" % (key,): mod.prior[key].grad for key in pairs})
        res.append({k: v.detach().double().cpu().numpy() for k, v in grads.items()})
        masked_prior_grad = max(float(mod.prior[key].grad[:, all_masked[n]].abs().max()) for n, key in enumerate(pairs))
        assert masked_prior_grad > 0, "grad_prior at the all-masked pixels"
    got, want = res
    for key, w_ in want.items():
        scale = max(float(np.abs(w_).max()), 1e-30)
        err = float(np.abs(got[key] - w_).max())
        print("%s %s, the fixture's prior against prior 0 at all-masked pixels: max difference %.3g of %.3g" % (name, key, err, scale))
        assert np.isfinite(got[key]).all() and err <= TOL_GRAD_REL * scale, (key, err, scale)


# ---- the module ---------------------------------------------------------------------------------------------------------
def _layer(cam, h, c, k, attn_grad):
    from epipolar_transformers_amd import default_cfg
    from epipolar_transformers_amd.epipolar import Epipolar

    cfg = default_cfg()
    cfg.merge_from_list(["KEYPOINT.HEATMAP_SIZE", (h, h), "KEYPOINT.NFEATS", c, "EPIPOLAR.SAMPLESIZE", k, "EPIPOLAR.ATTENTION", "avg",
                         "EPIPOLAR.PARAMETERIZED", ("z",), "EPIPOLAR.ZRESIDUAL", True, "EPIPOLAR.USE_CORRECT_NORMALIZE", True] +
                        (["EPIPOLAR_AMD.ATTN_GRAD", True] if attn_grad else []))
    mod = Epipolar(cfg=cfg).cuda()
    mod._cams.get = lambda *a, **kw: cam
    return mod


def test_module_depth_carries_gradient_with_the_knob(env, oracle_mod):
    _lib, camera, ops = env
    h, c, k = 10, 8, 16
    case = _case(oracle_mod, camera, h, h, c, k, True)
    mod = _layer(case["cam"].cuda(), h, c, k, True)
    f1, f2 = case["f1"].cuda().requires_grad_(True), case["f2"].cuda().requires_grad_(True)
    P = torch.zeros(N, 3, 4)
    _, _, depth, _ = mod(f1, f2, P, P)
    assert depth.requires_grad
    (depth * case["GA"].cuda()).sum().backward()
    for what, got, want in (("feat1.grad", f1.grad, case["d_att"][0]), ("feat2.grad", f2.grad, case["d_att"][1])):
        _assert_close("module " + what, got.permute(0, 2, 3, 1), want)


def _attend_and_backpropagate_out(case, h, c, k, knob):
    mod = _layer(case["cam"].cuda(), h, c, k, knob)
    f1, f2 = case["f1"].cuda().requires_grad_(True), case["f2"].cuda().requires_grad_(True)
    P = torch.zeros(N, 3, 4)
    out, depth, _ = mod.attend(f1, f2, P, P)
    assert depth.requires_grad == knob
    if not knob:
        depth.cpu().numpy()         # (what existing callers do with that return, autograd on)
    (out * case["G"].cuda()).sum().backward()
    return f1.grad, f2.grad


def test_module_default_depth_has_no_gradient(env, oracle_mod):
    """The default (no knob set): `depth` is detached, a loss on `out` gives the gradients of the backward without grad_attn."""
    _lib, camera, ops = env
    h, c, k = 10, 8, 16
    case = _case(oracle_mod, camera, h, h, c, k, True)
    g1, g2 = _attend_and_backpropagate_out(case, h, c, k, False)
    _assert_close("default knob feat1.grad", g1.permute(0, 2, 3, 1), case["d_out"][0])
    _assert_close("default knob feat2.grad", g2.permute(0, 2, 3, 1), case["d_out"][1])
    # C = 8: the gather form, bit-reproducible
    spec = ops.LayerSpec(H=h, W=h, K=k)
    gr, gs = ops.backward_nhwc(spec, ops.to_nhwc(case["f1"].cuda()), ops.to_nhwc(case["f2"].cuda()), case["cam"].cuda(),
                               ops.to_nhwc(case["G"].cuda()))
    assert hx.same_bits(g1.permute(0, 2, 3, 1), gr) and hx.same_bits(g2.permute(0, 2, 3, 1), gs)


def test_module_knob_leaves_a_loss_on_out_bit_for_bit(env, oracle_mod):
    """With the knob and a loss on `out` alone the attention's gradient arrives as None: the backward without it, same bits."""
    _lib, camera, ops = env
    h, c, k = 10, 8, 16
    case = _case(oracle_mod, camera, h, h, c, k, True)
    off = _attend_and_backpropagate_out(case, h, c, k, False)
    on = _attend_and_backpropagate_out(case, h, c, k, True)
    assert hx.same_bits(off[0], on[0]) and hx.same_bits(off[1], on[1])
