"""Non-finite feature maps, incoming gradients and prior tables through the HIP kernels, against what the REAL reference returned
for them (tests/golden/nonfinite/, made by tests/golden/make_nonfinite_golden.py; read by tests/nonfinite_fixture.py).

One value of pair 1 of 3 is NaN, +Inf or -Inf.  Every route is held to the rule of include/epipolar_amd.h ("Non-finite values"):
  R1 never lost   where the reference's result is non-finite, ours is -- of the same kind (NaN, +Inf, -Inf) on the per-pixel routes;
                  on the matrix-core routes the finiteness mask alone (a split-fp16 product turns Inf into NaN);
  R2 confined     where the reference's result is finite, ours is finite and within the suite's tolerances on finite inputs
                  (TOL_ATTN, TOL_OUT, TOL_GRAD_REL of tests/test_gpu_parity.py; the bound of test_residual_gemm_abi for x);
  R3 arg-max      corr_pos is the reference's at every pixel, under conftest.assert_corr_pos's tie rule and nothing looser;
  R4 pair         pairs 0 and 2 return the bits of the same call with finite inputs (forward routes, gather backward; the atomic
                  backward and the general kernels' atomic map gradients within TOL_GRAD_REL), no error bit in the workspace's
                  sticky word, and their tiles on the overflow list are the same.
Outputs start as NaN under test (ops.POISON_OUTPUTS), so confinement cannot be read off an output alone: every check of R4
compares with the finite call.  The routes are forced by `variant` as in tests/test_gpu_rigs.py / tests/test_gpu_limits.py.

The tiled backward forms ("tile", "tile_det") keep R1 and R4 and, in place of R2, the documented spread: entries of the value's
own pair only ("Non-finite values"; test_backward_tiled)."""
import numpy as np
import pytest
import torch

import nonfinite_fixture as nf

pytestmark = pytest.mark.gpu

TOL_ATTN, TOL_OUT, TOL_GRAD_REL = 1e-5, 1e-4, 1e-4          # tests/test_gpu_parity.py
RTOL = 2e-6                                                 # ... and the relative term of its _close() (forward outputs)
N = 3
OTHERS = [0, 2]

NO_TILE, TILE_SPLIT, TILE_CLASSIC, TILE_EXACT, WS_BAND = 16384, 32768, 65536, 524288, 1048576
# name -> (variant, per-pixel route: the kind of a non-finite value must match)
TILE_ROUTES = {"persistent": 0, "persistent-band": WS_BAND, "block-per-tile": TILE_CLASSIC, "block-per-tile-exact": TILE_CLASSIC | TILE_EXACT}
# row-set capacity 64 on the 16 x 16 head (tests/test_gpu_fused.py's overflow shape): the tiles ALSO overflow their arrays and are split / listed for that
# reason -- asserted on the finite call (_finite_forward)
CAP64_ROUTES = {"persistent-cap64": TILE_SPLIT, "block-per-tile-cap64": TILE_CLASSIC | TILE_SPLIT}

PIXEL = nf.all_cases("pixel_")
HEAD = nf.all_cases("head_")
HEAD16 = nf.all_cases("head_10x10_c256_k16")
HEAD12 = nf.all_cases("cap_16x16_c256_k16")
MODES = nf.all_cases("mode_")
fwd_only = lambda cs: [c for c in cs if not c[1].startswith("gout_")]
_ids = lambda cs: ["%s-%s" % c for c in cs]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from epipolar_transformers_amd import _lib, ops

    _lib.load()
    assert ops.POISON_OUTPUTS
    return _lib, ops


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # (a copy: the fixture arrays are read-only)


def _spec(ops, d, variant):
    m = d["dims"]
    return ops.LayerSpec(H=m["H"], W=m["W"], K=m["K"], downsample=float(d["downsample"]), correct_normalize=m["correct"],
                         softmax_scale=float(d["softmax_scale"]), softmax_enabled=m["softmax"], variant=variant)


def _nchw(t):
    return t.permute(0, 3, 1, 2).cpu().numpy()


_locs = {}


def _sample_locs(ops, name, d, spec):
    if name not in _locs:
        _locs[name] = ops.sample_locs(spec, _dev(d["cam"])).cpu().numpy()
        assert np.array_equal(_locs[name][:, nf.POISONED], d["sample_locs1"])            # bit-equal to the reference's
    return _locs[name]


def _overflow_tiles(ops, spec, d, ws):
    """the tile ids on the workspace's overflow list (a set: the order is that of the blocks' atomics)"""
    import ctypes
    from epipolar_transformers_amd import _lib
    m = d["dims"]
    base = (-ws.data_ptr()) % 256
    count = int(ws[base:base + 4].view(torch.int32).item())
    tiles = N * ((m["H"] * m["W"] + 31) // 32)
    desc = spec.desc(N, m["C"])
    stats_off = base + int(_lib.load().et_epipolar_forward_workspace_stats_offset(ctypes.byref(desc)))
    lst = ws[stats_off - 4 * tiles: stats_off].view(torch.int32)[:count].tolist()
    assert len(set(lst)) == len(lst) and all(0 <= t < tiles for t in lst)
    return set(lst), tiles // N


def _tile_of_pixel(ops, spec, d, ws):
    """(H*W,) tile index of every reference pixel of pair 1, from the pixel order in front of the overflow list"""
    import ctypes
    from epipolar_transformers_amd import _lib
    m = d["dims"]
    base = (-ws.data_ptr()) % 256
    tiles = N * ((m["H"] * m["W"] + 31) // 32)
    desc = spec.desc(N, m["C"])
    list_off = base + int(_lib.load().et_epipolar_forward_workspace_stats_offset(ctypes.byref(desc))) - 4 * tiles
    perm = ws[list_off - 4 * 32 * tiles: list_off].view(torch.int32).view(tiles, 32).cpu().numpy()
    tpp = tiles // N
    tile = np.full(m["H"] * m["W"], -1)
    for t in range(nf.POISONED * tpp, (nf.POISONED + 1) * tpp):
        pix = perm[t][perm[t] >= 0]
        tile[pix] = t
    assert (tile >= 0).all()
    return tile


_CAP64_HITS = {}


def _over_capacity_holds_value(d, case, r, strict=False):
    """capacity 64: some pixel the case touches lies in a tile that is over capacity in the FINITE call `r` (split into pixel
    groups by the one-block-per-tile kernel, or on the persistent kernel's overflow list)"""
    touched = np.unpackbits(d[case + ".out.touched"])[: r["tile"].size].astype(bool)
    if not touched.any():
        return not strict                            # (a corner site no line taps: there is no poisoned tile)
    over = r["ovf"] | {t for t, st in enumerate(r["stats"]) if (st >> 16) > 1}
    return any(int(t) in over for t in r["tile"][touched])


def _forward(ops, spec, d, f1, f2, stream=None):
    ref, src, cam = ops.to_nhwc(_dev(f1)), ops.to_nhwc(_dev(f2)), _dev(d["cam"])
    ws = ops.tile_workspace(spec, N, d["dims"]["C"], ref.device) if not (spec.variant & NO_TILE) else None
    if ws is not None and ws.numel() == 0:
        ws = None
    out, attn, corr = ops.forward_nhwc(spec, ref, src, cam, workspace=ws)        # (raises if the sticky error word is set)
    torch.cuda.synchronize()
    r = dict(out=_nchw(out), attn=attn.cpu().numpy(), corr=corr.cpu().numpy())
    if ws is not None:
        r["ovf"], r["tpp"] = _overflow_tiles(ops, spec, d, ws)
        r["stats"] = ops.tile_stats(spec, N, d["dims"]["C"], ws).tolist()
        r["tile"] = _tile_of_pixel(ops, spec, d, ws)
    return r


_finite = {}


def _finite_forward(ops, name, route, spec, d):
    key = (name, route)
    if key not in _finite:
        r = _finite[key] = _forward(ops, spec, d, d["feat1"], d["feat2"])
        assert all(np.isfinite(r[o]).all() for o in ("out", "attn", "corr"))
        # the finite call itself against the reference's finite run (pair 1)
        nf.check_values(r["attn"][nf.POISONED], d["attn1"], TOL_ATTN, True, "attn (finite call)", RTOL)
        nf.check_values(r["out"][nf.POISONED], d["out1"], TOL_OUT, True, "out (finite call)", RTOL)
    return _finite[key]


def _check_forward(ops, name, case, route, variant, kinds):
    d = nf.load(name)
    spec = _spec(ops, d, variant)
    base = _finite_forward(ops, name, route, spec, d)
    f1, f2, _, _ = nf.poisoned_inputs(d, case)
    r = _forward(ops, spec, d, f1, f2)
    n = nf.POISONED
    ea = nf.check_values(r["attn"][n], nf.expected(d, case, "attn"), TOL_ATTN, kinds, "attn", RTOL)
    eo = nf.check_values(r["out"][n], nf.expected(d, case, "out"), TOL_OUT, kinds, "out", RTOL)
    print("%s %s %s: max error over the finite entries attn %.3g out %.3g" % (name, case, route, ea, eo))
    nf.check_corr_pos(d, case, _sample_locs(ops, name, d, spec), r["corr"], r["attn"])
    for o in ("out", "attn", "corr"):                                                   # R4
        for m in OTHERS:
            assert np.array_equal(r[o][m].view(np.uint32), base[o][m].view(np.uint32)), "R4 -- %s of pair %d changed" % (o, m)
    if "ovf" in r:
        others = lambda s: {t for t in s if t // r["tpp"] != n}
        assert others(r["ovf"]) == others(base["ovf"]), "R4 -- the overflow list of the finite pairs changed"
    return r


@pytest.mark.parametrize("name,case", fwd_only(PIXEL + HEAD), ids=_ids(fwd_only(PIXEL + HEAD)))
def test_forward_per_pixel(env, name, case):
    """epipolar_fwd_kernel (C = 8, soft-max on and off) and the four-pixels-per-wave / two-slot instances of the 256-channel head"""
    _check_forward(env[1], name, case, "per-pixel", NO_TILE, kinds=True)


@pytest.mark.parametrize("route", list(TILE_ROUTES))
@pytest.mark.parametrize("name,case", fwd_only(HEAD), ids=_ids(fwd_only(HEAD)))
def test_forward_tile_routes(env, name, case, route):
    """the persistent kernel (both instances; K = 101: both halves of the two-pass soft-max), one block per tile in split fp16 and
    in exact fp32, and each with the row-set capacity of 64 that also sends the poisoned tile down the splitting path"""
    _check_forward(env[1], name, case, route, TILE_ROUTES[route], kinds=False)


@pytest.mark.parametrize("route", list(CAP64_ROUTES))
@pytest.mark.parametrize("name,case", fwd_only(HEAD12), ids=_ids(fwd_only(HEAD12)))
def test_forward_tile_routes_capacity_64(env, name, case, route):
    """the same with tiles that are over capacity as well (which cases put their value into such a tile: the next test)"""
    _check_forward(env[1], name, case, route, CAP64_ROUTES[route], kinds=False)


@pytest.mark.parametrize("route", list(CAP64_ROUTES) + ["fused"])
def test_capacity_64_holds_a_poisoned_tile(env, route):
    """On every capacity-64 route at least one case has its value in a tile that is over capacity in the finite call too: split
    into pixel groups by the one-block-per-tile kernel, or on the overflow list of the persistent / fused kernel.  (The sites
    follow the reference's rule, not the tiling: not every case can.)"""
    _lib, ops = env
    name = "cap_16x16_c256_k16"
    d = nf.load(name)
    if route == "fused":
        for n_, c_ in fwd_only(HEAD12):
            if not _CAP64_HITS.get("fused"):
                test_fused_layer(env, n_, c_, TILE_SPLIT)
        hits = _CAP64_HITS.get("fused", set())
    else:
        base = _finite_forward(ops, name, route, _spec(ops, d, CAP64_ROUTES[route]), d)
        hits = {c for _, c in fwd_only(HEAD12) if _over_capacity_holds_value(d, c, base, strict=True)}
    print("capacity 64, %s: value in an over-capacity tile in %s" % (route, sorted(hits)))
    assert hits


def test_forward_side_stream_own_workspace(env):
    """the persistent route on a side stream with a caller-owned workspace: same bits as on the default stream"""
    _lib, ops = env
    name, case = "head_10x10_c256_k16", "src_one.nan"
    d = nf.load(name)
    spec = _spec(ops, d, 0)
    f1, f2, _, _ = nf.poisoned_inputs(d, case)
    want = _forward(ops, spec, d, f1, f2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = _forward(ops, spec, d, f1, f2)
    s.synchronize()
    for o in ("out", "attn", "corr"):
        assert np.array_equal(got[o], want[o], equal_nan=True), o
    assert got["ovf"] == want["ovf"]


# ---- the fused layer, et_residual_gemm, et_residual_epilogue: x = feat + bn(z(out)) + out ------------------------------------------
def _folded(d):
    C = d["dims"]["C"]
    if "z_weight" not in d:         # a fixture without the z branch: a seeded folded weight, as tests/test_gpu_fused.py draws it
        g = torch.Generator().manual_seed(12)
        return (torch.randn(C, C, generator=g) * 0.05 + torch.eye(C)).cuda(), torch.randn(C, generator=g).cuda()
    zw, zb = torch.from_numpy(np.array(d["z_weight"])).view(C, C), torch.from_numpy(np.array(d["z_bias"]))
    gamma, beta = torch.from_numpy(np.array(d["bn_weight"])), torch.from_numpy(np.array(d["bn_bias"]))
    mean, var = torch.from_numpy(np.array(d["bn_running_mean"])), torch.from_numpy(np.array(d["bn_running_var"]))
    s = gamma / torch.sqrt(var + 1e-5)
    return (zw * s[:, None] + torch.eye(C)).cuda(), (zb * s + beta - mean * s).cuda()


def _x_float64(out, feat, wf, bias):
    """x = feat + bias + out . Wf^T in float64 (NaN / Inf as IEEE arithmetic has them: a row of `out` that holds one gives a
    non-finite row)"""
    C = out.shape[0]
    o = out.reshape(C, -1).T.astype(np.float64)
    with np.errstate(all="ignore"):
        x = o @ wf.cpu().numpy().astype(np.float64).T + bias.cpu().numpy().astype(np.float64) + feat.reshape(C, -1).T.astype(np.float64)
        x[~np.isfinite(o).all(1)] = np.nan           # (the matrix product of a library may skip zeros: say it explicitly)
    return x.T.reshape(out.shape)


def _check_x(d, case, x, wf, f1, bias=None):
    """R1 / R2 of x = finalout + feat of pair 1 (finiteness mask: a matrix-core route) under test_residual_gemm_abi's bound"""
    n = nf.POISONED
    with np.errstate(invalid="ignore"):
        if "finalout1" in d:
            want = nf.expected(d, case, "finalout") + f1[n]                           # resnet.py:388: one float32 add
        else:
            want = _x_float64(nf.expected(d, case, "out"), f1[n], wf, bias)
    out = np.nan_to_num(nf.expected(d, case, "out"), nan=0.0, posinf=0.0, neginf=0.0)   # (only rows the reference keeps finite count)
    C = out.shape[0]
    mag = np.abs(out).reshape(C, -1).T.astype(np.float64) @ np.abs(wf.cpu().numpy().astype(np.float64)).T      # (HW,C)
    bound = 4e-6 * mag.T.reshape(want.shape) + 3e-7 * (np.abs(np.nan_to_num(want, nan=0.0, posinf=0.0, neginf=0.0)) + 1)
    fin = np.isfinite(want)
    nf.check_values(x, want, np.inf, kinds=False, what="x")
    ratio = float((np.abs(x[fin] - want[fin]) / bound[fin]).max())
    assert ratio <= 1.0, "x: R2 -- error / bound = %g" % ratio
    return ratio


@pytest.mark.parametrize("name,case,variant", [(n, c, 0) for n, c in fwd_only(HEAD16)] + [(n, c, TILE_SPLIT) for n, c in fwd_only(HEAD12)],
                         ids=_ids(fwd_only(HEAD16)) + [i + "-cap64" for i in _ids(fwd_only(HEAD12))])
def test_fused_layer(env, name, case, variant):
    """et_epipolar_forward_fused and its overflow follow-up (the poisoned tile always goes that way: the fp16 guard lists it)"""
    _lib, ops = env
    d = nf.load(name)
    spec = _spec(ops, d, variant)
    assert ops.fused_layer_applies(spec, 256, N)
    wf, bias = _folded(d)
    packed = ops.residual_gemm_pack(wf)
    cam = _dev(d["cam"])

    def run(f1, f2):
        ref, src = ops.to_nhwc(_dev(f1)), ops.to_nhwc(_dev(f2))
        ws = ops.tile_workspace(spec, N, 256, ref.device)
        x, attn, corr, out = ops.forward_fused_nhwc(spec, ref, src, cam, packed, bias, want_out=True, workspace=ws)
        torch.cuda.synchronize()
        ovf, tpp = _overflow_tiles(ops, spec, d, ws)
        return dict(x=_nchw(x), out=_nchw(out), attn=attn.cpu().numpy(), corr=corr.cpu().numpy(), ovf=ovf, tpp=tpp,
                    stats=[], tile=_tile_of_pixel(ops, spec, d, ws))

    key = (name, "fused", variant)
    if key not in _finite:
        b = _finite[key] = run(d["feat1"], d["feat2"])
        # the finite call itself against the reference's finite run (pair 1)
        nf.check_values(b["attn"][nf.POISONED], d["attn1"], TOL_ATTN, True, "attn (finite call)", RTOL)
        nf.check_values(b["out"][nf.POISONED], d["out1"], TOL_OUT, True, "out (finite call)", RTOL)
        xb = b["x"][nf.POISONED]
        xw = d["finalout1"] + d["feat1"][nf.POISONED] if "finalout1" in d else _x_float64(d["out1"], d["feat1"][nf.POISONED], wf, bias)
        mag = np.abs(d["out1"]).reshape(256, -1).T.astype(np.float64) @ np.abs(wf.cpu().numpy().astype(np.float64)).T
        bound = 4e-6 * mag.T.reshape(xw.shape) + 3e-7 * (np.abs(xw) + 1)
        assert np.isfinite(xb).all() and (np.abs(xb - xw) <= bound).all(), float((np.abs(xb - xw) / bound).max())
    base = _finite[key]
    if variant:
        _CAP64_HITS.setdefault("fused", set()).update([case] if _over_capacity_holds_value(d, case, base, strict=True) else [])
    f1, f2, _, _ = nf.poisoned_inputs(d, case)
    r = run(f1, f2)
    n = nf.POISONED
    nf.check_values(r["attn"][n], nf.expected(d, case, "attn"), TOL_ATTN, False, "attn")
    nf.check_values(r["out"][n], nf.expected(d, case, "out"), TOL_OUT, False, "out")
    _check_x(d, case, r["x"][n], wf, f1, bias)
    nf.check_corr_pos(d, case, _sample_locs(ops, name, d, spec), r["corr"], r["attn"])
    for o in ("x", "out", "attn", "corr"):
        for m in OTHERS:
            assert np.array_equal(r[o][m].view(np.uint32), base[o][m].view(np.uint32)), "R4 -- %s of pair %d changed" % (o, m)
    others = lambda s: {t for t in s if t // r["tpp"] != n}
    assert others(r["ovf"]) == others(base["ovf"])
    assert any(t // r["tpp"] == n for t in r["ovf"]), "the poisoned tile was meant to reach the overflow follow-up"


@pytest.mark.parametrize("name,case", fwd_only(HEAD16), ids=_ids(fwd_only(HEAD16)))
def test_residual_gemm_and_epilogue(env, name, case):
    """et_residual_gemm / et_residual_epilogue on the reference's own (poisoned) `out`: a row with a non-finite value gives a
    non-finite x row, every other row -- the rows of its 32-row MFMA block included -- stays finite and within the bound"""
    _lib, ops = env
    d = nf.load(name)
    wf, bias = _folded(d)
    f1, _, _, _ = nf.poisoned_inputs(d, case)
    C, H, W = d["out1"].shape
    out = np.stack([d["out1"], nf.expected(d, case, "out"), d["out1"]])               # pairs 0 / 2: finite rows around it
    rows = lambda a: _dev(np.ascontiguousarray(a.transpose(0, 2, 3, 1)).reshape(-1, C))
    feat = np.stack([f1[nf.POISONED]] * 3)
    out_d, feat_d = rows(out), rows(feat)
    x = ops.residual_gemm(out_d, ops.residual_gemm_pack(wf), bias, feat_d)
    x = x.view(3, H, W, C).permute(0, 3, 1, 2).cpu().numpy()
    _check_x(d, case, x[1], wf, f1)
    finite = ops.residual_gemm(rows(np.stack([d["out1"]] * 3)), ops.residual_gemm_pack(wf), bias, feat_d).view(3, H, W, C).permute(0, 3, 1, 2).cpu().numpy()
    if np.isfinite(feat).all():
        assert np.array_equal(x[0], finite[0]) and np.array_equal(x[2], finite[2]), "R4 -- rows of the finite blocks changed"
    # the epilogue kernel: finalout = out + y * scale + shift, x = feat + finalout, element by element
    y = out_d * 0.5
    scale, shift = torch.full((C,), 0.25, device="cuda"), torch.full((C,), 0.125, device="cuda")
    fin, xe = ops.residual_epilogue(feat_d, out_d.view(3, H, W, C), y, scale, shift)
    with np.errstate(invalid="ignore"):
        o = out_d.cpu().numpy()
        want_fin = o + (o * 0.5) * 0.25 + 0.125
        want_x = feat_d.cpu().numpy() + want_fin
    nf.check_values(fin.cpu().numpy().reshape(-1, C), want_fin, 1e-5, True, "finalout (epilogue)")
    nf.check_values(xe.cpu().numpy().reshape(-1, C), want_x, 1e-5, True, "x (epilogue)")


# ---- backward: the gather and atomic forms --------------------------------------------------------------------------------
_finite_bwd, _poisoned_bwd = {}, {}


@pytest.mark.parametrize("form", ["gather", "atomic"])
@pytest.mark.parametrize("name,case", PIXEL + HEAD, ids=_ids(PIXEL + HEAD))
def test_backward_gather_atomic(env, name, case, form):
    _lib, ops = env
    d = nf.load(name)
    spec = _spec(ops, d, NO_TILE)
    cam = _dev(d["cam"])

    def run(f1, f2, g):
        gr, gs = ops.backward_nhwc(spec, ops.to_nhwc(_dev(f1)), ops.to_nhwc(_dev(f2)), cam, ops.to_nhwc(_dev(g)), form=form)
        torch.cuda.synchronize()
        return dict(grad_feat1=_nchw(gr), grad_feat2=_nchw(gs))

    key = (name, form)
    if key not in _finite_bwd:
        _finite_bwd[key] = run(d["feat1"], d["feat2"], d["grad_out"])
    base = _finite_bwd[key]
    f1, f2, g, _ = nf.poisoned_inputs(d, case)
    r = _poisoned_bwd[(name, case, form)] = run(f1, f2, g)
    for o in ("grad_feat1", "grad_feat2"):
        scale = float(np.abs(d[o + "1"]).max())
        err = nf.check_values(r[o][nf.POISONED], nf.expected(d, case, o), TOL_GRAD_REL * scale, False, o)
        print("%s %s %s %s: max error over the finite entries %.3g (scale %.3g)" % (name, case, form, o, err, scale))
        for m in OTHERS:                                                                # R4
            if form == "gather" or o == "grad_feat1":
                assert np.array_equal(r[o][m].view(np.uint32), base[o][m].view(np.uint32)), "R4 -- %s of pair %d changed" % (o, m)
            else:
                assert np.isfinite(r[o][m]).all()
                assert np.abs(r[o][m] - base[o][m]).max() <= TOL_GRAD_REL * scale


@pytest.mark.parametrize("form", ["gather", "atomic"])
@pytest.mark.parametrize("name,case", PIXEL + HEAD, ids=_ids(PIXEL + HEAD))
def test_backward_gather_atomic_kinds(env, name, case, form):
    """The second half of R1 for the gradients of the per-pixel backward forms: the KIND of every non-finite value is the
    reference's.  (The results of test_backward_gather_atomic, which runs first; computed here when run alone.)
    With the soft-max off and an infinite value in feat_ref or grad_out this caught tap registers that kept a stale row while
    the tap was outside the image: weight 0 times an infinite a_k / ds_k put NaN into that row's gradient, where the reference's
    zero padding adds nothing and the entry stays +-Inf (14 of 2048 entries for the feat_ref sites, 8 for the grad_out site)."""
    key = (name, case, form)
    if key not in _poisoned_bwd:
        test_backward_gather_atomic(env, name, case, form)
    d = nf.load(name)
    for o in ("grad_feat1", "grad_feat2"):
        nf.check_kinds(_poisoned_bwd[key][o][nf.POISONED], nf.expected(d, case, o), o)


# ---- backward: the tiled forms -------------------------------------------------------------------------------------------
_finite_tiled = {}


@pytest.mark.parametrize("with_attn", [False, True], ids=["recompute", "saved-attn"])
@pytest.mark.parametrize("form", ["tile", "tile_det"])
@pytest.mark.parametrize("name,case", HEAD16, ids=_ids(HEAD16))
def test_backward_tiled(env, name, case, form, with_attn):
    """The MFMA tile backward, float-atomic and deterministic, with the recomputed and with the saved attention.  R1 (finiteness) and
    R4 -- bit-equal for "tile_det", TOL_GRAD_REL for "tile", no error bit, the deferred tiles of the finite pairs unchanged -- and,
    in place of R2, the spread INTEGRATION.md documents: within the pair the tiles that meet the value may turn other entries
    non-finite or inaccurate, so nothing but R1 is asserted of pair 1 in the poisoned call (its finite call is held to the
    reference)."""
    _lib, ops = env
    d = nf.load(name)
    spec = _spec(ops, d, 0)
    cam = _dev(d["cam"])
    det = form == "tile_det"

    def run(f1, f2, g):
        ref, src, go = ops.to_nhwc(_dev(f1)), ops.to_nhwc(_dev(f2)), ops.to_nhwc(_dev(g))
        attn = ops.forward_nhwc(spec, ref, src, cam, workspace=ops.tile_workspace(spec, N, 256, ref.device))[1] if with_attn else None
        ws = (ops.det_tile_workspace if det else ops.tile_workspace)(spec, N, 256, ref.device)
        assert ws.numel() > 0
        gr, gs = ops.backward_nhwc(spec, ref, src, cam, go, form=form, attn=attn, workspace=ws)
        torch.cuda.synchronize()
        ops.check_tile_errors(workspace=ws)                                             # no bit of the sticky error word
        deferred, tpp = _overflow_tiles(ops, spec, d, ws)
        return dict(grad_feat1=_nchw(gr), grad_feat2=_nchw(gs), deferred=deferred, tpp=tpp)

    key = (name, form, with_attn)
    if key not in _finite_tiled:
        b = _finite_tiled[key] = run(d["feat1"], d["feat2"], d["grad_out"])
        for o in ("grad_feat1", "grad_feat2"):
            assert np.isfinite(b[o]).all()
            nf.check_values(b[o][nf.POISONED], d[o + "1"], TOL_GRAD_REL * float(np.abs(d[o + "1"]).max()), False, o + " (finite call)")
    base = _finite_tiled[key]
    f1, f2, g, _ = nf.poisoned_inputs(d, case)
    r = run(f1, f2, g)
    n = nf.POISONED
    for o in ("grad_feat1", "grad_feat2"):
        want = nf.expected(d, case, o)
        lost = ~np.isfinite(want) & np.isfinite(r[o][n])
        assert not lost.any(), "%s: R1 -- %d non-finite values of the reference came out finite, first at %s" % (
            o, lost.sum(), tuple(np.argwhere(lost)[0]))
        scale = float(np.abs(d[o + "1"]).max())
        for m in OTHERS:                                                                # R4: the spread ends at the pair
            if det or o == "grad_feat1":
                assert np.array_equal(r[o][m].view(np.uint32), base[o][m].view(np.uint32)), "R4 -- %s of pair %d changed" % (o, m)
            else:
                assert np.isfinite(r[o][m]).all()
                assert np.abs(r[o][m] - base[o][m]).max() <= TOL_GRAD_REL * scale
    others = lambda s: {t for t in s if t // r["tpp"] != n}
    assert others(r["deferred"]) == others(base["deferred"]), "R4 -- the deferred tiles of the finite pairs changed"


# ---- the general kernels, every mode of the fixtures, through the module --------------------------------------------------
def _mode_module(d, prior1):
    from epipolar_transformers_amd import default_cfg
    from epipolar_transformers_amd.epipolar import Epipolar

    m = d["dims"]
    cfg = default_cfg()
    cfg.merge_from_list(["KEYPOINT.HEATMAP_SIZE", (m["H"], m["H"]), "KEYPOINT.NFEATS", m["C"], "EPIPOLAR.SAMPLESIZE", m["K"],
                         "DATASETS.IMAGE_SIZE", (m["image"], m["image"]), "EPIPOLAR.USE_CORRECT_NORMALIZE", True,
                         "EPIPOLAR.ATTENTION", "avg", "EPIPOLAR.PARAMETERIZED", ("z",), "EPIPOLAR.ZRESIDUAL", True,
                         "EPIPOLAR.MERGE", "late", "EPIPOLAR.SHARE_WEIGHTS", True] + [str(v) for v in d["overrides"]])
    mod = Epipolar(cfg=cfg).cuda().eval()
    sd = {k[3:]: torch.from_numpy(np.array(d[k])) for k in d if k.startswith("sd.")}
    assert sorted(mod.state_dict()) == sorted(sd)
    mod.load_state_dict(sd)
    for k in d:
        if k.startswith("prior."):
            _, i, j = k.split(".")
            v = prior1 if (prior1 is not None and k == "prior.2.3") else d[k]
            mod.prior[(int(i), int(j))] = torch.nn.Parameter(torch.from_numpy(np.array(v)).cuda())
    cam = _dev(d["cam"])
    mod._cams.get = lambda *a, **k: cam
    return mod


_finite_mode = {}


@pytest.mark.parametrize("name,case", MODES, ids=_ids(MODES))
def test_general_kernels(env, name, case):
    """et_epipolar_forward_general / _backward_general in every mode of tests/golden/nonfinite/mode_*: POOLING (+ theta / phi / g),
    ATTENTION max, cosine, prior added / multiplied.  attn comes straight from the kernel: the kind of a non-finite value must
    match; finalout and the gradients also pass torch's 1x1 convolutions (library GEMMs): the finiteness mask."""
    _lib, ops = env
    d = nf.load(name)

    def run(f1, f2, g, prior1):
        mod = _mode_module(d, prior1)
        assert not mod._fused_mode() and mod._general_kernel_applies(_dev(f1), _dev(f2), None, None, d["camera"], d["other_camera"])
        a1, a2 = _dev(f1).requires_grad_(True), _dev(f2).requires_grad_(True)
        fin, corr, attn, _ = mod(a1, a2, torch.from_numpy(np.array(d["P1"])), torch.from_numpy(np.array(d["P2"])),
                                 camera=torch.from_numpy(np.array(d["camera"])), other_camera=torch.from_numpy(np.array(d["other_camera"])))
        (fin * _dev(g)).sum().backward()
        torch.cuda.synchronize()
        z = lambda t, like: np.zeros_like(like) if t is None else t.cpu().numpy()
        return dict(finalout=fin.detach().cpu().numpy(), attn=attn.detach().cpu().numpy(), corr=corr.cpu().numpy(),
                    grad_feat1=z(a1.grad, f1), grad_feat2=z(a2.grad, f2)), mod

    if name not in _finite_mode:
        _finite_mode[name] = run(d["feat1"], d["feat2"], d["grad_out"], None)[0]
    base = _finite_mode[name]
    f1, f2, g, prior1 = nf.poisoned_inputs(d, case)
    r, mod = run(f1, f2, g, prior1)
    n = nf.POISONED
    nf.check_values(r["attn"][n], nf.expected(d, case, "attn"), TOL_ATTN * max(1.0, float(np.abs(d["attn1"]).max())), True, "attn")
    locs = ops.sample_locs(mod.layer_spec(), _dev(d["cam"])).cpu().numpy()
    ties = nf.check_corr_pos(d, case, locs, r["corr"], r["attn"])
    # ATTENTION max GATHERS the arg-max sample: at a PROVEN tie the other, equally good sample's features come out -- those
    # pixels, and the entries of d(feat2) around the taps of the two tied samples, are exempt as in tests/test_gpu_modes.py
    ex1 = ex2 = None
    if "attention_max" in name and ties.any():
        assert ties.mean() <= 0.1
        H = W = d["dims"]["H"]
        ex1, ex2 = ties, np.zeros((H, W), dtype=bool)
        for pos in (r["corr"][n], d[case + ".corr_pos"]):
            for h, w in zip(*np.nonzero(ties)):
                gx = ((pos[h, w, 0] * 2.0 / (W - 1)) * W - 1) / 2
                gy = ((pos[h, w, 1] * 2.0 / (H - 1)) * H - 1) / 2
                for yy in range(int(np.floor(gy)) - 1, int(np.floor(gy)) + 3):
                    for xx in range(int(np.floor(gx)) - 1, int(np.floor(gx)) + 3):
                        if 0 <= yy < H and 0 <= xx < W:
                            ex2[yy, xx] = True
    nf.check_values(r["finalout"][n], nf.expected(d, case, "finalout"), 1e-4 * max(1.0, float(np.abs(d["finalout1"]).max())), False, "finalout",
                    exempt=ex1)
    for o, ex in (("grad_feat1", ex1), ("grad_feat2", ex2)):
        scale = max(float(np.abs(d[o + "1"]).max()), 1e-6)
        nf.check_values(r[o][n], nf.expected(d, case, o), TOL_GRAD_REL * scale, False, o, exempt=ex)
    for m in OTHERS:                                                                    # R4
        for o in ("finalout", "attn", "corr"):
            assert np.array_equal(r[o][m].view(np.uint32), base[o][m].view(np.uint32)), "R4 -- %s of pair %d changed" % (o, m)
        for o in ("grad_feat1", "grad_feat2"):                                          # (float atomics: to rounding)
            assert np.isfinite(r[o][m]).all()
            assert np.abs(r[o][m] - base[o][m]).max() <= TOL_GRAD_REL * max(float(np.abs(d[o + "1"]).max()), 1e-6)
