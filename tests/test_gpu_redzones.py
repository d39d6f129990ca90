"""Every export of the C ABI that writes device memory, with guard bands around everything it may write.

Feature maps go through bounded buffer resources, but the workspace regions, the per-block partial results of the et_z_*
kernels and most outputs are plain pointers: a store a few words past a region or past `*_workspace_bytes` lands in the next
region or in another tensor of the caching allocator and shows up, if ever, as a wrong number somewhere else.  Here every
output and every workspace of a call is carved out of one allocation (abi_harness.Arena) with 64 KiB of the byte 0xA5 on both
sides, workspaces get EXACTLY the size the `*_workspace_bytes` function returns (the tile workspace at the base torch returns
and at a base moved by 16 bytes: the library rounds the base up to 256 bytes itself), every guard byte is checked after the
call and every input is compared bit for bit with its clone from before.  Shapes: one regular and one ragged per export (H * W
not a multiple of 32, rows not a multiple of 64, non-square; the layout kernels with C and H * W not multiples of 64), the
overflow-heavy and deferred-tile cases for the tile kernels.  Inside the tile workspace the regions are checked against each
other: overflow count <= tiles, the list's entries distinct valid tile indices, a statistics word written for every tile.
Nothing here is meant to make the GPU fault; guard bytes are written and read back.
"""
import ctypes

import pytest
import torch

import abi_harness as hx
from abi_harness import C, Arena, call

pytestmark = pytest.mark.gpu

SPLIT, CLASSIC, BAND = 32768, 65536, 1048576
STATS_MARKER = 0x5A5A5A5A            # no U | groups << 16 a kernel writes (U <= 512, groups <= 32)


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from epipolar_transformers_amd import _lib, ops

    return _lib.load(), ops


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _consts(ops, spec):
    return spec.constants(torch.device("cuda", torch.cuda.current_device()))


def _finite(*tensors):
    for t in tensors:
        assert torch.isfinite(t).all(), "an output holds NaN / inf: part of it was not written"


# (n, h, w, k, c): regular, ragged
PIXEL_SHAPES = [(2, 16, 16, 16, 64), (3, 9, 7, 5, 36)]


@pytest.mark.parametrize("n,h,w,k,c", PIXEL_SHAPES, ids=["16x16-K16-C64", "9x7-K5-C36"])
def test_sample_locs_and_per_pixel_forward(env, n, h, w, k, c):
    lib, ops = env
    ref, src, cam = hx.pair_inputs(n, h, w, 60 + h)
    ref, src = ref[..., :c].contiguous(), src[..., :c].contiguous()
    bias = torch.randn(c, device="cuda", generator=_gen(1))
    spec = ops.LayerSpec(H=h, W=w, K=k)
    xs, ys, steps = _consts(ops, spec)
    d = spec.desc(n, c)
    a = (Arena().add("locs", (k, n, h, w, 2)).add("out", (n, h, w, c)).add("attn", (n, k, h, w)).add("corr", (n, h, w, 2))
         .add("base", (n, h, w, c)).build())
    snap = hx.frozen(xs=xs, ys=ys, steps=steps, cam=cam, ref=ref, src=src, bias=bias)
    call("et_sample_locs", d, xs, ys, steps, cam, a["locs"])
    call("et_epipolar_forward", d, xs, ys, steps, cam, ref, src, a["out"], a["attn"], a["corr"], bias, a["base"])
    a.check()
    hx.assert_unchanged(snap)
    _finite(a["locs"], a["out"], a["attn"], a["corr"], a["base"])
    want = ops.forward_nhwc(spec, ref, src, cam, res_bias=bias, want_res_base=True)
    assert all(hx.same_bits(a[nm], t) for nm, t in zip(("out", "attn", "corr", "base"), want))
    assert hx.same_bits(a["locs"], ops.sample_locs(spec, cam))


def T(name, n, h, w, k, variant=0, rig="ring", outlier=False, seed=None, expect=None):
    return dict(name=name, n=n, h=h, w=w, k=k, variant=variant, rig=rig, outlier=outlier, expect=expect,
                seed=seed if seed is not None else 5000 + 7 * h + 3 * w + k + n)


TILE_CASES = [T("regular-64x64-K64", 2, 64, 64, 64, expect="none"), T("ragged-33x20-K20", 3, 33, 20, 20),
              T("ragged-band-72x81-K40", 2, 72, 81, 40), T("ragged-two-pass-21x13-K70", 3, 21, 13, 70),
              T("ragged-classic-9x7-K5", 3, 9, 7, 5, variant=CLASSIC),
              T("split-16x16-K16-some-overflow", 4, 16, 16, 16, variant=SPLIT, expect="some"),
              T("split-band-72x88-K16-overflow", 2, 72, 88, 16, variant=SPLIT, expect="overflow"),
              T("fp16-guard-64x64-K64", 2, 64, 64, 64, outlier=True, expect="some"),
              T("epipole-inside-64x64-K64", 2, 64, 64, 64, rig="epipole_inside", seed=778)]
FUSED_CASES = [t for t in TILE_CASES if t["k"] <= 64 and not t["variant"] & CLASSIC]
BWD_CASES = [TILE_CASES[0], TILE_CASES[1], TILE_CASES[2], TILE_CASES[3], TILE_CASES[4],
             dict(TILE_CASES[8], expect="deferred"), T("split-in-place-16x16-K16", 4, 16, 16, 16, variant=SPLIT)]


def _tile_inputs(t):
    ref, src, cam = hx.pair_inputs(t["n"], t["h"], t["w"], t["seed"], t["rig"])
    if t["outlier"]:
        src[t["n"] - 1, 5, 6, 100] = 4.0e4
    return ref, src, cam


def _tile_ws(arena, lib, d, shift):
    nbytes = int(lib.et_epipolar_forward_workspace_bytes(ctypes.byref(d)))
    assert nbytes > 0
    arena.add("ws", nbytes, torch.uint8, fill=0, shift=shift)       # EXACTLY the size asked for; zero-initialised once
    return nbytes


def _mark_stats(ops, spec, t, ws):
    ops.tile_stats(spec, t["n"], C, ws).fill_(STATS_MARKER)


def _check_regions(ops, spec, t, ws):
    """The regions of the tile workspace against each other, after a forward."""
    tiles = hx.tiles_of(t["n"], t["h"], t["w"])
    cnt = hx.assert_overflow_list_is_sane(ws, t["n"], t["h"], t["w"])
    stats = ops.tile_stats(spec, t["n"], C, ws)
    assert stats.numel() == tiles and not (stats == STATS_MARKER).any(), "a tile's statistics word was not written"
    assert int((stats & 0xFFFF).max()) <= 512
    if t["expect"] == "overflow":
        assert cnt > tiles // 2, "the case was meant to put most tiles on the overflow list (%d of %d)" % (cnt, tiles)
    elif t["expect"] == "none":
        assert cnt == 0
    elif t["expect"] == "some":
        assert cnt > 0, "the case was meant to trip the fp16 guard"
    return cnt


@pytest.mark.parametrize("shift", [0, 16], ids=["base-as-allocated", "base-plus-16"])
@pytest.mark.parametrize("t", TILE_CASES, ids=[t["name"] for t in TILE_CASES])
def test_forward_tiled(env, t, shift):
    lib, ops = env
    ref, src, cam = _tile_inputs(t)
    n, h, w, k = t["n"], t["h"], t["w"], t["k"]
    bias = torch.randn(C, device="cuda", generator=_gen(2))
    spec = ops.LayerSpec(H=h, W=w, K=k, variant=t["variant"])
    xs, ys, steps = _consts(ops, spec)
    d = spec.desc(n, C)
    a = Arena().add("out", (n, h, w, C)).add("attn", (n, k, h, w)).add("corr", (n, h, w, 2)).add("base", (n, h, w, C))
    nbytes = _tile_ws(a, lib, d, shift)
    a.build()
    assert a["ws"].data_ptr() % 256 == shift
    _mark_stats(ops, spec, t, a["ws"])
    snap = hx.frozen(xs=xs, ys=ys, steps=steps, cam=cam, ref=ref, src=src, bias=bias)
    call("et_epipolar_forward_tiled", d, xs, ys, steps, cam, ref, src, a["out"], a["attn"], a["corr"], bias, a["base"], a["ws"],
         ctypes.c_size_t(nbytes))
    a.check()
    hx.assert_unchanged(snap)
    ops.check_tile_errors(workspace=a["ws"])
    _finite(a["out"], a["attn"], a["corr"], a["base"])
    _check_regions(ops, spec, t, a["ws"])
    want = ops.forward_nhwc(spec, ref, src, cam, res_bias=bias, want_res_base=True, workspace=ops.tile_workspace(spec, n, C, "cuda"))
    assert all(hx.same_bits(a[nm], x) for nm, x in zip(("out", "attn", "corr", "base"), want)), "differs from the call through ops"


@pytest.mark.parametrize("want_out", [0, 1], ids=["x-only", "want-out"])
@pytest.mark.parametrize("t", FUSED_CASES, ids=[t["name"] for t in FUSED_CASES])
def test_forward_fused(env, t, want_out):
    lib, ops = env
    ref, src, cam = _tile_inputs(t)
    n, h, w, k = t["n"], t["h"], t["w"], t["k"]
    g = _gen(3)
    wf = torch.randn(C, C, device="cuda", generator=g) * 0.05 + torch.eye(C, device="cuda")
    bias = torch.randn(C, device="cuda", generator=g)
    packed = ops.residual_gemm_pack(wf)
    spec = ops.LayerSpec(H=h, W=w, K=k, variant=t["variant"])
    assert ops.fused_layer_applies(spec, C, n)
    xs, ys, steps = _consts(ops, spec)
    d = spec.desc(n, C)
    a = Arena().add("x", (n, h, w, C)).add("attn", (n, k, h, w)).add("corr", (n, h, w, 2)).add("out", (n, h, w, C))
    nbytes = _tile_ws(a, lib, d, 16 * want_out)
    a.build()
    _mark_stats(ops, spec, t, a["ws"])
    snap = hx.frozen(xs=xs, ys=ys, steps=steps, cam=cam, ref=ref, src=src, bias=bias, packed=packed)
    call("et_epipolar_forward_fused", d, xs, ys, steps, cam, ref, src, packed, bias, a["x"], a["attn"], a["corr"], a["out"],
         want_out, a["ws"], ctypes.c_size_t(nbytes))
    a.check()
    hx.assert_unchanged(snap)
    ops.check_tile_errors(workspace=a["ws"])
    _finite(a["x"], a["attn"], a["corr"])
    _check_regions(ops, spec, t, a["ws"])
    want = ops.forward_fused_nhwc(spec, ref, src, cam, packed, bias, want_out=True, workspace=ops.tile_workspace(spec, n, C, "cuda"))
    names = ("x", "attn", "corr", "out") if want_out else ("x", "attn", "corr")
    assert all(hx.same_bits(a[nm], x) for nm, x in zip(names, want)), "differs from the call through ops"


def test_two_pass_tile_that_fails_in_both_halves_is_listed_once(env):
    """ADVICE r6, first item: in the two-pass kernel (64 < K <= 128) S2 of half 1 runs on the vector waves while G1 of half 0
    runs on the matrix waves; a tile whose half 0 trips the fp16 guard (claimed with atomicExch) while its half 1 does not fit
    (s2_publish: plain loads and stores) could be appended to the overflow list by both, and a list of more than `tiles`
    entries would run into the statistics region.  The case: 64-row capacity (ET_VARIANT_TILE_SPLIT: 16 x 16 maps, K = 100, so
    that row sets of a half do and do not fit from tile to tile) and source values beyond fp16's range on a grid of source
    pixels, so that every tile that reaches G1 trips the guard.  Every tile must be on the list exactly once, the regions
    intact, the results those of the per-pixel kernels."""
    lib, ops = env
    n, h, w, k = 8, 16, 16, 100
    t = T("two-pass-split-guard", n, h, w, k, variant=SPLIT)
    ref, src, cam = _tile_inputs(t)
    spec = ops.LayerSpec(H=h, W=w, K=k, variant=SPLIT)
    tiles = hx.tiles_of(n, h, w)
    # without outliers: some tiles leave through a half that does not fit, not all of them
    ws0 = ops.tile_workspace(spec, n, C, "cuda")
    ops.forward_nhwc(spec, ref, src, cam, workspace=ws0)
    torch.cuda.synchronize()
    unfit = hx.assert_overflow_list_is_sane(ws0, n, h, w)
    print("two-pass, 64-row capacity: %d of %d tiles have a half that does not fit" % (unfit, tiles))
    assert unfit > 0, "the case was meant to have tiles whose row set does not fit a half"
    src[:, :, 1::4, 100] = 4.0e4               # (the scale estimate reads every fourth pixel row of a 16 x 16 map, x % 4 == 0: it sees
    src[:, ::2, 2::4, 7] = -6.0e4              #  none of these, so every tile that converts its rows trips the guard)
    ref[..., 100] = 0                          # (... and the logits stay O(1): a logit of 5e3 would carry an fp32 rounding of 5e-4,
    ref[..., 7] = 0                            #  which no kernel's attention survives to 1e-5)
    xs, ys, steps = _consts(ops, spec)
    d = spec.desc(n, C)
    a = Arena().add("out", (n, h, w, C)).add("attn", (n, k, h, w)).add("corr", (n, h, w, 2))
    nbytes = _tile_ws(a, lib, d, 0)
    a.build()
    _mark_stats(ops, spec, t, a["ws"])
    snap = hx.frozen(cam=cam, ref=ref, src=src)
    call("et_epipolar_forward_tiled", d, xs, ys, steps, cam, ref, src, a["out"], a["attn"], a["corr"], None, None, a["ws"],
         ctypes.c_size_t(nbytes))
    a.check()
    hx.assert_unchanged(snap)
    ops.check_tile_errors(workspace=a["ws"])
    cnt = _check_regions(ops, spec, t, a["ws"])
    print("two-pass, 64-row capacity, fp16 outliers: %d of %d tiles on the overflow list" % (cnt, tiles))
    assert cnt >= unfit
    assert cnt > max(unfit, tiles // 2), "the outliers were meant to send most tiles to the list through the fp16 guard"
    want_out, want_attn, want_corr = ops.forward_nhwc(ops.LayerSpec(H=h, W=w, K=k, variant=16384), ref, src, cam)
    _finite(a["out"], a["attn"], a["corr"])
    assert (a["attn"] - want_attn).abs().max().item() <= 1e-5
    assert (a["out"] - want_out).abs().max().item() <= 1e-4 * max(1.0, want_out.abs().max().item())


@pytest.mark.parametrize("with_attn", [False, True], ids=["recompute", "attn"])
@pytest.mark.parametrize("t", BWD_CASES, ids=[t["name"] for t in BWD_CASES])
def test_backward_tiled(env, t, with_attn):
    lib, ops = env
    ref, src, cam = _tile_inputs(t)
    n, h, w, k = t["n"], t["h"], t["w"], t["k"]
    gout = torch.randn(n, h, w, C, device="cuda", generator=_gen(4))
    spec = ops.LayerSpec(H=h, W=w, K=k, variant=t["variant"])
    attn = ops.forward_nhwc(ops.LayerSpec(H=h, W=w, K=k, variant=16384), ref, src, cam)[1] if with_attn else None
    xs, ys, steps = _consts(ops, spec)
    d = spec.desc(n, C)
    nbytes = int(lib.et_epipolar_backward_tiled_workspace_bytes(ctypes.byref(d)))
    assert nbytes == int(lib.et_epipolar_forward_workspace_bytes(ctypes.byref(d))) > 0
    a = Arena().add("gref", (n, h, w, C)).add("gsrc", (n, h, w, C)).add("ws", nbytes, torch.uint8, fill=0, shift=16 * with_attn).build()
    snap = hx.frozen(xs=xs, ys=ys, steps=steps, cam=cam, ref=ref, src=src, gout=gout, attn=attn)
    if with_attn:
        call("et_epipolar_backward_tiled_attn", d, xs, ys, steps, cam, ref, src, attn, gout, a["gref"], a["gsrc"], a["ws"], ctypes.c_size_t(nbytes))
    else:
        call("et_epipolar_backward_tiled", d, xs, ys, steps, cam, ref, src, gout, a["gref"], a["gsrc"], a["ws"], ctypes.c_size_t(nbytes))
    a.check()
    hx.assert_unchanged(snap)
    deferred = ops.backward_deferred_tiles("cuda", workspace=a["ws"])
    assert 0 <= deferred <= hx.tiles_of(n, h, w)
    lst = hx.ws_overflow_list(a["ws"], n, h, w, deferred).cpu().tolist()
    assert len(set(lst)) == deferred and all(0 <= v < hx.tiles_of(n, h, w) for v in lst)
    if t["expect"] == "deferred":
        assert deferred > 0, "the case was meant to defer tiles to the second launch"
    g_ref, g_src = ops.backward_nhwc(spec, ref, src, cam, gout, form="gather")
    for got, want in ((a["gref"], g_ref), (a["gsrc"], g_src)):
        _finite(got)
        assert (got - want).abs().max().item() <= 1e-4 * max(want.abs().max().item(), 1e-30)      # TOL_GRAD_REL (test_gpu_parity.py)


@pytest.mark.parametrize("form", ["gather", "atomic"])
@pytest.mark.parametrize("n,h,w,k,c", PIXEL_SHAPES + [(2, 33, 20, 20, 256)], ids=["16x16-K16-C64", "9x7-K5-C36", "33x20-K20-C256"])
def test_backward_gather_and_atomic(env, n, h, w, k, c, form):
    lib, ops = env
    ref, src, cam = hx.pair_inputs(n, h, w, 70 + h)
    ref, src = ref[..., :c].contiguous(), src[..., :c].contiguous()
    gout = torch.randn(n, h, w, c, device="cuda", generator=_gen(5))
    spec = ops.LayerSpec(H=h, W=w, K=k)
    xs, ys, steps = _consts(ops, spec)
    d = spec.desc(n, c)
    a = Arena().add("gref", (n, h, w, c)).add("gsrc", (n, h, w, c))
    nbytes = 0
    if form == "gather":
        nbytes = int(lib.et_epipolar_backward_workspace_bytes(ctypes.byref(d)))
        a.add("ws", nbytes, torch.uint8)                 # (0xFF-filled: "no initialisation needed")
    a.build()
    snap = hx.frozen(xs=xs, ys=ys, steps=steps, cam=cam, ref=ref, src=src, gout=gout)
    call("et_epipolar_backward", d, xs, ys, steps, cam, ref, src, gout, a["gref"], a["gsrc"], a["ws"] if nbytes else None, ctypes.c_size_t(nbytes))
    a.check()
    hx.assert_unchanged(snap)
    _finite(a["gref"], a["gsrc"])
    g_ref, g_src = ops.backward_nhwc(spec, ref, src, cam, gout, form="gather")
    if form == "gather":
        assert hx.same_bits(a["gref"], g_ref) and hx.same_bits(a["gsrc"], g_src)
    else:
        for got, want in ((a["gref"], g_ref), (a["gsrc"], g_src)):
            assert (got - want).abs().max().item() <= 1e-4 * max(want.abs().max().item(), 1e-30)


# (n, h, w, k, c_sim, c_val, pooling, with prior)
GENERAL_SHAPES = [(2, 16, 16, 8, 64, 64, False, False), (3, 9, 7, 6, 12, 20, True, True)]


@pytest.mark.parametrize("n,h,w,k,cs,cv,pooling,with_prior", GENERAL_SHAPES, ids=["16x16-K8", "9x7-K6-pooling-prior"])
def test_forward_and_backward_general(env, n, h, w, k, cs, cv, pooling, with_prior):
    lib, ops = env
    _, _, cam = hx.pair_inputs(n, h, w, 80 + h)
    g = _gen(6)
    q = torch.randn(n, h, w, cs, device="cuda", generator=g)
    ms = torch.randn(n, h, w, cs, device="cuda", generator=g)
    mv = torch.randn(n, h, w, cv, device="cuda", generator=g)
    ks = k // 2 if pooling else k
    prior = torch.randn(n, ks, h, w, device="cuda", generator=g) * 0.1 if with_prior else None
    gout = torch.randn(n, h, w, cv, device="cuda", generator=g)
    spec = ops.LayerSpec(H=h, W=w, K=k)
    xs, ys, steps = _consts(ops, spec)
    d = spec.desc(n, 4)
    flags = 1 if pooling else 0
    a = (Arena().add("out", (n, h, w, cv)).add("attn", (n, ks, h, w)).add("corr", (n, h, w, 2)).add("gq", (n, h, w, cs))
         .add("gsim", (n, h, w, cs), fill=0).add("gval", (n, h, w, cv), fill=0).add("gprior", (n, ks, h, w)).build())   # (accumulated: zeroed)
    snap = hx.frozen(xs=xs, ys=ys, steps=steps, cam=cam, q=q, map_sim=ms, map_val=mv, prior=prior, gout=gout)
    call("et_epipolar_forward_general", d, xs, ys, steps, cam, q, ms, mv, prior, cs, cv, flags, a["out"], a["attn"], a["corr"])
    call("et_epipolar_backward_general", d, xs, ys, steps, cam, q, ms, mv, prior, gout, cs, cv, flags, a["gq"], a["gsim"], a["gval"],
         a["gprior"] if with_prior else None)
    a.check()
    hx.assert_unchanged(snap)
    _finite(a["out"], a["attn"], a["corr"], a["gq"], a["gsim"], a["gval"])
    want = ops.forward_general_nhwc(spec, q, ms, mv, cam, prior=prior, pooling=pooling)
    assert all(hx.same_bits(a[nm], x) for nm, x in zip(("out", "attn", "corr"), want))
    gq, gs, gv, gp = ops.backward_general_nhwc(spec, q, ms, mv, cam, gout, pooling=pooling, prior=prior, need_prior=with_prior)
    assert hx.same_bits(a["gq"], gq)
    for got, want_g in ((a["gsim"], gs), (a["gval"], gv)):                      # (float atomics: to rounding)
        assert (got - want_g).abs().max().item() <= 1e-4 * max(want_g.abs().max().item(), 1e-30)
    if with_prior:
        _finite(a["gprior"])
        assert hx.same_bits(a["gprior"], gp)


ROWS = [5, 112, 1587, 4096, 70000]            # regular (4096) and ragged: partial last blocks


@pytest.mark.parametrize("rows,c", [(4096, 256), (1587, 256), (63, 36)])
def test_residual_epilogue(env, rows, c):
    lib, ops = env
    g = _gen(7)
    feat, out, y = (torch.randn(rows, c, device="cuda", generator=g) for _ in range(3))
    scale, shift = torch.randn(c, device="cuda", generator=g), torch.randn(c, device="cuda", generator=g)
    a = Arena().add("fin", (rows, c)).add("x", (rows, c)).build()
    snap = hx.frozen(feat=feat, out=out, y=y, scale=scale, shift=shift)
    call("et_residual_epilogue", ctypes.c_int64(rows), c, feat, out, y, scale, shift, a["fin"], a["x"])
    a.check()
    hx.assert_unchanged(snap)
    fin, x = ops.residual_epilogue(feat.view(1, 1, rows, c), out.view(1, 1, rows, c), y, scale, shift)
    assert hx.same_bits(a["fin"], fin.view(rows, c)) and hx.same_bits(a["x"], x.view(rows, c))


@pytest.mark.parametrize("rows", ROWS)
def test_residual_gemm_pack_and_gemm(env, rows):
    lib, ops = env
    g = _gen(8)
    wf = torch.randn(C, C, device="cuda", generator=g) * 0.05 + torch.eye(C, device="cuda")
    out, feat = torch.randn(rows, C, device="cuda", generator=g), torch.randn(rows, C, device="cuda", generator=g)
    bias = torch.randn(C, device="cuda", generator=g)
    a = Arena().add("packed", int(lib.et_residual_gemm_packed_bytes()), torch.uint8).add("x", (rows, C)).build()
    snap = hx.frozen(wf=wf, out=out, feat=feat, bias=bias)
    call("et_residual_gemm_pack", wf, a["packed"])
    call("et_residual_gemm", ctypes.c_int64(rows), C, out, feat, a["packed"], bias, a["x"])
    a.check()
    hx.assert_unchanged(snap)
    _finite(a["x"])
    packed = ops.residual_gemm_pack(wf)
    assert hx.same_bits(a["x"], ops.residual_gemm(out, packed, bias, feat))


@pytest.mark.parametrize("rows", ROWS)
def test_z_kernels(env, rows):
    """et_z_batch_stats, et_z_backward, et_z_wgrad: workspaces of exactly the size asked for, 0xFF-filled."""
    lib, ops = env
    g = _gen(9 + rows)
    out = torch.randn(rows, C, device="cuda", generator=g).relu_()
    wz = torch.randn(C, C, device="cuda", generator=g) * 0.05
    bz, gamma = torch.randn(C, device="cuda", generator=g) * 0.1, 1 + 0.1 * torch.randn(C, device="cuda", generator=g)
    gx = torch.randn(rows, C, device="cuda", generator=g)
    packed, packed_t = ops.residual_gemm_pack(wz), ops.residual_gemm_pack(wz.t().contiguous())
    nb = [int(f(ctypes.c_int64(rows))) for f in (lib.et_z_batch_stats_workspace_bytes, lib.et_z_backward_workspace_bytes, lib.et_z_wgrad_workspace_bytes)]
    a = Arena()
    for nm in ("y", "gout", "gy"):
        a.add(nm, (rows, C))
    for nm in ("mean", "var", "ggamma", "gbeta", "gb"):
        a.add(nm, (C,))
    a.add("gw", (C, C))
    for nm, b in zip(("ws_stats", "ws_bwd", "ws_wgrad"), nb):
        a.add(nm, b, torch.uint8)
    a.build()
    snap = hx.frozen(out=out, packed=packed, packed_t=packed_t, bz=bz, gamma=gamma, gx=gx)
    call("et_z_batch_stats", ctypes.c_int64(rows), C, out, packed, bz, a["y"], a["mean"], a["var"], a["ws_stats"], ctypes.c_size_t(nb[0]))
    invstd = torch.rsqrt(a["var"] + 1e-5)
    snap.update(hx.frozen(invstd=invstd))
    call("et_z_backward", ctypes.c_int64(rows), C, gx, a["y"], a["mean"], invstd, gamma, packed_t, 1, a["gout"], a["gy"], a["ggamma"],
         a["gbeta"], a["ws_bwd"], ctypes.c_size_t(nb[1]))
    call("et_z_wgrad", ctypes.c_int64(rows), C, a["gy"], out, a["gw"], a["gb"], a["ws_wgrad"], ctypes.c_size_t(nb[2]))
    a.check()
    hx.assert_unchanged(snap)
    y, mean, var = ops.z_batch_stats(out, packed, bz)
    gout, gy, ggamma, gbeta = ops.z_backward(gx, y, mean, invstd, gamma, packed_t, True)
    gw, gb = ops.z_wgrad(gy, out)
    for nm, want in (("y", y), ("mean", mean), ("var", var), ("gout", gout), ("gy", gy), ("ggamma", ggamma), ("gbeta", gbeta), ("gw", gw), ("gb", gb)):
        _finite(a[nm])
        assert hx.same_bits(a[nm], want), nm


@pytest.mark.parametrize("maps,h,w", [(12, 64, 64), (7, 9, 23)], ids=["12x64x64", "7x9x23"])
def test_heatmap_peaks(env, maps, h, w):
    lib, ops = env
    hm = torch.rand(maps, h, w, device="cuda", generator=_gen(10))
    a = Arena().add("locs", (maps, 2)).add("scores", (maps,)).build()
    snap = hx.frozen(hm=hm)
    call("et_heatmap_peaks", ctypes.c_int64(maps), h, w, hm, ctypes.c_float(2.0), ctypes.c_float(4.0), ctypes.c_float(1e-6), 0, a["locs"], a["scores"])
    a.check()
    hx.assert_unchanged(snap)
    locs, scores = ops.heatmap_peaks(hm.view(1, maps, h, w), 2.0, 4.0)
    assert hx.same_bits(a["locs"], locs.view(maps, 2)) and hx.same_bits(a["scores"], scores.view(maps))


@pytest.mark.parametrize("n,c,h,w", [(2, 64, 16, 16), (3, 37, 5, 7), (2, 100, 9, 11)], ids=["C64-16x16", "C37-5x7", "C100-9x11"])
def test_layout_converters(env, n, c, h, w):
    lib, ops = env
    x = torch.randn(n, c, h, w, device="cuda", generator=_gen(11))
    a = Arena().add("nhwc", (n, h, w, c)).add("nchw", (n, c, h, w)).build()
    snap = hx.frozen(x=x)
    call("et_nchw_to_nhwc", n, c, h, w, x, a["nhwc"])
    call("et_nhwc_to_nchw", n, c, h, w, a["nhwc"], a["nchw"])
    a.check()
    hx.assert_unchanged(snap)
    assert torch.equal(a["nhwc"], x.permute(0, 2, 3, 1).contiguous()) and torch.equal(a["nchw"], x)
