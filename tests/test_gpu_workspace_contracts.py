"""The state the tile kernels start from (include/epipolar_amd.h, "workspace"; csrc/et_tile_host.h).

The parity tests give every call a fresh, zeroed workspace.  The product keeps ONE buffer per (device, stream, tag, host
thread) and reuses it for every shape, every forward instance, the one-kernel layer and the tiled backward.  Here:

  1. one caller-owned workspace, zeroed once, through a sequence of calls in which every call follows a call of another kind
     (map sizes down and up, N and K changing, every instance the forward's dispatcher picks, overflow-heavy before
     overflow-free, fp16 guard tripped before not tripped, the tiled backward between forwards and first of all).  Each call
     is repeated on a fresh zeroed workspace: forward / fused forward / tile statistics / overflow count BIT FOR BIT; the
     tiled backward (float atomics: reproducible to rounding only) against the bit-reproducible gather form at TOL_GRAD_REL,
     stale and fresh alike.  The fresh result of every forward step is itself compared with the per-pixel kernels
     (ET_VARIANT_NO_TILE) at the tolerances of tests/test_gpu_band.py.  The sticky error word reads 0 after every step; a
     bit written into it from the host survives calls of two shapes, is reported once and is clear afterwards.
     The product's own route: two layers of different map size alternating on the cached buffer, forward + backward.
  2. scratch that "needs no initialisation": et_z_batch_stats / et_z_backward / et_z_wgrad / the gather-form backward on
     zeroed, 0xFF-filled and random-filled workspaces, bit for bit; the tile workspace with everything behind its header
     0xFF / random and header words 0, 2..9 large positive / negative (word 1 zero; 10..63 are touched by nothing).
  4. two streams with their own cached workspaces, launches interleaved from one host thread, against the serial results.
(Section 3 -- guard bands around every buffer -- is tests/test_gpu_redzones.py.)
"""
import pytest
import torch

import abi_harness as hx
from abi_harness import C

pytestmark = pytest.mark.gpu

TOL_GRAD_REL = 1e-4                     # tests/test_gpu_parity.py, relative to the gradient's largest magnitude
TOL_ATTN, TOL_OUT_REL, TOL_CORR_FRAC = 1e-5, 1e-4, 1e-3      # tests/test_gpu_band.py (tile kernels vs per-pixel kernels)

SPLIT, CLASSIC, BAND, NO_TILE = 32768, 65536, 1048576, 16384


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from epipolar_transformers_amd import _lib, ops

    _lib.load()
    assert ops.POISON_OUTPUTS
    return _lib, ops


def S(name, kind, n, h, w, k, variant=0, softmax=True, rig="ring", outlier=False, scale=1.0, seed=None, expect=None):
    return dict(name=name, kind=kind, n=n, h=h, w=w, k=k, variant=variant, softmax=softmax, rig=rig, outlier=outlier, scale=scale,
                seed=seed if seed is not None else 4000 + 7 * h + 3 * w + k + n, expect=expect)


# kind: fwd = et_epipolar_forward_tiled; fused / fused_out = et_epipolar_forward_fused without / with want_out;
# bwd / bwd_attn = et_epipolar_backward_tiled_attn without / with the forward's attention.
# expect: "overflow" most tiles on the overflow list, "none" no tile there, "some" at least one (fp16 guard), "deferred" /
# "not_deferred" the backward's second launch got tiles / got none.
SEQUENCE = [
    S("bwd-first-16x16-K16", "bwd", 3, 16, 16, 16),                                      # on a workspace no forward has touched
    S("default-64x64-K64", "fwd", 4, 64, 64, 64, expect="none"),
    S("split-72x88-K16-overflow", "fwd", 2, 72, 88, 16, variant=SPLIT, expect="overflow"),
    S("band-40x96-K33", "fwd", 3, 40, 96, 33, expect="none"),                            # directly behind the overflow-heavy call
    S("fused-out-10x10-K16", "fused_out", 5, 10, 10, 16),
    S("split-16x16-K16-some-overflow", "fwd", 6, 16, 16, 16, variant=SPLIT, expect="some"),
    S("two-pass-64x64-K100", "fwd", 3, 64, 64, 100),
    S("bwd-attn-epipole-inside-64x64-K64", "bwd_attn", 2, 64, 64, 64, rig="epipole_inside", seed=778, expect="deferred"),
    S("bwd-ring-64x64-K64", "bwd", 6, 64, 64, 64, expect="not_deferred"),
    S("classic-48x48-K33", "fwd", 5, 48, 48, 33, variant=CLASSIC),
    S("default-64x64-K64-fp16-guard", "fwd", 4, 64, 64, 64, outlier=True, expect="some"),
    S("fused-64x64-K64", "fused", 3, 64, 64, 64, expect="none"),                         # directly behind the tripped guard
    S("softmax-off-16x16-K16", "fwd", 2, 16, 16, 16, softmax=False, scale=0.25),
    S("band-forced-33x20-K20", "fwd", 4, 33, 20, 20, variant=BAND, expect="none"),
    S("fused-out-split-96x96-K16-overflow", "fused_out", 2, 96, 96, 16, variant=SPLIT, expect="overflow"),
    S("band-forced-96x96-K64", "fwd", 3, 96, 96, 64, variant=BAND, expect="none"),
    S("bwd-attn-40x96-K33", "bwd_attn", 2, 40, 96, 33),
    S("two-pass-20x60-K128", "fwd", 3, 20, 60, 128),
    S("fused-guard-48x48-K33", "fused", 4, 48, 48, 33, outlier=True, expect="some"),
    S("config2-64x64-K64-N128", "fwd", 128, 64, 64, 64),
    S("default-10x10-K16", "fwd", 8, 10, 10, 16),
    S("default-64x64-K64-again", "fwd", 4, 64, 64, 64, expect="none"),
]
FORWARD_STEPS = [s for s in SEQUENCE if not s["kind"].startswith("bwd") and s["name"] != "default-64x64-K64-again"]


def _spec(ops, s, variant=None):
    return ops.LayerSpec(H=s["h"], W=s["w"], K=s["k"], softmax_enabled=s["softmax"], variant=s["variant"] if variant is None else variant)


def _inputs(s):
    ref, src, cam = hx.pair_inputs(s["n"], s["h"], s["w"], s["seed"], s["rig"], s["scale"])
    if s["outlier"]:                     # beyond fp16 under the estimated scale: those tiles are redone in exact fp32
        src[s["n"] - 1, 5, 6, 100] = 4.0e4
        src[0, s["h"] // 2, s["w"] // 3, 17] = -6.0e4
    g = torch.Generator(device="cuda").manual_seed(s["seed"] + 1)
    extra = {}
    if s["kind"].startswith("fused"):
        wf = torch.randn(C, C, device="cuda", generator=g) * 0.05 + torch.eye(C, device="cuda")
        extra = dict(wf=wf, bias=torch.randn(C, device="cuda", generator=g))
    if s["kind"].startswith("bwd"):
        extra = dict(gout=torch.randn(s["n"], s["h"], s["w"], C, device="cuda", generator=g))
    return ref, src, cam, extra


def _ws_bytes(ops, s):
    return ops.tile_workspace(_spec(ops, s), s["n"], C, "cpu").numel()


def _run(ops, s, inp, ws):
    """One step on workspace `ws`: dict of its results (for the forwards with the tile statistics and the overflow count)."""
    ref, src, cam, extra = inp
    spec = _spec(ops, s)
    kind = s["kind"]
    if kind == "fwd":
        out, attn, corr = ops.forward_nhwc(spec, ref, src, cam, workspace=ws)
        res = dict(out=out, attn=attn, corr=corr)
    elif kind.startswith("fused"):
        packed = ops.residual_gemm_pack(extra["wf"])
        r = ops.forward_fused_nhwc(spec, ref, src, cam, packed, extra["bias"], want_out=kind == "fused_out", workspace=ws)
        res = dict(x=r[0], attn=r[1], corr=r[2])
        if kind == "fused_out":
            res["out"] = r[3]
    else:
        attn = None
        if kind == "bwd_attn":           # (the forward's attention, from the per-pixel kernels: `ws` sees the backward only)
            attn = ops.forward_nhwc(_spec(ops, s, NO_TILE), ref, src, cam)[1]
        gr, gs = ops.backward_nhwc(spec, ref, src, cam, extra["gout"], form="tile", attn=attn, workspace=ws)
        torch.cuda.synchronize()
        return dict(gref=gr, gsrc=gs, deferred=ops.backward_deferred_tiles(ref.device, workspace=ws))
    torch.cuda.synchronize()
    res["stats"] = ops.tile_stats(spec, s["n"], C, ws).clone()
    res["overflow"] = hx.ws_overflow(ws)
    return res


def _assert_bit_equal(name, got, want):
    assert got.keys() == want.keys()
    for key in want:
        if isinstance(want[key], int):
            assert got[key] == want[key], "%s: %s %d on the used workspace, %d on a fresh one" % (name, key, got[key], want[key])
        else:
            assert hx.same_bits(got[key], want[key]), "%s: `%s` on the used workspace differs from a fresh workspace's" % (name, key)


def _assert_grad(name, which, got, want):
    assert torch.isfinite(got).all(), "%s: %s is not finite" % (name, which)
    scale = max(want.abs().max().item(), 1e-30)
    err = (got - want).abs().max().item()
    print("%s: %s max error %.3g of %.3g (bound %.3g)" % (name, which, err, scale, TOL_GRAD_REL * scale))
    assert err <= TOL_GRAD_REL * scale, (name, which, err, scale)


def _assert_expectation(s, res):
    tiles = hx.tiles_of(s["n"], s["h"], s["w"])
    if s["expect"] == "overflow":
        assert res["overflow"] > tiles // 2, "%s was meant to put most tiles on the overflow list (%d of %d)" % (s["name"], res["overflow"], tiles)
    elif s["expect"] == "none":
        assert res["overflow"] == 0, "%s was meant to put no tile on the overflow list (%d)" % (s["name"], res["overflow"])
    elif s["expect"] == "some":
        assert res["overflow"] > 0, "%s was meant to trip the fp16 guard" % s["name"]
    elif s["expect"] == "deferred":
        assert res["deferred"] > 0, "%s was meant to defer tiles to the backward's second launch" % s["name"]
    elif s["expect"] == "not_deferred":
        assert res["deferred"] == 0, "%s was meant to defer no tile" % s["name"]


def test_sequence_covers_every_forward_instance():
    """The sequence is what the test below is worth: every call follows a call of another kind, and every instance of the
    forward's dispatcher (csrc/et_forward_tile.hip) is in it."""
    for a, b in zip(SEQUENCE, SEQUENCE[1:]):
        assert (a["kind"], a["h"], a["w"], a["k"], a["variant"], a["rig"]) != (b["kind"], b["h"], b["w"], b["k"], b["variant"], b["rig"])
        assert a["n"] != b["n"]
    fw = [s for s in SEQUENCE if s["kind"] == "fwd"]
    assert any(s["variant"] == 0 and s["k"] <= 64 and max(s["h"], s["w"]) <= 64 and s["softmax"] for s in fw)         # default persistent
    assert any(s["variant"] == BAND and max(s["h"], s["w"]) > 64 for s in fw) and any(s["variant"] == BAND and max(s["h"], s["w"]) <= 64 for s in fw)
    assert any(64 < s["k"] <= 128 for s in fw) and any(s["variant"] == CLASSIC for s in fw) and any(s["variant"] == SPLIT for s in fw)
    assert any(not s["softmax"] for s in fw)
    assert {"fused", "fused_out", "bwd", "bwd_attn"} <= {s["kind"] for s in SEQUENCE}
    assert {16, 33, 64} <= {s["k"] for s in SEQUENCE}
    assert SEQUENCE[0]["kind"] == "bwd"
    names = [s["name"] for s in SEQUENCE]
    assert len(set(names)) == len(names)


def test_one_workspace_through_a_sequence_of_calls_of_different_kinds(env):
    _lib, ops = env
    shared = torch.zeros(max(_ws_bytes(ops, s) for s in SEQUENCE), dtype=torch.uint8, device="cuda")      # zeroed ONCE
    for s in SEQUENCE:
        inp = _inputs(s)
        got = _run(ops, s, inp, shared)
        ops.check_tile_errors(workspace=shared)          # (raises on a set bit)
        assert int(hx.ws_header(shared)[1].item()) == 0
        fresh_ws = ops.tile_workspace(_spec(ops, s), s["n"], C, "cuda")
        want = _run(ops, s, inp, fresh_ws)
        ops.check_tile_errors(workspace=fresh_ws)
        _assert_expectation(s, want)
        if s["kind"].startswith("bwd"):
            ref, src, cam, extra = inp
            g_ref, g_src = ops.backward_nhwc(_spec(ops, s), ref, src, cam, extra["gout"], form="gather")
            for label, res in (("used workspace", got), ("fresh workspace", want)):
                _assert_grad(s["name"] + ", " + label, "grad_ref", res["gref"], g_ref)
                _assert_grad(s["name"] + ", " + label, "grad_src", res["gsrc"], g_src)
            _assert_expectation(s, got)
        else:
            _assert_bit_equal(s["name"], got, want)
        del inp, got, want


@pytest.mark.parametrize("s", FORWARD_STEPS, ids=[s["name"] for s in FORWARD_STEPS])
def test_fresh_workspace_result_vs_per_pixel_kernels(env, s):
    """So that "the same call on a fresh workspace" is no unverified yardstick: each forward step against the per-pixel kernels."""
    _lib, ops = env
    inp = _inputs(s)
    ref, src, cam, extra = inp
    ws = ops.tile_workspace(_spec(ops, s), s["n"], C, "cuda")
    got = _run(ops, s, inp, ws)
    ops.check_tile_errors(workspace=ws)
    want_out, want_attn, want_corr = ops.forward_nhwc(_spec(ops, s, NO_TILE), ref, src, cam)
    assert torch.isfinite(got["attn"]).all()
    # (soft-max off: the "attention" is sim / K, unbounded, -1e10 / K on masked samples -- the relative term of
    #  tests/test_gpu_split_fp16.py::test_softmax_off_large_features beside the absolute bound; zero with the soft-max on)
    rel = 0.0 if s["softmax"] else 3e-6
    assert ((got["attn"] - want_attn).abs() - rel * want_attn.abs()).max().item() <= TOL_ATTN
    assert (got["corr"] != want_corr).any(-1).float().mean().item() <= TOL_CORR_FRAC      # (exact except at soft-max ties)
    if "out" in got:
        assert torch.isfinite(got["out"]).all()
        assert (got["out"] - want_out).abs().max().item() <= TOL_OUT_REL * max(1.0, want_out.abs().max().item())
    if "x" in got:
        want_x = ops.residual_gemm(want_out, ops.residual_gemm_pack(extra["wf"]), extra["bias"], ref)
        assert torch.isfinite(got["x"]).all()
        assert (got["x"] - want_x).abs().max().item() <= TOL_OUT_REL * max(1.0, want_x.abs().max().item())
    _assert_expectation(s, got)


def test_sticky_error_word_survives_calls_of_other_shapes_and_is_reported_once(env, monkeypatch):
    """A bit written into word 1 from the host (no kernel is made to fail): two calls of different shapes later it is still
    there, check_tile_errors raises once, the word is clear afterwards -- and the calls computed what they compute on a clean
    workspace."""
    _lib, ops = env
    steps = [next(x for x in SEQUENCE if x["name"] == nm) for nm in ("default-64x64-K64", "fused-out-10x10-K16")]                # default 64 x 64 / K 64, then the one-kernel layer at 10 x 10 / K 16
    ws = torch.zeros(max(_ws_bytes(ops, s) for s in steps), dtype=torch.uint8, device="cuda")
    hx.ws_header(ws)[1] = 2
    for s in steps:
        inp = _inputs(s)
        with monkeypatch.context() as m:      # (under POISON_OUTPUTS the wrappers check -- and clear -- the word after every call)
            m.setattr(ops, "check_tile_errors", lambda *a, **kw: None)
            got = _run(ops, s, inp, ws)
        assert int(hx.ws_header(ws)[1].item()) == 2, "the sticky error word lost its bit in %s" % s["name"]
        want = _run(ops, s, inp, ops.tile_workspace(_spec(ops, s), s["n"], C, "cuda"))
        _assert_bit_equal(s["name"], got, want)
    with pytest.raises(_lib.EpipolarAmdError, match="0x2"):
        ops.check_tile_errors(workspace=ws)
    assert int(hx.ws_header(ws)[1].item()) == 0
    ops.check_tile_errors(workspace=ws)               # reported once


def _layer(h, k, seed):
    from epipolar_transformers_amd import default_cfg
    from epipolar_transformers_amd.epipolar import Epipolar

    cfg = default_cfg()
    cfg.merge_from_list(["KEYPOINT.HEATMAP_SIZE", (h, h), "KEYPOINT.NFEATS", C, "EPIPOLAR.SAMPLESIZE", k, "EPIPOLAR.ATTENTION", "avg",
                         "EPIPOLAR.PARAMETERIZED", ("z",), "EPIPOLAR.ZRESIDUAL", True, "EPIPOLAR.USE_CORRECT_NORMALIZE", True,
                         "DATASETS.IMAGE_SIZE", (4 * h, 4 * h)])
    torch.manual_seed(seed)
    return Epipolar(cfg=cfg).cuda()


def _layer_round(ops, layers):
    """Forward + backward of every layer through EpipolarAttend (cached workspace), then its eval-mode one-kernel forward."""
    res = []
    for mod, (P1, P2, f1, f2, g) in layers:
        a1, a2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        mod.train()
        out, attn, corr = mod.attend(a1, a2, P1, P2)
        (out * g).sum().backward()
        mod.eval()
        with torch.no_grad():
            x = mod.forward_fused(f1, f2, P1, P2)[0]
        torch.cuda.synchronize()
        res.append(dict(out=out.detach().clone(), attn=attn.clone(), corr=corr.clone(), x=x.clone(), g1=a1.grad.clone(), g2=a2.grad.clone()))
    ops.check_tile_errors()
    return res


def test_two_layers_of_different_map_size_alternate_on_the_cached_workspace(env):
    """EPIPOLAR.MERGE both: two layers of different map size take turns on the one cached buffer in every step, forward and
    backward.  The small layer goes first, so the cache grows in round 1 (a new zeroed tensor is swapped in); rounds 2 and 3
    run on what round 1 left behind and must return round 1's results (forward bit for bit, gradients to TOL_GRAD_REL)."""
    _lib, ops = env
    from epipolar_transformers_amd import synthetic as syn

    ops.release_workspaces()
    layers = []
    for h, k, n, seed in ((16, 16, 4, 21), (64, 64, 8, 22)):
        P1, P2 = syn.make_pairs(n // 4, 4, 4 * h, seed=seed, jitter=(0.05, 8.0))
        f1, f2 = syn.make_features(n, C, h, h, seed=seed)
        g = torch.randn(n, C, h, h, generator=torch.Generator().manual_seed(seed + 1))
        layers.append((_layer(h, k, seed), (P1, P2, f1.cuda(), f2.cuda(), g.cuda())))
    rounds = [_layer_round(ops, layers) for _ in range(3)]
    # (one cached buffer per host thread: the forwards share the caller's, the tiled backwards the autograd thread's)
    fwd_keys = [key for key in ops._workspaces if key[3] == "fwd"]
    assert 1 <= len(fwd_keys) <= 2 and len({key[4] for key in fwd_keys}) == len(fwd_keys), fwd_keys
    for r in (1, 2):
        for first, later in zip(rounds[0], rounds[r]):
            for key in ("out", "attn", "corr", "x"):
                assert hx.same_bits(later[key], first[key]), "round %d: `%s` differs from round 1" % (r + 1, key)
            for key in ("g1", "g2"):
                _assert_grad("round %d" % (r + 1), key, later[key], first[key])


# ---------------------------------------------------------------------------------------------------------------------
# 2. scratch that "needs no initialisation"
# ---------------------------------------------------------------------------------------------------------------------

FILLS = ["ff", "random"]
ROWS = [5, 112, 1587, 70000]             # the ragged row counts of tests/test_gpu_fused.py: partial last blocks included


def _z_inputs(rows, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.randn(rows, C, device="cuda", generator=g).relu_()
    wz = torch.randn(C, C, device="cuda", generator=g) * 0.05
    bz = torch.randn(C, device="cuda", generator=g) * 0.1
    return out, wz, bz, g


def _filled(nbytes, how, seed=0):
    return hx.fill_bytes(torch.empty(nbytes, dtype=torch.uint8, device="cuda"), how, seed)


def _same_on_every_fill(run, nbytes, what):
    want = run(_filled(nbytes, "zero"))
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in want)
    for how in FILLS:
        got = run(_filled(nbytes, how, seed=nbytes % 97))
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(got, want)):
            assert hx.same_bits(a, b), "%s: result %d on a %s-filled workspace differs from a zeroed workspace's" % (what, i, how)


@pytest.mark.parametrize("rows", ROWS)
def test_z_batch_stats_ignores_workspace_contents(env, rows):
    _lib, ops = env
    out, wz, bz, _ = _z_inputs(rows, 10 + rows)
    packed = ops.residual_gemm_pack(wz)
    nbytes = int(_lib.load().et_z_batch_stats_workspace_bytes(rows))
    _same_on_every_fill(lambda ws: ops.z_batch_stats(out, packed, bz, workspace=ws), nbytes, "et_z_batch_stats")


@pytest.mark.parametrize("rows", ROWS)
def test_z_backward_ignores_workspace_contents(env, rows):
    _lib, ops = env
    out, wz, bz, g = _z_inputs(rows, 20 + rows)
    y, mean, var = ops.z_batch_stats(out, ops.residual_gemm_pack(wz), bz)
    invstd = torch.rsqrt(var + 1e-5)
    gamma = 1 + 0.1 * torch.randn(C, device="cuda", generator=g)
    gx = torch.randn(rows, C, device="cuda", generator=g)
    packed_t = ops.residual_gemm_pack(wz.t().contiguous())
    nbytes = int(_lib.load().et_z_backward_workspace_bytes(rows))
    _same_on_every_fill(lambda ws: ops.z_backward(gx, y, mean, invstd, gamma, packed_t, True, workspace=ws), nbytes, "et_z_backward")


@pytest.mark.parametrize("rows", ROWS)
def test_z_wgrad_ignores_workspace_contents(env, rows):
    _lib, ops = env
    out, _, _, g = _z_inputs(rows, 30 + rows)
    gy = torch.randn(rows, C, device="cuda", generator=g)
    nbytes = int(_lib.load().et_z_wgrad_workspace_bytes(rows))
    _same_on_every_fill(lambda ws: ops.z_wgrad(gy, out, workspace=ws), nbytes, "et_z_wgrad")


@pytest.mark.parametrize("n,h,w,k,c", [(3, 16, 16, 16, 256), (2, 9, 7, 5, 36), (2, 33, 20, 20, 256)], ids=["16x16-K16", "9x7-K5-C36", "33x20-K20"])
def test_gather_backward_ignores_workspace_contents(env, n, h, w, k, c):
    import ctypes

    _lib, ops = env
    ref, src, cam = hx.pair_inputs(n, h, w, 40 + h)
    ref, src = ref[..., :c].contiguous(), src[..., :c].contiguous()
    gout = torch.randn(n, h, w, c, device="cuda", generator=torch.Generator(device="cuda").manual_seed(h))
    spec = ops.LayerSpec(H=h, W=w, K=k)
    nbytes = int(_lib.load().et_epipolar_backward_workspace_bytes(ctypes.byref(spec.desc(n, c))))
    _same_on_every_fill(lambda ws: ops.backward_nhwc(spec, ref, src, cam, gout, form="gather", workspace=ws), nbytes, "et_epipolar_backward")


DIRTY = [S("default-64x64-K64", "fwd", 3, 64, 64, 64), S("split-16x16-K16-some-overflow", "fwd", 4, 16, 16, 16, variant=SPLIT, expect="some"), S("split-72x88-K16-overflow", "fwd", 2, 72, 88, 16, variant=SPLIT, expect="overflow"),
         S("band-80x72-K40", "fwd", 2, 80, 72, 40), S("two-pass-48x48-K65", "fwd", 3, 48, 48, 65),
         S("two-pass-split-16x16-K100-overflow", "fwd", 4, 16, 16, 100, variant=SPLIT),
         S("classic-33x20-K20", "fwd", 3, 33, 20, 20, variant=CLASSIC), S("softmax-off-16x16-K16", "fwd", 2, 16, 16, 16, softmax=False, scale=0.25),
         S("fp16-guard-64x64-K64", "fwd", 2, 64, 64, 64, outlier=True, expect="some"),
         S("fused-out-48x48-K33", "fused_out", 3, 48, 48, 33), S("fused-split-96x96-K16-overflow", "fused", 2, 96, 96, 16, variant=SPLIT, expect="overflow")]


@pytest.mark.parametrize("s", DIRTY, ids=[s["name"] for s in DIRTY])
def test_tile_forward_relies_on_the_error_word_only(env, s):
    """Everything behind the 64-word header 0xFF / random bytes, header words 0 and 2..9 large positive / negative; word 1 zero
    (words 10..63 are touched by nothing and stay zero): the results, statistics and overflow count of a zeroed workspace."""
    _lib, ops = env
    inp = _inputs(s)
    want = _run(ops, s, inp, ops.tile_workspace(_spec(ops, s), s["n"], C, "cuda"))
    _assert_expectation(s, want)
    for how, header_value in (("ff", 0x7FFFFF00), ("random", -123456789), ("random", 0x40000000), ("ff", -1)):
        ws = hx.dirty_tile_workspace(ops.tile_workspace(_spec(ops, s), s["n"], C, "cuda"), how, header_value, seed=header_value % 89)
        got = _run(ops, s, inp, ws)
        ops.check_tile_errors(workspace=ws)
        _assert_bit_equal("%s, %s-filled, header %d" % (s["name"], how, header_value), got, want)
        assert not ws_header_tail(ws).any(), "header words 10..63 are documented as touched by nothing"


def ws_header_tail(ws):
    return hx.ws_header(ws)[10:]


def test_tiled_backward_relies_on_nothing_in_the_workspace(env):
    """The tiled backward on a dirty workspace (as above) against the gather form, on the rig that defers tiles."""
    _lib, ops = env
    s = next(x for x in SEQUENCE if x["name"] == "bwd-attn-epipole-inside-64x64-K64")
    inp = _inputs(s)
    ref, src, cam, extra = inp
    g_ref, g_src = ops.backward_nhwc(_spec(ops, s), ref, src, cam, extra["gout"], form="gather")
    for how, header_value in (("ff", 0x7FFFFF00), ("random", -123456789)):
        ws = hx.dirty_tile_workspace(ops.tile_workspace(_spec(ops, s), s["n"], C, "cuda"), how, header_value)
        got = _run(ops, s, inp, ws)
        _assert_expectation(s, got)
        assert got["deferred"] <= hx.tiles_of(s["n"], s["h"], s["w"])
        _assert_grad(s["name"] + ", %s-filled" % how, "grad_ref", got["gref"], g_ref)
        _assert_grad(s["name"] + ", %s-filled" % how, "grad_src", got["gsrc"], g_src)
        assert int(hx.ws_header(ws)[1].item()) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. two streams
# ---------------------------------------------------------------------------------------------------------------------

def _stream_program(ops, s, rounds=3):
    """The calls one stream makes: (forward, backward, one-kernel layer) x rounds of one layer shape, cached workspaces."""
    ref, src, cam, _ = _inputs(s)
    g = torch.Generator(device="cuda").manual_seed(s["seed"] + 5)
    gout = torch.randn(s["n"], s["h"], s["w"], C, device="cuda", generator=g)
    wf = torch.randn(C, C, device="cuda", generator=g) * 0.05 + torch.eye(C, device="cuda")
    bias = torch.randn(C, device="cuda", generator=g)
    packed = ops.residual_gemm_pack(wf)
    spec = _spec(ops, s)
    calls = []
    for _ in range(rounds):
        calls.append(lambda: ops.forward_nhwc(spec, ref, src, cam))
        calls.append(lambda: ops.backward_nhwc(spec, ref, src, cam, gout, form="gather"))
        calls.append(lambda: ops.forward_fused_nhwc(spec, ref, src, cam, packed, bias, want_out=False))
    torch.cuda.synchronize()
    return calls


def test_two_streams_with_their_own_cached_workspaces_do_not_disturb_each_other(env, monkeypatch):
    """Two side streams, one layer shape each, launches interleaved from one host thread with no synchronisation between them
    until the end: every result bit-equal to the same calls run serially (forward, one-kernel layer and the bit-reproducible
    gather backward -- three cached buffers per stream).  What the stream in ops._workspace's key exists for."""
    _lib, ops = env
    shapes = [S("stream-a", "fwd", 4, 64, 64, 64), S("stream-b", "fwd", 6, 24, 40, 16, variant=SPLIT)]
    programs = [_stream_program(ops, s) for s in shapes]
    ops.release_workspaces()
    serial = [[c() for c in prog] for prog in programs]
    torch.cuda.synchronize()
    ops.release_workspaces()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    inter = [[], []]
    with monkeypatch.context() as m:
        # (the wrappers' per-call check_tile_errors under POISON_OUTPUTS synchronises the host with the device: off while the
        #  launches are interleaved, the words are read once at the end)
        m.setattr(ops, "check_tile_errors", lambda *a, **kw: None)
        for i in range(len(programs[0])):
            for j in (0, 1):
                with torch.cuda.stream(streams[j]):
                    inter[j].append(programs[j][i]())
    torch.cuda.synchronize()
    ops.check_tile_errors()
    for j in (0, 1):
        for i, (got, want) in enumerate(zip(inter[j], serial[j])):
            for a, b in zip(got, want):
                assert hx.same_bits(a, b), "stream %d, call %d: differs from the serial run" % (j, i)
    for tag in ("fwd", "bwd", "fwd_out_scratch"):
        bufs = {key[2]: buf for key, buf in ops._workspaces.items() if key[3] == tag}
        assert set(bufs) == {st.cuda_stream for st in streams}, (tag, sorted(bufs))
        a, b = (bufs[st.cuda_stream] for st in streams)
        assert a.data_ptr() != b.data_ptr() and (a.data_ptr() + a.numel() <= b.data_ptr() or b.data_ptr() + b.numel() <= a.data_ptr())
