"""Every kernel family at the ENDS of the ranges its argument check admits -- where register arrays, template instances and loop
trips run full or nearly empty -- against a plain reference of the same operation:

  A. the main operator (validate(): C a multiple of 4 in [4, 512], K in [2, 256]; the tile path and the one-kernel layer at maps
     smaller than one tile, K = 2 and K = 256) against the float32 C oracle, which tests/test_limits_cpu.py holds to float64 at
     these very shapes within a quarter of the tolerances used here;
  B. the general kernels at the ABI level (c_sim in [1, 512], c_val in [1, 4096], K' <= 256) against the float64 restatement of
     tests/general_restatement.py, itself pinned to Epipolar._attend_general_chunk in float64;
  C. the lifting kernels (et_rpsm: J = 1 and 32, depth 0 and 16, any tree, align_corners; et_triangulate_epipolar: V = 1) against
     their NumPy restatements.

The outputs start as NaN (conftest: ops.POISON_OUTPUTS), so an element a kernel did not write shows."""
import numpy as np
import pytest
import torch

from conftest import assert_corr_pos, denormalized_locations

import general_restatement
import rpsm_restatement as rpsm_restate
import triangulation_epipolar_restatement as tri_restate
from test_gpu_parity import TOL_ATTN, TOL_GRAD_REL, TOL_OUT, _assert_corr_pos, _close
from test_limits_cpu import SHAPES, grad_ref_terms, inputs, layer_kwargs, reference, shape_id
from test_rpsm_cpu import TOLERANCE_MM
from test_triangulate_epipolar_cpu import within_tolerance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from epipolar_transformers_amd import _lib, camera, ops

    _lib.load()
    assert ops.POISON_OUTPUTS
    return _lib, camera, ops


def held(what, err, bound):
    """Print the figure, then hold it to its bound."""
    print("    %-34s %.3e  (bound %.3e)" % (what, err, bound))
    assert err <= bound, (what, err, bound)


# =====================================================================================================================
# A. the main operator
# =====================================================================================================================
ROUTES = ("default", "no_tile", "tile_classic")
MAIN_CASES = [(shape, route) for shape in SHAPES for route in ROUTES if route != "tile_classic" or shape[2] == 256]


def test_main_shape_list_reaches_the_ends_of_the_ranges():
    """The shape list is test_limits_cpu.SHAPES; a later edit must not drop an end of a range."""
    Cs, Ks = {s[2] for s in SHAPES}, {s[3] for s in SHAPES}
    assert {4, 512} <= Cs and {2, 3, 4, 256} <= Ks
    c256 = [s for s in SHAPES if s[2] == 256]
    assert any(s[0] * s[1] < 16 for s in c256) and any(s[3] == 2 for s in c256) and any(s[3] == 256 for s in c256)
    assert any(s[0] == 1 for s in c256) and any(s[1] == 1 for s in c256)
    assert any(not s[4].get("softmax_enabled", True) and s[2] == 512 and s[3] == 256 for s in SHAPES)
    # every one-row / one-column map runs under legacy normalize: correct_normalize divides by W - 1 = 0 there (the oracle
    # returns NaN), and that combination is deliberately not run on the GPU
    assert all(not s[4].get("correct_normalize", True) for s in SHAPES if min(s[0], s[1]) == 1)


@pytest.mark.parametrize("shape,route", MAIN_CASES, ids=lambda v: v if isinstance(v, str) else shape_id(v))
def test_main_operator_at_the_limits_vs_oracle(env, shape, route):
    """Forward (attn, out, corr_pos, sample_locs, residual base), every backward form that applies, and the one-kernel layer
    where it applies -- asserted as tests/test_gpu_parity.py::test_ragged_shapes_vs_oracle asserts them."""
    _lib, camera, ops = env
    H, W, C, K, _ = shape
    variant = dict(default=0, no_tile=_lib.ET_VARIANT_NO_TILE, tile_classic=_lib.ET_VARIANT_TILE_CLASSIC)[route]
    kw = layer_kwargs(shape)
    want = reference(shape)
    _, _, f1, f2, go = inputs(shape)
    spec = ops.LayerSpec(H=H, W=W, K=K, variant=variant, **kw)
    cam = want["cam"].cuda()
    ref, src, gout = ops.to_nhwc(f1.cuda()), ops.to_nhwc(f2.cuda()), ops.to_nhwc(go.cuda())
    print("\n  %s, %s" % (shape_id(shape), route))
    if C == 256 and route != "no_tile":          # the route really is the tile path
        import ctypes
        assert int(_lib.load().et_epipolar_forward_workspace_bytes(ctypes.byref(spec.desc(3, C)))) > 0
    out, attn, corr, base = ops.forward_nhwc(spec, ref, src, cam, want_res_base=True)
    assert torch.equal(base, ref)
    attn_np, out_np = attn.cpu().numpy(), out.permute(0, 3, 1, 2).cpu().numpy()
    print("    attn max|d| %.3e, out max|d| %.3e" % (np.abs(attn_np - want["attn"]).max(), np.abs(out_np - want["out"]).max()))
    _close(attn_np, want["attn"], TOL_ATTN)
    _close(out_np, want["out"], TOL_OUT)
    _assert_corr_pos(ops, spec, cam, corr.cpu().numpy(), want["corr_pos"], attn_np, max_frac=5e-2)
    assert np.array_equal(ops.sample_locs(spec, cam).cpu().numpy(), want["sample_locs"])
    forms = ["gather", "atomic"]
    # (the tile forms of a C = 256 shape run on the default and the one-block-per-tile route; under ET_VARIANT_NO_TILE the layer
    #  has left the tile path, and they would only repeat the default route's run)
    if C == 256 and route != "no_tile":
        forms += ["tile"] + (["tile_det"] if spec.softmax_enabled else [])
    for form in forms:
        gr, gs = ops.backward_nhwc(spec, ref, src, cam, gout, form=form)
        for name, got, wantg in (("d feat_ref", gr, want["grad_ref"]), ("d feat_src", gs, want["grad_src"])):
            got = got.permute(0, 3, 1, 2).cpu().numpy()
            if name == "d feat_ref" and min(H, W) == 1:
                # all K samples of a pixel coincide on a one-row map: d(feat_ref) = scale sum_k a_k (e_k - e^) S_k is ZERO
                # analytically (the oracle returns 1e-15) and has no maximum to be relative to.  What float32 returns is the
                # rounding of its n terms t_i.  With signs at random the partial sums grow like sqrt(i) rms(t), each addition
                # rounds by at most u = 2^-24 of its partial sum, and n such errors add in quadrature to u rms(t) sqrt(sum i)
                # = 0.7 u n rms(t), i.e. about u sum|t_i| -- the bound, on the un-cancelled size of the sum (the worst case is
                # n times that)
                assert np.abs(wantg).max() <= 1e-12
                held("%s (%s), zero analytically" % (name, form), np.abs(got).max(), 2.0 ** -24 * grad_ref_terms(shape))
                continue
            scale = max(np.abs(wantg).max(), 1e-6)
            held("%s (%s)" % (name, form), np.abs(got - wantg).max() / scale, TOL_GRAD_REL)
    if route == "default" and ops.fused_layer_applies(spec, C, 3):
        _fused_layer(ops, spec, ref, src, cam, out, attn, corr)
        if (H, W, K) == (2, 2, 8):               # one partial tile for a whole persistent grid
            _fused_layer(ops, spec, ref[:1].contiguous(), src[:1].contiguous(), cam[:1].contiguous(), out[:1], attn[:1], corr[:1])


def _fused_layer(ops, spec, ref, src, cam, out, attn, corr):
    """et_epipolar_forward_fused against the separate forward + et_residual_gemm, at the bound of tests/test_gpu_fused.py."""
    g = torch.Generator().manual_seed(7)
    wf = (torch.randn(256, 256, generator=g) * 0.05 + torch.eye(256)).cuda()
    bias = torch.randn(256, generator=g).cuda()
    packed = ops.residual_gemm_pack(wf)
    want_x = ops.residual_gemm(out.contiguous(), packed, bias, ref)
    x, attn_f, corr_f = ops.forward_fused_nhwc(spec, ref, src, cam, packed, bias)
    assert torch.isfinite(x).all()
    assert torch.equal(attn_f, attn) and torch.equal(corr_f, corr)
    held("fused layer x (N=%d)" % ref.shape[0], (x - want_x).abs().max().item() / max(1.0, want_x.abs().max().item()), 2e-5)


def test_fused_layer_applies_at_the_small_256_channel_shapes(env):
    """Which of the shapes above the one-kernel layer takes (so that the test above cannot quietly stop covering it)."""
    _lib, camera, ops = env
    took = [s[:4] for s in SHAPES if s[2] == 256 and ops.fused_layer_applies(ops.LayerSpec(H=s[0], W=s[1], K=s[3], **layer_kwargs(s)), 256, 3)]
    assert (2, 2, 256, 8) in took and (3, 3, 256, 2) in took and (1, 9, 256, 6) in took
    assert (9, 1, 256, 6) not in took and (20, 24, 256, 256) not in took        # W < 2; K > 64


# =====================================================================================================================
# B. the general kernels at the ABI level
# =====================================================================================================================
GH, GW, GIMAGE = 6, 5, 24

# (K, c_sim, c_val, flags, with a grad_attn)
GENERAL_CASES = [
    (2, 1, 1, dict(pooling=True), False),                               # K' = 1
    (3, 3, 257, dict(), True),                                          # one channel past the first 256-channel trip
    (256, 512, 64, dict(), False),                                      # four sample slots and eight query slots, all full
    (256, 65, 1000, dict(pooling=True, prior="add"), False),            # K' = 128, four ragged output trips
    (150, 128, 4096, dict(cosine=True), False),                         # third sample slot partly filled, sixteen output trips
    # (its own camera seed: the one at which the float64 arg-max is clear outside exact ties, asserted in the test)
    (200, 448, 300, dict(attention_max=True, cam_seed=33), False),
    (256, 512, 512, dict(prior="mul"), False),
    (256, 64, 64, dict(softmax_enabled=False), True),
    (256, 16, 16, dict(pooling=True, prior="sim"), False),
]


def general_id(case):
    K, cs, cv, fl, ga = case
    return "K%d-cs%d-cv%d" % (K, cs, cv) + "".join("-%s%s" % (k, "" if v is True else v) for k, v in fl.items()) + ("-ga" if ga else "")


def _mode(fl):
    """The wrapper's keyword flags of a case."""
    return dict(pooling=bool(fl.get("pooling")), cosine=bool(fl.get("cosine")), attention_max=bool(fl.get("attention_max")),
                prior_mul=fl.get("prior") == "mul", sim_prior=fl.get("prior") == "sim")


def test_general_cases_fill_every_slot():
    """Pure Python over the parameter list: the union of cases reaches the eighth query slot, every count of sample slots and
    a second and a sixteenth trip of the output loop -- a later edit cannot quietly drop one."""
    ceil = lambda a, b: -(-a // b)
    ks = lambda c: c[0] // 2 if c[3].get("pooling") else c[0]
    assert max(ceil(c[1], 64) for c in GENERAL_CASES) == 8
    assert {ceil(ks(c), 64) for c in GENERAL_CASES} == {1, 2, 3, 4}
    assert {2, 16} <= {ceil(c[2], 256) for c in GENERAL_CASES}
    assert min(ks(c) for c in GENERAL_CASES) == 1 and min(c[1] for c in GENERAL_CASES) == 1 and min(c[2] for c in GENERAL_CASES) == 1
    assert sum(c[4] for c in GENERAL_CASES) >= 2
    combos = {tuple(sorted(_mode(c[3]).items())) + (c[3].get("prior") == "add", c[3].get("softmax_enabled", True)) for c in GENERAL_CASES}
    pinned = {tuple(sorted(_mode(f).items())) + (f.get("prior") == "add", f.get("softmax_enabled", True)) for f in PINNED_FLAGS}
    assert combos <= pinned, "a flag combination of the cases is not pinned to _attend_general_chunk"


PINNED_FLAGS = [dict(), dict(pooling=True), dict(pooling=True, prior="add"), dict(cosine=True), dict(attention_max=True),
                dict(prior="mul"), dict(softmax_enabled=False), dict(pooling=True, prior="sim")]


@pytest.mark.parametrize("fl", PINNED_FLAGS, ids=lambda f: "-".join("%s%s" % (k, "" if v is True else v) for k, v in f.items()) or "plain")
def test_general_restatement_is_pinned_to_the_module_restatement(env, fl):
    """Before use: in float64 the ABI-level restatement equals Epipolar._attend_general_chunk (pinned to the real reference's
    outputs by tests/test_gpu_modes.py) at a c_sim = c_val shape, once per flag combination of the cases below."""
    _lib, camera, ops = env
    from epipolar_transformers_amd import default_cfg, synthetic as syn
    from epipolar_transformers_amd.epipolar import Epipolar

    H, C, K, N = 6, 8, 8, 2
    prior = fl.get("prior")
    cfg = default_cfg()
    cfg.merge_from_list(["KEYPOINT.HEATMAP_SIZE", (H, H), "KEYPOINT.NFEATS", C, "EPIPOLAR.SAMPLESIZE", K,
                         "DATASETS.IMAGE_SIZE", (4 * H, 4 * H), "EPIPOLAR.USE_CORRECT_NORMALIZE", True,
                         "EPIPOLAR.ATTENTION", "max" if fl.get("attention_max") else "avg",
                         "EPIPOLAR.SIMILARITY", "cos" if fl.get("cosine") else ("prior" if prior == "sim" else "dot"),
                         "EPIPOLAR.PARAMETERIZED", ("z",), "EPIPOLAR.ZRESIDUAL", True, "EPIPOLAR.POOLING", bool(fl.get("pooling")),
                         "EPIPOLAR.PRIOR", prior is not None, "EPIPOLAR.PRIORMUL", prior == "mul",
                         "EPIPOLAR.SOFTMAX_ENABLED", fl.get("softmax_enabled", True), "DATASETS.CAMERAS", (0, 1, 2, 3)])
    torch.manual_seed(3)
    mod = Epipolar(cfg=cfg).cuda().eval().double()
    Ks = K // 2 if fl.get("pooling") else K
    if prior:
        mod.prior = {k: torch.nn.Parameter(torch.rand(Ks, H, H, device="cuda", dtype=torch.float64) * 0.5 + 0.05) for k in mod.prior}
    P1, P2 = syn.make_pairs(1, 4, 4 * H, seed=11, jitter=(0.05, 2.0))
    P1, P2 = P1[:N], P2[:N]
    g = torch.Generator().manual_seed(5)
    f1 = torch.randn(N, C, H, H, generator=g, dtype=torch.float64).cuda()
    f2 = torch.randn(N, C, H, H, generator=g, dtype=torch.float64).cuda()
    f2[:, :, 2, 3] = 0.0
    f1[:, :, 4, 1] = 0.0
    cams = torch.arange(N) % 4, (torch.arange(N) + 1) % 4
    real = ops.sample_locs
    ops.sample_locs = lambda *a, **k: real(*a, **k).double()
    try:
        with torch.no_grad():
            out_m, attn_m, corr_m = mod._attend_general_chunk(f1, f2, P1, P2, cams[0], cams[1])
    finally:
        ops.sample_locs = real
    spec = mod.layer_spec()
    locs = ops.sample_locs(spec, mod._cam(P1, P2, f1.device)).double()
    pr = torch.stack([mod.prior[(int(a), int(b))] for a, b in zip(*cams)]).detach() if prior else None
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    with torch.no_grad():
        args = (spec, nhwc(f1), nhwc(f2), nhwc(f2), locs, pr, _mode(fl))
        out_r, attn_r, corr_r, idx_r = general_restatement.attend(*args)
        # the module takes torch.argmax; where its choice is another member of the arg-max SET (general_restatement.near_maxima:
        # samples that see one source pixel have equal cosines to the last bit, and the two evaluations round them differently)
        # the restatement is evaluated at that member -- in float64 the set is held to 1e-12
        idx_m = attn_m.argmax(1)
        member = general_restatement.near_maxima(attn_r, 1e-12).gather(1, idx_m.unsqueeze(1)).squeeze(1)
        print("    arg-max differs at %d pixels, %d of them inside the arg-max set" % (int((idx_m != idx_r).sum()), int(((idx_m != idx_r) & member).sum())))
        out_r, attn_r, corr_r, _ = general_restatement.attend(*args, idx=torch.where(member, idx_m, idx_r))
    held("out vs the module's restatement", (out_r.permute(0, 3, 1, 2) - out_m).abs().max().item(), 1e-10)
    held("attn vs the module's restatement", (attn_r - attn_m).abs().max().item(), 1e-10)
    assert torch.equal(corr_r, corr_m)
    assert out_m.abs().max().item() > 1e-2 and tuple(attn_r.shape) == (N, Ks, H, H)


@pytest.mark.parametrize("case", GENERAL_CASES, ids=general_id)
def test_general_kernels_at_the_limits_vs_float64(env, case):
    """ops.forward_general_nhwc / backward_general_nhwc on 6 x 5 maps against the float64 restatement and autograd through it,
    at the project's tolerances for these kernels (tests/test_gpu_modes.py)."""
    _lib, camera, ops = env
    from epipolar_transformers_amd import synthetic as syn

    K, cs, cv, fl, with_ga = case
    N = 2
    mode = _mode(fl)
    is_max, prior_kind = mode["attention_max"], fl.get("prior")
    Ks = K // 2 if mode["pooling"] else K
    spec = ops.LayerSpec(H=GH, W=GW, K=K, softmax_enabled=fl.get("softmax_enabled", True))
    P1, P2 = syn.make_pairs(1, 4, GIMAGE, seed=fl.get("cam_seed", 17), jitter=(0.05, 1.0))
    cam = camera.pair_algebra(P1[:N], P2[:N]).cuda()
    g = torch.Generator().manual_seed(K * 7 + cs)
    q = torch.randn(N, GH, GW, cs, generator=g) * cs ** -0.25          # the similarity then has unit variance at every width
    m_sim = torch.randn(N, GH, GW, cs, generator=g) * cs ** -0.25
    m_val = torch.randn(N, GH, GW, cv, generator=g)
    gout = torch.randn(N, GH, GW, cv, generator=g)
    gattn = torch.randn(N, Ks, GH, GW, generator=g) if with_ga else None
    prior = (torch.rand(N, Ks, GH, GW, generator=g) * 0.5 + 0.05) if prior_kind else None
    m_sim[:, 2, 3] = 0.0                                               # an all-zero source pixel: exact-zero taps
    m_val[:, 2, 3] = 0.0
    q[:, 4, 1] = 0.0                                                   # an all-zero query pixel: masked everywhere
    dev = lambda t: None if t is None else t.cuda()
    q_d, sim_d, val_d, gout_d, gattn_d, prior_d = [dev(t) for t in (q, m_sim, m_val, gout, gattn, prior)]
    print("\n  %s" % general_id(case))
    out, attn, corr = ops.forward_general_nhwc(spec, q_d, sim_d, val_d, cam, prior=prior_d, **mode)
    grads = ops.backward_general_nhwc(spec, q_d, sim_d, val_d, cam, gout_d, prior=prior_d, need_prior=prior_kind is not None,
                                      grad_attn=gattn_d, **mode)
    again = ops.backward_general_nhwc(spec, q_d, sim_d, val_d, cam, gout_d, prior=prior_d, need_prior=prior_kind is not None,
                                      grad_attn=gattn_d, **mode)
    # the float64 restatement at the (float32, bit-exact) locations of the geometry kernel, widened
    locs32 = ops.sample_locs(spec, cam)
    leaf = lambda t: None if t is None else t.cuda().double().requires_grad_(True)
    q64, sim64, val64, prior64 = leaf(q), leaf(m_sim), leaf(m_val), leaf(prior)
    rargs = (spec, q64, sim64, val64, locs32.double(), prior64, mode)
    locs_np = locs32.cpu().numpy()
    den = denormalized_locations(locs_np, GH, GW, True)                                                           # (K,N,H,W,2)
    idx, swapped = None, 0
    if is_max:
        # ATTENTION max gathers the arg-max sample, so `out` and the gradients hang on WHICH maximum is taken.  Samples that see one
        # source pixel only (beyond the outermost pixel centres in both directions) carry multiples of one vector: their cosines
        # are EQUAL, to 1e-12 in float64, and which of them float32 rounding prefers is not the operator's business.  Stated for
        # the restatement alone, before the kernel's answer is looked at: outside those exact ties the float64 arg-max is clear (no
        # other sample within the 2e-6 tie tolerance of it -- what the case's camera seed was chosen for), and at most 2 of
        # the 60 pixels have an exact tie.  At those pixels, and no others, the restatement is evaluated at the member of the
        # exact set the kernel took.  All that remains goes through assert_corr_pos as for every other case.
        with torch.no_grad():
            attn_0, idx0 = general_restatement.attend(*rargs, absorb=torch.float32)[1::2]
        exact = general_restatement.near_maxima(attn_0, 1e-12)                                                     # (N,K',H,W)
        flat = exact.all(1)                                         # (all-zero query / no epipolar line: every cosine is 0)
        runner_up = torch.where(exact, torch.full_like(attn_0, -2.0), attn_0).amax(1)
        assert ((attn_0.amax(1) - runner_up)[~flat] > 2e-6).all(), "the float64 arg-max is not clear outside exact ties"
        tied = (exact.sum(1) > 1) & ~flat
        assert int(tied.sum()) <= 2, "more exact arg-max ties than stated"
        at_corr = (torch.from_numpy(den[:Ks]).cuda().permute(1, 0, 2, 3, 4) == corr.unsqueeze(1)).all(-1)
        took = at_corr & exact & tied.unsqueeze(1)
        first = torch.where(took, torch.arange(Ks, device="cuda").view(1, -1, 1, 1), Ks).amin(1)
        idx = torch.where(took.any(1), first, idx0)
        swapped = int((idx != idx0).sum())
        print("    exact arg-max ties at %d of %d pixels; the kernel took another member at %d" % (int(tied.sum()), idx.numel(), swapped))
        assert swapped <= int(tied.sum())
    out_r, attn_r, _, idx = general_restatement.attend(*rargs, absorb=torch.float32, idx=idx)
    loss = (out_r * gout_d.double()).sum()
    if with_ga:
        loss = loss + (attn_r * gattn_d.double()).sum()
    loss.backward()
    assert tuple(out.shape) == (N, GH, GW, cv) and tuple(attn.shape) == (N, Ks, GH, GW)
    assert torch.isfinite(out).all() and torch.isfinite(attn).all() and torch.isfinite(corr).all()
    # attn <= 1e-5 max(1, |attn|) element by element and out <= 1e-4 max(1, |out|) with the pixel's own largest |out|: with the
    # soft-max off the all-masked query pixel carries weights of -1e10 / K', and a bound scaled by the TENSOR's maximum would
    # hold every other pixel to nothing
    held("attn", ((attn.double() - attn_r).abs() / attn_r.abs().clamp_min(1.0)).max().item(), 1e-5)
    # corr_pos: the float32 de-normalisation of the arg-max sample's location; a difference must be a proven tie in the kernel's
    # own weights, within the budget
    want_corr = np.take_along_axis(den, idx.cpu().numpy()[None, ..., None], 0)[0]
    ties = assert_corr_pos(locs_np, corr.cpu().numpy(), want_corr, attn.cpu().numpy(), True, tie=2e-6, max_frac=2e-2)
    ties = torch.from_numpy(ties).cuda()
    err_out = (out.double() - out_r).abs().amax(-1) / out_r.abs().amax(-1).clamp_min(1.0)       # (N,H,W)
    if is_max:                                   # a proven tie gathers the other, equally good sample: those pixels only are exempt
        err_out = err_out[~ties]
    held("out", err_out.max().item(), 1e-4)
    names = ["grad_q", "grad_map_sim", "grad_map_val", "grad_prior"]
    wants = [q64.grad, sim64.grad, val64.grad, None if prior64 is None else prior64.grad]
    for name, got, want_g, like in zip(names, grads, wants, (q_d, sim_d, val_d, prior_d)):
        if got is None:
            assert name == "grad_prior" and prior_kind is None
            continue
        want_g = torch.zeros_like(like, dtype=torch.float64) if want_g is None else want_g
        assert torch.isfinite(got).all(), name
        err = (got.double() - want_g).abs()
        scale = max(want_g.abs().max().item(), 1e-6)
        if is_max and ties.any():
            # a pixel that took the other sample of a proven tie sends its whole gradient there: its own grad_q row is exempt,
            # and of a map's gradient the share of entries off by more than the bound is held as
            # tests/test_gpu_modes.py::test_option_branch_gradients_vs_torch_restatement holds it
            flipped = ties.float().mean().item()
            if name == "grad_q":
                err = err[~ties]
            else:
                bad = (err > 2e-4 * scale).float().mean().item()
                held("%s: share of entries off (%d tie pixels)" % (name, int(ties.sum())), bad, 5e-3 + 40 * flipped)
                continue
        held(name, err.max().item() / scale, 2e-4)
    assert torch.equal(grads[0], again[0]), "grad_q is written by one wave per pixel: bit-equal on a second call"
    if prior_kind:
        assert torch.equal(grads[3], again[3]), "grad_prior is written by one wave per pixel: bit-equal on a second call"
        if not (prior_kind == "mul" and not spec.softmax_enabled):
            assert grads[3].abs().max().item() > 0
    # the case is not empty: the attention is not uniform, the output is there
    assert out_r.abs().max().item() > 1e-2
    if Ks > 1 and not is_max and prior_kind != "sim":
        spread = (attn_r - attn_r.mean(1, keepdim=True)).abs().amax(1) / attn_r.abs().amax(1)         # relative to the pixel's largest weight
        assert (spread > 1e-2).float().mean().item() >= 0.4


# =====================================================================================================================
# C. the lifting kernels
# =====================================================================================================================
RPSM = dict(image_size=(256, 256), grid_size=900, first_nbins=4, recur_nbins=2, recur_depth=3, tolerance=150.0)
PARENT_32 = rpsm_restate.H36M_PARENT + (16, 17, 18, 3, 20, 21, 6, 23, 24, 10, 26, 13, 28, 29, 30)


def _rpsm(sc, params, parent=None):
    from epipolar_transformers_amd import ops

    J = sc["heat"].shape[2]
    return ops.rpsm(*[torch.from_numpy(sc[k]).cuda() for k in rpsm_restate.ARRAYS],
                    parent=rpsm_restate.H36M_PARENT[:J] if parent is None else parent, want_path=True, **params)


def _rpsm_equals(sc, params, restated, parent=None):
    pose, path, margins, band = restated
    assert rpsm_restate.condition_holds(margins, band)       # every decision on the path is clear: the bins must be the restatement's
    X, p = _rpsm(sc, params, parent)
    F, J = sc["heat"].shape[0], sc["heat"].shape[2]
    assert X.dtype == torch.float32 and tuple(X.shape) == (F, J, 3)
    assert p.dtype == torch.int32 and tuple(p.shape) == (F, 1 + params["recur_depth"], J)
    X = X.cpu().numpy()
    assert np.isfinite(X).all()
    assert np.array_equal(p.cpu().numpy(), path)
    held("pose vs restatement (mm)", np.abs(X - pose).max(), TOLERANCE_MM)
    return X, p.cpu().numpy()


def test_rpsm_one_joint(env):
    """J = 1: no limb, limb_length is (F, 0), no message launch -- the root's arg-max and its refinement alone."""
    sc, restated = rpsm_restate.scene(201, 2, 3, 1, 16, 20, RPSM)
    assert sc["limb_length"].shape == (2, 0)
    _rpsm_equals(sc, RPSM, restated)


def test_rpsm_depth_zero(env):
    """recur_depth = 0: the first stage's bin centres are the pose, path is (F, 1, J)."""
    params = dict(RPSM, recur_depth=0)
    sc, restated = rpsm_restate.scene(202, 2, 3, 5, 16, 20, params)
    X, p = _rpsm_equals(sc, params, restated)
    assert p.shape == (2, 1, 5)


def test_rpsm_align_corners(env):
    params = dict(RPSM, align_corners=True)
    sc, restated = rpsm_restate.scene(203, 2, 4, 9, 18, 22, params)
    _rpsm_equals(sc, params, restated)
    # the setting matters on this scene: without it the sampling differs
    other = rpsm_restate.run(sc, dict(params, align_corners=False))
    assert np.abs(other[0] - restated[0]).max() > 0


def test_rpsm_any_tree_on_the_device(env):
    """tests/test_rpsm_cpu.py::test_host_hook_takes_any_tree on the device path (one launch per tree level over by_level /
    level_begin): a root that is not joint 0 and children listed before their parents; the same scene, relabelled."""
    params = dict(RPSM, recur_depth=3)
    sc, (pose, path, margins, band) = rpsm_restate.scene(77, 1, 3, 5, 16, 16, params)
    perm = [4, 2, 0, 3, 1]                                   # new label of old joint j
    old_parent = rpsm_restate.H36M_PARENT[:5]
    new_parent = [0] * 5
    for j, p in enumerate(old_parent):
        new_parent[perm[j]] = -1 if p < 0 else perm[p]
    assert new_parent.index(-1) != 0 and any(new_parent[j] > j for j in range(5))
    inv = np.argsort(perm)                                   # old joint at each new label
    relabelled = dict(sc, heat=np.ascontiguousarray(sc["heat"][:, :, inv]))
    ends = [j for j in range(5) if new_parent[j] >= 0]       # limb e ends at the e-th non-root joint in ascending NEW order
    relabelled["limb_length"] = np.ascontiguousarray(np.stack([sc["limb_length"][:, inv[j] - 1] for j in ends], 1))
    restated = rpsm_restate.run(relabelled, params, parent=new_parent)
    assert np.array_equal(restated[1][:, :, perm], path) and np.abs(restated[0][:, perm] - pose).max() <= 1e-9
    X, p = _rpsm_equals(relabelled, params, restated, parent=new_parent)
    base, base_path = _rpsm(sc, params)
    assert np.array_equal(X[:, perm], base.cpu().numpy()) and np.array_equal(p[:, :, perm], base_path.cpu().numpy())


def test_rpsm_thirty_two_joints(env):
    """J = 32, the most the entry point admits: H36M plus fifteen joints hanging off its leaves and limbs."""
    params = dict(RPSM, grid_size=1200)
    assert len(PARENT_32) == 32
    sc, restated = rpsm_restate.scene(204, 1, 4, 32, 24, 24, params, parent=PARENT_32)
    assert sc["limb_length"].shape == (1, 31)
    _rpsm_equals(sc, params, restated, parent=PARENT_32)


def test_rpsm_depth_sixteen(env):
    """recur_depth = 16, the most the entry point admits, on the frame and under the k* rule of
    tests/test_gpu_rpsm.py::test_config_defaults_depth_10: the deep levels are decided at float32 rounding, so the bins must
    agree up to the first level k* whose margin in the float64 restatement is below 1e-4 (measured: level 6) and the pose within
    sqrt(3) x that level's grid size.  New here: half[11..16] and path rows 11..16, every entry a bin of the 2 x 2 x 2 grid."""
    from epipolar_transformers_amd import default_cfg

    ps = default_cfg().PICT_STRUCT
    params = dict(image_size=(256, 256), grid_size=ps.GRID_SIZE, first_nbins=ps.FIRST_NBINS, recur_nbins=ps.RECUR_NBINS,
                  recur_depth=16, tolerance=float(ps.LIMB_LENGTH_TOLERANCE))
    fr = rpsm_restate.frame(2024, 4, 17, 32, 32)
    sc = {k: np.ascontiguousarray(fr[k][None]) for k in rpsm_restate.ARRAYS}
    pose, path, margins, band = rpsm_restate.run(sc, params)
    close = np.nonzero(margins[0] < rpsm_restate.MARGIN)[0]
    k_star = int(close[0]) if close.size else 17
    X, p = _rpsm(sc, params)
    X, p = X.cpu().numpy(), p.cpu().numpy()
    print("margins", margins[0], "k* =", k_star)
    assert p.shape == (1, 17, 17) and np.isfinite(X).all()
    assert np.array_equal(p[0, :k_star], path[0, :k_star])
    assert (p[0, 0] >= 0).all() and (p[0, 0] < params["first_nbins"] ** 3).all()
    assert (p[0, 1:] >= 0).all() and (p[0, 1:] < params["recur_nbins"] ** 3).all()
    bound = TOLERANCE_MM if k_star == 17 else np.sqrt(3.0) * rpsm_restate.level_size(params["grid_size"], 16, 2, k_star)
    held("pose vs restatement (mm)", np.linalg.norm(X[0] - pose[0], axis=1).max(), bound)


@pytest.mark.parametrize("shape", [(3, 1, 5), (2, 1, 1)], ids=lambda s: "F%d_V%d_J%d" % s)
def test_triangulate_epipolar_one_view(env, shape):
    """V = 1: no pair of views, so every joint is solved from its one view and that view's correspondence (branch 1: confident,
    branch 2: not), whatever `dlt` says."""
    _lib, camera, ops = env
    kw = dict(downsample=64.0, resize=1.0, conf_thres=0.85, ransac_thres=35.0)
    arrays, truth = tri_restate.random_scene(*shape, seed=sum(shape))
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    for dlt in (False, True):
        Xr, info_r, margin = tri_restate.triangulate_epipolar(*arrays, dlt=dlt, **kw)
        assert margin == np.inf and set(((info_r >> 16) & 3).ravel().tolist()) <= {1, 2}
        X, info = ops.triangulate_epipolar(*dev, dlt=dlt, want_info=True, **kw)
        assert X.dtype == torch.float64 and tuple(X.shape) == (shape[0], shape[2], 3)
        X = X.cpu().numpy()
        assert np.isfinite(X).all()
        assert np.array_equal(info.cpu().numpy(), info_r)
        ok, worst = within_tolerance(X, Xr, truth)
        print(shape, "dlt=%d kernel vs restatement: worst err / bound %.3g" % (dlt, worst))
        assert ok, worst
