"""Pairs named by index into one stack of feature maps (ET_HAS_PAIR_INDEX: the *_ix entry points, the ref_index / src_index
arguments of ops.forward_nhwc / forward_fused_nhwc / backward_nhwc, ops.EpipolarAttendIndexed, EPIPOLAR_AMD.PAIR_INDEX).

Every case: C = 256, a pool of M = 4 maps of 12 x 20, K = 16, N = 6 pairs, ref_index = [0,1,2,3,0,3], src_index = [1,2,3,0,2,2]
(one map three times, order not monotone) unless it says otherwise.  The cameras are six pairs of the ring rig
(synthetic.rig_pairs); they belong to the PAIRS, whichever maps a pair names.

  forward / fused layer   the indexed call equals the same call on pool[index] copies BIT FOR BIT (same arithmetic, other
                          addresses) -- after two runs of the gathered call were found equal, so that run-to-run noise is ruled out;
  tile backward           against float64 index_add of the oracle's per-pair d(feat_src) (oracle.backward; the grad_attn term:
                          float64 autograd through oracle.torch_ref_path, the reference of tests/test_gpu_attn_grad.py) at
                          TOL_GRAD_REL = 1e-4 of each tensor's largest magnitude (tests/test_gpu_rigs.py), the gathered route +
                          float64 index_add held to the same bound as a control;
  autograd, model         the gathered formulation at the same bound / torch.equal, the saved tensors and the memory peak.
No case hands a kernel an index outside its pool (the host checks: tests/test_pair_index_cpu.py)."""
import numpy as np
import pytest
import torch

from test_gpu_rigs import TOL_GRAD_REL

pytestmark = pytest.mark.gpu

C, M, H, W, K, N = 256, 4, 12, 20, 16, 6
REF_INDEX = [0, 1, 2, 3, 0, 3]
SRC_INDEX = [1, 2, 3, 0, 2, 2]
SRC_INDEX_UNUSED = [1, 1, 3, 0, 1, 3]           # map 2 is nobody's source

_cache = {}


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from epipolar_transformers_amd import _lib, camera, ops

    _lib.load()
    assert ops.POISON_OUTPUTS
    return _lib, camera, ops


def _inputs(camera, h=H, w=W):
    """The pools (NCHW on the host), the six pairs' algebra, G and GA: seeded, made once per map size, never modified."""
    key = ("inputs", h, w)
    if key not in _cache:
        from epipolar_transformers_amd import synthetic as syn

        P1, P2 = syn.rig_pairs("ring", 2, 4 * max(h, w), seed=31, jitter=(0.05, 8.0))
        cam = camera.pair_algebra(P1[:N], P2[:N])
        f1, f2 = syn.make_features(M, C, h, w, seed=32)
        f1[0, :, h // 2, w // 3] = 0                      # an all-masked reference pixel, a partly masked source patch
        f2[:, :, h // 3:h // 3 + 2, w // 2:w // 2 + 2] = 0
        gen = torch.Generator().manual_seed(33)
        _cache[key] = dict(f1=f1, f2=f2, cam=cam, G=torch.randn(N, C, h, w, generator=gen))
    return _cache[key]


def _device(ops, case, same_pool=False):
    ref = ops.to_nhwc(case["f1"].cuda())
    src = ref if same_pool else ops.to_nhwc(case["f2"].cuda())
    return ref, src, case["cam"].cuda()


def _gathered(pool, index):
    return pool[torch.tensor(index, device=pool.device)].contiguous()


def _equal(what, a, b):
    for name, x, y in zip(("first", "attn", "corr_pos"), a, b):
        assert torch.isfinite(x).all() or name == "corr_pos", (what, name)
        assert torch.equal(x, y), (what, name, float((x - y).abs().max()))


# ---- 1. forward, bit for bit -----------------------------------------------------------------------------------------------
def _variants(_lib):
    return {"default": {}, "ws-band": dict(variant=_lib.ET_VARIANT_WS_BAND), "tile-classic": dict(variant=_lib.ET_VARIANT_TILE_CLASSIC),
            "tile-exact": dict(variant=_lib.ET_VARIANT_TILE_EXACT),
            "tile-classic-exact": dict(variant=_lib.ET_VARIANT_TILE_CLASSIC | _lib.ET_VARIANT_TILE_EXACT),
            "tile-split": dict(variant=_lib.ET_VARIANT_TILE_SPLIT), "softmax-off": dict(softmax_enabled=False),
            "K80": dict(K=80), "K130": dict(K=130), "8x72": dict(H=8, W=72)}


FORWARD_CASES = ["default", "ws-band", "tile-classic", "tile-exact", "tile-classic-exact", "tile-split", "softmax-off", "K80", "K130",
                 "8x72", "default-one-pool"]


@pytest.mark.parametrize("name", FORWARD_CASES)
def test_forward_indexed_equals_gathered_bit_for_bit(env, name):
    _lib, camera, ops = env
    same_pool = name.endswith("-one-pool")
    kw = dict(dict(H=H, W=W, K=K), **_variants(_lib)[name.replace("-one-pool", "")])
    spec = ops.LayerSpec(**kw)
    assert ops.pair_index_applies(spec, C, "forward")
    ref, src, cam = _device(ops, _inputs(camera, kw["H"], kw["W"]), same_pool)
    g_ref, g_src = _gathered(ref, REF_INDEX), _gathered(src, SRC_INDEX)
    first = ops.forward_nhwc(spec, g_ref, g_src, cam)
    again = ops.forward_nhwc(spec, g_ref, g_src, cam)
    _equal(name + ": two gathered runs", first, again)
    got = ops.forward_nhwc(spec, ref, src, cam, ref_index=REF_INDEX, src_index=torch.tensor(SRC_INDEX))
    torch.cuda.synchronize()
    assert tuple(got[0].shape) == (N, kw["H"], kw["W"], C)
    _equal(name + ": indexed vs gathered", got, first)
    # one index alone: the other operand holds a map per pair
    half = ops.forward_nhwc(spec, g_ref, src, cam, src_index=SRC_INDEX)
    _equal(name + ": src_index alone", half, first)
    half = ops.forward_nhwc(spec, ref, g_src, cam, ref_index=REF_INDEX)
    _equal(name + ": ref_index alone", half, first)


def test_forward_res_base_reads_the_reference_pool_through_the_index(env):
    _lib, camera, ops = env
    spec = ops.LayerSpec(H=H, W=W, K=K)
    ref, src, cam = _device(ops, _inputs(camera))
    bias = torch.randn(C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    want = ops.forward_nhwc(spec, _gathered(ref, REF_INDEX), _gathered(src, SRC_INDEX), cam, res_bias=bias, want_res_base=True)
    got = ops.forward_nhwc(spec, ref, src, cam, res_bias=bias, want_res_base=True, ref_index=REF_INDEX, src_index=SRC_INDEX)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_fallback_routes_give_the_gathered_result(env):
    """What the indexed kernels do not take runs on gathered maps inside the same call: the per-pixel kernels (NO_TILE), C != 256,
    and an index that lives on the device (never read on the host)."""
    _lib, camera, ops = env
    ref, src, cam = _device(ops, _inputs(camera))
    g_ref, g_src = _gathered(ref, REF_INDEX), _gathered(src, SRC_INDEX)
    spec = ops.LayerSpec(H=H, W=W, K=K, variant=_lib.ET_VARIANT_NO_TILE)
    _equal("per-pixel", ops.forward_nhwc(spec, ref, src, cam, ref_index=REF_INDEX, src_index=SRC_INDEX),
           ops.forward_nhwc(spec, g_ref, g_src, cam))
    spec = ops.LayerSpec(H=H, W=W, K=K)
    r8, s8 = ref[..., :8].contiguous(), src[..., :8].contiguous()
    _equal("C = 8", ops.forward_nhwc(spec, r8, s8, cam, ref_index=REF_INDEX, src_index=SRC_INDEX),
           ops.forward_nhwc(spec, _gathered(r8, REF_INDEX), _gathered(s8, SRC_INDEX), cam))
    _equal("device index", ops.forward_nhwc(spec, ref, src, cam, ref_index=torch.tensor(REF_INDEX, device="cuda"),
                                            src_index=torch.tensor(SRC_INDEX, device="cuda", dtype=torch.int32)),
           ops.forward_nhwc(spec, g_ref, g_src, cam))


# ---- 2. the one-kernel layer, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "ws-band", "tile-split"])
def test_fused_layer_indexed_equals_gathered_bit_for_bit(env, name):
    """tile-split: 64-row tiles, so that tiles go to the left-over list and their x rows come from et_internal_residual_rows_list,
    whose feat row is read through ref_index."""
    _lib, camera, ops = env
    spec = ops.LayerSpec(H=H, W=W, K=K, **_variants(_lib)[name])
    assert ops.pair_index_applies(spec, C, "fused")
    ref, src, cam = _device(ops, _inputs(camera))
    g = torch.Generator(device="cuda").manual_seed(7)
    wf = torch.randn(C, C, device="cuda", generator=g) * 0.05 + torch.eye(C, device="cuda")
    bf = torch.randn(C, device="cuda", generator=g) * 0.1
    packed = ops.residual_gemm_pack(wf)
    g_ref, g_src = _gathered(ref, REF_INDEX), _gathered(src, SRC_INDEX)
    ws = ops.tile_workspace(spec, N, C, ref.device)
    first = ops.forward_fused_nhwc(spec, g_ref, g_src, cam, packed, bf, workspace=ws)
    left_over = int(ws[(-ws.data_ptr()) % 256:][:4].view(torch.int32).item())
    again = ops.forward_fused_nhwc(spec, g_ref, g_src, cam, packed, bf, workspace=ws)
    _equal(name + ": two gathered runs", first, again)
    got = ops.forward_fused_nhwc(spec, ref, src, cam, packed, bf, workspace=ws, ref_index=REF_INDEX, src_index=SRC_INDEX)
    torch.cuda.synchronize()
    ops.check_tile_errors(workspace=ws)
    _equal(name + ": indexed vs gathered", got, first)
    if name == "tile-split":
        assert left_over > 0, "the case must reach the left-over list"
    # with `out` on request
    want4 = ops.forward_fused_nhwc(spec, g_ref, g_src, cam, packed, bf, want_out=True)
    got4 = ops.forward_fused_nhwc(spec, ref, src, cam, packed, bf, want_out=True, ref_index=REF_INDEX, src_index=SRC_INDEX)
    assert all(torch.equal(a, b) for a, b in zip(got4, want4))


# ---- 3. tile backward ------------------------------------------------------------------------------------------------------
def _oracle_case(oracle_mod, camera, k, src_index, with_ga=False):
    """float64 references for K = k and a source table: want_ref (N maps), want_src (M maps, index_add of the per-pair gradient) of
    the G term (oracle.backward) and, on request, of the GA term (float64 autograd through oracle.torch_ref_path); computed once,
    shared."""
    key = ("oracle", k, tuple(src_index), with_ga)
    if key in _cache:
        return _cache[key]
    from oracle import torch_ref_path as trp

    case = _inputs(camera)
    f1, f2 = case["f1"][REF_INDEX].contiguous(), case["f2"][src_index].contiguous()
    so = oracle_mod.LayerSpec(H, W, k)
    with np.errstate(all="ignore"):
        fwd = oracle_mod.forward(so, f1, f2, None, None, cam=case["cam"].numpy())
        g1, g2 = oracle_mod.backward(so, f1.numpy(), f2.numpy(), fwd["sample_locs"], case["G"].numpy())
    idx = torch.tensor(src_index)
    add = lambda t: torch.zeros(M, C, H, W, dtype=torch.float64).index_add_(0, idx, torch.as_tensor(t).double()).numpy()
    _cache[key] = dict(want_ref=np.asarray(g1, np.float64), want_src=add(g2))
    if with_ga:
        GA = torch.randn(N, k, H, W, generator=torch.Generator().manual_seed(34 + k))
        a, b = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
        _, attn, _ = trp.forward(a, b, torch.from_numpy(fwd["sample_locs"]).double(), softmax_scale=0.125)
        a1, a2 = torch.autograd.grad((attn * GA.double()).sum(), (a, b))
        assert float(a2.abs().max()) > 0, "the attention term must carry a gradient"
        _cache[key].update(GA=GA, ga_ref=a1.numpy(), ga_src=add(a2))
    return _cache[key]


def _close(what, got, want):
    got = got.permute(0, 3, 1, 2).double().cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all(), what
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max())
    print("%s: max error %.3g of %.3g (bound %.3g)" % (what, err, scale, TOL_GRAD_REL * scale))
    assert err <= TOL_GRAD_REL * scale, (what, err, scale)


def _backward_case(env, oracle_mod, kw, with_attn, with_ga=False, src_index=SRC_INDEX):
    _lib, camera, ops = env
    spec = ops.LayerSpec(**dict(dict(H=H, W=W, K=K), **kw))
    assert ops.pair_index_applies(spec, C, "tile")
    case = _inputs(camera)
    want = _oracle_case(oracle_mod, camera, spec.K, src_index, with_ga)
    ref, src, cam = _device(ops, case)
    g = ops.to_nhwc(case["G"].cuda())
    ga = want["GA"].cuda() if with_ga else None
    want_ref = want["want_ref"] + (want["ga_ref"] if with_ga else 0)
    want_src = want["want_src"] + (want["ga_src"] if with_ga else 0)
    g_ref, g_src = _gathered(ref, REF_INDEX), _gathered(src, src_index)
    attn = ops.forward_nhwc(spec, g_ref, g_src, cam)[1] if with_attn else None
    # control: the gathered route + float64 index_add meets the bound
    c_ref, c_src = ops.backward_nhwc(spec, g_ref, g_src, cam, g, form="tile", attn=attn, grad_attn=ga)
    c_pool = torch.zeros(M, H, W, C, dtype=torch.float64, device="cuda").index_add_(0, torch.tensor(src_index, device="cuda"), c_src.double())
    _close("control d(feat_ref)", c_ref, want_ref)
    _close("control d(pool_src)", c_pool, want_src)
    gr, gs = ops.backward_nhwc(spec, ref, src, cam, g, form="tile", attn=attn, grad_attn=ga, ref_index=REF_INDEX, src_index=src_index)
    torch.cuda.synchronize()
    assert tuple(gr.shape) == (N, H, W, C) and tuple(gs.shape) == (M, H, W, C)
    _close("indexed d(feat_ref)", gr, want_ref)
    _close("indexed d(pool_src)", gs, want_src)
    return gs


def _backward_variants(_lib):
    return {"merged": {}, "tile-classic": dict(variant=_lib.ET_VARIANT_TILE_CLASSIC), "tile-split": dict(variant=_lib.ET_VARIANT_TILE_SPLIT),
            "split-in-place": dict(variant=_lib.ET_VARIANT_BWD_SPLIT_IN_PLACE), "K80": dict(K=80)}


@pytest.mark.parametrize("with_attn", [False, True], ids=["recompute", "forward-attn"])
@pytest.mark.parametrize("name", ["merged", "tile-classic", "tile-split", "split-in-place", "K80"])
def test_tile_backward_indexed_vs_float64(env, oracle_mod, name, with_attn):
    _backward_case(env, oracle_mod, _backward_variants(env[0])[name], with_attn)


@pytest.mark.parametrize("with_attn", [False, True], ids=["recompute", "forward-attn"])
def test_tile_backward_indexed_with_grad_attn(env, oracle_mod, with_attn):
    _backward_case(env, oracle_mod, {}, with_attn, with_ga=True)


def test_tile_backward_leaves_an_unnamed_source_map_exactly_zero(env, oracle_mod):
    """Outputs start as NaN under test (ops.POISON_OUTPUTS): map 2, which no pair names, must have been cleared and not touched."""
    assert 2 not in SRC_INDEX_UNUSED
    gs = _backward_case(env, oracle_mod, {}, True, src_index=SRC_INDEX_UNUSED)
    assert int(torch.count_nonzero(gs[2])) == 0 and bool((gs[2] == 0).all())
    assert float(gs[1].abs().max()) > 0


def test_backward_forms_without_an_indexed_kernel_reduce_into_the_pool(env, oracle_mod):
    """gather / atomic / tile_det: the gathered route inside the same call, d(src) over the source pool."""
    _lib, camera, ops = env
    case = _inputs(camera)
    want = _oracle_case(oracle_mod, camera, K, SRC_INDEX)
    ref, src, cam = _device(ops, case)
    g = ops.to_nhwc(case["G"].cuda())
    for form in ("gather", "atomic", "tile_det"):
        gr, gs = ops.backward_nhwc(ops.LayerSpec(H=H, W=W, K=K), ref, src, cam, g, form=form, ref_index=REF_INDEX, src_index=SRC_INDEX)
        _close(form + " d(feat_ref)", gr, want["want_ref"])
        _close(form + " d(pool_src)", gs, want["want_src"])


# ---- 4. autograd -------------------------------------------------------------------------------------------------------------
def test_autograd_one_shared_pool(env):
    _lib, camera, ops = env
    case = _inputs(camera)
    spec = ops.LayerSpec(H=H, W=W, K=K)
    cam, G = case["cam"].cuda(), case["G"].cuda()
    base = case["f1"].cuda().contiguous(memory_format=torch.channels_last)
    want_pool = base.clone().requires_grad_(True)
    ri, si = torch.tensor(REF_INDEX, device="cuda"), torch.tensor(SRC_INDEX, device="cuda")
    out, _, _ = ops.EpipolarAttend.apply(want_pool[ri], want_pool[si], cam, spec)
    (out * G).sum().backward()
    pool = base.clone().requires_grad_(True)
    got, attn, corr = ops.EpipolarAttendIndexed.apply(pool, pool, cam, spec, REF_INDEX, SRC_INDEX)
    assert torch.equal(got, out) and not attn.requires_grad and not corr.requires_grad
    node = got.grad_fn
    while node is not None and not hasattr(node, "saved_tensors"):
        node = node.next_functions[0][0]
    saved = node.saved_tensors
    assert len(saved) == 4 and type(node).__name__.startswith("EpipolarAttendIndexed")
    for t in saved:                 # the pools, the cameras, the attention: nothing of N maps
        assert t.numel() != N * H * W * C and not (t.dim() == 4 and t.shape[0] == N and t.shape[-1] == C), tuple(t.shape)
    assert sum(t.numel() == M * H * W * C for t in saved) == 2 and saved[0].data_ptr() == saved[1].data_ptr() == pool.data_ptr()
    (got * G).sum().backward()
    torch.cuda.synchronize()
    w = want_pool.grad.double()
    scale = float(w.abs().max())
    err = float((pool.grad.double() - w).abs().max())
    print("pool.grad: max error %.3g of %.3g (bound %.3g)" % (err, scale, TOL_GRAD_REL * scale))
    assert tuple(pool.grad.shape) == (M, C, H, W) and scale > 0 and err <= TOL_GRAD_REL * scale


def test_autograd_two_pools_and_a_loss_on_the_attention(env):
    _lib, camera, ops = env
    case = _inputs(camera)
    spec = ops.LayerSpec(H=H, W=W, K=K)
    cam, G = case["cam"].cuda(), case["G"].cuda()
    GA = torch.randn(N, K, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    ri, si = torch.tensor(REF_INDEX, device="cuda"), torch.tensor(SRC_INDEX, device="cuda")
    grads = []
    for indexed in (False, True):
        a = case["f1"].cuda().requires_grad_(True)
        b = case["f2"].cuda().requires_grad_(True)
        if indexed:
            out, attn, _ = ops.EpipolarAttendIndexed.apply(a, b, cam, spec, REF_INDEX, SRC_INDEX, True)
        else:
            out, attn, _ = ops.EpipolarAttend.apply(a[ri], b[si], cam, spec, True)
        ((out * G).sum() + (attn * GA).sum()).backward()
        grads.append((a.grad.double(), b.grad.double()))
    for got, want in zip(grads[1], grads[0]):
        assert float((got - want).abs().max()) <= TOL_GRAD_REL * float(want.abs().max())


# ---- 5. model ----------------------------------------------------------------------------------------------------------------
def _model(**over):
    from epipolar_transformers_amd import default_cfg
    from epipolar_transformers_amd.model import MultiViewPoseModel

    size, hs = 64, 16
    cfg = default_cfg()
    cfg.merge_from_list(["BACKBONE.BODY", "epipolarposeR-18", "BACKBONE.PRETRAINED", False, "DATASETS.TASK", "multiview_keypoint",
                         "KEYPOINT.HEATMAP_SIZE", (hs, hs), "KEYPOINT.NUM_PTS", 17, "KEYPOINT.SIGMA", 2.0,
                         "DATASETS.IMAGE_SIZE", (size, size), "EPIPOLAR.MERGE", "late", "EPIPOLAR.ATTENTION", "avg",
                         "EPIPOLAR.PARAMETERIZED", ("z",), "EPIPOLAR.ZRESIDUAL", True, "EPIPOLAR.USE_CORRECT_NORMALIZE", True,
                         "EPIPOLAR.SAMPLESIZE", 16, "VIS.MULTIVIEW", True])
    for k, v in over.items():
        cfg.merge_from_list([k, v])
    torch.manual_seed(11)
    m = MultiViewPoseModel(cfg).cuda().eval()
    with torch.no_grad():
        m.reference.epipolar_sampler.bn.weight.normal_(1, 0.1)
        m.reference.epipolar_sampler.bn.bias.normal_(0, 0.1)
        m.reference.final_layer.weight.mul_(30.0)        # (a random-initialised head is nearly flat: give it contrast)
    return m, cfg, size


class _Calls:
    """The library exports ops calls, by name, while the block runs."""

    def __enter__(self):
        from epipolar_transformers_amd import ops

        self.ops, self.real, self.names = ops, ops._call, []

        def spy(name, on, *args):
            self.names.append(name)
            return self.real(name, on, *args)

        ops._call = spy
        return self.names

    def __exit__(self, *exc):
        self.ops._call = self.real


@pytest.mark.parametrize("share", [True, False], ids=["one-network", "two-networks"])
def test_model_with_the_knob_equals_the_model_without(env, share):
    """SHARE_WEIGHTS: the trunk's own stack is the source pool (model.py's trunk-once route); without it the sources are the
    second network's stack (feats[source_index] in the reference's two-pass form)."""
    from epipolar_transformers_amd import synthetic as syn
    from epipolar_transformers_amd.model import ring_sources

    frames, V = 2, 3
    m, cfg, size = _model(**{"EPIPOLAR.SHARE_WEIGHTS": share})
    assert (m.backbone is m.reference) == share
    P = torch.from_numpy(syn.ring_cameras(V, size)).float().repeat(frames, 1, 1)
    img = torch.randn(frames * V, 3, size, size, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    src = ring_sources(frames, V)                        # a host index
    with torch.no_grad():
        feat = m.reference.trunk(img)
        assert feat.shape[1] == C                        # the fusion point of the tile kernels
        # One trunk result per network for every run: what differs between the runs is the layer's route, not the convolution
        # library's choice of algorithm (which changes between calls of one shape: two runs WITHOUT the knob differ otherwise).
        class Const(torch.nn.Module):
            def __init__(self, value):
                super().__init__()
                self.value = value

            def forward(self, t):
                return self.value

        if share:
            m.reference.trunk = lambda x: feat
        else:
            feat_b = m.backbone(img)[0]
            m.backbone.forward = lambda x, *a, **k: (feat_b,)
            m.reference.deconv_layers = Const(feat)      # (PoseResNet.forward runs its stages inline: their result is replaced)
        fl = m.reference.final_layer
        w64, b64 = fl.weight.double().flatten(1), fl.bias.double()

        class Head64(torch.nn.Module):                   # (the library also picks its algorithm for the 1x1 head call by call)
            def forward(self, t):
                return (torch.einsum("nchw,jc->njhw", t.double(), w64) + b64[None, :, None, None]).float()

        m.reference.final_layer = Head64()
        res = []
        for knob in (False, False, False, True):         # (the first run settles the convolutions' algorithms)
            cfg.merge_from_list(["EPIPOLAR_AMD.PAIR_INDEX", knob])
            with _Calls() as names:
                views = m.forward_views(img, P, src)
                multi = m.forward_multitest(img, P, V)
            torch.cuda.synchronize()
            res.append((views, multi))
            assert names.count("et_epipolar_forward_fused_ix") == (2 if knob else 0), names
            assert names.count("et_epipolar_forward_fused") == (0 if knob else 2), names
    _, off0, off, on = res
    # two runs without the knob agree to the bit: a difference below cannot be blamed on run-to-run noise
    assert torch.equal(off0[0][1][0], off[0][1][0]) and torch.equal(off0[1][1], off[1][1])
    assert torch.equal(on[0][1][0], off[0][1][0])                                   # heat maps
    assert torch.equal(on[0][2], off[0][2]) and torch.equal(on[0][3], off[0][3])    # locations, scores
    assert torch.equal(on[0][4], off[0][4]) and torch.equal(on[0][5], off[0][5])    # corr_pos, depth
    assert torch.equal(on[1][0], off[1][0]) and torch.equal(on[1][1], off[1][1])    # MULTITEST: locations, scores


def test_multitest_layer_call_needs_no_gathered_stacks(env):
    """forward_multitest's layer call gathers 2 x F*V*(V-1) maps without the knob and none with it: the peak of the call drops by at
    least those bytes minus one map (the slack: allocator rounding of the small tensors both routes make)."""
    frames, V = 2, 3
    m, cfg, size = _model()
    from epipolar_transformers_amd import synthetic as syn

    P = torch.from_numpy(syn.ring_cameras(V, size)).float().repeat(frames, 1, 1)
    img = torch.randn(frames * V, 3, size, size, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    peak, xs = {}, {}
    with torch.no_grad():
        feat = m.reference.trunk(img)
        for knob in (False, True):
            cfg.merge_from_list(["EPIPOLAR_AMD.PAIR_INDEX", knob])
            m._multitest_layer(feat, feat, P, V)          # (workspaces, the packed weight, the cached tables: made once)
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            xs[knob] = m._multitest_layer(feat, feat, P, V)
            torch.cuda.synchronize()
            peak[knob] = torch.cuda.max_memory_allocated() - before
    assert torch.equal(xs[True], xs[False])
    pairs = frames * V * (V - 1)
    map_bytes = feat[0].numel() * 4
    print("peak of the layer call: gathered %d bytes, indexed %d bytes; one map %d bytes, %d pairs" % (peak[False], peak[True], map_bytes, pairs))
    assert peak[False] - peak[True] >= (2 * pairs - 1) * map_bytes
