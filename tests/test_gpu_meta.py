"""The Meta fusion layer on the GPU (ops.meta_fuse over et_meta_pack / et_meta_gemm / et_meta_wgrad, meta.Meta, the metaHG* hourglass
callers behind EPIPOLAR_AMD.META_FUSION) against outputs of the REAL reference (tests/golden/meta/layer_*.npz,
tests/golden/hourglass_meta_*.npz, made by tests/golden/make_meta_golden.py).

Gates: y within 1e-4 max(1, max|want|); every gradient within 1e-4 max|want| of that tensor -- the project's output and gradient
gates; the reference itself lies about 300 x inside them (the fixture's ref_dist_*).  The whole net: the tolerances of
tests/test_gpu_hourglass.py.  Every comparison prints its largest error relative to its gate (profiles/meta_fusion.txt)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

import abi_harness as ah

pytestmark = pytest.mark.gpu

sys.path.insert(0, GOLDEN_DIR)
from make_meta_golden import HG_CASES, LAYER_CASES, LAYER_DIR, meta_inputs, meta_weights  # noqa: E402

LAYER_NAMES = [c["name"] for c in LAYER_CASES]
GATE = 1e-4


def _report(what, got, want, gate):
    err = float((got.double() - want.double()).abs().max())
    print("%-44s max error %.3e = %.4f of its gate %.3e" % (what, err, err / gate, gate))
    assert err <= gate, what


def _grad_gate(want):
    return GATE * float(want.abs().max())


@functools.lru_cache(maxsize=None)
def _layer_case(case):
    """fixture, rebuilt weights and maps of a layer case, on the GPU (shared by the tests; nothing modifies them)"""
    d = dict(np.load(os.path.join(LAYER_DIR, "layer_%s.npz" % case)))
    d["y"] = np.load(os.path.join(LAYER_DIR, "layer_%s_y.npz" % case))["y"]
    d["grad_input"] = np.load(os.path.join(LAYER_DIR, "layer_%s_gin.npz" % case))["grad_input"]
    sd = meta_weights("", float(d["f_scale"]))
    inp, feat, gout = [t.cuda() for t in meta_inputs(case)]
    return d, sd, inp, feat, gout


def _module(sd):
    from epipolar_transformers_amd.meta import Meta

    m = Meta(256)
    m.load_state_dict(sd, strict=True)
    return m.cuda()


def _rows(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("case", LAYER_NAMES)
def test_meta_layer_against_reference(case):
    """Meta(fundamental=F) and ops.meta_fuse: y and every gradient the fixture holds"""
    from epipolar_transformers_amd import ops

    d, sd, inp, feat, gout = _layer_case(case)
    cuda = lambda k: torch.from_numpy(d[k]).cuda()
    m = _module(sd)
    x = inp.clone().requires_grad_()
    f = feat.clone().requires_grad_()
    y = m(torch.from_numpy(d["P_ref"]), torch.from_numpy(d["P_src"]), x, feat=f, fundamental=cuda("F"))
    assert tuple(y.shape) == tuple(inp.shape)
    y.backward(gout)
    want_y = cuda("y")
    _report(case + " Meta y", y.detach(), want_y, GATE * max(1.0, float(want_y.abs().max())))
    _report(case + " Meta d input", x.grad, cuda("grad_input"), _grad_gate(cuda("grad_input")))
    assert torch.equal(f.grad, gout)                                          # d feat = g
    for k in ("share.weight", "share.bias", "fc0.weight", "fc0.bias", "fc1.bias"):
        want = cuda("grad_" + k)
        _report("%s Meta d %s" % (case, k), dict(m.named_parameters())[k].grad, want, _grad_gate(want))
    g1 = m.fc1.weight.grad
    step = int(d["fc1_row_step"])
    _report(case + " Meta d fc1.weight (every %dth row)" % step, g1[::step], cuda("grad_fc1.weight_rows"), GATE * float(d["grad_fc1.weight_max"]))
    total, want_total = float(g1.double().abs().sum()), float(d["grad_fc1.weight_abs_sum"])
    print("%-44s %.9e against %.9e: %.2e relative" % (case + " Meta sum|d fc1.weight|", total, want_total, abs(total - want_total) / want_total))
    assert abs(total - want_total) <= GATE * want_total

    # the operator itself, on the weight the two linear layers make (torch on the device): the same bits as the module's pass
    with torch.no_grad():
        weight = m.fc1(torch.relu(m.fc0(cuda("F").reshape(-1, 9)))).view(-1, 256, 256)
    weight.requires_grad_()
    src = _rows(inp).requires_grad_()
    sw, sb = m.share.weight.detach().clone().requires_grad_(), m.share.bias.detach().clone().requires_grad_()
    y2 = ops.meta_fuse(src, weight, sw, sb, _rows(feat))
    y2.backward(_rows(gout))
    assert ah.same_bits(y2.detach().permute(0, 3, 1, 2).contiguous(), y.detach().contiguous())
    assert ah.same_bits(src.grad.permute(0, 3, 1, 2).contiguous(), x.grad.contiguous())
    want = cuda("grad_fc1.bias")                                              # = sum over the pairs of the per-pair weight gradient
    _report(case + " meta_fuse sum_n d weight[n]", weight.grad.sum(0).reshape(-1), want, _grad_gate(want))
    _report(case + " meta_fuse d share_weight", sw.grad, cuda("grad_share.weight"), _grad_gate(cuda("grad_share.weight")))
    _report(case + " meta_fuse d share_bias", sb.grad, cuda("grad_share.bias"), _grad_gate(cuda("grad_share.bias")))

    # feat = None (EPIPOLAR.OTHER_ONLY): the fused result minus feat
    with torch.no_grad():
        alone = m(None, None, inp, fundamental=cuda("F"))
    _report(case + " Meta y, feat=None", alone, want_y - feat, GATE * max(1.0, float(want_y.abs().max())))


def _operands(n, hw, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    src = torch.randn(n, hw, 256, device="cuda", generator=g).relu_()
    feat = torch.randn(n, hw, 256, device="cuda", generator=g)
    gout = torch.randn(n, hw, 256, device="cuda", generator=g)
    weight = torch.randn(n, 256, 256, device="cuda", generator=g) * (0.05 * (1 + torch.arange(n, device="cuda").view(n, 1, 1)))
    share = torch.randn(256, 256, device="cuda", generator=g) / 16
    bias = torch.randn(256, device="cuda", generator=g) * 0.05
    return src, feat, gout, weight, share, bias


def _all_three(src, feat, gout, weight, share, bias):
    """x, d src, grad_w, grad_b through the three exports"""
    from epipolar_transformers_amd import ops

    x = ops.meta_gemm(src, ops.meta_pack(weight, share), bias, feat)
    dsrc = ops.meta_gemm(gout, ops.meta_pack(weight, share, transpose=True))
    gw, gb = ops.meta_wgrad(gout, src)
    return x, dsrc, gw, gb


@pytest.mark.parametrize("n,hw", [(3, 35), (3, 65), (2, 2100)])
def test_pair_alone_equals_pair_in_batch_and_runs_repeat(n, hw):
    """a pair's x, d src and grad_w: the same bits alone and inside the batch (each pair is packed under a scale of its own -- the
    pairs' weights differ in magnitude here --, tiles and weight-gradient blocks are per pair); two runs: identical bits.
    (2, 2100): 33 tiles per pair with a last tile of 52 rows, and two weight-gradient blocks per pair (more than 2048 rows)."""
    ops_in = _operands(n, hw, seed=7 + hw)
    first = _all_three(*ops_in)
    again = _all_three(*ops_in)
    for a, b in zip(first, again):
        assert ah.same_bits(a, b)
    src, feat, gout, weight, share, bias = ops_in
    for i in range(n):
        one = _all_three(src[i:i + 1], feat[i:i + 1], gout[i:i + 1], weight[i:i + 1], share, bias)
        for name, a, b in zip(("x", "d src", "grad_w"), one, (first[0][i:i + 1], first[1][i:i + 1], first[2][i:i + 1])):
            assert ah.same_bits(a.contiguous(), b.contiguous()), (name, i)
    # against float64 (the three shapes; at 2100 rows the only check of the multi-block weight gradient's values)
    w64 = (weight + share).double()
    _report("(%d, %d) x vs float64" % (n, hw), first[0], torch.einsum("nmc,noc->nmo", src.double(), w64) + bias.double() + feat.double(),
            GATE * max(1.0, float(first[0].abs().max())))
    want = torch.einsum("nmo,noc->nmc", gout.double(), w64)
    _report("(%d, %d) d src vs float64" % (n, hw), first[1], want, _grad_gate(want))
    want = torch.einsum("nmo,nmc->noc", gout.double(), src.double())
    _report("(%d, %d) grad_w vs float64" % (n, hw), first[2], want, _grad_gate(want))
    want = gout.double().sum((0, 1))
    _report("(%d, %d) grad_b vs float64" % (n, hw), first[3], want, _grad_gate(want))


@pytest.mark.parametrize("n", [3, 1])
@pytest.mark.parametrize("hw", [35, 65])
def test_outputs_and_workspace_between_guard_bands(n, hw):
    """the three exports through the C ABI with every output and the workspace between guard bands, 0xFF-filled (NaN): the bands are
    untouched -- the rows of the last pair's masked tail lie in one --, every row of x / d src comes back finite, and so do
    grad_w / grad_b from a workspace of exactly the size asked for."""
    from epipolar_transformers_amd import _lib

    lib = _lib.load()
    src, feat, gout, weight, share, bias = _operands(n, hw, seed=100 + hw + n)
    pb = int(lib.et_residual_gemm_packed_bytes())
    ws_bytes = int(lib.et_meta_wgrad_workspace_bytes(n, hw))
    a = (ah.Arena().add("packed", n * pb, torch.uint8).add("packed_t", n * pb, torch.uint8).add("x", (n, hw, 256)).add("dsrc", (n, hw, 256))
         .add("gw", (n, 256, 256)).add("gb", 256).add("ws", ws_bytes, torch.uint8).build())
    snap = ah.frozen(src=src, feat=feat, gout=gout, weight=weight, share=share, bias=bias)
    ah.call("et_meta_pack", n, 256, weight, share, 0, a["packed"])
    ah.call("et_meta_pack", n, 256, weight, share, 1, a["packed_t"])
    ah.call("et_meta_gemm", n, hw, 256, src, feat, a["packed"], bias, a["x"])
    ah.call("et_meta_gemm", n, hw, 256, gout, None, a["packed_t"], None, a["dsrc"])
    ah.call("et_meta_wgrad", n, hw, 256, gout, src, a["gw"], a["gb"], a["ws"], ctypes.c_size_t(ws_bytes))
    a.check()
    ah.assert_unchanged(snap)
    for k in ("x", "dsrc", "gw", "gb"):
        assert bool(torch.isfinite(a[k]).all()), k
    want = _all_three(src, feat, gout, weight, share, bias)
    for k, w in zip(("x", "dsrc", "gw", "gb"), want):
        assert ah.same_bits(a[k].contiguous().view(w.shape), w), k
    # without the bias gradient nothing is written to it
    a["gb"].fill_(float("nan"))
    ah.call("et_meta_wgrad", n, hw, 256, gout, src, a["gw"], None, a["ws"], ctypes.c_size_t(ws_bytes))
    a.check()
    assert bool(torch.isnan(a["gb"]).all())


def test_twenty_poisoned_runs_give_identical_bits():
    """forward and backward at N = 3, 5 x 13, output buffers NaN-poisoned (conftest: ops.POISON_OUTPUTS): the same bits every time,
    no NaN -- the fence every MFMA kernel family of the library has."""
    from epipolar_transformers_amd import ops

    assert ops.POISON_OUTPUTS
    src, feat, gout, weight, share, bias = _operands(3, 65, seed=3)
    first = None
    for _ in range(20):
        leaves = [t.clone().requires_grad_() for t in (src, weight, share, bias, feat)]
        y = ops.meta_fuse(*leaves[:4], leaves[4])
        y.backward(gout)
        got = [y.detach()] + [t.grad for t in leaves]
        assert all(bool(torch.isfinite(t).all()) for t in got)
        if first is None:
            first = got
        else:
            assert all(ah.same_bits(a, b) for a, b in zip(first, got))


def _build_net(d, train=False):
    from epipolar_transformers_amd import backbones, default_cfg
    from make_hourglass_golden import apply_weight_scales
    from model_weights import deterministic_state_dict

    size, hs, j, n = [int(v) for v in d["meta"]]
    cfg = default_cfg()
    cfg.merge_from_list(["BACKBONE.BODY", str(d["body"]), "BACKBONE.PRETRAINED", False, "EPIPOLAR.MERGE", str(d["merge"]),
                         "KEYPOINT.HEATMAP_SIZE", (hs, hs), "KEYPOINT.NUM_PTS", j, "KEYPOINT.SIGMA", 2.0, "KEYPOINT.NFEATS", 256,
                         "DATASETS.IMAGE_SIZE", (size, size), "EPIPOLAR_AMD.META_FUSION", True])
    net = backbones.build_backbone(cfg)
    sd = deterministic_state_dict(net.state_dict())
    for prefix in sorted({k.rsplit(".", 2)[0] + "." for k in sd if k.startswith(("meta.", "testmeta."))}):
        sd.update(meta_weights(prefix, float(d["f_scale"])))
    net.load_state_dict(apply_weight_scales(sd, d["weight_scales"], net.nStack), strict=True)
    assert sorted(net.state_dict()) == [str(k) for k in d["state_dict_keys"]]
    net = net.cuda()
    F = torch.from_numpy(d["F"]).cuda()
    for m in net.meta:
        m._fundamental.get = lambda *a, **kw: F                              # the matrices the reference computed for the fixture
    return net.train() if train else net.eval()


@pytest.mark.parametrize("case", [c["name"] for c in HG_CASES])
def test_meta_hourglass_vs_reference(case):
    d = np.load(os.path.join(GOLDEN_DIR, "hourglass_meta_%s.npz" % case))
    net = _build_net(d)
    img = torch.from_numpy(d["img"]).cuda()
    src = torch.from_numpy(d["src"]).cuda()
    KRT = torch.from_numpy(d["KRT"])
    with torch.no_grad():
        own = net(img)[0]
        assert len(own) == int(d["n_own"])
        other = [f[src] for f in own]
        features, heatmaps, locs, scos, corr_pos, depth, sample_locs, warped = net(
            img, other_inputs=[other, KRT[d["src"]], None, KRT, None, None, img[src]])
    assert corr_pos is None and depth is None and sample_locs is None and warped is None
    assert len(features) == int(d["n_features"]) and len(heatmaps) == int(d["n_heatmaps"])
    for i, h in enumerate(heatmaps):
        want = torch.from_numpy(d["heatmap%d" % i]).cuda()
        _report("%s heat map %d" % (case, i), h, want, 5e-4 * max(1.0, float(want.abs().max())))
    want = torch.from_numpy(d["feature_last"]).cuda()
    _report(case + " last fused feature", features[-1], want, 5e-4 * max(1.0, float(want.abs().max())))
    for f, chk in zip(features, d["feature_checksum"]):
        assert abs(float(f.double().abs().sum()) - chk) <= 1e-3 * chk
    want = torch.from_numpy(d["scos"]).cuda()
    _report(case + " scos", scos, want, 5e-4 * max(1.0, float(want.abs().max())))
    # detections: the arg-max cell may flip between near-equal heat-map values; where the peak cell agrees the sub-pixel location does too
    dl = np.abs(locs.cpu().numpy() - d["locs"]).max(-1)
    assert (dl <= 0.05).mean() >= 0.9, dl


def test_merge_both_has_no_meta_layer_for_its_second_point():
    """the reference builds one Meta layer per stack and indexes them by fusion point: under MERGE both the stack's second point
    raises IndexError there (ProHG.py:185-187, 220, 263-271) -- and here"""
    d = dict(np.load(os.path.join(GOLDEN_DIR, "hourglass_meta_hg11_late.npz")))
    d["merge"] = np.array("both")
    net = _build_net(d)
    img = torch.from_numpy(d["img"]).cuda()
    KRT = torch.from_numpy(d["KRT"])
    with torch.no_grad(), pytest.raises(IndexError):
        own = net(img)[0]
        net(img, other_inputs=[[f.flip(0) for f in own], KRT.flip(0), None, KRT, None, None, img.flip(0)])


def test_training_backward_reaches_the_meta_parameters():
    d = np.load(os.path.join(GOLDEN_DIR, "hourglass_meta_hg1_late.npz"))
    net = _build_net(d, train=True)
    img = torch.from_numpy(d["img"]).cuda()
    src = torch.from_numpy(d["src"]).cuda()
    KRT = torch.from_numpy(d["KRT"])
    with torch.no_grad():
        other = [f[src] for f in net(img)[0]]
    heatmaps = net(img, other_inputs=[other, KRT[d["src"]], None, KRT, None, None, img[src]])[1]
    heatmaps[-1].square().mean().backward()
    for k in ("meta.0.fc0.weight", "meta.0.fc0.bias", "meta.0.fc1.weight", "meta.0.fc1.bias", "meta.0.share.weight", "meta.0.share.bias"):
        g = dict(net.named_parameters())[k].grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
    assert net.testmeta.fc0.weight.grad is None                              # (unused in forward, as in the reference)
