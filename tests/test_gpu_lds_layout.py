"""The LDS placements of csrc/et_lds_layout.h (fp16 A stage of G1, staged `out` tile of G3, G1's lane trade) on the GPU, through
every instance of the persistent forward kernel that shares them: the 256-row instance, the band-table instance, the two-pass
instance (K = 72) and the one-kernel layer.  tests/test_lds_layout_cpu.py checks the placements as functions; here a writer and
a reader that disagree about them have to show in the results.

The smallest shape at which they can: 16 x 16 maps = 256 pixels = 8 tiles per pair, so every tile row, both pixel halves and
every one of the 256 channels are in use; 2 pairs; C = 256.  Inputs that turn a misplaced 16-byte chunk into an O(1) error:
feat_ref[p] is ONE-HOT in channel (37 p) mod 256 with a value in {1, 2, 3} and feat_src[q, c] = g(q) (1 + c / 256), g uniform
in [0.5, 1.5] -- every logit carries the weight of exactly one channel, and a chunk read from another slot moves it by up to a
factor of two.  A second case runs on post-ReLU random maps.  Reference: the per-pixel fp32 kernels (ET_VARIANT_NO_TILE), at
the tolerances tests/test_gpu_split_fp16.py holds the split-fp16 arithmetic to (attention 1e-5, `out` 1e-4 of its magnitude);
corr_pos equal.  The one-kernel layer's x against forward_nhwc + residual_gemm at the tolerance of tests/test_gpu_fused.py
(2e-5 of its magnitude), with a folded weight whose 65 536 entries are all distinct."""
import functools

import pytest
import torch

import abi_harness as hx
from abi_harness import C

pytestmark = pytest.mark.gpu

N, H, W = 2, 16, 16
TOL_ATTN, TOL_OUT_REL, TOL_X_REL = 1e-5, 1e-4, 2e-5


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from epipolar_transformers_amd import _lib, ops

    _lib.load()
    return _lib, ops


@functools.lru_cache(maxsize=None)
def _inputs(kind):
    rnd_ref, rnd_src, cam = hx.pair_inputs(N, H, W, seed=6100)
    if kind == "randn":
        return rnd_ref, rnd_src, cam
    g = torch.Generator(device="cuda").manual_seed(6101)
    p = torch.arange(H * W, device="cuda")
    ref = torch.zeros(N, H * W, C, device="cuda")
    for n in range(N):
        ref[n, p, (37 * p) % C] = (1 + (p + n) % 3).float()
    gq = torch.rand(N, H * W, 1, device="cuda", generator=g) + 0.5
    src = gq * (1.0 + torch.arange(C, device="cuda").float() / C)
    return ref.view(N, H, W, C), src.view(N, H, W, C).contiguous(), cam


@functools.lru_cache(maxsize=None)
def _reference(kind, k):
    """Per-pixel fp32 kernels, once per (inputs, K); shared by the instances and left unchanged."""
    from epipolar_transformers_amd import _lib, ops

    ref, src, cam = _inputs(kind)
    out, attn, corr = ops.forward_nhwc(ops.LayerSpec(H=H, W=W, K=k, variant=_lib.ET_VARIANT_NO_TILE), ref, src, cam)
    torch.cuda.synchronize()
    return out, attn, corr


@functools.lru_cache(maxsize=None)
def _weight():
    g = torch.Generator(device="cuda").manual_seed(6102)
    wf = (torch.randn(C, C, device="cuda", generator=g) * 0.05 + torch.eye(C, device="cuda")).flatten()
    for _ in range(16):      # (65 536 fp32 draws collide a few dozen times: the later of two equal entries moves up by one ulp)
        s, idx = wf.sort()
        dup = torch.zeros_like(s, dtype=torch.bool)
        dup[1:] = s[1:] == s[:-1]
        if not dup.any():
            break
        wf[idx[dup]] = torch.nextafter(s[dup], torch.full_like(s[dup], float("inf")))
    assert torch.unique(wf).numel() == C * C
    return wf.view(C, C), torch.randn(C, device="cuda", generator=g)


def _check(ops, ws, got_out, got_attn, got_corr, kind, k):
    want_out, want_attn, want_corr = _reference(kind, k)
    ops.check_tile_errors(workspace=ws)
    # the persistent kernel itself has to have computed the tiles: the overflow list goes to the one-block-per-tile kernels
    assert hx.ws_overflow(ws) == 0
    ea = (got_attn - want_attn).abs().max().item()
    eo = (got_out - want_out).abs().max().item() / max(1.0, want_out.abs().max().item())
    print("%s K=%d: attention error %.3g (bound %.3g), out error %.3g of its magnitude (bound %.3g)" % (kind, k, ea, TOL_ATTN, eo, TOL_OUT_REL))
    assert torch.isfinite(got_attn).all() and torch.isfinite(got_out).all()
    assert ea <= TOL_ATTN
    assert eo <= TOL_OUT_REL
    assert torch.equal(got_corr, want_corr)


@pytest.mark.parametrize("kind", ["one-hot", "randn"])
@pytest.mark.parametrize("k,variant", [(16, 0), (16, "band"), (72, 0)], ids=["K16-default", "K16-band-table", "K72-two-pass"])
def test_sample_and_attention_instances_vs_per_pixel_kernels(env, kind, k, variant):
    _lib, ops = env
    ref, src, cam = _inputs(kind)
    spec = ops.LayerSpec(H=H, W=W, K=k, variant=_lib.ET_VARIANT_WS_BAND if variant == "band" else 0)
    ws = ops.tile_workspace(spec, N, C, "cuda")
    out, attn, corr = ops.forward_nhwc(spec, ref, src, cam, workspace=ws)
    torch.cuda.synchronize()
    _check(ops, ws, out, attn, corr, kind, k)


@pytest.mark.parametrize("kind", ["one-hot", "randn"])
def test_one_kernel_layer_vs_per_pixel_kernels_and_two_kernels(env, kind):
    _lib, ops = env
    k = 16
    ref, src, cam = _inputs(kind)
    wf, bias = _weight()
    packed = ops.residual_gemm_pack(wf)
    spec = ops.LayerSpec(H=H, W=W, K=k)
    assert ops.fused_layer_applies(spec, C, N)
    ws = ops.tile_workspace(spec, N, C, "cuda")
    x, attn, corr, out = ops.forward_fused_nhwc(spec, ref, src, cam, packed, bias, want_out=True, workspace=ws)
    torch.cuda.synchronize()
    _check(ops, ws, out, attn, corr, kind, k)
    want_x = ops.residual_gemm(ops.forward_nhwc(spec, ref, src, cam)[0], packed, bias, ref)
    ex = (x - want_x).abs().max().item() / max(1.0, want_x.abs().max().item())
    print("%s: x error %.3g of its magnitude (bound %.3g)" % (kind, ex, TOL_X_REL))
    assert torch.isfinite(x).all()
    assert ex <= TOL_X_REL
    ops.check_tile_errors()
