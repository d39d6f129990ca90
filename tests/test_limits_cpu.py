"""The yardstick of tests/test_gpu_limits.py, checked without a GPU: at the ends of the ranges validate() admits (C = 4 and 512,
K = 2 and 256, maps smaller than a tile, one-row and one-column maps) the float32 C oracle is itself a float32 sum of up to 512
terms, so before a kernel is held to it the oracle is held to the reference's op sequence in float64
(oracle.torch_ref_path.forward on float64 inputs, gradients by autograd) within a QUARTER of the project's tolerances
(tests/test_gpu_parity.py: TOL_ATTN, TOL_OUT, TOL_GRAD_REL) -- which leaves the kernels three quarters of them.

The shape list and the inputs live here and are imported by the GPU module, so both see the same cases and the oracle runs once
per shape and process (`reference`)."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_parity import TOL_ATTN, TOL_GRAD_REL, TOL_OUT

# (H, W, C, K, settings of the layer)
SHAPES = [
    # the bottom of C and K
    (3, 5, 4, 3, {}), (9, 7, 4, 2, {}), (9, 7, 8, 4, {}),
    # the top: every lane of the second float4 group live, all four sample slots full, the emit kernel's LDS at 64 KiB
    (9, 7, 512, 12, {}), (9, 7, 384, 72, {}), (9, 7, 512, 256, {}),
    # a map smaller than one 32-pixel tile and one 16-pixel block; K = 2 on the 256-channel kernels
    (2, 2, 256, 8, {}), (3, 3, 256, 2, {}),
    # K = 256 on the tile path
    (20, 24, 256, 256, {}),
    # one-row and one-column maps.  Legacy normalize only: with correct_normalize the reference divides by W - 1 = 0 (or
    # H - 1) and the oracle returns NaN -- nothing to compare with, so that combination is not run on the GPU
    (1, 9, 256, 6, dict(correct_normalize=False, image=36)), (9, 1, 256, 6, dict(correct_normalize=False, image=36)),
    # the soft-max off at the top of both ranges
    (9, 7, 512, 256, dict(softmax_enabled=False)),
]


def shape_id(shape):
    H, W, C, K, kw = shape
    return "%dx%d-C%d-K%d" % (H, W, C, K) + "".join("-%s%s" % (k, v) for k, v in sorted(kw.items()))


def layer_kwargs(shape):
    return {k: v for k, v in shape[4].items() if k != "image"}


def inputs(shape):
    """Three pairs as tests/test_gpu_parity.py::test_ragged_shapes_vs_oracle draws them, with the image 4 x the map's larger side
    (with that test's 64-pixel image a 2 x 2 map would sample nothing): P1, P2 (3,3,4), f1, f2, grad_out (3,C,H,W) float32."""
    from epipolar_transformers_amd import synthetic as syn

    H, W, C, K, kw = shape
    P1, P2 = syn.make_pairs(1, 4, kw.get("image", 4 * max(H, W)), seed=21, jitter=(0.05, 2.0))
    g = torch.Generator().manual_seed(H * 100 + W)
    f1 = torch.randn(3, C, H, W, generator=g).relu()
    f2 = torch.randn(3, C, H, W, generator=g).relu()
    go = torch.randn(3, C, H, W, generator=g)
    return P1[:3], P2[:3], f1, f2, go


@functools.lru_cache(maxsize=None)
def _reference(key):
    from epipolar_transformers_amd import camera
    from oracle import oracle as orc

    shape = SHAPES[key]
    H, W, C, K, _ = shape
    P1, P2, f1, f2, go = inputs(shape)
    so = orc.LayerSpec(H, W, K, **layer_kwargs(shape))
    cam = camera.pair_algebra(P1, P2)
    want = orc.forward(so, f1, f2, None, None, cam=cam.numpy())
    g1, g2 = orc.backward(so, f1.numpy(), f2.numpy(), want["sample_locs"], go.numpy())
    want.update(grad_ref=g1, grad_src=g2, cam=cam, spec=so)
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return want


def reference(shape):
    """The C oracle's forward and backward for `shape` (read-only arrays, computed once): out, attn, corr_pos, sample_locs,
    grad_ref, grad_src, the per-pair algebra `cam` (a CPU tensor) and the oracle's layer `spec`."""
    return _reference(SHAPES.index(shape))


def grad_ref_terms(shape):
    """The un-cancelled size of d(feat_ref): max over elements of  scale * sum_k a_k (E_k + E^) |S_kc|,  E_k = |grad_out| . |S_k|,
    E^ = sum_k a_k E_k -- every term of  d(feat_ref)_c = scale * sum_k a_k (e_k - e^) S_kc,  e_k = grad_out . S_k, taken by
    magnitude (float64, from the oracle's attention and sample locations).  On a one-row (one-column) map the K samples of a
    pixel coincide, e_k = e^ and the gradient is zero analytically: what float32 arithmetic returns for it is rounding of these
    terms, and it has no other scale."""
    import torch.nn.functional as F

    want = reference(shape)
    _, _, _, f2, go = inputs(shape)
    so, K, worst = want["spec"], shape[3], 0.0
    for n in range(f2.shape[0]):
        S = F.grid_sample(f2[n].double().expand(K, -1, -1, -1), torch.from_numpy(want["sample_locs"][:, n].astype(np.float64)),
                          mode="bilinear", padding_mode="zeros", align_corners=so.align_corners)   # (K,C,H,W)
        a = torch.from_numpy(want["attn"][n].astype(np.float64))                                   # (K,H,W)
        e = (go[n].double().abs() * S.abs()).sum(1)
        mag = a * (e + (a * e).sum(0, keepdim=True))
        worst = max(worst, float((so.softmax_scale * (mag.unsqueeze(1) * S.abs()).sum(0)).max()))
    return worst


def close_err(got, want):
    """The error tests/test_gpu_parity.py::_close holds to its atol: |got - want| - 2e-6 |want|, at its worst."""
    return float((np.abs(got - want) - 2e-6 * np.abs(want)).max())


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_oracle_is_within_a_quarter_of_the_tolerances_of_float64(shape):
    from oracle import torch_ref_path

    H, W, C, K, kw = shape
    want = reference(shape)
    _, _, f1, f2, go = inputs(shape)
    a, b = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    out, attn, _ = torch_ref_path.forward(a, b, torch.from_numpy(want["sample_locs"].astype(np.float64)),
                                          softmax_enabled=kw.get("softmax_enabled", True),
                                          correct_normalize=kw.get("correct_normalize", True))
    (out * go.double()).sum().backward()
    for k in ("out", "attn", "grad_ref", "grad_src", "corr_pos"):
        assert np.isfinite(want[k]).all(), k
    err_attn = close_err(want["attn"], attn.detach().numpy())
    err_out = close_err(want["out"], out.detach().numpy())
    # relative to the tensor's maximum, with the floor of test_ragged_shapes_vs_oracle: on a one-row map all K samples of a pixel
    # coincide, d(feat_ref) is zero analytically and 1e-15 of rounding in float64 -- a tensor without a scale of its own
    err_grad = max(float(np.abs(want[k] - g.numpy()).max() / max(np.abs(g.numpy()).max(), 1e-6))
                   for k, g in (("grad_ref", a.grad), ("grad_src", b.grad)))
    share = float((np.abs(want["attn"] - 1.0 / K).max(1) > 1e-3).mean())
    print("%s: oracle vs float64 attn %.2e out %.2e grad %.2e (relative); non-uniform pixels %.2f; |out| max %.2f" %
          (shape_id(shape), err_attn, err_out, err_grad, share, np.abs(want["out"]).max()))
    assert err_attn <= TOL_ATTN / 4
    assert err_out <= TOL_OUT / 4
    assert err_grad <= TOL_GRAD_REL / 4
    # the case is not empty: the attention is not the uniform one of all-masked pixels -- except on a one-row (one-column) map,
    # where the segment is degenerate and every sample lands on one point: there the output itself must be there
    if min(H, W) == 1:
        assert np.abs(want["out"]).max() > 0.5
    else:
        assert share >= 0.4
