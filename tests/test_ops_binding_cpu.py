"""Host logic of the Python binding (ops.py) that needs no GPU: the default backward form, the argument checks in front of
every export (a tensor the library must not see never gets as far as loading it) and the one reader of the workspace header."""
import pytest
import torch

from epipolar_transformers_amd import _lib, ops

V = _lib


DET, NO_TILE = V.ET_VARIANT_BWD_DETERMINISTIC, V.ET_VARIANT_NO_TILE
# backward_nhwc(form=None) with a workspace: variant -> the form for (soft-max on, tile_bytes) = (1, 0), (1, 1), (0, 0), (0, 1)
DEFAULT_FORM = {
    0:                        ("gather", "tile", "gather", "tile"),
    V.ET_VARIANT_BWD_ATOMIC:   ("gather", "gather", "gather", "gather"),
    V.ET_VARIANT_BWD_UNSORTED: ("gather", "gather", "gather", "gather"),
    NO_TILE:                  ("gather", "gather", "gather", "gather"),
    DET:                      ("gather", "tile_det", "gather", "gather"),
    DET | NO_TILE:            ("gather", "gather", "gather", "gather"),
}


@pytest.mark.parametrize("variant", sorted(DEFAULT_FORM))
def test_default_backward_form(variant):
    """The choice backward_nhwc makes when the caller names no form: "atomic" without a workspace; with one, "tile" where the tile
    path applies (tile_bytes > 0) unless the variant names BWD_ATOMIC / BWD_UNSORTED / NO_TILE, else "gather"; the deterministic
    bit turns "tile" into "tile_det" with the soft-max on and into "gather" with it off."""
    cases = ((True, 0), (True, 1), (False, 0), (False, 1))
    for (softmax, tile_bytes), want in zip(cases, DEFAULT_FORM[variant]):
        spec = ops.LayerSpec(H=4, W=4, K=4, softmax_enabled=softmax, variant=variant)
        assert ops._default_backward_form(spec, tile_bytes, True) == want, (softmax, tile_bytes)
        assert ops._default_backward_form(spec, tile_bytes, False) == "atomic", (softmax, tile_bytes)


class _OnGpu(torch.Tensor):
    """A host tensor that answers `is_cuda` with True: what the argument checks see of a device tensor, on a machine without
    one.  (Its address must never reach the library: the tests below fail the moment the library is asked for.)"""
    is_cuda = True


def _gpu(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_OnGpu)


@pytest.fixture
def no_library(monkeypatch):
    def load():
        pytest.fail("an invalid call reached the library")

    monkeypatch.setattr(_lib, "load", load)


N, H, C, K = 1, 4, 8, 4


def test_host_tensors_never_reach_the_library(no_library):
    spec = ops.LayerSpec(H=H, W=H, K=K)
    x, cam = torch.zeros(N, H, H, C), torch.zeros(N, _lib.ET_CAM_STRIDE)
    rows = torch.zeros(3, 256)
    for call in (lambda: ops.backward_nhwc(spec, x, x, cam, x),
                 lambda: ops.backward_nhwc(spec, x, x, cam, x, form="atomic"),
                 lambda: ops.backward_general_nhwc(spec, x, x, x, cam, x),
                 lambda: ops.residual_gemm(rows, torch.zeros(8, dtype=torch.uint8), torch.zeros(256)),
                 lambda: ops.residual_gemm_pack(torch.zeros(256, 256)),
                 lambda: ops.z_wgrad(rows, rows),
                 lambda: ops.forward_nhwc(spec, x, x, cam)):
        with pytest.raises(_lib.EpipolarAmdError, match="no CPU fallback"):
            call()
    # ... nor does one argument on the host among device tensors: grad_out, cam, a bias, a packed weight
    g, gcam = _gpu(N, H, H, C), _gpu(N, _lib.ET_CAM_STRIDE)
    for call in (lambda: ops.backward_nhwc(spec, g, g, gcam, x),
                 lambda: ops.backward_nhwc(spec, g, g, cam, g),
                 lambda: ops.forward_nhwc(spec, g, g, gcam, res_bias=torch.zeros(C), want_res_base=True),
                 lambda: ops.residual_gemm(_gpu(3, 256), torch.zeros(8, dtype=torch.uint8), torch.zeros(256))):
        with pytest.raises(_lib.EpipolarAmdError, match="no CPU fallback"):
            call()


def test_backward_checks_dtype_and_shape_before_the_library(no_library):
    spec = ops.LayerSpec(H=H, W=H, K=K)
    x, cam = _gpu(N, H, H, C), _gpu(N, _lib.ET_CAM_STRIDE)
    with pytest.raises(TypeError, match="feat_ref"):
        ops.backward_nhwc(spec, _gpu(N, H, H, C, dtype=torch.float64), x, cam, x)
    with pytest.raises(TypeError, match="grad_out"):
        ops.backward_nhwc(spec, x, x, cam, _gpu(N, H, H, C, dtype=torch.float64))
    with pytest.raises(ValueError, match="feature maps"):
        ops.backward_nhwc(spec, x, _gpu(N, H, H, C + 4), cam, x)
    with pytest.raises(ValueError, match="feature maps"):
        ops.backward_nhwc(ops.LayerSpec(H=H + 1, W=H, K=K), x, x, cam, x)
    with pytest.raises(ValueError, match="cam"):
        ops.backward_nhwc(spec, x, x, _gpu(N, _lib.ET_CAM_STRIDE - 1), x)
    with pytest.raises(ValueError, match="grad_out"):
        ops.backward_nhwc(spec, x, x, cam, _gpu(N, H, H, C + 4))
    with pytest.raises(ValueError, match="contiguous"):
        ops.backward_nhwc(spec, _gpu(N, C, H, H).permute(0, 2, 3, 1), x, cam, x)
    # the checks that were assertions are raised errors (they must survive `python -O`)
    with pytest.raises(ValueError, match="contiguous"):
        ops.forward_nhwc(spec, x, _gpu(N, C, H, H).permute(0, 2, 3, 1), cam)
    with pytest.raises(ValueError, match="res_bias"):
        ops.forward_nhwc(spec, x, x, cam, res_bias=_gpu(C + 1), want_res_base=True)
    with pytest.raises(ValueError, match="256-channel"):
        ops.residual_gemm_pack(_gpu(256, 128))
    with pytest.raises(ValueError, match="bias"):
        ops.residual_gemm(_gpu(3, 256), _gpu(8, dtype=torch.uint8), _gpu(255))
    with pytest.raises(ValueError, match="feat"):
        ops.residual_gemm(_gpu(3, 256), _gpu(8, dtype=torch.uint8), _gpu(256), feat=_gpu(2, 256))


def _offset_buffer(nbytes=1024, past=16, fill=0xAB):
    """A host uint8 buffer whose address lies `past` bytes behind a 256-byte boundary."""
    raw = torch.full((nbytes + 512,), fill, dtype=torch.uint8)
    start = (-raw.data_ptr()) % 256 + past
    buf = raw[start:start + nbytes]
    assert buf.data_ptr() % 256 == past
    return buf


def test_workspace_header_is_read_from_the_aligned_base():
    buf = _offset_buffer()
    base = 256 - 16
    assert ops._aligned_base(buf) == base
    hdr = ops._header(buf)
    assert hdr.dtype == torch.int32 and hdr.numel() == 64 and hdr.data_ptr() == buf.data_ptr() + base and hdr.data_ptr() % 256 == 0
    hdr.zero_()
    hdr[ops._HEADER_ERROR] = 0x6
    assert buf[base + 4:base + 8].tolist() == [6, 0, 0, 0]              # word 1, little endian
    assert ops._read_tile_error(buf) == 6
    with pytest.raises(_lib.EpipolarAmdError, match="0x6"):
        ops.check_tile_errors(workspace=buf, reset=False)
    assert ops._read_tile_error(buf) == 6                                # reset=False: the word stays


def test_clearing_the_error_word_touches_no_other_byte():
    buf = _offset_buffer()
    base = 256 - 16
    buf[base + 4:base + 8] = torch.tensor([6, 0, 0, 0], dtype=torch.uint8)
    want = buf.clone()
    want[base + 4:base + 8] = 0
    ops._clear_tile_error(buf)
    assert ops._read_tile_error(buf) == 0
    assert torch.equal(buf, want)                                        # everything else still 0xAB
    assert int((buf == 0xAB).sum()) == buf.numel() - 4
