"""CPU-side checks of the pair table (ET_HAS_PAIR_INDEX, no GPU): the three *_ix symbols in header, binding and library with the
ABI number unchanged; the host validation of an index (ValueError before anything touches a device); and the rule that sends a
call to the gathered route (ops.pair_index_applies)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

from epipolar_transformers_amd import _lib, build, ops

NEW = ("et_epipolar_forward_tiled_ix", "et_epipolar_forward_fused_ix", "et_epipolar_backward_tiled_ix")
SIBLING = {"et_epipolar_forward_tiled_ix": "et_epipolar_forward_tiled", "et_epipolar_forward_fused_ix": "et_epipolar_forward_fused",
           "et_epipolar_backward_tiled_ix": "et_epipolar_backward_tiled_ga"}


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_the_three_symbols_the_macro_and_the_abi_number(lib):
    text = open(os.path.join(ROOT, "include", "epipolar_amd.h")).read()
    assert int(re.search(r"#define ET_ABI_VERSION (\d+)", text).group(1)) == 14 == _lib.ET_ABI_VERSION == lib.et_abi_version()
    assert re.search(r"^#define ET_HAS_PAIR_INDEX 1$", text, flags=re.M) and _lib.ET_HAS_PAIR_INDEX == 1
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*(et_\w+)\(", text, flags=re.M))
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
        # its sibling's arguments + (ref_index, src_index, M_ref, M_src)
        assert _lib._SIGNATURES[name][1] == _lib._SIGNATURES[SIBLING[name]][1] + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                                                                 ctypes.c_int32]


def test_the_entry_points_check_their_pools_before_any_launch(lib):
    """Pool sizes are checked on the host, in front of every other check: no pointer of these calls is dereferenced."""
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    d = ops.LayerSpec(H=16, W=16, K=16).desc(6, 256)
    tail = (ctypes.c_size_t(1 << 30), null)
    calls = {"et_epipolar_forward_tiled_ix": [one] * 12, "et_epipolar_backward_tiled_ix": [one] * 12,
             "et_epipolar_forward_fused_ix": [one] * 12 + [0, one]}          # (+ want_out, workspace)
    for name, args in calls.items():
        fn = getattr(lib, name)
        assert fn(ctypes.byref(d), *args, *tail, one, one, 0, 4) != 0 and b"pools" in lib.et_last_error(), name
        assert fn(ctypes.byref(d), *args, *tail, one, one, 4, -1) != 0 and b"pools" in lib.et_last_error(), name
        # a NULL index is the identity: its pool holds exactly N maps
        assert fn(ctypes.byref(d), *args, *tail, null, one, 4, 4) != 0 and b"ref_index is NULL" in lib.et_last_error(), name
        assert fn(ctypes.byref(d), *args, *tail, one, null, 4, 4) != 0 and b"src_index is NULL" in lib.et_last_error(), name
    # and behind them the siblings' own checks, under the indexed name
    assert lib.et_epipolar_forward_tiled_ix(ctypes.byref(d), *[null] * 12, ctypes.c_size_t(0), null, null, null, 6, 6) != 0
    assert b"et_epipolar_forward_tiled_ix: NULL" in lib.et_last_error()
    assert lib.et_epipolar_backward_tiled_ix(ctypes.byref(d), *[one] * 12, ctypes.c_size_t(1024), null, one, one, 4, 4) != 0
    assert b"smaller than" in lib.et_last_error()
    d64 = ops.LayerSpec(H=16, W=16, K=16).desc(6, 64)
    assert lib.et_epipolar_forward_tiled_ix(ctypes.byref(d64), *[one] * 12, *tail, one, one, 4, 4) != 0
    assert b"C == 256" in lib.et_last_error()


BAD = [([0, 1, 2], "length"),                                      # wrong length (N = 6)
       ([0, 1, 2, 3, 0, 1, 2], "length"),
       ([0, 1, 2, -1, 0, 3], "outside"),                           # negative
       ([0, 1, 2, 4, 0, 3], "outside"),                            # >= M (M = 4)
       ([0.0, 1.0, 2.0, 3.0, 0.0, 3.0], "integer"),                # float dtype
       (torch.tensor([0, 1, 2, 3, 0, 3], dtype=torch.float32), "integer"),
       (torch.tensor([0, 1, 2, 3, 0, 4], dtype=torch.int64), "outside"),
       (np.array([[0, 1, 2], [3, 0, 3]]), "length")]


@pytest.mark.parametrize("index,word", BAD, ids=[str(i) for i in range(len(BAD))])
def test_index_validation_raises_value_error_on_the_host(index, word):
    with pytest.raises(ValueError, match=word):
        ops.check_pair_index(index, "src_index", 6, 4)
    # through the public wrappers, with tensors that live on the CPU: the index is judged before the device of anything is
    # (a CPU feature map is an EpipolarAmdError, which the good index below reaches)
    spec = ops.LayerSpec(H=12, W=20, K=16)
    pool, cam = torch.zeros(4, 12, 20, 256), torch.zeros(6, _lib.ET_CAM_STRIDE)
    good = [1, 2, 3, 0, 2, 2]
    for call in (lambda **kw: ops.forward_nhwc(spec, pool, pool, cam, **kw),
                 lambda **kw: ops.forward_fused_nhwc(spec, pool, pool, cam, torch.zeros(1, dtype=torch.uint8), torch.zeros(256), **kw),
                 lambda **kw: ops.backward_nhwc(spec, pool, pool, cam, torch.zeros(6, 12, 20, 256), **kw)):
        with pytest.raises(ValueError, match=word):
            call(ref_index=good, src_index=index)
        with pytest.raises(ValueError, match=word):
            call(ref_index=index, src_index=good)
        with pytest.raises(_lib.EpipolarAmdError, match="no CPU fallback"):
            call(ref_index=good, src_index=good)


def test_a_good_index_becomes_int32_whatever_it_came_as():
    want = np.array([1, 2, 3, 0, 2, 2], np.int32)
    for index in ([1, 2, 3, 0, 2, 2], (1, 2, 3, 0, 2, 2), np.array(want, np.int64), torch.tensor(want.tolist()),
                  torch.tensor(want.tolist(), dtype=torch.int32), torch.tensor(want.tolist(), dtype=torch.uint8)):
        got = ops.check_pair_index(index, "src_index", 6, 4)
        assert got.dtype == np.int32 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, want)


def test_pair_index_applies_names_every_fallback(lib):
    spec = ops.LayerSpec(H=12, W=20, K=16)
    for form in ("forward", "fused", "tile"):
        assert ops.pair_index_applies(spec, 256, form) is True
        assert ops.pair_index_applies(spec, 8, form) is False and ops.pair_index_applies(spec, 128, form) is False     # C != 256
        det = ops.LayerSpec(H=12, W=20, K=16, variant=_lib.ET_VARIANT_BWD_DETERMINISTIC)
        assert ops.pair_index_applies(det, 256, form) is False                                  # the deterministic variant
    # the deterministic tile backward, the gather and atomic per-pixel backward, the per-pixel forward, the general kernels
    for form in ("tile_det", "gather", "atomic", "pixel", "general"):
        assert ops.pair_index_applies(spec, 256, form) is False
    # a variant bit that leaves the tile path: the per-pixel kernels
    no_tile = ops.LayerSpec(H=12, W=20, K=16, variant=_lib.ET_VARIANT_NO_TILE)
    assert all(ops.pair_index_applies(no_tile, 256, form) is False for form in ("forward", "fused", "tile"))
    assert ops.pair_index_applies(ops.LayerSpec(H=12, W=20, K=16, variant=_lib.ET_VARIANT_BWD_ATOMIC), 256, "tile") is False
    # the bits that tune the tile path stay on it
    for bit in (_lib.ET_VARIANT_WS_BAND, _lib.ET_VARIANT_TILE_CLASSIC, _lib.ET_VARIANT_TILE_CLASSIC | _lib.ET_VARIANT_TILE_EXACT,
                _lib.ET_VARIANT_TILE_SPLIT):
        assert ops.pair_index_applies(ops.LayerSpec(H=12, W=20, K=16, variant=bit), 256, "forward") is True
    assert ops.pair_index_applies(ops.LayerSpec(H=12, W=20, K=16, variant=_lib.ET_VARIANT_BWD_SPLIT_IN_PLACE), 256, "tile") is True
    # shapes the tile path does not take; the one-kernel layer's narrower range (K <= 64, soft-max on, no classic kernel)
    assert ops.pair_index_applies(ops.LayerSpec(H=160, W=160, K=16), 256, "forward") is False
    assert ops.pair_index_applies(ops.LayerSpec(H=12, W=20, K=80), 256, "forward") is True
    assert ops.pair_index_applies(ops.LayerSpec(H=12, W=20, K=80), 256, "fused") is False
    assert ops.pair_index_applies(ops.LayerSpec(H=12, W=20, K=16, softmax_enabled=False), 256, "fused") is False
    assert ops.pair_index_applies(ops.LayerSpec(H=12, W=20, K=16, variant=_lib.ET_VARIANT_TILE_CLASSIC), 256, "fused") is False
    with pytest.raises(ValueError):
        ops.pair_index_applies(spec, 256, "sideways")


def test_the_knob_and_the_signatures():
    """EPIPOLAR_AMD.PAIR_INDEX exists and is off by default; every layer of the call path takes the two indices, defaulting to None."""
    from epipolar_transformers_amd import default_cfg
    from epipolar_transformers_amd.backbones import PoseResNet
    from epipolar_transformers_amd.epipolar import Epipolar

    assert default_cfg().EPIPOLAR_AMD.PAIR_INDEX is False
    for fn in (ops.forward_nhwc, ops.forward_fused_nhwc, ops.backward_nhwc, Epipolar.forward, Epipolar.forward_fused, Epipolar.attend,
               PoseResNet._fuse, ops.EpipolarAttendIndexed.forward):
        par = inspect.signature(fn).parameters
        assert par["ref_index"].default is None and par["src_index"].default is None, fn
