"""CPU-side checks of ABI 14, the deterministic tiled backward (no GPU): the three new symbols in header, binding and library;
the workspace size; and the quantum -- the bound of include/epipolar_amd.h through the host hook et_debug_host_det_quantum."""
import ctypes
import math
import os
import re

import pytest

from conftest import ROOT

from epipolar_transformers_amd import _lib, build, ops

NEW = ("et_epipolar_backward_tiled_det_workspace_bytes", "et_epipolar_backward_tiled_det", "et_debug_host_det_quantum")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_abi_14_and_the_new_symbols(lib):
    text = open(os.path.join(ROOT, "include", "epipolar_amd.h")).read()
    assert int(re.search(r"#define ET_ABI_VERSION (\d+)", text).group(1)) == 14 == _lib.ET_ABI_VERSION == lib.et_abi_version()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*(et_\w+)\(", text, flags=re.M))
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert int(re.search(r"#define ET_VARIANT_BWD_DETERMINISTIC (\d+)", text).group(1)) == 4194304 == _lib.ET_VARIANT_BWD_DETERMINISTIC


SHAPES = [dict(N=2, C=256, H=64, W=64, K=64), dict(N=128, C=256, H=64, W=64, K=64), dict(N=3, C=256, H=96, W=96, K=64),
          dict(N=2, C=256, H=128, W=128, K=128), dict(N=1, C=256, H=16, W=16, K=16), dict(N=2, C=256, H=33, W=20, K=20),
          dict(N=2, C=64, H=16, W=16, K=16), dict(N=2, C=256, H=160, W=160, K=64), dict(N=2, C=36, H=9, W=7, K=5),
          dict(N=0, C=256, H=16, W=16, K=16), dict(N=2, C=256, H=64, W=64, K=64, variant=32768),
          dict(N=2, C=256, H=64, W=64, K=256, variant=32768), dict(N=2, C=256, H=64, W=64, K=64, softmax_enabled=False)]


@pytest.mark.parametrize("s", SHAPES, ids=lambda s: "-".join("%s%s" % kv for kv in s.items()))
def test_workspace_bytes(lib, s):
    s = dict(s)
    spec = ops.LayerSpec(H=s["H"], W=s["W"], K=s["K"], variant=s.pop("variant", 0), softmax_enabled=s.pop("softmax_enabled", True))
    d = spec.desc(s["N"], s["C"])
    tiled = int(lib.et_epipolar_backward_tiled_workspace_bytes(ctypes.byref(d)))
    det = int(lib.et_epipolar_backward_tiled_det_workspace_bytes(ctypes.byref(d)))
    assert (det == 0) == (tiled == 0)
    if tiled:
        assert det >= tiled + s["N"] * s["H"] * s["W"] * 256 * 8


def test_null_and_small_workspace_and_softmax_off_are_errors(lib):
    null = ctypes.c_void_p(0)
    d = ops.LayerSpec(H=16, W=16, K=16).desc(2, 256)
    assert lib.et_epipolar_backward_tiled_det(ctypes.byref(d), *[null] * 11, ctypes.c_size_t(0), null) != 0
    assert b"NULL" in lib.et_last_error()
    one = ctypes.c_void_p(16)          # (never dereferenced: the checks below come first)
    assert lib.et_epipolar_backward_tiled_det(ctypes.byref(d), *[one] * 6, null, *[one] * 4, ctypes.c_size_t(1024), null) != 0
    assert b"smaller than" in lib.et_last_error()
    d = ops.LayerSpec(H=16, W=16, K=16).desc(2, 64)
    assert lib.et_epipolar_backward_tiled_det(ctypes.byref(d), *[one] * 6, null, *[one] * 4, ctypes.c_size_t(1 << 30), null) != 0
    assert b"C == 256" in lib.et_last_error()
    q, b = ctypes.c_float(), ctypes.c_float()
    d = ops.LayerSpec(H=16, W=16, K=16, softmax_enabled=False).desc(2, 256)
    assert lib.et_debug_host_det_quantum(ctypes.byref(d), 1.0, 1.0, 1.0, ctypes.byref(q), ctypes.byref(b)) != 0
    assert b"soft-max" in lib.et_last_error()


MAXIMA = [1e-6, 1e-3, 0.37, 1.0, 7.0, 1e3, 1e6]


@pytest.mark.parametrize("scale", [0.0, 1e-3, 0.125, 1.0, 8.0, -0.125])
def test_quantum_over_a_grid_of_maxima(lib, scale):
    d = ops.LayerSpec(H=64, W=64, K=64, softmax_scale=scale).desc(2, 256)
    q, b = ctypes.c_float(), ctypes.c_float()
    for m_ref in MAXIMA:
        for m_src in MAXIMA:
            for m_g in MAXIMA:
                assert lib.et_debug_host_det_quantum(ctypes.byref(d), m_ref, m_src, m_g, ctypes.byref(q), ctypes.byref(b)) == 0
                qv, bv = float(q.value), float(b.value)
                # the bound of the header: 32 (2 |scale| 256 M_g M_src M_ref + M_g), and some slack for the products' rounding
                want = 32.0 * (2.0 * abs(scale) * 256.0 * m_g * m_src * m_ref + m_g)
                assert want <= bv <= want * 1.02
                mant, _ = math.frexp(qv)
                assert mant == 0.5 and qv >= 2.0 ** -100, qv                     # a normal power of two
                assert bv * 2.0 ** 14 / qv < 2.0 ** 62
                if qv > 2.0 ** -100:                                             # away from the clamp: 47 bits at the bound
                    assert bv / qv >= 2.0 ** 47


def test_quantum_of_zero_and_of_vanishing_gradients(lib):
    d = ops.LayerSpec(H=64, W=64, K=64).desc(2, 256)
    q, b = ctypes.c_float(), ctypes.c_float()
    assert lib.et_debug_host_det_quantum(ctypes.byref(d), 1.0, 1.0, 0.0, ctypes.byref(q), ctypes.byref(b)) == 0
    assert b.value == 0.0 and q.value == 1.0
    assert lib.et_debug_host_det_quantum(ctypes.byref(d), 1.0, 1.0, 1e-30, ctypes.byref(q), ctypes.byref(b)) == 0
    assert q.value == 2.0 ** -100 and 0 < b.value * 2.0 ** 14 / q.value < 2.0 ** 62


def test_the_variant_bit_reaches_no_kernel():
    """LayerSpec.desc() strips ET_VARIANT_BWD_DETERMINISTIC (the binding reads it; the forward must stay the default forward),
    and the knob sets it."""
    from epipolar_transformers_amd import default_cfg
    from epipolar_transformers_amd.epipolar import Epipolar

    bit = _lib.ET_VARIANT_BWD_DETERMINISTIC
    assert ops.LayerSpec(H=16, W=16, K=16, variant=bit | 32768).desc(1, 256).variant == 32768
    cfg = default_cfg()
    assert cfg.EPIPOLAR_AMD.DETERMINISTIC is False
    assert Epipolar(cfg=cfg).layer_spec().variant & bit == 0
    cfg = default_cfg()
    cfg.merge_from_list(["EPIPOLAR_AMD.DETERMINISTIC", True])
    assert Epipolar(cfg=cfg).layer_spec().variant & bit == bit
