"""CPU-side checks of the gradient through the returned attention (ET_HAS_ATTN_GRAD, no GPU): the five *_ga symbols in header,
binding and library with the ABI number unchanged; their argument checks; and the deterministic form's quantum with the
max |grad_attn| term -- the bound of include/epipolar_amd.h,
    32 (2 |scale| (256 M_g M_src + M_ga) M_ref + M_g) (1 + 1/64),
through the host hook et_debug_host_det_quantum_ga."""
import ctypes
import math
import os
import re
import struct

import pytest

from conftest import ROOT

from epipolar_transformers_amd import _lib, build, ops

NEW = ("et_epipolar_backward_ga", "et_epipolar_backward_tiled_ga", "et_epipolar_backward_tiled_det_ga",
       "et_debug_host_det_quantum_ga", "et_epipolar_backward_general_ga")
MAXIMA = [1e-6, 1e-3, 0.37, 1.0, 7.0, 1e3, 1e6]            # the grid of tests/test_det_abi_cpu.py
SCALES = [0.0, 1e-3, 0.125, 1.0, 8.0, -0.125]


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def _bits(x: float) -> bytes:
    return struct.pack("<f", x)


def test_the_five_symbols_and_the_abi_number(lib):
    text = open(os.path.join(ROOT, "include", "epipolar_amd.h")).read()
    assert int(re.search(r"#define ET_ABI_VERSION (\d+)", text).group(1)) == 14 == _lib.ET_ABI_VERSION == lib.et_abi_version()
    assert re.search(r"^#define ET_HAS_ATTN_GRAD 1$", text, flags=re.M)
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*(et_\w+)\(", text, flags=re.M))
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert "are not provided" not in text        # the sentence about missing attention gradients is gone


def test_null_pointers_and_a_small_workspace_are_errors(lib):
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)          # (`one` is never dereferenced: the checks come first)
    d = ops.LayerSpec(H=16, W=16, K=16).desc(2, 256)
    for name in ("et_epipolar_backward_tiled_ga", "et_epipolar_backward_tiled_det_ga"):
        fn = getattr(lib, name)
        assert fn(ctypes.byref(d), *[null] * 12, ctypes.c_size_t(0), null) != 0
        assert b"NULL" in lib.et_last_error()
        # attn and grad_attn are the nullable ones: grad_out is not
        assert fn(ctypes.byref(d), *[one] * 6, null, null, one, one, one, one, ctypes.c_size_t(1 << 30), null) != 0
        assert b"NULL" in lib.et_last_error()
        assert fn(ctypes.byref(d), *[one] * 6, null, one, null, one, one, one, ctypes.c_size_t(1024), null) != 0
        assert b"smaller than" in lib.et_last_error()
        d64 = ops.LayerSpec(H=16, W=16, K=16).desc(2, 64)
        assert fn(ctypes.byref(d64), *[one] * 6, null, one, one, one, one, one, ctypes.c_size_t(1 << 30), null) != 0
        assert b"C == 256" in lib.et_last_error()
    doff = ops.LayerSpec(H=16, W=16, K=16, softmax_enabled=False).desc(2, 256)
    need = int(lib.et_epipolar_backward_tiled_det_workspace_bytes(ctypes.byref(doff)))
    assert lib.et_epipolar_backward_tiled_det_ga(ctypes.byref(doff), *[one] * 6, null, one, one, one, one, one, ctypes.c_size_t(need), null) != 0
    assert b"soft-max" in lib.et_last_error()
    # per-pixel form: grad_out NULL; a workspace that is too small for the gather form
    d8 = ops.LayerSpec(H=10, W=10, K=16).desc(2, 8)
    assert lib.et_epipolar_backward_ga(ctypes.byref(d8), *[one] * 6, null, one, one, one, null, ctypes.c_size_t(0), null) != 0
    assert b"NULL" in lib.et_last_error()
    assert lib.et_epipolar_backward_ga(ctypes.byref(d8), *[one] * 7, null, one, one, one, ctypes.c_size_t(64), null) != 0
    assert b"smaller than" in lib.et_last_error()
    # general form: grad_out NULL, grad_attn given
    assert lib.et_epipolar_backward_general_ga(ctypes.byref(d8), *[one] * 7, null, null, one, 8, 8, 0, one, one, one, null, null) != 0
    assert b"NULL" in lib.et_last_error()
    assert lib.et_epipolar_backward_general_ga(ctypes.byref(d8), *[one] * 7, null, one, one, 8, 8, 64, one, one, one, null, null) != 0
    assert b"unknown flag" in lib.et_last_error()
    q, b = ctypes.c_float(), ctypes.c_float()
    assert lib.et_debug_host_det_quantum_ga(ctypes.byref(doff), 1.0, 1.0, 1.0, 1.0, ctypes.byref(q), ctypes.byref(b)) != 0
    assert b"soft-max" in lib.et_last_error()
    assert lib.et_debug_host_det_quantum_ga(ctypes.byref(d), 1.0, 1.0, 1.0, -1.0, ctypes.byref(q), ctypes.byref(b)) != 0
    assert b">= 0" in lib.et_last_error()


def test_the_workspace_size_is_unchanged(lib):
    """M_ga lives in the maxima region the deterministic form already has: N H W 256 x 8 bytes of accumulator, 16 bytes of quanta
    and 32 x 16 bytes of partial maxima per pair, and at most 256 bytes of alignment, behind the tile workspace."""
    for n, h, w, k in ((2, 64, 64, 64), (3, 33, 20, 20), (1, 16, 16, 16)):
        d = ops.LayerSpec(H=h, W=w, K=k).desc(n, 256)
        tiled = int(lib.et_epipolar_backward_tiled_workspace_bytes(ctypes.byref(d)))
        det = int(lib.et_epipolar_backward_tiled_det_workspace_bytes(ctypes.byref(d)))
        assert det == tiled + 256 + n * h * w * 256 * 8 + n * 16 + n * 32 * 16


@pytest.mark.parametrize("scale", SCALES)
def test_quantum_without_grad_attn_is_todays_bits(lib, scale):
    d = ops.LayerSpec(H=64, W=64, K=64, softmax_scale=scale).desc(2, 256)
    q0, b0, q1, b1 = ctypes.c_float(), ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
    for m_ref in MAXIMA + [0.0]:
        for m_src in MAXIMA + [0.0]:
            for m_g in MAXIMA + [0.0]:
                assert lib.et_debug_host_det_quantum(ctypes.byref(d), m_ref, m_src, m_g, ctypes.byref(q0), ctypes.byref(b0)) == 0
                assert lib.et_debug_host_det_quantum_ga(ctypes.byref(d), m_ref, m_src, m_g, 0.0, ctypes.byref(q1), ctypes.byref(b1)) == 0
                assert _bits(q0.value) == _bits(q1.value) and _bits(b0.value) == _bits(b1.value), (m_ref, m_src, m_g)


@pytest.mark.parametrize("scale", SCALES)
def test_quantum_with_grad_attn_over_the_grid(lib, scale):
    d = ops.LayerSpec(H=64, W=64, K=64, softmax_scale=scale).desc(2, 256)
    q, b = ctypes.c_float(), ctypes.c_float()
    for m_ref in MAXIMA:
        for m_src in MAXIMA:
            for m_g in MAXIMA:
                for m_ga in MAXIMA:
                    assert lib.et_debug_host_det_quantum_ga(ctypes.byref(d), m_ref, m_src, m_g, m_ga, ctypes.byref(q), ctypes.byref(b)) == 0
                    qv, bv = float(q.value), float(b.value)
                    want = 32.0 * (2.0 * abs(scale) * (256.0 * m_g * m_src + m_ga) * m_ref + m_g)
                    assert want <= bv <= want * 1.02, (m_ref, m_src, m_g, m_ga, want, bv)
                    mant, _ = math.frexp(qv)
                    assert mant == 0.5 and qv >= 2.0 ** -100, qv                 # a normal power of two
                    assert bv * 2.0 ** 14 / qv < 2.0 ** 62
                    if qv > 2.0 ** -100:
                        assert bv / qv >= 2.0 ** 47


def test_a_loss_on_the_attention_alone_gets_a_quantum(lib):
    """M_g = 0, M_ga = 1: the formula without M_ga gives bound 0 and q = 1 (nothing to scale); with it the similarity path's
    contributions, up to 32 x 2 |scale| M_ga M_ref, get their own power of two."""
    d = ops.LayerSpec(H=64, W=64, K=64).desc(2, 256)
    q, b = ctypes.c_float(), ctypes.c_float()
    assert lib.et_debug_host_det_quantum(ctypes.byref(d), 1.0, 1.0, 0.0, ctypes.byref(q), ctypes.byref(b)) == 0
    assert b.value == 0.0 and q.value == 1.0
    assert lib.et_debug_host_det_quantum_ga(ctypes.byref(d), 1.0, 1.0, 0.0, 1.0, ctypes.byref(q), ctypes.byref(b)) == 0
    want = 32.0 * 2.0 * 0.125
    assert want <= b.value <= want * 1.02 and b.value > 0
    mant, exp = math.frexp(float(q.value))
    assert mant == 0.5 and 2.0 ** -100 < q.value < 1.0
    assert b.value * 2.0 ** 14 / q.value < 2.0 ** 62 and b.value / q.value >= 2.0 ** 47


def test_the_knob_and_the_autograd_signatures():
    """EPIPOLAR_AMD.ATTN_GRAD exists, is off by default, and the attend functions take the trailing switch."""
    import inspect

    from epipolar_transformers_amd import default_cfg
    from epipolar_transformers_amd.epipolar import Epipolar

    cfg = default_cfg()
    assert cfg.EPIPOLAR_AMD.ATTN_GRAD is False
    assert Epipolar(cfg=cfg)._attn_grad() is False
    cfg = default_cfg()
    cfg.merge_from_list(["EPIPOLAR_AMD.ATTN_GRAD", True])
    assert Epipolar(cfg=cfg)._attn_grad() is True
    for fn in (ops.EpipolarAttend, ops.GeneralAttend):
        par = list(inspect.signature(fn.forward).parameters.values())[-1]
        assert par.name == "attn_grad" and par.default is False
    for fn in (ops.backward_nhwc, ops.backward_general_nhwc):
        assert inspect.signature(fn).parameters["grad_attn"].default is None
