"""CPU-side checks of the Meta fusion layer (no GPU): the fixture's recorded conditions (tests/golden/make_meta_golden.py), the host
algebra `camera.fundamental_matrices` against float64, the three et_meta_* exports in header, binding and library with their argument
checks, and the registry behind EPIPOLAR_AMD.META_FUSION."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

from epipolar_transformers_amd import _lib, build, camera

sys.path.insert(0, GOLDEN_DIR)
from make_meta_golden import GRAD_KEYS, HG_CASES, LAYER_CASES, LAYER_DIR, meta_inputs  # noqa: E402

LAYER_NAMES = [c["name"] for c in LAYER_CASES]
META_EXPORTS = ("et_meta_pack", "et_meta_gemm", "et_meta_wgrad_workspace_bytes", "et_meta_wgrad")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def _layer(case):
    return np.load(os.path.join(LAYER_DIR, "layer_%s.npz" % case))


@pytest.mark.parametrize("case", LAYER_NAMES)
def test_fixture_conditions_hold(case):
    """what the maker asserted, from the values it recorded -- and the shapes of the issue's four cases"""
    d = _layer(case)
    n, c, h, w = [int(v) for v in d["dims"]]
    assert (n, c, h * w) == {"n3_5x7": (3, 256, 35), "n2_5x13": (2, 256, 65), "n2_16x16": (2, 256, 256), "n1_5x7": (1, 256, 35)}[case]
    assert 0.5 <= float(d["max_abs_y"]) <= 20.0
    assert float(d["hyper_share"]) >= 0.25
    assert n == 1 or float(d["pair_contrast"]) >= 0.05
    assert float(d["ref_dist_y"]) < 1e-5
    for k in GRAD_KEYS:
        assert float(d["ref_dist_grad_" + k]) < 1e-5, k
    y = np.load(os.path.join(LAYER_DIR, "layer_%s_y.npz" % case))["y"]
    gin = np.load(os.path.join(LAYER_DIR, "layer_%s_gin.npz" % case))["grad_input"]
    assert y.shape == gin.shape == (n, c, h, w) and abs(float(np.abs(y).max()) - float(d["max_abs_y"])) < 1e-6
    # the stored float32 results against the stored samples of the float64 evaluation: the recorded distances are what they say
    assert np.abs(y.reshape(-1)[::17] - d["y_64s"]).max() <= float(d["ref_dist_y"]) * np.abs(y).max() * 1.001
    inp, feat, gout = meta_inputs(case)
    assert tuple(inp.shape) == (n, c, h, w) and float(inp.min()) == 0.0 and feat.shape == gout.shape == inp.shape


@pytest.mark.parametrize("case", LAYER_NAMES)
def test_fundamental_matrices_against_float64(case):
    """camera.fundamental_matrices against F64, per matrix, relative to its largest entry: within 4 x the reference's own recorded
    float32 distance from F64 (both are float32 evaluations of the same ill-conditioned formulas; the margin peaks_grad uses)."""
    d = _layer(case)
    F = camera.fundamental_matrices(torch.from_numpy(d["P_ref"]), torch.from_numpy(d["P_src"]))
    assert F.dtype == torch.float32 and F.device.type == "cpu" and tuple(F.shape) == d["F"].shape
    for i in range(F.shape[0]):
        scale = np.abs(d["F64"][i]).max()
        got = np.abs(F[i].numpy().astype(np.float64) - d["F64"][i]).max() / scale
        ref = np.abs(d["F"][i].astype(np.float64) - d["F64"][i]).max() / scale
        assert abs(ref - float(d["ref_dist_F"][i])) <= 1e-12 + 1e-6 * ref
        print("%s pair %d: ours %.2e, the reference's %.2e of max|F64|" % (case, i, got, ref))
        assert got <= 4.0 * ref, (case, i, got, ref)
    with pytest.raises(ValueError):
        camera.fundamental_matrices(torch.zeros(2, 3, 4), torch.zeros(3, 3, 4))


def test_fundamental_cache_is_keyed_by_value():
    d = _layer("n3_5x7")
    P1, P2 = torch.from_numpy(d["P_ref"]), torch.from_numpy(d["P_src"])
    cache = camera.PairAlgebraCache(algebra=camera.fundamental_matrices)
    a = cache.get(P1, P2, "cpu")
    assert cache.get(P1.clone(), P2.clone(), "cpu") is a and torch.equal(a, camera.fundamental_matrices(P1, P2))
    assert cache.get(P2, P1, "cpu") is not a
    assert camera.PairAlgebraCache().algebra is camera.pair_algebra         # (the epipolar layer's cache: unchanged)


def test_meta_exports_in_header_binding_and_library(lib):
    text = open(os.path.join(ROOT, "include", "epipolar_amd.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*(et_\w+)\(", text, flags=re.M))
    for name in META_EXPORTS:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert int(re.search(r"#define ET_ABI_VERSION (\d+)", text).group(1)) == 14 == _lib.ET_ABI_VERSION == lib.et_abi_version()
    assert re.search(r"^#define ET_HAS_META_FUSION 1$", text, flags=re.M) and _lib.ET_HAS_META_FUSION == 1
    # the header's parameter lists against the binding's argument types
    kinds = {"int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t}
    for name in META_EXPORTS:
        params = re.search(r"^(?:int|size_t)\s+%s\(([^)]*)\)" % name, text, flags=re.M).group(1).split(",")
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
        assert want == _lib._SIGNATURES[name][1], name


def test_meta_argument_checks_without_a_gpu(lib):
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    err = lambda: lib.et_last_error()
    assert lib.et_meta_pack(2, 128, null, null, 0, null, null) != 0 and b"256-channel" in err()
    assert lib.et_meta_pack(0, 256, null, null, 0, null, null) != 0 and b"bad sizes" in err()
    assert lib.et_meta_pack(2, 256, null, null, 0, null, null) != 0 and b"NULL" in err()
    assert lib.et_meta_pack(2, 256, one, null, 0, ctypes.c_void_p(24), null) != 0 and b"16-byte aligned" in err()
    assert lib.et_meta_pack(1 << 30, 256, one, null, 0, one, null) != 0 and b"too many" in err()
    assert lib.et_meta_gemm(2, 35, 128, *[null] * 6) != 0 and b"256-channel" in err()
    assert lib.et_meta_gemm(0, 35, 256, *[null] * 6) != 0 and b"bad sizes" in err()
    assert lib.et_meta_gemm(2, 0, 256, *[null] * 6) != 0 and b"bad sizes" in err()
    assert lib.et_meta_gemm(2, 35, 256, *[null] * 6) != 0 and b"NULL" in err()
    assert lib.et_meta_gemm(2, 35, 256, one, null, ctypes.c_void_p(24), null, one, null) != 0 and b"16-byte aligned" in err()
    assert lib.et_meta_gemm((1 << 31) - 1, 65, 256, one, null, one, null, one, null) != 0 and b"too many tiles" in err()
    assert lib.et_meta_wgrad(2, 35, 128, *[null] * 5, ctypes.c_size_t(0), null) != 0 and b"256-channel" in err()
    assert lib.et_meta_wgrad(2, -1, 256, *[null] * 5, ctypes.c_size_t(0), null) != 0 and b"bad sizes" in err()
    assert lib.et_meta_wgrad(2, 35, 256, *[null] * 5, ctypes.c_size_t(0), null) != 0 and b"NULL" in err()
    assert lib.et_meta_wgrad(2, 35, 256, one, one, one, null, one, ctypes.c_size_t(64), null) != 0 and b"smaller than" in err()
    assert lib.et_meta_wgrad(1 << 24, 35, 256, one, one, one, null, one, ctypes.c_size_t(1 << 62), null) != 0 and b"too many pairs" in err()
    # one partial result (256 x 256 + 256 floats) per block, ceil(HW / 2048) blocks per pair: a function of N and HW alone
    size = lambda n, hw: int(lib.et_meta_wgrad_workspace_bytes(n, hw))
    assert size(0, 35) == size(3, 0) == 0
    assert size(1, 35) == size(1, 2048) == (65536 + 256) * 4 and size(3, 2049) == 3 * 2 * (65536 + 256) * 4
    assert size(128, 4096) == 128 * 2 * (65536 + 256) * 4


def _cfg(body, knob):
    from epipolar_transformers_amd import default_cfg

    cfg = default_cfg()
    cfg.merge_from_list(["BACKBONE.BODY", body, "BACKBONE.PRETRAINED", False, "KEYPOINT.HEATMAP_SIZE", (16, 16), "DATASETS.IMAGE_SIZE", (64, 64),
                         "KEYPOINT.NUM_PTS", 7, "EPIPOLAR.PARAMETERIZED", ("z",), "EPIPOLAR.ZRESIDUAL", True] +
                        (["EPIPOLAR_AMD.META_FUSION", True] if knob else []))
    return cfg


def test_meta_names_raise_with_the_knob_off():
    from epipolar_transformers_amd import backbones, default_cfg

    assert default_cfg().EPIPOLAR_AMD.META_FUSION is False
    for body in ("metaHG", "metaHG1", "metaepipolarHG"):
        with pytest.raises(NotImplementedError, match="Meta fusion layer"):
            backbones.build_backbone(_cfg(body, False))


def test_meta_hourglass_has_the_references_state_dict_keys():
    from epipolar_transformers_amd import backbones
    from epipolar_transformers_amd.meta import Meta

    for c in HG_CASES:
        want = [str(k) for k in np.load(os.path.join(GOLDEN_DIR, "hourglass_meta_%s.npz" % c["name"]))["state_dict_keys"]]
        net = backbones.build_backbone(_cfg(c["body"], True))
        assert sorted(net.state_dict()) == want, c["body"]
        assert len(net.meta) == net.nStack and isinstance(net.testmeta, Meta) and not hasattr(net, "epipolar_sampler")
        assert tuple(net.meta[0].fc0.weight.shape) == (100, 9) and tuple(net.meta[0].fc1.weight.shape) == (65536, 100)
    # metaepipolarHG* builds what epipolarHG* builds ('metaHG' in 'metaepipolarHG' is false, 'epipolarHG' in it is true)
    a, b = backbones.build_backbone(_cfg("metaepipolarHG1", True)), backbones.build_backbone(_cfg("epipolarHG1", True))
    assert sorted(a.state_dict()) == sorted(b.state_dict()) and hasattr(a, "epipolar_sampler") and not hasattr(a, "meta")


def test_meta_rejects_other_channel_counts_and_cpu_tensors():
    from epipolar_transformers_amd import ops
    from epipolar_transformers_amd.meta import Meta

    with pytest.raises(ValueError, match="KEYPOINT.NFEATS"):
        Meta(128)
    x = torch.zeros(1, 4, 256)
    with pytest.raises(_lib.EpipolarAmdError):                                   # no CPU fallback
        ops.meta_fuse(x, torch.zeros(1, 256, 256), torch.zeros(256, 256), torch.zeros(256))
