"""Non-finite feature maps, incoming gradients and prior tables on the CPU: the C oracle, the reference's op sequence in torch
(oracle/torch_ref_path.py) and the module's torch restatement (Epipolar._attend_general_chunk with the stock-op epilogue) against
what the REAL reference returned for them (tests/golden/nonfinite/, tests/golden/make_nonfinite_golden.py).

The fixture is the yardstick.  The GPU tests (tests/test_gpu_nonfinite.py) compare the kernels with the fixture directly and take
nothing from the oracle, so what the oracle is held to here is the same three rules:
  R1 a non-finite value of the reference is non-finite here, and of the same kind (NaN, +Inf, -Inf);
  R2 a finite value of the reference is finite here, within the tolerances tests/test_oracle_golden.py uses on finite inputs;
  R3 corr_pos is the reference's at every pixel (torch.argmax: the first NaN wins, then the value, then the lowest index)."""
import numpy as np
import pytest
import torch

import nonfinite_fixture as nf

HEAD = nf.all_cases("head_") + nf.all_cases("pixel_")
HEAD_FWD = [c for c in HEAD if not c[1].startswith("gout_")] + nf.all_cases("cap_")    # (an incoming gradient does not enter the forward; cap_: forward only)
MODES = nf.all_cases("mode_")
_ids = lambda cs: ["%s-%s" % c for c in cs]


def test_fixtures_present():
    """every shape of the issue has its file, every file its NaN / +Inf / -Inf case of every site"""
    assert set(nf.names()) >= {"head_10x10_c256_k16", "head_10x10_c256_k101", "head_nosoftmax_10x10_c256_k16", "cap_16x16_c256_k16", "pixel_16x16_c8_k8", "pixel_nosoftmax_16x16_c8_k8",
                               "mode_param_pool_c16_k16", "mode_attention_max_c8_k8", "mode_cosine_c8_k8", "mode_prior_add_c8_k8",
                               "mode_prior_mul_c8_k8"}
    for name in nf.names():
        cs = nf.cases(name)
        sites = {c.split(".")[0] for c in cs}
        assert sites | ({"gout_one"} if name.startswith("cap_") else set()) >= {"src_one", "src_all", "ref_one", "ref_zero", "gout_one", "src_stale",
                                                                                  "src_corner_one", "src_corner_all"}, (name, sites)
        assert ("prior_one" in sites) == ("prior" in name), (name, sites)
        for s in sites:
            assert {c.split(".")[1] for c in cs if c.startswith(s + ".")} == {"nan", "pinf", "ninf"}, (name, s)
        d = nf.load(name)
        assert not np.array_equal(d["ref_one.nan.site"], d["ref_zero.nan.site"]), name
    # a sample exactly on a source grid point (zero-weight taps the reference still multiplies) exists in the K = 101 lines
    assert "src_grid.nan" in nf.cases("head_10x10_c256_k101")


def _spec(orc, d):
    m = d["dims"]
    return orc.LayerSpec(m["H"], m["W"], m["K"], downsample=float(d["downsample"]), correct_normalize=m["correct"],
                         softmax_scale=float(d["softmax_scale"]), softmax_enabled=m["softmax"], align_corners=False)


@pytest.fixture(scope="module")
def locs_of(oracle_mod):
    memo = {}

    def get(name):
        if name not in memo:
            d = nf.load(name)
            memo[name] = oracle_mod.sample_locs(_spec(oracle_mod, d), None, None, cam=d["cam"])
            assert np.array_equal(memo[name][:, nf.POISONED], d["sample_locs1"])          # bit-equal to the reference's
        return memo[name]
    return get


@pytest.mark.parametrize("name,case", HEAD_FWD, ids=_ids(HEAD_FWD))
def test_oracle_forward(oracle_mod, locs_of, name, case):
    d = nf.load(name)
    f1, f2, _, _ = nf.poisoned_inputs(d, case)
    locs = locs_of(name)
    r = oracle_mod.forward(_spec(oracle_mod, d), f1, f2, None, None, locs=locs)
    n = nf.POISONED
    want_attn, want_out = nf.expected(d, case, "attn"), nf.expected(d, case, "out")
    nf.check_values(r["attn"][n], want_attn, 1e-6 + 2e-6 * float(np.abs(d["attn1"]).max()), what="attn")
    nf.check_values(r["out"][n], want_out, 5e-6 + 2e-6 * float(np.abs(d["out1"]).max()), what="out")
    nf.check_corr_pos(d, case, locs, r["corr_pos"], r["attn"])


@pytest.mark.parametrize("name,case", HEAD, ids=_ids(HEAD))
def test_oracle_backward(oracle_mod, locs_of, name, case):
    d = nf.load(name)
    f1, f2, g, _ = nf.poisoned_inputs(d, case)
    g1, g2 = oracle_mod.backward(_spec(oracle_mod, d), f1, f2, locs_of(name), g)
    for got, o in ((g1, "grad_feat1"), (g2, "grad_feat2")):
        nf.check_values(got[nf.POISONED], nf.expected(d, case, o), 1e-4 * float(np.abs(d[o + "1"]).max()), what=o)


@pytest.mark.parametrize("name,case", HEAD_FWD, ids=_ids(HEAD_FWD))
def test_torch_op_sequence(locs_of, name, case):
    from oracle import torch_ref_path as trp

    d = nf.load(name)
    f1, f2, _, _ = nf.poisoned_inputs(d, case)
    m, locs = d["dims"], locs_of(name)
    out, attn, corr = trp.forward(torch.from_numpy(f1), torch.from_numpy(f2), torch.from_numpy(locs),
                                  softmax_scale=float(d["softmax_scale"]), softmax_enabled=m["softmax"], correct_normalize=m["correct"])
    n = nf.POISONED
    nf.check_values(attn.numpy()[n], nf.expected(d, case, "attn"), 1e-6 * max(1.0, float(np.abs(d["attn1"]).max())), what="attn")
    nf.check_values(out.numpy()[n], nf.expected(d, case, "out"), 5e-6 * max(1.0, float(np.abs(d["out1"]).max())), what="out")
    nf.check_corr_pos(d, case, locs, corr.numpy(), attn.numpy())


def _mode_module(d, prior1, oracle_mod, monkeypatch):
    """The product module of a mode fixture on the CPU: the reference's parameters, the fixture's camera algebra, and the sample
    locations from the C oracle in place of the HIP geometry kernel (bit-equal to the reference's, asserted)."""
    from epipolar_transformers_amd import default_cfg, ops
    from epipolar_transformers_amd.epipolar import Epipolar

    m = d["dims"]
    cfg = default_cfg()
    cfg.merge_from_list(["KEYPOINT.HEATMAP_SIZE", (m["H"], m["H"]), "KEYPOINT.NFEATS", m["C"], "EPIPOLAR.SAMPLESIZE", m["K"],
                         "DATASETS.IMAGE_SIZE", (m["image"], m["image"]), "EPIPOLAR.USE_CORRECT_NORMALIZE", True,
                         "EPIPOLAR.ATTENTION", "avg", "EPIPOLAR.PARAMETERIZED", ("z",), "EPIPOLAR.ZRESIDUAL", True,
                         "EPIPOLAR.MERGE", "late", "EPIPOLAR.SHARE_WEIGHTS", True] + [str(v) for v in d["overrides"]])
    mod = Epipolar(cfg=cfg).eval()
    sd = {k[3:]: torch.from_numpy(np.array(d[k])) for k in d if k.startswith("sd.")}
    assert sorted(mod.state_dict()) == sorted(sd)
    mod.load_state_dict(sd)
    for k in d:
        if k.startswith("prior."):
            _, i, j = k.split(".")
            v = prior1 if (prior1 is not None and k == "prior.2.3") else d[k]
            mod.prior[(int(i), int(j))] = torch.nn.Parameter(torch.from_numpy(np.array(v)))
    cam = torch.from_numpy(np.array(d["cam"]))
    mod._cams.get = lambda *a, **k: cam
    spec = mod.layer_spec()
    ospec = oracle_mod.LayerSpec(spec.H, spec.W, spec.K, downsample=spec.downsample, correct_normalize=spec.correct_normalize,
                                 softmax_scale=spec.softmax_scale, softmax_enabled=spec.softmax_enabled, align_corners=False)
    locs = oracle_mod.sample_locs(ospec, None, None, cam=d["cam"])
    assert np.array_equal(locs[:, nf.POISONED], d["sample_locs1"])
    monkeypatch.setattr(ops, "sample_locs", lambda s, c: torch.from_numpy(locs))
    return mod, locs


@pytest.mark.parametrize("name,case", MODES, ids=_ids(MODES))
def test_module_restatement(oracle_mod, monkeypatch, name, case):
    """Epipolar._attend_general_chunk + the stock-op epilogue (the route of CPU tensors) in every mode of the fixtures, forward and
    autograd."""
    d = nf.load(name)
    f1, f2, g, prior1 = nf.poisoned_inputs(d, case)
    mod, locs = _mode_module(d, prior1, oracle_mod, monkeypatch)
    a1, a2 = torch.from_numpy(f1).requires_grad_(True), torch.from_numpy(f2).requires_grad_(True)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fin, corr, attn, _ = mod(a1, a2, torch.from_numpy(np.array(d["P1"])), torch.from_numpy(np.array(d["P2"])),
                                 camera=torch.from_numpy(np.array(d["camera"])), other_camera=torch.from_numpy(np.array(d["other_camera"])))
    (fin * torch.from_numpy(g)).sum().backward()
    n = nf.POISONED
    attn_np = attn.detach().numpy()
    nf.check_values(attn_np[n], nf.expected(d, case, "attn"), 1e-5 * max(1.0, float(np.abs(d["attn1"]).max())), what="attn")
    nf.check_values(fin.detach().numpy()[n], nf.expected(d, case, "finalout"), 1e-4 * max(1.0, float(np.abs(d["finalout1"]).max())), what="finalout")
    nf.check_corr_pos(d, case, locs, corr.numpy(), attn_np)
    for grad, o in ((a1.grad, "grad_feat1"), (a2.grad, "grad_feat2")):
        got = np.zeros_like(f1) if grad is None else grad.numpy()
        nf.check_values(got[n], nf.expected(d, case, o), 1e-4 * max(float(np.abs(d[o + "1"]).max()), 1e-6), what=o)
