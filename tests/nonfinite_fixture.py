"""Reader of tests/golden/nonfinite/*.npz (tests/golden/make_nonfinite_golden.py: what the REAL reference returns when one value
of a feature map, of the incoming gradient or of a prior table is NaN, +Inf or -Inf) and the three rules the tests hold an
implementation to.  Shared by tests/test_nonfinite_cpu.py and tests/test_gpu_nonfinite.py.

The sites sit in pair POISONED = 1 of 3; the fixture stores the reference's outputs of that pair only (the maker asserts that
the reference leaves pairs 0 and 2 bit-equal to the finite run)."""
import glob
import os

import numpy as np

from conftest import GOLDEN_DIR, assert_corr_pos

DIR = os.path.join(GOLDEN_DIR, "nonfinite")
POISONED = 1
SRC, REF, GOUT, PRIOR = 0, 1, 2, 3
VALUES = (float("nan"), float("inf"), float("-inf"))
_cache = {}


def names(prefix=""):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DIR, prefix + "*.npz")))


def load(name):
    """The fixture as a dict of arrays (read once per session, never modified: the accessors below copy)."""
    if name not in _cache:
        d = dict(np.load(os.path.join(DIR, name + ".npz"), allow_pickle=False))
        if name.startswith("mode_"):
            H, C, K, N, image = [int(v) for v in d["meta"]]
            d["dims"] = dict(H=H, W=H, C=C, K=K, N=N, image=image, correct=True, softmax=True)
        else:
            H, W, C, K, N, image, correct, softmax, _ = [int(v) for v in d["meta"]]
            d["dims"] = dict(H=H, W=W, C=C, K=K, N=N, image=image, correct=bool(correct), softmax=bool(softmax))
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = d
    return _cache[name]


def cases(name, sites=None):
    """Case names `<site>.<kind>` of a fixture, optionally only those of the given site kinds (src_one, src_all, ref_one, ref_zero,
    gout_one, src_grid, src_stale, src_corner_one, src_corner_all, prior_one)."""
    return [str(c) for c in load(name)["cases"] if sites is None or str(c).split(".")[0] in sites]


def all_cases(prefix="", sites=None):
    return [(n, c) for n in names(prefix) for c in cases(n, sites)]


def site_tensor(d, case):
    return int(d[case + ".site"][0][0])


def poisoned_inputs(d, case, prior_key="prior.2.3"):
    """Copies of (feat1, feat2, grad_out, prior table of pair 1 or None) with the case's value at its sites."""
    val = VALUES[int(d[case + ".kind"])]
    t = {REF: d["feat1"].copy(), SRC: d["feat2"].copy(), GOUT: d["grad_out"].copy(),
         PRIOR: d[prior_key].copy() if prior_key in d else None}
    for tid, y, x, c in d[case + ".site"]:
        if tid == PRIOR:
            t[PRIOR].reshape(t[PRIOR].shape[0], -1)[y, x] = val
        elif c < 0:
            t[tid][POISONED, :, y, x] = val
        else:
            t[tid][POISONED, c, y, x] = val
    return t[REF], t[SRC], t[GOUT], t[PRIOR]


def expected(d, case, out):
    """The reference's `out` (out, attn, finalout, grad_feat1, grad_feat2) of pair 1 in the poisoned run."""
    base = d[out + "1"]
    want = base.copy().ravel()
    want[d["%s.%s.idx" % (case, out)]] = d["%s.%s.val" % (case, out)]
    nan, pinf, ninf = (np.unpackbits(m)[: want.size].astype(bool) for m in d["%s.%s.mask" % (case, out)])
    want[nan], want[pinf], want[ninf] = np.nan, np.inf, -np.inf
    return want.reshape(base.shape)


def check_values(got, want, tol, kinds=True, what="", rtol=0.0, exempt=None):
    """R1 and R2 for one output of pair 1.  R1, never lost: wherever the reference is non-finite so are we -- with `kinds` the
    same kind (NaN, +Inf, -Inf; the per-pixel routes), without only the finiteness mask (matrix-core routes: a split-fp16 product
    turns Inf into NaN, lo = v - hi = inf - inf).  R2, confined: wherever the reference is finite we are finite and within `tol`
    (absolute) + `rtol` x |reference| (tests/test_gpu_parity.py::_close: with the soft-max off a masked sample keeps its -1e10 / K
    as a weight).  `exempt` (H,W) bool: pixels left out of every check (proven arg-max ties under ATTENTION max, which gathers
    the tied sample).  Returns the largest error over the finite entries, beyond the relative term."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if exempt is not None and exempt.any():
        keep = ~exempt
        got, want = got[..., keep], want[..., keep]
    fin_w, fin_g = np.isfinite(want), np.isfinite(got)
    lost = ~fin_w & fin_g
    assert not lost.any(), "%s: R1 -- %d non-finite values of the reference came out finite, first at %s" % (
        what, lost.sum(), tuple(np.argwhere(lost)[0]))
    spread = fin_w & ~fin_g
    assert not spread.any(), "%s: R2 -- %d values are non-finite where the reference is finite (%d reference entries are non-finite), first at %s" % (
        what, spread.sum(), (~fin_w).sum(), tuple(np.argwhere(spread)[0]))
    if kinds:
        for nm, f in (("NaN", np.isnan), ("+Inf", np.isposinf), ("-Inf", np.isneginf)):
            bad = f(want) != f(got)
            assert not bad.any(), "%s: R1 -- the %s masks differ in %d entries, first at %s" % (what, nm, bad.sum(), tuple(np.argwhere(bad)[0]))
    err = float((np.abs(got[fin_w] - want[fin_w]) - rtol * np.abs(want[fin_w])).max()) if fin_w.any() else 0.0
    assert err <= tol, "%s: R2 -- max error %g over the finite entries, tolerance %g" % (what, err, tol)
    return err


def check_kinds(got, want, what=""):
    """The second half of R1 on its own: NaN where the reference has NaN, +Inf where it has +Inf, -Inf where it has -Inf."""
    got, want = np.asarray(got), np.asarray(want)
    for nm, f in (("NaN", np.isnan), ("+Inf", np.isposinf), ("-Inf", np.isneginf)):
        bad = f(want) != f(got)
        assert not bad.any(), "%s: R1 -- the %s masks differ in %d entries (the reference has %d), first at %s" % (
            what, nm, bad.sum(), f(want).sum(), tuple(np.argwhere(bad)[0]))


def check_corr_pos(d, case, locs, corr, weights, n_of=POISONED):
    """R3: corr_pos of pair 1 equals the reference's at every pixel -- including the pixels whose weights are all NaN (sample 0)
    or partly NaN with the soft-max off (the first NaN) -- under the tie rule of conftest.assert_corr_pos and nothing looser.
    `locs` (K,N,H,W,2), `corr` (N,H,W,2), `weights` (N,K',H,W): ours, whole batch.  A pixel whose weights hold a NaN has no tie to
    prove: there the location must be bit-equal."""
    corr, weights = np.asarray(corr), np.asarray(weights)
    want = d[case + ".corr_pos"]
    n = n_of
    nanpix = np.isnan(weights[n]).any(0)                                             # (H,W)
    wrong = (corr[n] != want).any(-1) & nanpix
    assert not wrong.any(), "R3 -- corr_pos differs at %d pixels whose weights hold a NaN, first at %s: got %s, reference %s" % (
        wrong.sum(), tuple(np.argwhere(wrong)[0]), corr[n][tuple(np.argwhere(wrong)[0])], want[tuple(np.argwhere(wrong)[0])])
    # the rest through the suite's tie rule (NaN-free pixels only: give the others the reference's value, already proven equal)
    w1 = np.where(nanpix[None], 0.0, weights[n])
    return assert_corr_pos(locs[:, n:n + 1], corr[n:n + 1], want[None], w1[None], d["dims"]["correct"])[0]      # (H,W): proven ties
