"""find_tensor_peak_batch (modeling/backbones/basic_batch.py:17-63) restated in NumPy float64, one heat map at a time, and the
heat maps of tests/golden/lifting/peaks.npz (made by tests/golden/make_peaks_golden.py, read by tests/test_peaks_cpu.py and
tests/test_gpu_peaks.py).

The operator: the first maximum of the map (torch.max: a NaN ranks above every value); a (2 r + 1)^2 window around it, r =
int(radius + 0.5), resampled bilinearly as F.affine_grid + F.grid_sample (align_corners False, zero padding) do for the box
[index -+ radius] normalised with -1 + 2 x / (L - 1); samples <= threshold dropped; the centre of mass under the ramp
arange(-radius, radius + 1e-4, radius / r), plus the index; pix2coord.

float32 appears only where the operator's DATA are float32 by definition: the map's values, the threshold the kernel receives,
and -- without the legacy knob -- index_h = float32(index) / float32(W), the true division torch >= 1.5 performs on the index
tensor.  Everything else is float64.  The one decision float32 and float64 can take differently is sample <= threshold; peak()
returns how close any sample came to it, and the fixture's maker refuses maps that come close.
"""
import numpy as np

EPS = float(np.finfo(float).eps)

# (H, W, radius): the smallest shapes at which each mechanism of the kernel is still exercised
CASES = {
    "64x64_r8": (64, 64, 8.0),          # a 17 x 17 window = 289 elements > 256 threads: a second trip of the window loop
    "16x16_r2": (16, 16, 2.0),          # head size
    "24x40_r3": (24, 40, 3.0),          # non-square
    "4x4_r8": (4, 4, 8.0),              # map smaller than its window, H W < 256
    "2x2_r1": (2, 2, 1.0),              # the smallest map admitted
    "3x100_r2.5": (3, 100, 2.5),        # int(radius + 0.5) = 3, ramp step 0.8333
    "96x96_r1.4": (96, 96, 1.4),        # int(radius + 0.5) = 1, non-integer radius
    "128x84_r4": (128, 84, 4.0),        # the shape in the reference's own comment: 42 trips of the arg-max loop
    "17x5_r0.6": (17, 5, 0.6),          # radius below 1
}
# (case, downsample, threshold): every case as the head calls it, one case at other downsample factors, one at other thresholds
RUNS = [(c, 4.0, 1e-6) for c in CASES] + [("24x40_r3", 1.0, 1e-6), ("24x40_r3", 8.0, 1e-6), ("16x16_r2", 4.0, 0.0), ("16x16_r2", 4.0, 0.1)]
NONFINITE_CASES = ("24x40_r3", "4x4_r8")
NONFINITE_MAPS = ("nan_far", "nan_cell0", "all_nan", "plus_inf", "all_minus_inf")
MAP_KINDS = ("corner00", "corner01", "corner10", "corner11", "edge_top", "edge_right", "inside0", "inside1", "inside2", "constant",
             "negative", "tiny", "ties_spread", "ties_strided", "straddle_inside", "straddle_corner")
DENSE_BELOW = 1024          # maps of up to this many cells carry noise everywhere; larger ones are exactly zero away from their bump


def run_name(case, downsample, threshold):
    return "%s@ds%g_thr%g" % (case, downsample, threshold)


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def bound(ref_err, locs):
    """The tolerance of a case: 4 x the reference's own distance from float64 (the summation order differs from torch's, and ref_err
    is a maximum over some twenty maps of a quantity the last three roundings dominate), at least 2 ulp of the largest location."""
    finite = np.abs(np.asarray(locs, np.float64)[np.isfinite(locs)])
    return max(4.0 * float(ref_err), 2.0 * ulp32(finite.max() if finite.size else 1.0))


def peak(heat, radius, downsample, threshold=1e-6, legacy_floor_division=False):
    """One (H, W) float32 map -> (location (2,) float64 in image coordinates (x, y), score float32, index, margin): margin is the
    smallest |sample - threshold| / |threshold| over the non-zero window samples (inf when there is none, or threshold is 0)."""
    heat = np.asarray(heat)
    assert heat.dtype == np.float32 and heat.ndim == 2
    H, W = heat.shape
    flat = heat.reshape(-1)
    nan = np.isnan(flat)
    index = int(np.argmax(nan)) if nan.any() else int(np.argmax(flat))          # the FIRST maximum
    score = flat[index]
    index_w = float(index % W)
    index_h = float(index // W) if legacy_floor_division else float(np.float32(index) / np.float32(W))
    radius, downsample, threshold = float(radius), float(downsample), float(np.float32(threshold))

    def normalize(x, length):
        return -1.0 + 2.0 * x / (length - 1)

    x0, x1 = normalize(index_w - radius, W), normalize(index_w + radius, W)
    y0, y1 = normalize(index_h - radius, H), normalize(index_h + radius, H)
    iradius = int(radius + 0.5)
    side = 2 * iradius + 1
    base = (2.0 * np.arange(side) + 1.0) / side - 1.0                           # affine_grid, align_corners False
    gx, gy = (x1 - x0) / 2 * base + (x1 + x0) / 2, (y1 - y0) / 2 * base + (y1 + y0) / 2
    px, py = ((gx + 1.0) * W - 1.0) / 2.0, ((gy + 1.0) * H - 1.0) / 2.0         # grid_sample, align_corners False
    fx, fy = np.floor(px), np.floor(py)
    wx, wy = (px - fx)[None, :], (py - fy)[:, None]
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    padded = np.zeros((H + 2, W + 2))                                           # padding_mode zeros
    padded[1:-1, 1:-1] = heat

    def taps(dy, dx):
        yy, xx = np.clip(iy + dy + 1, 0, H + 1), np.clip(ix + dx + 1, 0, W + 1)
        return padded[yy[:, None], xx[None, :]]

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        sub = taps(0, 0) * (1 - wx) * (1 - wy) + taps(0, 1) * wx * (1 - wy) + taps(1, 0) * (1 - wx) * wy + taps(1, 1) * wx * wy
        nonzero = sub[np.isfinite(sub) & (sub != 0)]
        margin = float(np.abs(nonzero - threshold).min() / abs(threshold)) if nonzero.size and threshold != 0 else np.inf
        sub = np.where(sub <= threshold, 0.0, sub)                              # F.threshold: a NaN is kept
        ramp = -radius + radius / iradius * np.arange(side)
        total = sub.sum() + EPS
        x = (sub * ramp[None, :]).sum() / total + index_w
        y = (sub * ramp[:, None]).sum() / total + index_h
        loc = np.array([x * downsample + downsample / 2.0 - 0.5, y * downsample + downsample / 2.0 - 0.5])     # pix2coord
    return loc, score, index, margin


def peaks(maps, radius, downsample, threshold=1e-6, legacy_floor_division=False):
    """(M, H, W) float32 -> locations (M, 2) float64, scores (M) float32, indices (M) int64, margins (M) float64."""
    out = [peak(m, radius, downsample, threshold, legacy_floor_division) for m in maps]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.float32), np.array([o[2] for o in out], np.int64),
            np.array([o[3] for o in out]))


def cell_location(index, W, downsample, legacy_floor_division=False):
    """The location of a map whose window sums to zero, (2,) float32: pix2coord of the arg-max cell's own (index_w, index_h), each
    operation rounded to float32 as torch and the kernel round it."""
    f = np.float32
    index_h = f(index // W) if legacy_floor_division else f(index) / f(W)
    half = f(downsample / 2.0)
    return np.array([f(index % W) * f(downsample) + half - f(0.5), index_h * f(downsample) + half - f(0.5)], np.float32)


def host_peaks(lib, maps, radius, downsample, threshold=1e-6, legacy=False):
    """et_debug_host_heatmap_peaks on (M, H, W) maps -> locs (M, 2), scores (M) float32; `lib`: the loaded library."""
    import ctypes

    maps = np.ascontiguousarray(maps, np.float32)
    m, h, w = maps.shape
    locs, scores = np.full((m, 2), np.nan, np.float32), np.full(m, np.nan, np.float32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.et_debug_host_heatmap_peaks(m, h, w, ptr(maps), radius, downsample, threshold, int(legacy), ptr(locs), ptr(scores))
    assert rc == 0, lib.et_last_error()
    return locs, scores


def same_bits(a, b):
    """Equal shape, dtype and bits; a NaN equals a NaN whatever its sign and payload."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.where(np.isnan(a), 0, a).tobytes() == np.where(np.isnan(b), 0, b).tobytes()


def check_nonfinite(locs, scores, ref_locs, ref_scores, W, downsample=4.0):
    """The reference's answer on the maps of NONFINITE_MAPS: NaN score and NaN coordinates for a NaN anywhere, +inf score and NaN
    coordinates for a +inf cell.  The map of -inf alone: score -inf and the location of cell 0 or NaN (the reference's finite
    answer hangs on rounding noise in its bilinear weights) -- never anything else."""
    for k in ("nan_far", "nan_cell0", "all_nan", "plus_inf"):
        i = NONFINITE_MAPS.index(k)
        assert np.isnan(ref_locs[i]).all() and np.isnan(locs[i]).all(), (k, locs[i])
        assert same_bits(scores[i], ref_scores[i]), (k, scores[i])
    assert np.isnan(scores[:3]).all() and scores[3] == np.inf
    i = NONFINITE_MAPS.index("all_minus_inf")
    assert scores[i] == -np.inf and ref_scores[i] == -np.inf
    cell0 = cell_location(0, W, downsample)
    assert np.isnan(locs[i]).all() or same_bits(locs[i], cell0), locs[i]


# ---- the maps of the fixture ------------------------------------------------------------------------------------------------------
def tie_indices(H, W):
    """Flat indices of equal maxima: `spread` falls to different threads and different waves of the 256-thread reduction (45, 300
    and 813 at 24 x 40), `strided` to ONE thread's successive trips where the map is large enough (7, 263, 519), else to the
    map's second and last cell."""
    hw = H * W
    spread = sorted({int(f * hw) for f in (0.047, 0.3125, 0.847)})
    strided = [7, 263, 519] if hw > 519 else [1, hw - 1]
    return spread, strided


def _bump(H, W, cy, cx, radius, amplitude):
    yy, xx = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    return amplitude * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * radius))


def make_maps(case, seed):
    """The finite maps of a case, (len(MAP_KINDS), H, W) float32, in the order of MAP_KINDS."""
    H, W, radius = CASES[case]
    rng = np.random.default_rng(seed)
    dense = H * W <= DENSE_BELOW
    sub = lambda: rng.uniform(-0.45, 0.45)                                      # sub-pixel offset of a centre
    inner = lambda n: rng.uniform(min(radius, (n - 1) / 2.0), max(n - 1 - radius, (n - 1) / 2.0))
    centres = {"corner00": (sub(), sub()), "corner01": (sub(), W - 1 + sub()), "corner10": (H - 1 + sub(), sub()),
               "corner11": (H - 1 + sub(), W - 1 + sub()), "edge_top": (sub(), inner(W)), "edge_right": (inner(H), W - 1 + sub()),
               "inside0": (inner(H), inner(W)), "inside1": (inner(H), inner(W)), "inside2": (inner(H), inner(W)),
               "straddle_inside": (inner(H), inner(W)), "straddle_corner": (H - 1 + sub(), sub())}
    spread, strided = tie_indices(H, W)
    maps = []
    for kind in MAP_KINDS:
        if kind in centres:
            cy, cx = centres[kind]
            if kind.startswith("straddle"):
                m = _bump(H, W, cy, cx, radius, 5e-6)                           # samples on both sides of 1e-6, no noise
                floor = 1e-8
            else:
                m = _bump(H, W, cy, cx, radius, rng.uniform(0.6, 1.0)) * (1.0 + 0.1 * rng.uniform(-1, 1, (H, W)))
                floor = 1e-4
                if dense:
                    m = m + 0.005 * np.abs(rng.standard_normal((H, W)))
            if not dense:
                m = np.where(m < floor, 0.0, m)
        elif kind == "constant":
            m = np.full((H, W), 0.5)                                            # every cell ties: index 0
        elif kind == "negative":
            m = -(0.5 + 0.25 * ((np.arange(H * W).reshape(H, W) * 5 + 3) % 7) / 7.0)
        elif kind == "tiny":
            m = np.full((H, W), 1e-8)                                           # everything below the threshold
        else:
            m = 0.01 * np.abs(rng.standard_normal((H, W))) if dense else np.full((H, W), 0.0625)
            m.reshape(-1)[spread if kind == "ties_spread" else strided] = 0.75
        maps.append(m.astype(np.float32))
    return np.stack(maps)


def make_nonfinite_maps(case, seed):
    """(len(NONFINITE_MAPS), H, W) float32, in the order of NONFINITE_MAPS: an interior bump with noise, and the non-finite cells."""
    H, W, radius = CASES[case]
    rng = np.random.default_rng(seed)
    cy, cx = (H - 1) * 0.6, (W - 1) * 0.3
    base = (_bump(H, W, cy, cx, radius, 0.8) + 0.005 * np.abs(rng.standard_normal((H, W)))).astype(np.float32)
    maps = {k: base.copy() for k in NONFINITE_MAPS}
    maps["nan_far"][0, W - 1] = np.nan                                          # far from the maximum
    maps["nan_cell0"][0, 0] = np.nan
    maps["all_nan"][:] = np.nan
    maps["plus_inf"][H - 1, W - 2] = np.inf
    maps["all_minus_inf"][:] = -np.inf
    return np.stack([maps[k] for k in NONFINITE_MAPS])
