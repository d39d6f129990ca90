// The soft-argmax peak finder -- find_tensor_peak_batch (modeling/backbones/basic_batch.py:17-63) -- for ONE heat map: the pieces
// heatmap_peaks_kernel (kernels_misc.inc) and the host test hook et_debug_host_heatmap_peaks share (plain C++, __host__ __device__;
// included by et_misc.hip only).
//
//   takes_over() / outranks()   the order of the arg-max, torch.max's: a NaN ranks above every value, among equals the lower
//                     index wins -- inside one ascending scan, and between two scans
//   resolve_index()   "no candidate" (a map without an element above -inf and without a NaN) is index 0, as torch.max's
//   make_window()     index -> index_w, index_h, the box [index -+ radius] normalised with -1 + 2 x / (L - 1), the affine parameters
//   window_sample()   element e of the (2 r + 1)^2 window: F.affine_grid + F.grid_sample (bilinear, align_corners = False, zero
//                     padding), F.threshold, and the two ramp values torch.arange(-radius, radius + 1e-4, radius / r) gives it
//   finish()          centre of mass + index, then pix2coord (vision/multiview.py:154-157)
//   host_peak()       the whole map serially, in the kernel's summation order: 256 strided partial sums, an xor butterfly over each
//                     64 of them, then (w0 + w1) + (w2 + w3)
//   cell_grad()       the backward (heatmap_peaks_bwd_kernel, et_debug_host_heatmap_peaks_bwd): what the location's gradient leaves
//                     in one cell of the map, from the same index, window and sums; host_peak_bwd() is the whole map serially
//
// Non-finite maps follow the reference: a NaN anywhere is the maximum (score NaN) and reaches the sums through its window (NaN
// coordinates); a sample is dropped when it is <= threshold, so a NaN sample is kept, as F.threshold keeps it.
// float32 throughout, each operation rounded once (the library is built with -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

namespace et_peaks {

constexpr int kThreads = 256;              // block size of the kernel = partial sums of host_peak
constexpr int kNoCandidate = 0x7fffffff;   // index of a thread / map that has seen nothing above -inf

#define ET_PEAKS_HD __host__ __device__ inline __attribute__((always_inline))

// scanning a map in ascending index order: does v replace the best so far?  (the first NaN stays; nothing replaces -inf but a
// larger value or a NaN, so a map of -inf alone ends without a candidate)
// (both predicates are written with | and & on purpose: straight-line code, no branch inside the kernel's loops)
ET_PEAKS_HD bool takes_over(float v, float best) { return (v > best) | ((v != v) & (best == best)); }

// merging two scans: does (v, i) outrank (b, bi)?  NaN first, then the larger value, then the lower index
ET_PEAKS_HD bool outranks(float v, int i, float b, int bi)
{
    const bool vnan = v != v, bnan = b != b, lower = i < bi;
    // one NaN: it wins.  Both or neither: the larger value (never true of two NaNs), else equal values or two NaNs by the index
    return (vnan & !bnan) | ((vnan == bnan) & ((v > b) | (((v == b) | vnan) & lower)));
}

ET_PEAKS_HD int resolve_index(int index) { return index == kNoCandidate ? 0 : index; }

struct Window {
    float index_w, index_h;
    float t00, t02, t11, t12;      // affine_parameter[:, 0, 0], [:, 0, 2], [:, 1, 1], [:, 1, 2]
    float radius, rstep, threshold;
    int side;                      // 2 * int(radius + 0.5) + 1
};

ET_PEAKS_HD float normalize(float x, int L) { return -1.f + 2.f * x / (float)(L - 1); }

// index_h = index / W: TRUE division under torch >= 1.5, integer division in the torch the authors used (`legacy_floor`)
ET_PEAKS_HD Window make_window(int index, int H, int W, float radius, float threshold, int legacy_floor)
{
    Window w;
    w.index_w = (float)(index % W);
    w.index_h = legacy_floor ? (float)(index / W) : (float)index / (float)W;
    const float x0 = normalize(w.index_w - radius, W), x1 = normalize(w.index_w + radius, W);
    const float y0 = normalize(w.index_h - radius, H), y1 = normalize(w.index_h + radius, H);
    w.t00 = (x1 - x0) / 2.f;
    w.t02 = (x1 + x0) / 2.f;
    w.t11 = (y1 - y0) / 2.f;
    w.t12 = (y1 + y0) / 2.f;
    const int ir = (int)(radius + 0.5f);
    w.side = 2 * ir + 1;
    w.radius = radius;
    w.rstep = radius * 1.0f / (float)ir;
    w.threshold = threshold;
    return w;
}

ET_PEAKS_HD float tap(const float *hm, int H, int W, int y, int x)
{
    return ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) ? hm[y * W + x] : 0.f;      // padding_mode = 'zeros'
}

// one axis of window element i (ix along x with t00, t02, W; iy along y with t11, t12, H): the lower tap and the upper tap's weight
struct AxisSample {
    int lo;                        // floor(pixel coordinate): the taps are lo and lo + 1
    float frac;                    // bilinear weight of lo + 1; lo has 1 - frac
};

ET_PEAKS_HD AxisSample axis_sample(float scale, float offset, int i, int side, int L)
{
    // affine_grid, align_corners = False: output coordinate (2 i + 1) / side - 1
    const float g = scale * ((2.f * i + 1.f) / (float)side - 1.f) + offset;
    // grid_sample, align_corners = False
    const float p = ((g + 1.f) * (float)L - 1.f) / 2.f;
    const float f = floorf(p);
    AxisSample a;
    a.lo = (int)f;                                                   // (finite and small: the entry points bound the radius)
    a.frac = p - f;
    return a;
}

// the bilinear sample at (ax, ay), before the threshold
ET_PEAKS_HD float window_value(const float *hm, int H, int W, const AxisSample &ax, const AxisSample &ay)
{
    const float wx = ax.frac, wy = ay.frac;
    const int x_ = ax.lo, y_ = ay.lo;
    return tap(hm, H, W, y_, x_) * (1.f - wx) * (1.f - wy) + tap(hm, H, W, y_, x_ + 1) * wx * (1.f - wy) +
           tap(hm, H, W, y_ + 1, x_) * (1.f - wx) * wy + tap(hm, H, W, y_ + 1, x_ + 1) * wx * wy;
}

ET_PEAKS_HD bool kept(float v, const Window &w) { return !(v <= w.threshold); }      // F.threshold: a NaN is kept

ET_PEAKS_HD float ramp(const Window &w, int i) { return -w.radius + w.rstep * (float)i; }      // torch.arange(-radius, radius + 1e-4, radius / r)

// window element e = iy * side + ix: its value after the threshold, and its ramp values along x and y
ET_PEAKS_HD float window_sample(const float *hm, int H, int W, const Window &w, int e, float &ramp_x, float &ramp_y)
{
    const int iy = e / w.side, ix = e - iy * w.side;
    float v = window_value(hm, H, W, axis_sample(w.t00, w.t02, ix, w.side, W), axis_sample(w.t11, w.t12, iy, w.side, H));
    v = kept(v, w) ? v : 0.f;
    ramp_x = ramp(w, ix);
    ramp_y = ramp(w, iy);
    return v;
}

// the three window sums -> the location in image coordinates
ET_PEAKS_HD float total(float sum) { return sum + 2.220446049250313e-16f; }      // np.finfo(float).eps

ET_PEAKS_HD void finish(float sum, float sx, float sy, const Window &w, float downsample, float &x, float &y)
{
    const float tot = total(sum);
    const float mx = sx / tot + w.index_w, my = sy / tot + w.index_h;
    x = mx * downsample + downsample / 2.0f - 0.5f;                  // pix2coord
    y = my * downsample + downsample / 2.0f - 0.5f;
}

// ---- the gradient of one map (et_heatmap_peaks_bwd) --------------------------------------------------------------------------------
// With S, Sx, Sy the forward's sums and tot = S + eps, the location's gradient reaches window element e through its thresholded
// value v_e with the coefficient   c_e = downsample (g_x (rx_e - Sx / tot) + g_y (ry_e - Sy / tot)) / tot   when the sample was
// kept and 0 when it was dropped (F.threshold's backward), and c_e reaches the map through the element's four bilinear taps
// (F.grid_sample's backward; a tap outside the map receives nothing).  index_w, index_h and the box are constants (the reference
// takes .data of them).  c_e is EVALUATED as   downsample (g_x (rx_e tot - Sx) + g_y (ry_e tot - Sy)) / tot / tot:   the same
// cancellation in general, but where ONE sample survives the threshold Sx = v rx_e and
// rx_e tot = rx_e v are the same product, so the gradient of a location that does not depend on the map is exactly 0 and not the
// rounding noise of Sx / tot.  GATHER form: a cell of the map sums, in ascending element order, the elements whose taps include it.  The
// pixel coordinate of an axis never decreases with the element's index (every operation of axis_sample is monotonic and rounded
// monotonically), so those elements are one run per axis, found by bisection: the cost of a cell does not depend on the window.

// everything a cell needs besides the map
struct GradCoef {
    float gx, gy;                  // the location's incoming gradient
    float sx, sy, tot;             // the window's sums Sx, Sy and tot = S + eps
    float downsample;
};

ET_PEAKS_HD GradCoef make_coef(float sum, float sx, float sy, float gx, float gy, float downsample)
{
    GradCoef c;
    c.gx = gx;
    c.gy = gy;
    c.tot = total(sum);
    c.sx = sx;
    c.sy = sy;
    c.downsample = downsample;
    return c;
}

// [first, last] cell an axis of the window taps, clipped to the map; empty (first > last) when the window misses the map
ET_PEAKS_HD void footprint(float scale, float offset, int side, int L, int &first, int &last)
{
    const int lo = axis_sample(scale, offset, 0, side, L).lo, hi = axis_sample(scale, offset, side - 1, side, L).lo + 1;
    first = lo < 0 ? 0 : lo;
    last = hi > L - 1 ? L - 1 : hi;
}

// the elements [begin, end) of an axis whose taps (lo, lo + 1) include `cell`: lo == cell - 1 or lo == cell
ET_PEAKS_HD void axis_run(float scale, float offset, int side, int L, int cell, int &begin, int &end)
{
    int a = 0, b = side;                                             // the first element with lo >= cell - 1
    while (a < b) {
        const int m = (a + b) >> 1;
        if (axis_sample(scale, offset, m, side, L).lo >= cell - 1)
            b = m;
        else
            a = m + 1;
    }
    begin = a;
    b = side;                                                        // the first element with lo > cell
    while (a < b) {
        const int m = (a + b) >> 1;
        if (axis_sample(scale, offset, m, side, L).lo > cell)
            b = m;
        else
            a = m + 1;
    }
    end = a;
}

// what the location's gradient leaves in cell (y, x) of the map
ET_PEAKS_HD float cell_grad(const float *hm, int H, int W, const Window &w, const GradCoef &c, int y, int x)
{
    int ix0, ix1, iy0, iy1;
    axis_run(w.t00, w.t02, w.side, W, x, ix0, ix1);
    axis_run(w.t11, w.t12, w.side, H, y, iy0, iy1);
    float acc = 0.f;
    for (int iy = iy0; iy < iy1; ++iy) {
        const AxisSample ay = axis_sample(w.t11, w.t12, iy, w.side, H);
        const float wy = ay.lo == y ? 1.f - ay.frac : ay.frac;
        const float dy = c.gy * (ramp(w, iy) * c.tot - c.sy);
        for (int ix = ix0; ix < ix1; ++ix) {
            const AxisSample ax = axis_sample(w.t00, w.t02, ix, w.side, W);
            const float wx = ax.lo == x ? 1.f - ax.frac : ax.frac;
            if (!kept(window_value(hm, H, W, ax, ay), w)) continue;
            const float ce = c.downsample * (c.gx * (ramp(w, ix) * c.tot - c.sx) + dy) / c.tot / c.tot;
            acc += ce * (wx * wy);
        }
    }
    return acc;
}

// sum of `p[0 .. 63]` as the kernel's wave reduction leaves it in lane 0: a += shfl_xor(a, o) for o = 32, 16, ..., 1
inline float host_butterfly(float *p)
{
    for (int o = 32; o >= 1; o >>= 1) {
        float q[64];
        for (int l = 0; l < 64; ++l) q[l] = p[l] + p[l ^ o];
        for (int l = 0; l < 64; ++l) p[l] = q[l];
    }
    return p[0];
}

inline int host_index(const float *hm, int H, int W, float *score)
{
    float best = -HUGE_VALF;
    int bidx = kNoCandidate;
    for (int i = 0; i < H * W; ++i)
        if (takes_over(hm[i], best)) {
            best = hm[i];
            bidx = i;
        }
    *score = best;
    return resolve_index(bidx);
}

// tot[0 .. 2] = the window's three sums in the kernel's order
inline void host_sums(const float *hm, int H, int W, const Window &w, float *tot)
{
    float part[3][kThreads];
    for (int t = 0; t < kThreads; ++t) {
        float sum = 0.f, sx = 0.f, sy = 0.f;
        for (int e = t; e < w.side * w.side; e += kThreads) {
            float rx, ry;
            const float v = window_sample(hm, H, W, w, e, rx, ry);
            sum += v;
            sx += v * rx;
            sy += v * ry;
        }
        part[0][t] = sum;
        part[1][t] = sx;
        part[2][t] = sy;
    }
    for (int k = 0; k < 3; ++k) {
        float wave[kThreads / 64];
        for (int v = 0; v < kThreads / 64; ++v) wave[v] = host_butterfly(part[k] + 64 * v);
        tot[k] = (wave[0] + wave[1]) + (wave[2] + wave[3]);
    }
}

inline void host_peak(const float *hm, int H, int W, float radius, float downsample, float threshold, int legacy_floor, float *loc,
                      float *score)
{
    const Window w = make_window(host_index(hm, H, W, score), H, W, radius, threshold, legacy_floor);
    float tot[3];
    host_sums(hm, H, W, w, tot);
    finish(tot[0], tot[1], tot[2], w, downsample, loc[0], loc[1]);
}

// the whole gradient of one map serially, every cell as the kernel's thread computes it; g_loc / g_score may be NULL (not both)
inline void host_peak_bwd(const float *hm, int H, int W, float radius, float downsample, float threshold, int legacy_floor,
                          const float *g_loc, const float *g_score, float *grad)
{
    float score;
    const int index = host_index(hm, H, W, &score);
    for (int i = 0; i < H * W; ++i) grad[i] = 0.f;
    if (g_loc) {
        const Window w = make_window(index, H, W, radius, threshold, legacy_floor);
        float tot[3];
        host_sums(hm, H, W, w, tot);
        const GradCoef c = make_coef(tot[0], tot[1], tot[2], g_loc[0], g_loc[1], downsample);
        int x0, x1, y0, y1;
        footprint(w.t00, w.t02, w.side, W, x0, x1);
        footprint(w.t11, w.t12, w.side, H, y0, y1);
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) grad[y * W + x] = cell_grad(hm, H, W, w, c, y, x);
    }
    if (g_score) grad[index] = grad[index] + *g_score;              // torch.max's backward: the first maximum
}

#undef ET_PEAKS_HD

}  // namespace et_peaks
