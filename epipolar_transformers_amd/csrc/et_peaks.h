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

// window element e = iy * side + ix: its value after the threshold, and its ramp values along x and y
ET_PEAKS_HD float window_sample(const float *hm, int H, int W, const Window &w, int e, float &ramp_x, float &ramp_y)
{
    const int iy = e / w.side, ix = e - iy * w.side;
    // affine_grid, align_corners = False: output coordinate (2 i + 1) / side - 1
    const float gx = w.t00 * ((2.f * ix + 1.f) / (float)w.side - 1.f) + w.t02;
    const float gy = w.t11 * ((2.f * iy + 1.f) / (float)w.side - 1.f) + w.t12;
    // grid_sample, align_corners = False
    const float px = ((gx + 1.f) * (float)W - 1.f) / 2.f, py = ((gy + 1.f) * (float)H - 1.f) / 2.f;
    const float fx = floorf(px), fy = floorf(py);
    const float wx = px - fx, wy = py - fy;
    const int x_ = (int)fx, y_ = (int)fy;                            // (finite and small: the entry points bound the radius)
    float v = tap(hm, H, W, y_, x_) * (1.f - wx) * (1.f - wy) + tap(hm, H, W, y_, x_ + 1) * wx * (1.f - wy) +
              tap(hm, H, W, y_ + 1, x_) * (1.f - wx) * wy + tap(hm, H, W, y_ + 1, x_ + 1) * wx * wy;
    v = v <= w.threshold ? 0.f : v;                                  // F.threshold: a NaN is kept
    ramp_x = -w.radius + w.rstep * (float)ix;                        // torch.arange(-radius, radius + 1e-4, radius / r)
    ramp_y = -w.radius + w.rstep * (float)iy;
    return v;
}

// the three window sums -> the location in image coordinates
ET_PEAKS_HD void finish(float sum, float sx, float sy, const Window &w, float downsample, float &x, float &y)
{
    const float tot = sum + 2.220446049250313e-16f;                  // np.finfo(float).eps
    const float mx = sx / tot + w.index_w, my = sy / tot + w.index_h;
    x = mx * downsample + downsample / 2.0f - 0.5f;                  // pix2coord
    y = my * downsample + downsample / 2.0f - 0.5f;
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

inline void host_peak(const float *hm, int H, int W, float radius, float downsample, float threshold, int legacy_floor, float *loc,
                      float *score)
{
    float best = -HUGE_VALF;
    int bidx = kNoCandidate;
    for (int i = 0; i < H * W; ++i)
        if (takes_over(hm[i], best)) {
            best = hm[i];
            bidx = i;
        }
    const Window w = make_window(resolve_index(bidx), H, W, radius, threshold, legacy_floor);
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
    float tot[3];
    for (int k = 0; k < 3; ++k) {
        float wave[kThreads / 64];
        for (int v = 0; v < kThreads / 64; ++v) wave[v] = host_butterfly(part[k] + 64 * v);
        tot[k] = (wave[0] + wave[1]) + (wave[2] + wave[3]);
    }
    finish(tot[0], tot[1], tot[2], w, downsample, loc[0], loc[1]);
    *score = best;
}

#undef ET_PEAKS_HD

}  // namespace et_peaks
