// The training side of Modelbuilder.forward after `final_layer`: the heat-map targets of the data loader (Heatmapcreator.get,
// data/transforms/keypoints2d.py:3-36) and the three criteria KEYPOINT.LOSS names (modeling/model.py:59-71) -- JointsMSELoss,
// KeypointsMSESmoothLoss and MaskedMSELoss with masks=None (modeling/metrics/metrics2d.py:18-81) -- for ONE element: the pieces
// the device kernels and the host test hooks share (plain C++, __host__ __device__; included by et_loss.hip only).
//
//   make_grid() / axis_term() / target_value()   one pixel of Heatmapcreator.get's map, float64 rounded once to float32
//   term()                         one element's float32 contribution to the loss, the reference's operations in its order
//   grad_element()                 one element of d loss / d pred, float64 from the float32 difference, rounded once
//   Span / span_of()               which elements of a map lane t of its block owns: whole 16-byte quads of the flat tensor
//   walk()                         a lane's quads in ascending order, operands loaded (float4 where whole and aligned)
//   lane_partial()                 that lane's float64 sum in ascending order; host_tree(): the pairwise tree over the 256 lanes
//   lane_gradient() / lane_targets()   that lane's elements of the gradient / of the target map
//   column_sum()                   the per-map sums added per joint over n ascending, then over the joints ascending
//
// Nothing here may be contracted into an FMA: each operation rounds once, as NumPy's and torch's do.  (The library is built with
// -ffp-contract=off; the pragmas below say so where it matters.)
#pragma once
#include <math.h>
#include <stdint.h>

namespace et_loss {

constexpr int kMaxMapElements = 16384;   // the library's map limit (128 x 128)
constexpr int kLanes = 256;              // lanes of a map's block = partial sums of the tree
constexpr double kClip = 4.60517019;     // Heatmapcreator.get clips the squared distance here: the background is exp(-kClip)
constexpr float kSmoothThreshold = 400.f;
constexpr double kSmoothScale = 219.71210866122357;   // threshold ** 0.9 as Python evaluates it

enum Kind { kJoint = ET_LOSS_JOINT, kSmoothMse = ET_LOSS_SMOOTHMSE, kMse = ET_LOSS_MSE };

#define ET_LOSS_HD __host__ __device__ inline __attribute__((always_inline))

ET_LOSS_HD float div_rn(float a, float b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// ---- targets ---------------------------------------------------------------------------------------------------------------------
// Heatmapcreator.__init__: sigma * 2**.5 in float64; grid = (float32 index * downsample + (downsample / 2.0 - 0.5)) / that, every
// operation in float32 (a float32 array against Python scalars).
struct Grid {
    double s;                 // sigma * 2**.5
    float s32, ds32, off32;   // float32(s), float32(downsample), float32(downsample / 2.0 - 0.5)
    float background;         // float32(exp(-kClip)), by the exp of the side that runs
};

ET_LOSS_HD Grid make_grid(double sigma, double downsample)
{
#pragma clang fp contract(off)
    Grid g;
    g.s = sigma * 1.4142135623730951;          // 2**.5 as Python evaluates it
    g.s32 = (float)g.s;
    g.ds32 = (float)downsample;
    g.off32 = (float)(downsample / 2.0 - 0.5);
    g.background = (float)exp(-kClip);
    return g;
}

// the grid value of row (or column) i: ONE float32 division, not a reciprocal multiply
ET_LOSS_HD float grid_value(const Grid &g, int i)
{
#pragma clang fp contract(off)
    const float a = (float)i * g.ds32;
    const float b = a + g.off32;
    return div_rn(b, g.s32);
}

// a point's coordinate over s, float64 (coords_uv / self.sigma)
ET_LOSS_HD double scaled(const Grid &g, double coordinate) { return coordinate / g.s; }

// one axis' share of the squared distance: (coordinate / s - grid value of index i) squared, float64
ET_LOSS_HD double axis_term(const Grid &g, double scaled_coordinate, int i)
{
#pragma clang fp contract(off)
    const double d = scaled_coordinate - (double)grid_value(g, i);
    return d * d;
}

// exp(-clip(rr + cc, 0, kClip)) rounded once to float32; rr = axis_term of v / s and the ROW (coords_uv[:, 1::-1] pairs v with
// the first grid axis), cc = axis_term of u / s and the column.  A clipped pixel is the background constant: the same exp of
// the same argument, taken once.  (A walk keeps rr while it stays in a row.)
ET_LOSS_HD float target_value(const Grid &g, double rr, double cc)
{
#pragma clang fp contract(off)
    const double q = rr + cc;
    if (q < kClip) return (float)exp(-q);      // (q >= 0 always)
    return q != q ? (float)q : g.background;    // NaN stays NaN, as np.clip and np.exp leave it
}

// The pixel a walk stands on, with its row's term kept until the row changes.
struct Cursor {
    int i, k;
    double rr;
};

ET_LOSS_HD Cursor cursor_at(const Grid &g, double vs, int element, int W)
{
    Cursor c;
    c.i = element / W;
    c.k = element - c.i * W;
    c.rr = axis_term(g, vs, c.i);
    return c;
}

// the target value of the cursor's pixel; the cursor moves on by one element
ET_LOSS_HD float next_value(const Grid &g, double vs, double us, int W, Cursor &c)
{
    const float value = target_value(g, c.rr, axis_term(g, us, c.k));
    if (++c.k == W) {
        c.k = 0;
        c.rr = axis_term(g, vs, ++c.i);
    }
    return value;
}

// ---- terms -----------------------------------------------------------------------------------------------------------------------
// the float32 difference the gradient is built from
template <int KIND>
ET_LOSS_HD float difference(float pred, float gt, float w)
{
#pragma clang fp contract(off)
    if (KIND == kJoint) {
        const float a = pred * w, b = gt * w;   // heatmap_pred.mul(w), heatmap_gt.mul(w)
        return a - b;
    }
    return KIND == kSmoothMse ? gt - pred : pred - gt;
}

// KeypointsMSESmoothLoss's unreplaced term (d * d) * w
ET_LOSS_HD float smooth_raw(float d, float w)
{
#pragma clang fp contract(off)
    const float dd = d * d;
    return dd * w;
}

template <int KIND>
ET_LOSS_HD float term(float pred, float gt, float w)
{
#pragma clang fp contract(off)
    const float d = difference<KIND>(pred, gt, w);
    if (KIND != kSmoothMse) return d * d;
    const float t = smooth_raw(d, w);
    if (!(t > kSmoothThreshold)) return t;
    const float root = (float)pow((double)t, 0.1);          // float32 pow: the correctly rounded value
    return root * (float)kSmoothScale;                      // torch multiplies by the scalar as float32
}

// d loss / d pred of one element: `c` = grad_output / the loss's denominator, float64
template <int KIND>
ET_LOSS_HD float grad_element(float pred, float gt, float w, double c)
{
#pragma clang fp contract(off)
    const float d = difference<KIND>(pred, gt, w);
    if (KIND == kMse) return (float)(2.0 * (double)d * c);
    if (KIND == kJoint) return (float)(2.0 * (double)d * (double)w * c);
    double g = -2.0 * (double)d * (double)w * c;
    const float t = smooth_raw(d, w);
    if (t > kSmoothThreshold) g *= 0.1 * pow((double)t, -0.9) * kSmoothScale;
    return (float)g;
}

// the denominator: joint N*H*W (* J unless per_joint), mse N*J*H*W, smoothmse H*W * max(1, sum of the weights)
ET_LOSS_HD double denominator(int kind, int N, int J, int HW, int per_joint, double weight_sum)
{
#pragma clang fp contract(off)
    if (kind == kJoint) return (double)N * (double)HW * (per_joint ? 1.0 : (double)J);
    if (kind == kMse) return (double)N * (double)J * (double)HW;
    return (double)HW * (weight_sum > 1.0 ? weight_sum : 1.0);
}

// ---- who owns what -----------------------------------------------------------------------------------------------------------------
// The (N, J, H, W) tensor is a flat array cut into quads of four floats (16 bytes when its base is so aligned).  Map `item`
// covers the flat elements [item * HW, (item + 1) * HW); lane t of its block owns the quads first + t, first + t + kLanes, ...
// with first = (item * HW) / 4, and of a quad the elements that lie inside the map, in ascending order.  A map of 63 or 323
// floats starts in the middle of a quad: its first and last quads are partial.
struct Span {
    long long begin, end;   // flat elements of the map
    long long quad, quads;  // this lane's first quad, one past the map's last quad
};

ET_LOSS_HD Span span_of(long long item, int HW, int lane)
{
    Span s;
    s.begin = item * HW;
    s.end = s.begin + HW;
    s.quad = (s.begin >> 2) + lane;
    s.quads = (s.end + 3) >> 2;
    return s;
}

// what every kernel and hook needs to produce one element's operands
struct Operands {
    const float *pred, *target;     // target NULL: on the fly from the points
    const double *points;
    const float *weight;            // NULL: ones
    Grid grid;
    int W;
    bool vec;                       // pred and target (and the gradient) start on 16-byte boundaries: whole quads move as float4
};

// Walks lane `lane`'s quads of map `item` in ascending order and hands each to visit(base, lo, hi, p, g, w, whole): the quad
// starts at flat element `base`, its elements [lo, hi) lie inside the map, p[e] / g[e] are their predicted and target values
// (the target read, or made by target_value), w the map's weight, `whole` says the quad may be stored as one float4.
template <class Visit>
ET_LOSS_HD void walk(const Operands &o, long long item, int HW, int lane, Visit &&visit)
{
    const Span s = span_of(item, HW, lane);
    const float w = o.weight ? o.weight[item] : 1.f;
    const double vs = o.target ? 0.0 : scaled(o.grid, o.points[2 * item + 1]);
    const double us = o.target ? 0.0 : scaled(o.grid, o.points[2 * item]);
    for (long long q = s.quad; q < s.quads; q += kLanes) {
        const long long base = q * 4;
        const int lo = base < s.begin ? (int)(s.begin - base) : 0;
        const int hi = base + 4 > s.end ? (int)(s.end - base) : 4;
        const bool whole = o.vec && lo == 0 && hi == 4;
        float p[4], g[4];
        if (whole) {
            const float4 v = *reinterpret_cast<const float4 *>(o.pred + base);
            p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
        } else {
            for (int e = lo; e < hi; ++e) p[e] = o.pred[base + e];
        }
        if (o.target && whole) {
            const float4 v = *reinterpret_cast<const float4 *>(o.target + base);
            g[0] = v.x, g[1] = v.y, g[2] = v.z, g[3] = v.w;
        } else if (o.target) {
            for (int e = lo; e < hi; ++e) g[e] = o.target[base + e];
        } else {
            Cursor at = cursor_at(o.grid, vs, (int)(base + lo - s.begin), o.W);
            for (int e = lo; e < hi; ++e) g[e] = next_value(o.grid, vs, us, o.W, at);
        }
        visit(base, lo, hi, p, g, w, whole);
    }
}

// lane `lane`'s partial sum of map `item`: its elements' float32 terms, each converted to float64, added in ascending order
template <int KIND>
ET_LOSS_HD double lane_partial(const Operands &o, long long item, int HW, int lane)
{
    double sum = 0.0;
    walk(o, item, HW, lane, [&sum](long long, int lo, int hi, const float *p, const float *g, float w, bool) {
        for (int e = lo; e < hi; ++e) sum += (double)term<KIND>(p[e], g[e], w);
    });
    return sum;
}

// lane `lane`'s elements of d loss / d pred of map `item`; c = grad_output / denominator
template <int KIND>
ET_LOSS_HD void lane_gradient(const Operands &o, long long item, int HW, int lane, double c, float *grad)
{
    walk(o, item, HW, lane, [c, grad](long long base, int lo, int hi, const float *p, const float *g, float w, bool whole) {
        float r[4];
        for (int e = lo; e < hi; ++e) r[e] = grad_element<KIND>(p[e], g[e], w, c);
        if (whole) {
            *reinterpret_cast<float4 *>(grad + base) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
            for (int e = lo; e < hi; ++e) grad[base + e] = r[e];
        }
    });
}

// lane `lane`'s pixels of the target map `item` (Heatmapcreator.get): the walk with nothing read
ET_LOSS_HD void lane_targets(const Grid &grid, const double *points, long long item, int HW, int W, int lane, bool vec, float *out)
{
    const Span s = span_of(item, HW, lane);
    const double vs = scaled(grid, points[2 * item + 1]), us = scaled(grid, points[2 * item]);
    for (long long q = s.quad; q < s.quads; q += kLanes) {
        const long long base = q * 4;
        const int lo = base < s.begin ? (int)(s.begin - base) : 0;
        const int hi = base + 4 > s.end ? (int)(s.end - base) : 4;
        Cursor at = cursor_at(grid, vs, (int)(base + lo - s.begin), W);
        float g[4];
        for (int e = lo; e < hi; ++e) g[e] = next_value(grid, vs, us, W, at);
        if (vec && lo == 0 && hi == 4) {
            *reinterpret_cast<float4 *>(out + base) = make_float4(g[0], g[1], g[2], g[3]);
        } else {
            for (int e = lo; e < hi; ++e) out[base + e] = g[e];
        }
    }
}

// one level after another of the pairwise tree over the lanes' partial sums: p[t] += p[t + half], half = 128, 64, ..., 1
inline void host_tree(double *p)
{
    for (int half = kLanes / 2; half > 0; half >>= 1)
        for (int t = 0; t < half; ++t) p[t] += p[t + half];
}

// The sum over a batch of per-(n, j) values of joint j: over n ascending.  The values are loaded kColumnBatch at a time before
// they are added -- the additions keep their order, the loads no longer wait for one another (one thread walks a column).
constexpr int kColumnBatch = 32;

template <class T>
inline __host__ __device__ double column_sum(const T *values, int N, int J, int j)
{
    double s = 0.0;
    int n = 0;
    for (; n + kColumnBatch <= N; n += kColumnBatch) {
        T v[kColumnBatch];
#pragma unroll
        for (int i = 0; i < kColumnBatch; ++i) v[i] = values[(size_t)(n + i) * J + j];
#pragma unroll
        for (int i = 0; i < kColumnBatch; ++i) s += (double)v[i];
    }
    for (; n < N; ++n) s += (double)values[(size_t)n * J + j];
    return s;
}

#undef ET_LOSS_HD

}  // namespace et_loss
