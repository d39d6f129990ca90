// The evaluation metrics of Modelbuilder.forward's test-time branch -- JDR (modeling/metrics/metrics2d.py:294-324 with
// get_max_preds, basic_batch.py:67-95, calc_dists :269-281 and dist_acc :284-291), calculate_err / calc_pck (:199-265) and
// EPEmean (modeling/metrics/metrics3d.py:5-46) -- for ONE item: the pieces the device kernels and the host test hooks share
// (plain C++, __host__ __device__; included by et_metrics.hip only).
//
//   peak_xy()          get_max_preds' coordinates of a map's first maximum: (idx % W, idx / W), both 0 unless the maximum is > 0
//   jdr_distance()     calc_dists for one (sample, joint): -1 unless the TARGET's x > 1 and y > 1
//   ratio()            count / count as float64 (dist_acc, the PCK percentages), 0 / 0 = NaN
//   pck_error()        the error calculate_err thresholds: |x - x_gt| -- x ONLY
//   epe_error()        EPEmean's clamped error of one joint
//   strided_partial()  the fixed summation order of EPEmean's mean: kSumLanes strided partial sums, then a pairwise tree
//                      (host_tree here, the same walk through LDS in the kernel)
//
// Every value is a count of exact integer decisions or a float64 expression the reference evaluates with the same operands in the
// same order, and nothing here may be contracted into an FMA: each operation rounds once, as NumPy's and torch's do.  (The
// library is built with -ffp-contract=off; the pragmas below say so where it matters.)
#pragma once
#include <math.h>
#include <stdint.h>

namespace et_metrics {

constexpr int kMaxMapElements = 16384;   // the library's map limit (128 x 128)
constexpr int kSumLanes = 256;           // partial sums of strided_sum (the block size of the mean kernel)

#define ET_MET_HD __host__ __device__ inline __attribute__((always_inline))

ET_MET_HD double sqrt_rn(double x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __dsqrt_rn(x);
#else
    return sqrt(x);
#endif
}

// get_max_preds: x = idx % W, y = floor(idx / W), both multiplied by (maximum > 0)
ET_MET_HD void peak_xy(int idx, float maxval, int W, float &x, float &y)
{
    const bool keep = maxval > 0.f;
    x = keep ? (float)(idx % W) : 0.f;
    y = keep ? (float)(idx / W) : 0.f;
}

// calc_dists under JDR's normalize = (H / 10, W / 10): the reference divides (x, y) by it IN THAT ORDER, x by the height term.
// float32 coordinates / float64 normalize -> float64; prediction and target are divided separately, then subtracted.
ET_MET_HD double jdr_distance(float px, float py, float tx, float ty, int H, int W)
{
#pragma clang fp contract(off)
    if (!(tx > 1.f && ty > 1.f)) return -1.0;
    const double nx = (double)H / 10.0, ny = (double)W / 10.0;
    const double dx = (double)px / nx - (double)tx / nx;
    const double dy = (double)py / ny - (double)ty / ny;
    return sqrt_rn(dx * dx + dy * dy);
}

ET_MET_HD double ratio(long long count, long long of, double scale = 1.0)
{
#pragma clang fp contract(off)
    return (double)count * scale / (double)of;        // 0 * scale / 0 = NaN
}

// dist_acc of one joint from its two counts: -1 when no sample counts
ET_MET_HD double joint_accuracy(long long below, long long counted) { return counted > 0 ? ratio(below, counted) : -1.0; }

// JDR's average: the non-negative per-joint values summed in joint order, divided by their number (none: NaN -- the reference
// divides zero by zero there and raises)
inline __host__ __device__ double average_accuracy(const double *per_joint, int J)
{
    double sum = 0.0;
    long long n = 0;
    for (int j = 0; j < J; ++j)
        if (per_joint[j] >= 0.0) {
            sum += per_joint[j];
            ++n;
        }
    return sum / (double)n;
}

// calculate_err / calc_pck: np.linalg.norm(detected_points[:1, j] - ground_truth_points[:1, j]) -- `[:1]` selects the first ROW of
// the (2, J) array, so the error is the x difference alone (sqrt(d * d) = |d| exactly in binary floating point)
ET_MET_HD double pck_error(const float *locs, const double *gt, long long item) { return fabs((double)locs[2 * item] - gt[2 * item]); }

ET_MET_HD bool visible(const float *vis, long long item) { return !vis || vis[item] != 0.f; }

// EPEmean: sqrt((dx^2 + dy^2) + dz^2) * unit, replaced by max_dist where it exceeds it
ET_MET_HD double epe_error(const double *pred, const double *gt, long long item, double unit, double max_dist)
{
#pragma clang fp contract(off)
    const double dx = pred[3 * item] - gt[3 * item], dy = pred[3 * item + 1] - gt[3 * item + 1], dz = pred[3 * item + 2] - gt[3 * item + 2];
    const double e = sqrt_rn((dx * dx + dy * dy) + dz * dz) * unit;
    return e > max_dist ? max_dist : e;
}

// partial sum number `lane` of the mean: items lane, lane + kSumLanes, ... in ascending order
ET_MET_HD double strided_partial(const double *pred, const double *gt, long long items, double unit, double max_dist, int lane)
{
    double s = 0.0;
    for (long long i = lane; i < items; i += kSumLanes) s += epe_error(pred, gt, i, unit, max_dist);
    return s;
}

// one level of the pairwise tree over the partial sums: p[t] += p[t + half] for t < half, half = 128, 64, ..., 1
inline void host_tree(double *p)
{
    for (int half = kSumLanes / 2; half > 0; half >>= 1)
        for (int t = 0; t < half; ++t) p[t] += p[t + half];
}

#undef ET_MET_HD

}  // namespace et_metrics
