// libepipolar_amd.so: the evaluation metrics of Modelbuilder.forward's test-time branch on the device -- JDR, calculate_err /
// calc_pck (PCK@th and the per-sample curve counts) and EPEmean (et_metrics.h names the reference's lines).  The reference copies
// both heat-map stacks to the host and walks N * J items in Python; here nothing leaves the device and no call synchronises.
//
//   et_eval_jdr   jdr_peaks_kernel: one block per (sample, joint) finds the first maximum of the predicted and of the target map
//                 (per-thread strided scan, wave max / min on DPP, four waves through LDS) and writes the masked coordinates and
//                 the distance; jdr_accuracy_kernel: ONE block, a wave per joint counts over the samples (integers: any order
//                 gives the same count), then one thread averages in joint order.
//   et_eval_pck   pck_sample_kernel: one block per sample, a thread per curve point; pck_batch_kernel: one block per threshold
//                 counts over the whole batch.  Integer counts only.
//   et_eval_epe   epe_items_kernel: a lane per item writes the masked clamped error; epe_mean_kernel: ONE block, every thread sums
//                 its strided items in ascending order, then a pairwise tree in LDS -- the order et_metrics::host_tree walks.
// No float atomics, no scratch: every output is bit-reproducible from run to run, and the host hooks give the same bits.
#include "et_common.h"
#include "et_metrics.h"

namespace {
#include "et_wave_reduce.h"

constexpr int kBlock = 256;
constexpr int kNoIndex = 0x7fffffff;
static_assert(kBlock == et_metrics::kSumLanes && kBlock == kWave * kWavesPerBlock, "one partial sum per thread, four waves");

// first maximum of `map` (value, then lowest flat index; -0.0 and +0.0 tie), the same in every thread of the block.
// s_val / s_idx: kWavesPerBlock words each.  Indices are < 16384, exact in float, so the wave reductions run on floats.
__device__ __forceinline__ void block_argmax(const float *__restrict__ map, int HW, float *s_val, int *s_idx, float &maxval, int &index)
{
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    float best = -__builtin_huge_valf();
    int bidx = kNoIndex;
    for (int i = tid; i < HW; i += kBlock) {
        const float v = map[i];
        if (bidx == kNoIndex || v > best) {
            best = v;
            bidx = i;
        }
    }
    const float wmax = wave_all_max(best);
    // (a thread without an element holds -inf, which never equals a finite maximum)
    const float cand = (bidx != kNoIndex && best == wmax) ? (float)bidx : (float)et_metrics::kMaxMapElements;
    const float wmin = wave_all_min(cand);
    __syncthreads();                                  // the previous call's readers are done with s_val / s_idx
    if (lane == 0) {
        s_val[wave] = wmax;
        s_idx[wave] = (int)wmin;
    }
    __syncthreads();
    maxval = s_val[0];
    index = s_idx[0];
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) {
        const float v = s_val[w];
        const int i = s_idx[w];
        if (i < et_metrics::kMaxMapElements && (v > maxval || (v == maxval && i < index))) {
            maxval = v;
            index = i;
        }
    }
}

__global__ __launch_bounds__(kBlock) void jdr_peaks_kernel(int N, int J, int H, int W, const float *__restrict__ pred,
                                                            const float *__restrict__ target, double *__restrict__ dists,
                                                            float *__restrict__ pred_xy, float *__restrict__ target_xy)
{
    __shared__ float s_val[kWavesPerBlock];
    __shared__ int s_idx[kWavesPerBlock];
    const long long item = blockIdx.x;                // n * J + j
    const int HW = H * W;
    float pv, tv;
    int pi, ti;
    block_argmax(pred + item * HW, HW, s_val, s_idx, pv, pi);
    block_argmax(target + item * HW, HW, s_val, s_idx, tv, ti);
    if (threadIdx.x != 0) return;
    float px, py, tx, ty;
    et_metrics::peak_xy(pi, pv, W, px, py);
    et_metrics::peak_xy(ti, tv, W, tx, ty);
    const int n = (int)(item / J), j = (int)(item % J);
    dists[(size_t)j * N + n] = et_metrics::jdr_distance(px, py, tx, ty, H, W);
    if (pred_xy) {
        pred_xy[2 * item] = px;
        pred_xy[2 * item + 1] = py;
    }
    if (target_xy) {
        target_xy[2 * item] = tx;
        target_xy[2 * item + 1] = ty;
    }
}

__device__ __forceinline__ int wave_sum_int(int v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// sum of an int over the block, the same in every thread (s: kWavesPerBlock words)
__device__ __forceinline__ int block_sum_int(int v, int *s)
{
    v = wave_sum_int(v);
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s[0] + s[1]) + (s[2] + s[3]);
}

__global__ __launch_bounds__(kBlock) void jdr_accuracy_kernel(int N, int J, const double *__restrict__ dists, double thr,
                                                               double *acc)
{
    const int lane = threadIdx.x & (kWave - 1);
    for (int j = threadIdx.x >> 6; j < J; j += kWavesPerBlock) {      // wave-uniform
        int counted = 0, below = 0;
        for (int n = lane; n < N; n += kWave) {
            const double d = dists[(size_t)j * N + n];
            counted += d != -1.0;
            below += d != -1.0 && d < thr;
        }
        counted = wave_sum_int(counted);
        below = wave_sum_int(below);
        if (lane == 0) acc[1 + j] = et_metrics::joint_accuracy(below, counted);
    }
    __syncthreads();                                  // (orders the block's own global writes before thread 0 reads them)
    if (threadIdx.x == 0) acc[0] = et_metrics::average_accuracy(acc + 1, J);
}

__global__ __launch_bounds__(kBlock) void pck_sample_kernel(int J, const float *__restrict__ locs, const double *__restrict__ gt,
                                                             const float *__restrict__ vis, int M, const double *__restrict__ curve,
                                                             double *__restrict__ err_joints, double *__restrict__ total_joints)
{
    const long long n = blockIdx.x, first = n * J;
    for (int m = threadIdx.x; m < M; m += kBlock) {
        const double c = curve[m];
        int below = 0;
        for (int j = 0; j < J; ++j) below += et_metrics::visible(vis, first + j) && et_metrics::pck_error(locs, gt, first + j) < c;
        err_joints[n * M + m] = (double)below;
    }
    if (threadIdx.x == 0) {
        int counted = 0;
        for (int j = 0; j < J; ++j) counted += et_metrics::visible(vis, first + j);
        total_joints[n] = (double)counted;
    }
}

__global__ __launch_bounds__(kBlock) void pck_batch_kernel(long long items, const float *__restrict__ locs,
                                                            const double *__restrict__ gt, const float *__restrict__ vis,
                                                            const double *__restrict__ thresholds, double *__restrict__ pck)
{
    __shared__ int s[kWavesPerBlock];
    const double th = thresholds[blockIdx.x];
    int counted = 0, below = 0;
    for (long long i = threadIdx.x; i < items; i += kBlock) {
        const bool v = et_metrics::visible(vis, i);
        counted += v;
        below += v && et_metrics::pck_error(locs, gt, i) < th;
    }
    counted = block_sum_int(counted, s);
    below = block_sum_int(below, s);
    if (threadIdx.x == 0) pck[blockIdx.x] = et_metrics::ratio(below, counted, 100.0);
}

__global__ __launch_bounds__(kBlock) void epe_items_kernel(long long items, const double *__restrict__ pred,
                                                            const double *__restrict__ gt, const float *__restrict__ vis, double unit,
                                                            double max_dist, double *__restrict__ per_joint)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= items) return;
    per_joint[i] = et_metrics::visible(vis, i) ? et_metrics::epe_error(pred, gt, i, unit, max_dist) : 0.0;
}

__global__ __launch_bounds__(kBlock) void epe_mean_kernel(long long items, const double *__restrict__ pred,
                                                           const double *__restrict__ gt, double unit, double max_dist,
                                                           double *__restrict__ mean)
{
    __shared__ double p[kBlock];
    const int t = threadIdx.x;
    p[t] = et_metrics::strided_partial(pred, gt, items, unit, max_dist, t);
    __syncthreads();
    for (int half = kBlock / 2; half > 0; half >>= 1) {
        if (t < half) p[t] += p[t + half];
        __syncthreads();
    }
    if (t == 0) *mean = p[0] / (double)items;
}

int check_jdr(const char *what, int32_t N, int32_t J, int32_t H, int32_t W, const float *pred, const float *target, const double *dists,
              const double *acc)
{
    if (N < 1 || J < 1 || (long long)N * J > 0x7fffffffLL) return fail("%s: bad sizes N=%d J=%d", what, N, J);
    if (H < 2 || W < 2 || (long long)H * W > et_metrics::kMaxMapElements)
        return fail("%s: map %d x %d outside H >= 2, W >= 2, H * W <= %d", what, H, W, et_metrics::kMaxMapElements);
    if (!pred || !target || !dists || !acc) return fail("%s: NULL pointer", what);
    return 0;
}

int check_pck(const char *what, int32_t N, int32_t J, const float *locs, const double *gt, int32_t T, const double *thresholds, int32_t M,
              const double *curve, const double *pck, const double *err_joints, const double *total_joints)
{
    if (N < 1 || J < 1 || (long long)N * J > 0x7fffffffLL) return fail("%s: bad sizes N=%d J=%d", what, N, J);
    if (T < 0 || M < 0 || (long long)N * M > 0x7fffffffLL) return fail("%s: bad lengths T=%d M=%d", what, T, M);
    if (!locs || !gt || !total_joints || (T > 0 && (!thresholds || !pck)) || (M > 0 && (!curve || !err_joints)))
        return fail("%s: NULL pointer", what);
    return 0;
}

int check_epe(const char *what, int32_t F, int32_t J, const double *pred, const double *gt, const double *mean, const double *per_joint)
{
    if (F < 1 || J < 1 || (long long)F * J > 0x7fffffffLL) return fail("%s: bad sizes F=%d J=%d", what, F, J);
    if (!pred || !gt || !mean || !per_joint) return fail("%s: NULL pointer", what);
    return 0;
}

}  // namespace

extern "C" {

int et_eval_jdr(int32_t N, int32_t J, int32_t H, int32_t W, const float *pred, const float *target, double thr, double *dists,
                double *acc, float *pred_xy, float *target_xy, void *stream)
{
    if (int e = check_jdr("et_eval_jdr", N, J, H, W, pred, target, dists, acc)) return e;
    hipLaunchKernelGGL(jdr_peaks_kernel, dim3((unsigned)(N * J)), dim3(kBlock), 0, (hipStream_t)stream, N, J, H, W, pred, target, dists,
                       pred_xy, target_xy);
    hipLaunchKernelGGL(jdr_accuracy_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, N, J, dists, thr, acc);
    return check_launch("et_eval_jdr");
}

int et_debug_host_eval_jdr(int32_t N, int32_t J, int32_t H, int32_t W, const float *pred, const float *target, double thr,
                           double *dists, double *acc, float *pred_xy, float *target_xy)
{
    if (int e = check_jdr("et_debug_host_eval_jdr", N, J, H, W, pred, target, dists, acc)) return e;
    const int HW = H * W;
    auto first_maximum = [HW](const float *map, float &maxval, int &index) {
        maxval = map[0];
        index = 0;
        for (int i = 1; i < HW; ++i)
            if (map[i] > maxval) {
                maxval = map[i];
                index = i;
            }
    };
    for (long long item = 0; item < (long long)N * J; ++item) {
        float pv, tv, px, py, tx, ty;
        int pi, ti;
        first_maximum(pred + item * HW, pv, pi);
        first_maximum(target + item * HW, tv, ti);
        et_metrics::peak_xy(pi, pv, W, px, py);
        et_metrics::peak_xy(ti, tv, W, tx, ty);
        dists[(size_t)(item % J) * N + item / J] = et_metrics::jdr_distance(px, py, tx, ty, H, W);
        if (pred_xy) pred_xy[2 * item] = px, pred_xy[2 * item + 1] = py;
        if (target_xy) target_xy[2 * item] = tx, target_xy[2 * item + 1] = ty;
    }
    for (int j = 0; j < J; ++j) {
        long long counted = 0, below = 0;
        for (int n = 0; n < N; ++n) {
            const double d = dists[(size_t)j * N + n];
            counted += d != -1.0;
            below += d != -1.0 && d < thr;
        }
        acc[1 + j] = et_metrics::joint_accuracy(below, counted);
    }
    acc[0] = et_metrics::average_accuracy(acc + 1, J);
    return 0;
}

int et_eval_pck(int32_t N, int32_t J, const float *locs, const double *gt, const float *vis, int32_t T, const double *thresholds,
                int32_t M, const double *curve, double *pck, double *err_joints, double *total_joints, void *stream)
{
    if (int e = check_pck("et_eval_pck", N, J, locs, gt, T, thresholds, M, curve, pck, err_joints, total_joints)) return e;
    hipLaunchKernelGGL(pck_sample_kernel, dim3((unsigned)N), dim3(kBlock), 0, (hipStream_t)stream, J, locs, gt, vis, M, curve, err_joints,
                       total_joints);
    if (T > 0)
        hipLaunchKernelGGL(pck_batch_kernel, dim3((unsigned)T), dim3(kBlock), 0, (hipStream_t)stream, (long long)N * J, locs, gt, vis,
                           thresholds, pck);
    return check_launch("et_eval_pck");
}

int et_debug_host_eval_pck(int32_t N, int32_t J, const float *locs, const double *gt, const float *vis, int32_t T,
                           const double *thresholds, int32_t M, const double *curve, double *pck, double *err_joints,
                           double *total_joints)
{
    if (int e = check_pck("et_debug_host_eval_pck", N, J, locs, gt, T, thresholds, M, curve, pck, err_joints, total_joints)) return e;
    const long long items = (long long)N * J;
    long long all = 0;
    for (long long n = 0; n < N; ++n) {
        long long counted = 0;
        for (int j = 0; j < J; ++j) counted += et_metrics::visible(vis, n * J + j);
        total_joints[n] = (double)counted;
        all += counted;
        for (int m = 0; m < M; ++m) {
            long long below = 0;
            for (int j = 0; j < J; ++j)
                below += et_metrics::visible(vis, n * J + j) && et_metrics::pck_error(locs, gt, n * J + j) < curve[m];
            err_joints[n * M + m] = (double)below;
        }
    }
    for (int t = 0; t < T; ++t) {
        long long below = 0;
        for (long long i = 0; i < items; ++i) below += et_metrics::visible(vis, i) && et_metrics::pck_error(locs, gt, i) < thresholds[t];
        pck[t] = et_metrics::ratio(below, all, 100.0);
    }
    return 0;
}

int et_eval_epe(int32_t F, int32_t J, const double *pred, const double *gt, const float *vis, double unit, double max_dist,
                double *mean, double *per_joint, void *stream)
{
    if (int e = check_epe("et_eval_epe", F, J, pred, gt, mean, per_joint)) return e;
    const long long items = (long long)F * J;
    hipLaunchKernelGGL(epe_items_kernel, dim3((unsigned)((items + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, items,
                       pred, gt, vis, unit, max_dist, per_joint);
    hipLaunchKernelGGL(epe_mean_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, items, pred, gt, unit, max_dist, mean);
    return check_launch("et_eval_epe");
}

int et_debug_host_eval_epe(int32_t F, int32_t J, const double *pred, const double *gt, const float *vis, double unit, double max_dist,
                           double *mean, double *per_joint)
{
    if (int e = check_epe("et_debug_host_eval_epe", F, J, pred, gt, mean, per_joint)) return e;
    const long long items = (long long)F * J;
    for (long long i = 0; i < items; ++i)
        per_joint[i] = et_metrics::visible(vis, i) ? et_metrics::epe_error(pred, gt, i, unit, max_dist) : 0.0;
    double p[et_metrics::kSumLanes];
    for (int t = 0; t < et_metrics::kSumLanes; ++t) p[t] = et_metrics::strided_partial(pred, gt, items, unit, max_dist, t);
    et_metrics::host_tree(p);
    *mean = p[0] / (double)items;
    return 0;
}

}  // extern "C"
