// libepipolar_amd.so: KEYPOINT.TRIANGULATION epipolar / epipolar_dlt -- the lifting that consumes the layer's corr_pos
// (vision/triangulation.py:234-348).  One wave per (frame, joint), four waves per block, one lane per hypothesis; float64.
// No atomics, no LDS: the result is bit-reproducible from run to run.  KEYPOINT.TRIANGULATION naive / refine (:99-232) search the
// same hypotheses without corr_pos and take the same mapping; pymvg (:425-441) has nothing to search, so every LANE takes one
// (frame, joint).  So does every lane of the gradient (et_triangulate_bwd): the forward's info word names the DLT to differentiate.
#include "et_common.h"
#include "et_triangulate.h"

namespace {
#include "et_wave_reduce.h"

__global__ __launch_bounds__(kWave * kWavesPerBlock) void triangulate_epipolar_kernel(const et_tri::Problem pr)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long item = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (item >= (long long)pr.F * pr.J) return;      // (whole waves leave: the reductions below see 64 lanes)
    const int f = (int)(item / pr.J), j = (int)(item % pr.J);
    const et_tri::Selection s = et_tri::select(pr, f, j);
    if (s.branch != 0 || pr.dlt) {                    // wave-uniform: one solve, no search
        if (lane == 0) et_tri::solve_direct(pr, f, j, s);
        return;
    }
    const et_tri::Hypothesis hy = et_tri::evaluate_hypothesis(pr, f, j, s.mask, lane);
    // arg-max keyed on (count, -hypothesis index): the first hypothesis with the largest count.  Exact in float (<= 8 * 64 + 63),
    // and unique to its lane, so exactly one lane finds its own key back.
    const float key = hy.count >= 0 ? (float)(hy.count * kWave + (kWave - 1 - lane)) : -1.f;
    if (key == wave_all_max(key)) {
        double X[3];
        const int bits = et_tri::finish_hypothesis(pr, f, j, hy, X);
        et_tri::store(pr, f, j, X, s.mask | bits);
    }
}

// naive / refine: as the kernel above -- one wave per (frame, joint), one lane per hypothesis
__global__ __launch_bounds__(kWave * kWavesPerBlock) void triangulate_ransac_kernel(const et_tri::ViewsProblem vp)
{
    const et_tri::Problem &pr = vp.pr;
    const int lane = threadIdx.x & (kWave - 1);
    const long long item = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (item >= (long long)pr.F * pr.J) return;      // (whole waves leave: the reduction below sees 64 lanes)
    const int f = (int)(item / pr.J), j = (int)(item % pr.J);
    int n;
    const int selected = et_tri::select_above(pr, f, j, n);
    if (n < 2) {                                      // wave-uniform
        if (lane == 0) et_tri::store_zeros(pr, f, j, selected);
        return;
    }
    const et_tri::Hypothesis hy = et_tri::evaluate_hypothesis(pr, f, j, selected, lane);
    // (the key of triangulate_epipolar_kernel: the first hypothesis with the largest count, unique to its lane)
    const float key = hy.count >= 0 ? (float)(hy.count * kWave + (kWave - 1 - lane)) : -1.f;
    if (key == wave_all_max(key)) et_tri::finish_views(vp, f, j, selected, hy);
}

constexpr int kPymvgBlock = 256;

// pymvg: one lane per (frame, joint)
__global__ __launch_bounds__(kPymvgBlock) void triangulate_pymvg_kernel(const et_tri::ViewsProblem vp)
{
    const long long item = (long long)blockIdx.x * kPymvgBlock + threadIdx.x;
    if (item >= (long long)vp.pr.F * vp.pr.J) return;
    et_tri::pymvg_joint(vp, (int)(item / vp.pr.J), (int)(item % vp.pr.J));
}

// the gradient in the detections: one lane per (frame, joint), as pymvg -- the info word leaves nothing to search
__global__ __launch_bounds__(kPymvgBlock) void triangulate_bwd_kernel(const et_tri::BackwardProblem bp)
{
    const long long item = (long long)blockIdx.x * kPymvgBlock + threadIdx.x;
    if (item >= (long long)bp.pr.F * bp.pr.J) return;
    et_tri::backward_joint(bp, (int)(item / bp.pr.J), (int)(item % bp.pr.J));
}

// The forwards' checks.  other_krt / corr_pos NULL: the backward of et_triangulate_views (H, W, downsample, resize are not read).
int make_backward_problem(const char *what, int32_t F, int32_t V, int32_t J, int32_t H, int32_t W, const float *pts, const float *krt,
                          const float *other_krt, const float *corr_pos, float downsample, float resize, const int32_t *info,
                          const double *grad_out, float *grad_pts, et_tri::BackwardProblem *bp)
{
    if (F < 1 || J < 1 || (long long)F * J > 0x7fffffffLL - kWavesPerBlock) return fail("%s: bad sizes F=%d J=%d", what, F, J);
    if (V < 1 || V > et_tri::kMaxViews) return fail("%s: V=%d outside [1, %d]", what, V, et_tri::kMaxViews);
    if (!pts || !krt || !info || !grad_out || !grad_pts) return fail("%s: NULL pointer", what);
    if (!other_krt != !corr_pos) return fail("%s: other_krt and corr_pos must both be given or both be NULL", what);
    if (corr_pos) {
        if (H < 1 || W < 1) return fail("%s: bad map size H=%d W=%d", what, H, W);
        if (!(downsample > 0.f) || !(resize > 0.f)) return fail("%s: downsample / resize must be positive", what);
    } else {
        H = W = 0;
        downsample = resize = 0.f;
    }
    bp->pr = et_tri::Problem{F, V, J, H, W, pts, nullptr, krt, other_krt, corr_pos, (double)downsample, (double)resize, 0.0, 0.f, 0,
                             nullptr, nullptr};
    bp->word = info;
    bp->grad_out = grad_out;
    bp->grad_pts = grad_pts;
    return 0;
}

int make_views_problem(const char *what, int32_t F, int32_t V, int32_t J, const float *pts, const float *conf, const float *krt,
                       int32_t method, double conf_thres, double ransac_thres, double *out, int32_t *info, et_tri::ViewsProblem *vp)
{
    if (F < 1 || J < 1 || (long long)F * J > 0x7fffffffLL - kWavesPerBlock) return fail("%s: bad sizes F=%d J=%d", what, F, J);
    if (V < 1 || V > et_tri::kMaxViews) return fail("%s: V=%d outside [1, %d]", what, V, et_tri::kMaxViews);
    if (method != et_tri::kMethodPymvg && method != et_tri::kMethodNaive && method != et_tri::kMethodRefine)
        return fail("%s: method %d is none of 0 (pymvg), 1 (naive), 2 (refine)", what, method);
    if (!pts || !conf || !krt || !out) return fail("%s: NULL pointer", what);
    if (!std::isfinite(conf_thres) || conf_thres > et_tri::kMaxConfThres)
        return fail("%s: conf_thres must be finite and at most %g", what, et_tri::kMaxConfThres);
    vp->pr = et_tri::Problem{F, V, J, 0, 0, pts, conf, krt, nullptr, nullptr, 0.0, 0.0, ransac_thres, (float)conf_thres, 0, out, info};
    vp->conf_thres = conf_thres;
    vp->method = method;
    return 0;
}

int make_problem(const char *what, int32_t F, int32_t V, int32_t J, int32_t H, int32_t W, const float *pts, const float *conf,
                 const float *krt, const float *other_krt, const float *corr_pos, float downsample, float resize,
                 double conf_thres, double ransac_thres, int32_t dlt, double *out, int32_t *info, et_tri::Problem *pr)
{
    if (F < 1 || J < 1 || (long long)F * J > 0x7fffffffLL - kWavesPerBlock) return fail("%s: bad sizes F=%d J=%d", what, F, J);
    if (V < 1 || V > et_tri::kMaxViews) return fail("%s: V=%d outside [1, %d]", what, V, et_tri::kMaxViews);
    if (H < 1 || W < 1) return fail("%s: bad map size H=%d W=%d", what, H, W);
    if (!pts || !conf || !krt || !other_krt || !corr_pos || !out) return fail("%s: NULL pointer", what);
    if (!(downsample > 0.f) || !(resize > 0.f)) return fail("%s: downsample / resize must be positive", what);
    *pr = et_tri::Problem{F, V, J, H, W, pts, conf, krt, other_krt, corr_pos, (double)downsample, (double)resize, ransac_thres,
                          (float)conf_thres, dlt != 0, out, info};
    return 0;
}

}  // namespace

extern "C" {

int et_triangulate_epipolar(int32_t F, int32_t V, int32_t J, int32_t H, int32_t W, const float *pts, const float *conf,
                            const float *krt, const float *other_krt, const float *corr_pos, float downsample, float resize,
                            double conf_thres, double ransac_thres, int32_t dlt, double *out, int32_t *info, void *stream)
{
    et_tri::Problem pr;
    if (int e = make_problem("et_triangulate_epipolar", F, V, J, H, W, pts, conf, krt, other_krt, corr_pos, downsample, resize,
                             conf_thres, ransac_thres, dlt, out, info, &pr))
        return e;
    const unsigned blocks = (unsigned)(((long long)F * J + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(triangulate_epipolar_kernel, dim3(blocks), dim3(kWave * kWavesPerBlock), 0, (hipStream_t)stream, pr);
    return check_launch("et_triangulate_epipolar");
}

int et_debug_host_triangulate_epipolar(int32_t F, int32_t V, int32_t J, int32_t H, int32_t W, const float *pts, const float *conf,
                                       const float *krt, const float *other_krt, const float *corr_pos, float downsample,
                                       float resize, double conf_thres, double ransac_thres, int32_t dlt, double *out,
                                       int32_t *info)
{
    et_tri::Problem pr;
    if (int e = make_problem("et_debug_host_triangulate_epipolar", F, V, J, H, W, pts, conf, krt, other_krt, corr_pos, downsample,
                             resize, conf_thres, ransac_thres, dlt, out, info, &pr))
        return e;
    for (int f = 0; f < F; ++f)
        for (int j = 0; j < J; ++j) et_tri::joint_serial(pr, f, j);
    return 0;
}

int et_triangulate_views(int32_t F, int32_t V, int32_t J, const float *pts, const float *conf, const float *krt, int32_t method,
                         double conf_thres, double ransac_thres, double *out, int32_t *info, void *stream)
{
    et_tri::ViewsProblem vp;
    if (int e = make_views_problem("et_triangulate_views", F, V, J, pts, conf, krt, method, conf_thres, ransac_thres, out, info, &vp))
        return e;
    const long long items = (long long)F * J;
    if (method == et_tri::kMethodPymvg)
        hipLaunchKernelGGL(triangulate_pymvg_kernel, dim3((unsigned)((items + kPymvgBlock - 1) / kPymvgBlock)), dim3(kPymvgBlock), 0,
                           (hipStream_t)stream, vp);
    else
        hipLaunchKernelGGL(triangulate_ransac_kernel, dim3((unsigned)((items + kWavesPerBlock - 1) / kWavesPerBlock)),
                           dim3(kWave * kWavesPerBlock), 0, (hipStream_t)stream, vp);
    return check_launch("et_triangulate_views");
}

int et_debug_host_triangulate_views(int32_t F, int32_t V, int32_t J, const float *pts, const float *conf, const float *krt,
                                    int32_t method, double conf_thres, double ransac_thres, double *out, int32_t *info)
{
    et_tri::ViewsProblem vp;
    if (int e = make_views_problem("et_debug_host_triangulate_views", F, V, J, pts, conf, krt, method, conf_thres, ransac_thres, out,
                                   info, &vp))
        return e;
    for (int f = 0; f < F; ++f)
        for (int j = 0; j < J; ++j) et_tri::views_joint_serial(vp, f, j);
    return 0;
}

int et_triangulate_bwd(int32_t F, int32_t V, int32_t J, int32_t H, int32_t W, const float *pts, const float *krt,
                       const float *other_krt, const float *corr_pos, float downsample, float resize, const int32_t *info,
                       const double *grad_out, float *grad_pts, void *stream)
{
    et_tri::BackwardProblem bp;
    if (int e = make_backward_problem("et_triangulate_bwd", F, V, J, H, W, pts, krt, other_krt, corr_pos, downsample, resize, info,
                                      grad_out, grad_pts, &bp))
        return e;
    const long long items = (long long)F * J;
    hipLaunchKernelGGL(triangulate_bwd_kernel, dim3((unsigned)((items + kPymvgBlock - 1) / kPymvgBlock)), dim3(kPymvgBlock), 0,
                       (hipStream_t)stream, bp);
    return check_launch("et_triangulate_bwd");
}

int et_debug_host_triangulate_bwd(int32_t F, int32_t V, int32_t J, int32_t H, int32_t W, const float *pts, const float *krt,
                                  const float *other_krt, const float *corr_pos, float downsample, float resize,
                                  const int32_t *info, const double *grad_out, float *grad_pts)
{
    et_tri::BackwardProblem bp;
    if (int e = make_backward_problem("et_debug_host_triangulate_bwd", F, V, J, H, W, pts, krt, other_krt, corr_pos, downsample,
                                      resize, info, grad_out, grad_pts, &bp))
        return e;
    for (int f = 0; f < F; ++f)
        for (int j = 0; j < J; ++j) et_tri::backward_joint(bp, f, j);
    return 0;
}

}  // extern "C"
