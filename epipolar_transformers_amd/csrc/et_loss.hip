// libepipolar_amd.so: the training loss of Modelbuilder.forward on the device -- the heat-map targets of the data loader
// (Heatmapcreator.get) and the criteria KEYPOINT.LOSS names, joint / smoothmse / mse (et_loss.h names the reference's lines).
// The reference ships a dense target stack from the host and runs the loss as a chain of elementwise torch ops; here the loss is
// two streams in and one number out, its gradient two streams in and one out, and with the points instead of the stack the
// target is never stored at all.
//
//   et_heatmap_targets    targets_kernel: one block per map, a lane per 16-byte quad, float64 exp rounded once to float32.
//   et_heatmap_loss       loss_map_kernel: one block of 256 lanes per map; every lane adds the float64 of its float32 terms in
//                         ascending order (et_loss::walk: whole quads as float4, a map's partial first and last quad in scalar),
//                         then a pairwise tree through LDS; one double per map.  loss_total_kernel: ONE block adds per joint over
//                         n ascending, then over the joints ascending (and the weights, for smoothmse), divides, rounds once.
//   et_heatmap_loss_bwd   loss_grad_kernel: the same walk; each element of d loss / d pred in float64 from the float32
//                         difference, times grad_output / denominator read through device pointers, rounded once.
// With `points` instead of `target` each lane makes the target value of its own pixels with the device function
// et_heatmap_targets runs.  No float atomics: every output is bit-reproducible, and the host hooks walk the same order.
#include "et_common.h"
#include "et_loss.h"

namespace {

constexpr int kBlock = et_loss::kLanes;

struct LossArgs {
    et_loss::Operands o;
    int N, J, HW, kind, per_joint;
};

__global__ __launch_bounds__(kBlock) void targets_kernel(int HW, int W, const double *__restrict__ points, double sigma,
                                                          double downsample, bool vec, float *__restrict__ out)
{
    const et_loss::Grid grid = et_loss::make_grid(sigma, downsample);
    et_loss::lane_targets(grid, points, blockIdx.x, HW, W, threadIdx.x, vec, out);
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void loss_map_kernel(LossArgs a, double sigma, double downsample, double *__restrict__ partials)
{
    __shared__ double p[kBlock];
    const int t = threadIdx.x;
    if (!a.o.target) a.o.grid = et_loss::make_grid(sigma, downsample);
    p[t] = et_loss::lane_partial<KIND>(a.o, blockIdx.x, a.HW, t);
    __syncthreads();
    for (int half = kBlock / 2; half > 0; half >>= 1) {
        if (t < half) p[t] += p[t + half];
        __syncthreads();
    }
    if (t == 0) partials[blockIdx.x] = p[0];
}

// `partials` (N, J) -> loss, den.  Thread j owns column j: it leaves the column's sum in row 0, which nobody else reads or writes
// before the barrier; thread 0 then adds the joints in ascending order.
__global__ __launch_bounds__(kBlock) void loss_total_kernel(int kind, int N, int J, int HW, int per_joint, const float *__restrict__ weight,
                                                             double *partials, float *__restrict__ loss, double *__restrict__ den)
{
    __shared__ double wsum[kBlock];
    const int t = threadIdx.x;
    double ws = 0.0;
    for (int j = t; j < J; j += kBlock) {
        partials[j] = et_loss::column_sum(partials, N, J, j);
        if (kind == et_loss::kSmoothMse) ws += weight ? et_loss::column_sum(weight, N, J, j) : (double)N;
    }
    wsum[t] = ws;
    __syncthreads();
    if (t != 0) return;
    double total = 0.0, weights = 0.0;
    for (int j = 0; j < J; ++j) total += partials[j];
    for (int i = 0; i < kBlock && i < J; ++i) weights += wsum[i];
    const double d = et_loss::denominator(kind, N, J, HW, per_joint, weights);
    *den = d;
    *loss = (float)(total / d);
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void loss_grad_kernel(LossArgs a, double sigma, double downsample, const double *__restrict__ den,
                                                            const float *__restrict__ grad_out, float *__restrict__ grad_pred)
{
    if (!a.o.target) a.o.grid = et_loss::make_grid(sigma, downsample);
    const double c = (double)*grad_out / *den;
    et_loss::lane_gradient<KIND>(a.o, blockIdx.x, a.HW, threadIdx.x, c, grad_pred);
}

bool aligned16(const void *a, const void *b = nullptr, const void *c = nullptr)
{
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

int check_sizes(const char *what, int32_t N, int32_t J, int32_t H, int32_t W)
{
    if (N < 1 || J < 1 || (long long)N * J > 0x7fffffffLL) return fail("%s: bad sizes N=%d J=%d", what, N, J);
    if (H < 1 || W < 1 || (long long)H * W > et_loss::kMaxMapElements)
        return fail("%s: map %d x %d outside H >= 1, W >= 1, H * W <= %d", what, H, W, et_loss::kMaxMapElements);
    return 0;
}

int check_grid(const char *what, double sigma, double downsample)
{
    if (!(sigma > 0.0) || !(downsample > 0.0) || sigma > 1e30 || downsample > 1e30)
        return fail("%s: sigma %g and downsample %g must be positive and finite", what, sigma, downsample);
    return 0;
}

int check_targets(const char *what, int32_t N, int32_t J, int32_t H, int32_t W, const double *points, double sigma, double downsample,
                  const float *out)
{
    if (int e = check_sizes(what, N, J, H, W)) return e;
    if (!points || !out) return fail("%s: NULL pointer", what);
    return check_grid(what, sigma, downsample);
}

// the checks et_heatmap_loss and et_heatmap_loss_bwd share; r0, r1, r2: the pointers of their own, all required
int check_loss(const char *what, int32_t kind, int32_t N, int32_t J, int32_t H, int32_t W, const float *pred, const float *target,
               const double *points, double sigma, double downsample, const float *weight, const void *r0, const void *r1, const void *r2)
{
    if (int e = check_sizes(what, N, J, H, W)) return e;
    if (kind != et_loss::kJoint && kind != et_loss::kSmoothMse && kind != et_loss::kMse)
        return fail("%s: unknown kind %d (ET_LOSS_JOINT, ET_LOSS_SMOOTHMSE, ET_LOSS_MSE)", what, kind);
    if (kind == et_loss::kMse && weight) return fail("%s: ET_LOSS_MSE takes no weight (MaskedMSELoss with masks=None)", what);
    if (!pred || !r0 || !r1 || !r2) return fail("%s: NULL pointer", what);
    if (!target == !points) return fail("%s: give either target or points, not %s", what, target ? "both" : "neither");
    return points ? check_grid(what, sigma, downsample) : 0;
}

LossArgs loss_args(int32_t kind, int32_t N, int32_t J, int32_t H, int32_t W, const float *pred, const float *target, const double *points,
                   const float *weight, int32_t per_joint, const float *grad)
{
    LossArgs a{};
    a.o.pred = pred, a.o.target = target, a.o.points = points, a.o.weight = weight, a.o.W = W;
    a.o.vec = aligned16(pred, target, grad);
    a.N = N, a.J = J, a.HW = H * W, a.kind = kind, a.per_joint = per_joint;
    return a;
}

// runs `body<KIND>` for the runtime kind
#define ET_LOSS_DISPATCH(KIND_VALUE, BODY)                      \
    switch (KIND_VALUE) {                                       \
        case et_loss::kJoint: { BODY(et_loss::kJoint) } break;  \
        case et_loss::kSmoothMse: { BODY(et_loss::kSmoothMse) } break; \
        default: { BODY(et_loss::kMse) } break;                 \
    }

}  // namespace

extern "C" {

int et_heatmap_targets(int32_t N, int32_t J, int32_t H, int32_t W, const double *points, double sigma, double downsample, float *out,
                       void *stream)
{
    if (int e = check_targets("et_heatmap_targets", N, J, H, W, points, sigma, downsample, out)) return e;
    hipLaunchKernelGGL(targets_kernel, dim3((unsigned)(N * J)), dim3(kBlock), 0, (hipStream_t)stream, H * W, W, points, sigma, downsample,
                       aligned16(out), out);
    return check_launch("et_heatmap_targets");
}

int et_debug_host_heatmap_targets(int32_t N, int32_t J, int32_t H, int32_t W, const double *points, double sigma, double downsample,
                                  float *out)
{
    if (int e = check_targets("et_debug_host_heatmap_targets", N, J, H, W, points, sigma, downsample, out)) return e;
    const et_loss::Grid grid = et_loss::make_grid(sigma, downsample);
    for (long long item = 0; item < (long long)N * J; ++item)
        for (int t = 0; t < kBlock; ++t) et_loss::lane_targets(grid, points, item, H * W, W, t, aligned16(out), out);
    return 0;
}

int et_heatmap_loss(int32_t kind, int32_t N, int32_t J, int32_t H, int32_t W, const float *pred, const float *target,
                    const double *points, double sigma, double downsample, const float *weight, int32_t per_joint, double *partials,
                    float *loss, double *den, void *stream)
{
    if (int e = check_loss("et_heatmap_loss", kind, N, J, H, W, pred, target, points, sigma, downsample, weight, partials, loss, den)) return e;
    const LossArgs a = loss_args(kind, N, J, H, W, pred, target, points, weight, per_joint, nullptr);
#define ET_LOSS_LAUNCH(K) \
    hipLaunchKernelGGL(loss_map_kernel<K>, dim3((unsigned)(N * J)), dim3(kBlock), 0, (hipStream_t)stream, a, sigma, downsample, partials);
    ET_LOSS_DISPATCH(kind, ET_LOSS_LAUNCH)
#undef ET_LOSS_LAUNCH
    hipLaunchKernelGGL(loss_total_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, kind, N, J, H * W, per_joint, weight, partials, loss,
                       den);
    return check_launch("et_heatmap_loss");
}

int et_debug_host_heatmap_loss(int32_t kind, int32_t N, int32_t J, int32_t H, int32_t W, const float *pred, const float *target,
                               const double *points, double sigma, double downsample, const float *weight, int32_t per_joint,
                               double *partials, float *loss, double *den)
{
    if (int e = check_loss("et_debug_host_heatmap_loss", kind, N, J, H, W, pred, target, points, sigma, downsample, weight, partials, loss, den))
        return e;
    LossArgs a = loss_args(kind, N, J, H, W, pred, target, points, weight, per_joint, nullptr);
    if (points) a.o.grid = et_loss::make_grid(sigma, downsample);
    for (long long item = 0; item < (long long)N * J; ++item) {
        double p[kBlock];
#define ET_LOSS_LANES(K) \
    for (int t = 0; t < kBlock; ++t) p[t] = et_loss::lane_partial<K>(a.o, item, a.HW, t);
        ET_LOSS_DISPATCH(kind, ET_LOSS_LANES)
#undef ET_LOSS_LANES
        et_loss::host_tree(p);
        partials[item] = p[0];
    }
    // loss_total_kernel's order: a column's sum into row 0, the weights per thread (columns t, t + 256, ...), then both in order
    double wsum[kBlock] = {};
    for (int j = 0; j < J; ++j) {
        partials[j] = et_loss::column_sum(partials, N, J, j);
        if (kind == et_loss::kSmoothMse) wsum[j % kBlock] += weight ? et_loss::column_sum(weight, N, J, j) : (double)N;
    }
    double total = 0.0, weights = 0.0;
    for (int j = 0; j < J; ++j) total += partials[j];
    for (int i = 0; i < kBlock && i < J; ++i) weights += wsum[i];
    *den = et_loss::denominator(kind, N, J, a.HW, per_joint, weights);
    *loss = (float)(total / *den);
    return 0;
}

int et_heatmap_loss_bwd(int32_t kind, int32_t N, int32_t J, int32_t H, int32_t W, const float *pred, const float *target,
                        const double *points, double sigma, double downsample, const float *weight, const double *den,
                        const float *grad_out, float *grad_pred, void *stream)
{
    if (int e = check_loss("et_heatmap_loss_bwd", kind, N, J, H, W, pred, target, points, sigma, downsample, weight, den, grad_out, grad_pred))
        return e;
    const LossArgs a = loss_args(kind, N, J, H, W, pred, target, points, weight, 0, grad_pred);
#define ET_LOSS_LAUNCH(K) \
    hipLaunchKernelGGL(loss_grad_kernel<K>, dim3((unsigned)(N * J)), dim3(kBlock), 0, (hipStream_t)stream, a, sigma, downsample, den, grad_out, \
                       grad_pred);
    ET_LOSS_DISPATCH(kind, ET_LOSS_LAUNCH)
#undef ET_LOSS_LAUNCH
    return check_launch("et_heatmap_loss_bwd");
}

int et_debug_host_heatmap_loss_bwd(int32_t kind, int32_t N, int32_t J, int32_t H, int32_t W, const float *pred, const float *target,
                                   const double *points, double sigma, double downsample, const float *weight, const double *den,
                                   const float *grad_out, float *grad_pred)
{
    if (int e = check_loss("et_debug_host_heatmap_loss_bwd", kind, N, J, H, W, pred, target, points, sigma, downsample, weight, den, grad_out,
                           grad_pred))
        return e;
    LossArgs a = loss_args(kind, N, J, H, W, pred, target, points, weight, 0, grad_pred);
    if (points) a.o.grid = et_loss::make_grid(sigma, downsample);
    const double c = (double)*grad_out / *den;
    for (long long item = 0; item < (long long)N * J; ++item) {
#define ET_LOSS_LANES(K) \
    for (int t = 0; t < kBlock; ++t) et_loss::lane_gradient<K>(a.o, item, a.HW, t, c, grad_pred);
        ET_LOSS_DISPATCH(kind, ET_LOSS_LANES)
#undef ET_LOSS_LANES
    }
    return 0;
}

}  // extern "C"
