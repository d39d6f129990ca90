// libepipolar_amd.so: KEYPOINT.TRIANGULATION rpsm, the recursive pictorial structure model (modeling/pictorial_cuda.py:222-254),
// for a batch of frames.  Three kernels, float32 as the reference, no atomics: the same bits on every run.
//   rpsm_unary_kernel      first stage, one lane per (frame, joint, bin): the views in a loop
//   rpsm_message_kernel    first stage, one launch per tree level, deepest first: a block owns (frame, limb, 256 parent bins),
//                          the child's energies (<= 4096 floats, 16 KB) and its 3 x n axis positions sit in LDS, every lane
//                          walks the child's bins in ascending order -- all lanes read the same LDS word, a broadcast
//   rpsm_refine_kernel     one block per frame: the root's arg-max, the back-track, then all RECUR_DEPTH levels in LDS
// Bin positions follow from the bin index and limb compatibility is a distance band: there is no pairwise table.
#include "et_common.h"
#include "et_rpsm.h"

namespace {

constexpr int kBlock = 256;

struct Planes {     // the first stage's workspace, (F, J, B) each
    float *U, *M;
    int32_t *BP;
};

__global__ __launch_bounds__(kBlock) void rpsm_unary_kernel(const et_pict::Problem pr, float *U)
{
    const int n = pr.first_nbins, B = n * n * n;
    const long long item = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (item >= (long long)pr.F * pr.J * B) return;
    const int b = (int)(item % B), fj = (int)(item / B), f = fj / pr.J, j = fj % pr.J;
    const float *ctr = pr.center + (size_t)f * 3;
    U[item] = et_pict::unary(pr, f, j, et_pict::axis_offset(pr.half[0], n, b / (n * n)) + ctr[0],
                             et_pict::axis_offset(pr.half[0], n, b / n % n) + ctr[1], et_pict::axis_offset(pr.half[0], n, b % n) + ctr[2]);
}

// grid (slabs of parent bins, joints of this level, frames)
__global__ __launch_bounds__(kBlock) void rpsm_message_kernel(const et_pict::Problem pr, const Planes ws, int level)
{
    __shared__ float Ec[et_pict::kMaxFirstBins * et_pict::kMaxFirstBins * et_pict::kMaxFirstBins];
    __shared__ float ax[3][et_pict::kMaxFirstBins];
    const int n = pr.first_nbins, B = n * n * n;
    const int f = blockIdx.z, j = pr.by_level[pr.level_begin[level] + blockIdx.y];
    const size_t plane = (size_t)f * pr.J * B;
    for (int b = threadIdx.x; b < B; b += kBlock) Ec[b] = et_pict::energy(pr, ws.U + plane, ws.M + plane, B, j, b);
    if (threadIdx.x < 3 * n)
        ax[threadIdx.x / n][threadIdx.x % n] = et_pict::axis_offset(pr.half[0], n, threadIdx.x % n) + pr.center[(size_t)f * 3 + threadIdx.x / n];
    __syncthreads();
    const int a = blockIdx.x * kBlock + threadIdx.x;
    if (a >= B) return;
    float best;
    int arg;
    et_pict::message(ax[0][a / (n * n)], ax[1][a / n % n], ax[2][a % n], ax[0], ax[1], ax[2], n, Ec,
                     et_pict::limb_length(pr, f, j, true), pr.tolerance, &best, &arg);
    ws.M[plane + (size_t)j * B + a] = best;
    ws.BP[plane + (size_t)j * B + a] = arg;
}

__global__ __launch_bounds__(kBlock) void rpsm_refine_kernel(const et_pict::Problem pr, const Planes ws)
{
    __shared__ et_pict::Refine s;
    __shared__ float red_v[kBlock];
    __shared__ int red_i[kBlock];
    const int n = pr.first_nbins, B = n * n * n, f = blockIdx.x, tid = threadIdx.x;
    const size_t plane = (size_t)f * pr.J * B;
    // the root's FIRST arg-max: each lane walks its bins in ascending order, the tree keeps the smaller index among equals
    float best = -INFINITY;
    int arg = 0x7fffffff;
    for (int b = tid; b < B; b += kBlock) {
        const float e = et_pict::energy(pr, ws.U + plane, ws.M + plane, B, pr.root, b);
        if (e > best || arg == 0x7fffffff) {
            best = e;
            arg = b;
        }
    }
    red_v[tid] = best;
    red_i[tid] = arg;
    __syncthreads();
    for (int w = kBlock / 2; w >= 1; w >>= 1) {
        if (tid < w) {
            const float v = red_v[tid + w];
            const int i = red_i[tid + w];
            if (i != 0x7fffffff && (red_i[tid] == 0x7fffffff || v > red_v[tid] || (v == red_v[tid] && i < red_i[tid]))) {
                red_v[tid] = v;
                red_i[tid] = i;
            }
        }
        __syncthreads();
    }
    if (tid == 0) et_pict::first_stage_finish(pr, f, red_i[0], ws.BP + plane, s);
    __syncthreads();
    et_pict::refine_levels(pr, f, s, tid, kBlock);
}

size_t plane_bytes(long long F, int J, int first_nbins)
{
    return (size_t)F * J * first_nbins * first_nbins * first_nbins * 4;
}

int make_problem(const char *what, int32_t F, int32_t V, int32_t J, int32_t H, int32_t W, const float *heatmaps, const float *cams,
                 const float *trans, const float *center, const float *limb_length, const float *first_limb_length,
                 const int32_t *parent, float image_w, float image_h, double grid_size, int32_t first_nbins, int32_t recur_nbins,
                 int32_t recur_depth, float tolerance, int32_t align_corners, float *out, int32_t *path, et_pict::Problem *pr)
{
    using namespace et_pict;
    if (F < 1 || H < 1 || W < 1) return fail("%s: bad sizes F=%d H=%d W=%d", what, F, H, W);
    if (V < 1 || V > kMaxViews) return fail("%s: V=%d outside [1, %d]", what, V, kMaxViews);
    if (J < 1 || J > kMaxJoints) return fail("%s: J=%d outside [1, %d]", what, J, kMaxJoints);
    if (first_nbins < kMinBins || first_nbins > kMaxFirstBins)
        return fail("%s: first_nbins=%d outside [%d, %d]", what, first_nbins, kMinBins, kMaxFirstBins);
    if (recur_nbins < kMinBins || recur_nbins > kMaxRecurBins)
        return fail("%s: recur_nbins=%d outside [%d, %d]", what, recur_nbins, kMinBins, kMaxRecurBins);
    if (recur_depth < 0 || recur_depth > kMaxDepth) return fail("%s: recur_depth=%d outside [0, %d]", what, recur_depth, kMaxDepth);
    if (!heatmaps || !cams || !trans || !center || !parent || !out || (!limb_length && J > 1)) return fail("%s: NULL pointer", what);
    if (!(image_w > 0.f) || !(image_h > 0.f) || !(grid_size > 0.0) || !(tolerance > 0.f))
        return fail("%s: image size, grid_size and tolerance must be positive", what);
    if ((long long)F * J * first_nbins * first_nbins * first_nbins > 0x7fffffffLL - kBlock || F > 65535)
        return fail("%s: F=%d frames are too many for one call", what, F);
    *pr = Problem{};
    pr->F = F, pr->V = V, pr->J = J, pr->H = H, pr->W = W;
    pr->heat = heatmaps, pr->cams = cams, pr->trans = trans, pr->center = center;
    pr->limb = limb_length, pr->first_limb = first_limb_length;
    pr->image_w = image_w, pr->image_h = image_h, pr->tolerance = tolerance;
    pr->first_nbins = first_nbins, pr->recur_nbins = recur_nbins, pr->depth = recur_depth, pr->align_corners = align_corners != 0;
    pr->out = out, pr->path = path;
    // the reference halves a Python float (double) and hands it to torch.linspace, which rounds it to float32
    double size = grid_size;
    pr->half[0] = (float)(size / 2);
    size /= first_nbins;
    for (int k = 1; k <= recur_depth; ++k, size /= recur_nbins) pr->half[k] = (float)(size / 2);
    // the tree: one root, every other joint reaches it
    pr->root = -1;
    for (int j = 0, e = 0; j < J; ++j) {
        if (parent[j] == -1) {
            if (pr->root >= 0) return fail("%s: parent is not a tree with one root (joints %d and %d have none)", what, pr->root, j);
            pr->root = j;
            pr->limb_of[j] = -1;
        } else if (parent[j] < 0 || parent[j] >= J || parent[j] == j) {
            return fail("%s: parent is not a tree with one root (parent[%d] = %d)", what, j, parent[j]);
        } else {
            pr->limb_of[j] = (int8_t)e++;
        }
        pr->parent[j] = (int8_t)parent[j];
    }
    if (pr->root < 0) return fail("%s: parent is not a tree with one root (no joint has parent -1)", what);
    pr->levels = 0;
    for (int j = 0; j < J; ++j) {
        int lv = 0, k = j;
        while (k != pr->root && lv <= J) k = parent[k], ++lv;
        if (lv > J) return fail("%s: parent is not a tree with one root (joint %d never reaches the root)", what, j);
        pr->level[j] = (int8_t)lv;
        if (lv > pr->levels) pr->levels = lv;
    }
    int at = 0;
    for (int lv = 0; lv <= pr->levels; ++lv) {
        pr->level_begin[lv] = (int8_t)at;
        for (int j = 0; j < J; ++j)
            if (pr->level[j] == lv) pr->by_level[at++] = (int8_t)j;
    }
    pr->level_begin[pr->levels + 1] = (int8_t)at;
    return 0;
}

}  // namespace

extern "C" {

size_t et_rpsm_workspace_bytes(int32_t F, int32_t J, int32_t first_nbins, int32_t recur_nbins)
{
    (void)recur_nbins;      // the recursion lives in LDS
    if (F < 1 || J < 1 || J > et_pict::kMaxJoints || first_nbins < et_pict::kMinBins || first_nbins > et_pict::kMaxFirstBins) return 0;
    return 3 * plane_bytes(F, J, first_nbins) + 16;      // + 16: the planes start at the next 16-byte boundary
}

int et_rpsm(int32_t F, int32_t V, int32_t J, int32_t H, int32_t W, const float *heatmaps, const float *cams, const float *trans,
            const float *center, const float *limb_length, const float *first_limb_length, const int32_t *parent, float image_w,
            float image_h, double grid_size, int32_t first_nbins, int32_t recur_nbins, int32_t recur_depth, float tolerance,
            int32_t align_corners, float *out, int32_t *path, void *workspace, size_t workspace_bytes, void *stream)
{
    et_pict::Problem pr;
    // `parent` is a HOST array (J values): the tree shapes the launches
    if (int e = make_problem("et_rpsm", F, V, J, H, W, heatmaps, cams, trans, center, limb_length, first_limb_length, parent, image_w,
                             image_h, grid_size, first_nbins, recur_nbins, recur_depth, tolerance, align_corners, out, path, &pr))
        return e;
    if (!workspace) return fail("et_rpsm: NULL pointer");
    const size_t need = et_rpsm_workspace_bytes(F, J, first_nbins, recur_nbins);
    if (workspace_bytes < need) return fail("et_rpsm: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const size_t pb = plane_bytes(F, J, first_nbins);
    char *base = (char *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
    const Planes ws{(float *)base, (float *)(base + pb), (int32_t *)(base + 2 * pb)};
    hipStream_t st = (hipStream_t)stream;
    const int B = first_nbins * first_nbins * first_nbins;
    const unsigned items = (unsigned)(((long long)F * J * B + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(rpsm_unary_kernel, dim3(items), dim3(kBlock), 0, st, pr, ws.U);
    for (int lv = pr.levels; lv >= 1; --lv) {
        const int count = pr.level_begin[lv + 1] - pr.level_begin[lv];
        hipLaunchKernelGGL(rpsm_message_kernel, dim3((B + kBlock - 1) / kBlock, count, F), dim3(kBlock), 0, st, pr, ws, lv);
    }
    hipLaunchKernelGGL(rpsm_refine_kernel, dim3(F), dim3(kBlock), 0, st, pr, ws);
    return check_launch("et_rpsm");
}

int et_debug_host_rpsm(int32_t F, int32_t V, int32_t J, int32_t H, int32_t W, const float *heatmaps, const float *cams,
                       const float *trans, const float *center, const float *limb_length, const float *first_limb_length,
                       const int32_t *parent, float image_w, float image_h, double grid_size, int32_t first_nbins,
                       int32_t recur_nbins, int32_t recur_depth, float tolerance, int32_t align_corners, float *out, int32_t *path)
{
    et_pict::Problem pr;
    if (int e = make_problem("et_debug_host_rpsm", F, V, J, H, W, heatmaps, cams, trans, center, limb_length, first_limb_length,
                             parent, image_w, image_h, grid_size, first_nbins, recur_nbins, recur_depth, tolerance, align_corners,
                             out, path, &pr))
        return e;
    const size_t cells = (size_t)J * first_nbins * first_nbins * first_nbins;
    float *U = new float[2 * cells + cells / J];
    int32_t *BP = new int32_t[cells];
    for (int f = 0; f < F; ++f) et_pict::frame_serial(pr, f, U, U + cells, BP, U + 2 * cells);
    delete[] U;
    delete[] BP;
    return 0;
}

}  // extern "C"
