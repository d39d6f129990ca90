// KEYPOINT.TRIANGULATION rpsm, the recursive pictorial structure model (modeling/pictorial_cuda.py:17-254): the pieces the device
// kernels and the host test hook share (plain C++, float32 as the reference, __host__ __device__; included by et_rpsm.hip only).
//
//   axis_offset()      torch.linspace(-size/2, size/2, n)[i] as torch's CPU kernel rounds it; a bin's position is that plus the
//                      grid's centre, per axis, with bin b = (ix * n + iy) * n + iz (compute_grid, :93-104)
//   unary()            one bin of one joint: the sum over the views, in ascending order, of ONE bilinear sample of the view's heat
//                      map at the bin's projection (compute_unary_term, :140-199, F.grid_sample with zero padding)
//   message()          one parent bin of one limb: max over the child's bins, walked in ascending order with a strict >, of
//                      compat(a, c) * E_child[c], compat = | ||x_a - x_c + 1e-6|| + 1e-9 - L | < tolerance (compute_pairwise, pdist2);
//                      child positions come from three per-axis arrays, never from a table
//   energy()           E_j[b] = unary_j[b] * the messages of j's children in ascending joint index (infer, :17-71)
//   refine_levels()    the RECUR_DEPTH levels after the first stage for ONE frame, written for a team of `nt` workers that meet at
//                      team_sync(): the device runs it with one block per frame, the host hook with a team of one
//   frame_serial()     (host only) the whole frame: first stage in loops over the same unary() / message(), then refine_levels()
//
// The first stage keeps, per frame, joint and bin, the unary U, the message M the joint sends to its parent (indexed by the
// PARENT's bin) and the arg-max BP behind it; energies are never stored: whoever needs E_j multiplies U_j by its children's M.
// So no two limbs write the same word, nothing is accumulated with atomics, and the result is the same bits on every run.
#pragma once
#include <math.h>
#include <stdint.h>

namespace et_pict {

constexpr int kMaxViews = 8;
constexpr int kMaxJoints = 32;
constexpr int kMinBins = 2;
constexpr int kMaxFirstBins = 16;                                     // 4096 bins: one joint's energies are 16 KB of LDS
constexpr int kMaxRecurBins = 3;
constexpr int kMaxRecurCells = kMaxRecurBins * kMaxRecurBins * kMaxRecurBins;
constexpr int kMaxDepth = 16;
constexpr float kPairEps = 1e-6f;    // torch.pairwise_distance adds its eps to the difference vector
constexpr float kDistEps = 1e-9f;    // compute_pairwise adds this to the distance (absorbed by float32 above ~1e-2 mm; kept)

struct Problem {
    int F, V, J, H, W;
    const float *heat, *cams, *trans, *center;
    const float *limb, *first_limb;   // (F, J - 1): limb e ends at the e-th non-root joint in ascending order
    float image_w, image_h, tolerance;
    int first_nbins, recur_nbins, depth, align_corners;
    float half[1 + kMaxDepth];        // half the grid size of the first stage [0] and of recursion level k [k], halved in double
    int8_t parent[kMaxJoints];        // -1: the root
    int8_t level[kMaxJoints];         // distance from the root
    int8_t limb_of[kMaxJoints];       // joint -> its limb (the root: -1)
    int8_t by_level[kMaxJoints];      // joints sorted by level, ascending joint index inside a level
    int8_t level_begin[kMaxJoints + 1];
    int root, levels;                 // levels: the deepest level
    float *out;
    int32_t *path;                    // nullable
};

// What one frame of the recursion works on: LDS on the device, the stack on the host.
struct Refine {
    float E[kMaxJoints][kMaxRecurCells];      // unary, then energy
    float M[kMaxJoints][kMaxRecurCells];      // message of the joint to its parent, per PARENT bin
    int8_t BP[kMaxJoints][kMaxRecurCells];
    float axis[kMaxJoints][3][kMaxRecurBins + 1];
    float pose[kMaxJoints][3];
    int bin[kMaxJoints];
};

#define ET_RPSM_HD __host__ __device__ inline __attribute__((always_inline))

ET_RPSM_HD void team_sync()
{
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

ET_RPSM_HD float axis_offset(float half, int n, int i)
{
    const float start = -half, end = half;
    const float step = (end - start) / (float)(n - 1);
    return i < n / 2 ? start + step * (float)i : end - step * (float)(n - 1 - i);
}

// F.grid_sample(map, (gx, gy)), bilinear, zero padding.  A location whose four taps all lie outside (NaN and inf included:
// a bin on a camera's principal plane) gives 0 and reads nothing.
ET_RPSM_HD float sample_bilinear(const float *map, int H, int W, float gx, float gy, int align_corners)
{
    const float ix = align_corners ? (gx + 1.f) / 2.f * (float)(W - 1) : ((gx + 1.f) * (float)W - 1.f) / 2.f;
    const float iy = align_corners ? (gy + 1.f) / 2.f * (float)(H - 1) : ((gy + 1.f) * (float)H - 1.f) / 2.f;
    if (!(ix > -1.f && ix < (float)W && iy > -1.f && iy < (float)H)) return 0.f;
    const float x0f = floorf(ix), y0f = floorf(iy);
    const int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
    const float x1f = x0f + 1.f, y1f = y0f + 1.f;
    const float nw = (x1f - ix) * (y1f - iy), ne = (ix - x0f) * (y1f - iy), sw = (x1f - ix) * (iy - y0f), se = (ix - x0f) * (iy - y0f);
    const bool xa = x0 >= 0 && x0 < W, xb = x1 >= 0 && x1 < W, ya = y0 >= 0 && y0 < H, yb = y1 >= 0 && y1 < H;
    float out = 0.f;
    if (xa && ya) out += map[(size_t)y0 * W + x0] * nw;
    if (xb && ya) out += map[(size_t)y0 * W + x1] * ne;
    if (xa && yb) out += map[(size_t)y1 * W + x0] * sw;
    if (xb && yb) out += map[(size_t)y1 * W + x1] * se;
    return out;
}

ET_RPSM_HD float unary(const Problem &pr, int f, int j, float x, float y, float z)
{
    float sum = 0.f;
    for (int v = 0; v < pr.V; ++v) {
        const size_t fv = (size_t)f * pr.V + v;
        const float *c = pr.cams + fv * 12, *t = pr.trans + fv * 6;
        const float px = x * c[0] + y * c[1] + z * c[2] + c[3];
        const float py = x * c[4] + y * c[5] + z * c[6] + c[7];
        const float pz = x * c[8] + y * c[9] + z * c[10] + c[11];
        const float u = px / pz, w = py / pz;
        const float tx = (t[0] * u + t[1] * w + t[2]) * (float)pr.W / pr.image_w;
        const float ty = (t[3] * u + t[4] * w + t[5]) * (float)pr.H / pr.image_h;
        // (the reference divides x by h - 1 and y by w - 1: kept)
        const float gx = tx / (float)(pr.H - 1) * 2.f - 1.f, gy = ty / (float)(pr.W - 1) * 2.f - 1.f;
        const float s = sample_bilinear(pr.heat + (fv * pr.J + j) * ((size_t)pr.H * pr.W), pr.H, pr.W, gx, gy, pr.align_corners);
        sum = v == 0 ? s : sum + s;
    }
    return sum;
}

// max_c compat(a, c) * Ec[c] and its FIRST arg-max, for the parent bin at (xa, ya, za); cx / cy / cz: the child's n positions
// per axis.  An incompatible bin counts as 0, as 0 * E does in the reference.
ET_RPSM_HD void message(float xa, float ya, float za, const float *cx, const float *cy, const float *cz, int n, const float *Ec,
                        float L, float tol, float *best_out, int *arg_out)
{
    float best = -INFINITY;
    int arg = 0, c = 0;
    for (int ix = 0; ix < n; ++ix) {
        const float dx = xa - cx[ix] + kPairEps;
        const float dx2 = dx * dx;
        for (int iy = 0; iy < n; ++iy) {
            const float dy = ya - cy[iy] + kPairEps;
            const float dxy2 = dx2 + dy * dy;
            for (int iz = 0; iz < n; ++iz, ++c) {
                const float dz = za - cz[iz] + kPairEps;
                const float d = sqrtf(dxy2 + dz * dz) + kDistEps;
                const float val = fabsf(d - L) < tol ? Ec[c] : 0.f;
                if (val > best) {
                    best = val;
                    arg = c;
                }
            }
        }
    }
    *best_out = best;
    *arg_out = arg;
}

// first stage: E_j[b] from the frame's U and M planes ((J, B) each)
ET_RPSM_HD float energy(const Problem &pr, const float *U, const float *M, int B, int j, int b)
{
    float e = U[(size_t)j * B + b];
    for (int k = 0; k < pr.J; ++k)
        if (pr.parent[k] == j) e *= M[(size_t)k * B + b];
    return e;
}

ET_RPSM_HD float limb_length(const Problem &pr, int f, int child, bool first)
{
    const float *l = first && pr.first_limb ? pr.first_limb : pr.limb;
    return l[(size_t)f * (pr.J - 1) + pr.limb_of[child]];
}

// Recursion levels 1 .. depth of frame f, from the first stage's pose in s.pose; writes out (and path rows 1 ..).
ET_RPSM_HD void refine_levels(const Problem &pr, int f, Refine &s, int tid, int nt)
{
    const int n = pr.recur_nbins, nb = n * n * n, J = pr.J;
    for (int k = 1; k <= pr.depth; ++k) {
        for (int i = tid; i < J * 3 * n; i += nt) {
            const int j = i / (3 * n), a = i / n % 3, q = i % n;
            s.axis[j][a][q] = axis_offset(pr.half[k], n, q) + s.pose[j][a];
        }
        team_sync();
        for (int i = tid; i < J * nb; i += nt) {
            const int j = i / nb, b = i % nb;
            s.E[j][b] = unary(pr, f, j, s.axis[j][0][b / (n * n)], s.axis[j][1][b / n % n], s.axis[j][2][b % n]);
        }
        team_sync();
        for (int lv = pr.levels; lv >= 1; --lv) {      // deepest first: the children's messages are complete when E needs them
            const int begin = pr.level_begin[lv], count = pr.level_begin[lv + 1] - begin;
            for (int i = tid; i < count * nb; i += nt) {
                const int j = pr.by_level[begin + i / nb], b = i % nb;
                float e = s.E[j][b];
                for (int c = 0; c < J; ++c)
                    if (pr.parent[c] == j) e *= s.M[c][b];
                s.E[j][b] = e;
            }
            team_sync();
            for (int i = tid; i < count * nb; i += nt) {
                const int j = pr.by_level[begin + i / nb], a = i % nb, p = pr.parent[j];
                float best;
                int arg;
                message(s.axis[p][0][a / (n * n)], s.axis[p][1][a / n % n], s.axis[p][2][a % n], s.axis[j][0], s.axis[j][1],
                        s.axis[j][2], n, s.E[j], limb_length(pr, f, j, false), pr.tolerance, &best, &arg);
                s.M[j][a] = best;
                s.BP[j][a] = (int8_t)arg;
            }
            team_sync();
        }
        if (tid == 0) {
            const int r = pr.root;
            float best = -INFINITY;
            int arg = 0;
            for (int b = 0; b < nb; ++b) {
                float e = s.E[r][b];
                for (int c = 0; c < J; ++c)
                    if (pr.parent[c] == r) e *= s.M[c][b];
                if (e > best) {
                    best = e;
                    arg = b;
                }
            }
            for (int i = 0; i < J; ++i) {
                const int j = pr.by_level[i];
                s.bin[j] = j == r ? arg : s.BP[j][s.bin[pr.parent[j]]];
            }
            for (int j = 0; j < J; ++j) {
                const int b = s.bin[j];
                s.pose[j][0] = s.axis[j][0][b / (n * n)];      // (the level's grids are in s.axis: the old pose is not read again)
                s.pose[j][1] = s.axis[j][1][b / n % n];
                s.pose[j][2] = s.axis[j][2][b % n];
                if (pr.path) pr.path[((size_t)f * (1 + pr.depth) + k) * J + j] = b;
            }
        }
        team_sync();
    }
    for (int i = tid; i < J * 3; i += nt) pr.out[(size_t)f * J * 3 + i] = s.pose[i / 3][i % 3];
}

// The first stage's bin -> position, and the pose / path row 0 from the root's bin (one worker; U-less: BP is the frame's plane).
ET_RPSM_HD void first_stage_finish(const Problem &pr, int f, int root_bin, const int32_t *BP, Refine &s)
{
    const int n = pr.first_nbins, B = n * n * n;
    for (int i = 0; i < pr.J; ++i) {
        const int j = pr.by_level[i];
        s.bin[j] = j == pr.root ? root_bin : BP[(size_t)j * B + s.bin[pr.parent[j]]];
    }
    for (int j = 0; j < pr.J; ++j) {
        const int b = s.bin[j];
        s.pose[j][0] = axis_offset(pr.half[0], n, b / (n * n)) + pr.center[(size_t)f * 3 + 0];
        s.pose[j][1] = axis_offset(pr.half[0], n, b / n % n) + pr.center[(size_t)f * 3 + 1];
        s.pose[j][2] = axis_offset(pr.half[0], n, b % n) + pr.center[(size_t)f * 3 + 2];
        if (pr.path) pr.path[(size_t)f * (1 + pr.depth) * pr.J + j] = b;
    }
}

// Host only: one frame, serially.  U, M: (J, B) floats, BP: (J, B) int32 of scratch.
__host__ inline void frame_serial(const Problem &pr, int f, float *U, float *M, int32_t *BP, float *Ec)
{
    const int n = pr.first_nbins, B = n * n * n, J = pr.J;
    float ax[3][kMaxFirstBins];
    for (int a = 0; a < 3; ++a)
        for (int q = 0; q < n; ++q) ax[a][q] = axis_offset(pr.half[0], n, q) + pr.center[(size_t)f * 3 + a];
    for (int j = 0; j < J; ++j)
        for (int b = 0; b < B; ++b) U[(size_t)j * B + b] = unary(pr, f, j, ax[0][b / (n * n)], ax[1][b / n % n], ax[2][b % n]);
    for (int i = J - 1; i >= 0; --i) {                 // by_level backwards: deepest first
        const int j = pr.by_level[i];
        if (j == pr.root) continue;
        for (int b = 0; b < B; ++b) Ec[b] = energy(pr, U, M, B, j, b);
        for (int a = 0; a < B; ++a) {
            int arg;
            message(ax[0][a / (n * n)], ax[1][a / n % n], ax[2][a % n], ax[0], ax[1], ax[2], n, Ec, limb_length(pr, f, j, true),
                    pr.tolerance, &M[(size_t)j * B + a], &arg);
            BP[(size_t)j * B + a] = arg;
        }
    }
    float best = -INFINITY;
    int arg = 0;
    for (int b = 0; b < B; ++b) {
        const float e = energy(pr, U, M, B, pr.root, b);
        if (e > best) {
            best = e;
            arg = b;
        }
    }
    Refine s;
    first_stage_finish(pr, f, arg, BP, s);
    refine_levels(pr, f, s, 0, 1);
}

}  // namespace et_pict
