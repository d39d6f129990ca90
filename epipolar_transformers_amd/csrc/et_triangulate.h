// KEYPOINT.TRIANGULATION epipolar / epipolar_dlt (vision/triangulation.py:234-348) for ONE (frame, joint): the pieces the device
// kernel and the host test hook share (plain C++, float64 throughout, __host__ __device__; included by et_triangulate.hip only).
//
//   select()               the confidence rule: views above float32(conf_thres), else the first arg-max; the branch
//   solve_views()          DLT over a mask of views (+ the source view of a single one): rows x * P[2] - P[0], y * P[2] - P[1]
//                          rotated ONE AT A TIME into a 4 x 4 upper-triangular R (Givens), then smallest_right_vector(R)
//   evaluate_hypothesis()  hypothesis h = the h-th pair (a < b) of views: its two-view point and the selected views whose ray
//                          passes within ransac_thres of it
//   finish_hypothesis()    what the best hypothesis returns: nothing (no inlier), its own point, or the DLT over its inliers
//
// The second half of the file is KEYPOINT.TRIANGULATION pymvg / naive / refine (et_triangulate_views), built from the same pieces,
// and its end the gradient of all five methods in the detections (et_triangulate_bwd: backward_joint() replays the DLT that the
// forward's info word names and differentiates it).
//
// The kernel gives every lane one hypothesis and picks the winner with a wave arg-max; the host hook walks them in a loop.  Both
// take the FIRST hypothesis with the largest count, so they agree.
//
// The SVD never forms A^T A (its condition number, ~1e5 here, would be squared): the rows go into R by Givens rotations, and a
// one-sided Jacobi with a fixed number of sweeps orthogonalises R's four columns.  Every array below has compile-time indices
// after unrolling: nothing is indexed by a run-time value, so nothing goes to scratch memory.
#pragma once
#include <math.h>
#include <stdint.h>

namespace et_tri {

constexpr int kMaxViews = 8;
constexpr int kMaxPairs = kMaxViews * (kMaxViews - 1) / 2;   // 28 hypotheses at most: one wave holds them all
constexpr int kJacobiSweeps = 12;                            // (a 4 x 4 converges in 4-6; the rest rotate by nothing)
constexpr int kInfoNoInlier = 1 << 18;
constexpr int kInfoClamped = 1 << 19;

struct Problem {
    int F, V, J, H, W;
    const float *pts, *conf, *krt, *other_krt, *corr_pos;
    double ds, resize, ransac_thres;
    float conf_thres;   // float32(conf_thres): the reference compares its float32 scores with it IN float32
    int dlt;
    double *out;
    int32_t *info;
};

struct Selection {
    int mask;     // selected views
    int branch;   // 0: two or more selected, 1: exactly one, 2: none (the first arg-max stands in)
    int single;   // the one view of branches 1 and 2
};

struct Hypothesis {
    int count;    // inliers (-1: this index names no pair of selected views)
    int inliers;  // their mask
    int pair;     // the two views of the hypothesis
    double p[3];
};

#define ET_TRI_HD __host__ __device__ inline __attribute__((always_inline))

ET_TRI_HD size_t view_row(const Problem &pr, int f, int v) { return (size_t)f * pr.V + v; }

ET_TRI_HD Selection select(const Problem &pr, int f, int j)
{
    Selection s{0, 0, 0};
    int n = 0, arg = 0;
    float best = 0.f;
    for (int v = 0; v < pr.V; ++v) {
        const float c = pr.conf[view_row(pr, f, v) * pr.J + j];
        if (c > pr.conf_thres) {
            s.mask |= 1 << v;
            s.single = v;
            ++n;
        }
        if (v == 0 || c > best) {
            best = c;
            arg = v;
        }
    }
    if (n == 0) {
        s.mask = 1 << arg;
        s.single = arg;
        s.branch = 2;
    } else if (n == 1) {
        s.branch = 1;
    }
    return s;
}

// R <- the triangular factor of [R; row]
ET_TRI_HD void rotate_row_in(double (&R)[4][4], double (&row)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double a = R[k][k], b = row[k];
        if (b != 0.0) {
            const double h = sqrt(a * a + b * b);
            const double c = a / h, s = b / h;
#pragma unroll
            for (int i = k; i < 4; ++i) {
                const double t = c * R[k][i] + s * row[i];
                row[i] = c * row[i] - s * R[k][i];
                R[k][i] = t;
            }
        }
    }
}

// the two DLT rows of an observation (x, y) under the projection P (12 floats)
ET_TRI_HD void add_view(double (&R)[4][4], const float *P, double x, double y)
{
    double r0[4], r1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r0[i] = x * (double)P[8 + i] - (double)P[i];
        r1[i] = y * (double)P[8 + i] - (double)P[4 + i];
    }
    rotate_row_in(R, r0);
    rotate_row_in(R, r1);
}

// Right singular vector of R's smallest singular value, divided by its fourth component.  One-sided Jacobi: B = R V with V
// orthogonal, columns of B rotated in pairs until they are orthogonal; their norms are then the singular values.
ET_TRI_HD void smallest_right_vector(const double (&R)[4][4], double (&X)[3])
{
    double B[4][4], Vm[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            B[i][k] = k >= i ? R[i][k] : 0.0;
            Vm[i][k] = i == k ? 1.0 : 0.0;
        }
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    alpha += B[i][p] * B[i][p];
                    beta += B[i][q] * B[i][q];
                    gamma += B[i][p] * B[i][q];
                }
                if (fabs(gamma) > 1e-17 * sqrt(alpha * beta)) {
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const double bp = B[i][p], bq = B[i][q];
                        B[i][p] = c * bp - s * bq;
                        B[i][q] = s * bp + c * bq;
                        const double vp = Vm[i][p], vq = Vm[i][q];
                        Vm[i][p] = c * vp - s * vq;
                        Vm[i][q] = s * vp + c * vq;
                    }
                }
            }
    }
    double least = 0.0, x[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double n = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) n += B[i][k] * B[i][k];
        if (k == 0 || n < least) {
            least = n;
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = Vm[i][k];
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) X[i] = x[i] / x[3];
}

// Its sibling for the gradient, by the same route, operation for operation: all four right singular vectors (the columns of
// Vm), the squares n of their singular values, and the index of the column smallest_right_vector() takes (the FIRST smallest).
// The two do not share the sweeps as a routine: with them factored out the forward kernels take a third more registers.
ET_TRI_HD int right_vectors(const double (&R)[4][4], double (&Vm)[4][4], double (&n)[4])
{
    double B[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            B[i][k] = k >= i ? R[i][k] : 0.0;
            Vm[i][k] = i == k ? 1.0 : 0.0;
        }
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    alpha += B[i][p] * B[i][p];
                    beta += B[i][q] * B[i][q];
                    gamma += B[i][p] * B[i][q];
                }
                if (fabs(gamma) > 1e-17 * sqrt(alpha * beta)) {
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const double bp = B[i][p], bq = B[i][q];
                        B[i][p] = c * bp - s * bq;
                        B[i][q] = s * bp + c * bq;
                        const double vp = Vm[i][p], vq = Vm[i][q];
                        Vm[i][p] = c * vp - s * vq;
                        Vm[i][q] = s * vp + c * vq;
                    }
                }
            }
    }
    int least = 0;
    double least_n = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        n[k] = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) n[k] += B[i][k] * B[i][k];
        if (k == 0 || n[k] < least_n) {
            least_n = n[k];
            least = k;
        }
    }
    return least;
}

// image coordinates of joint j in view v
ET_TRI_HD void detection(const Problem &pr, int f, int v, int j, double &x, double &y)
{
    const float *p = pr.pts + (view_row(pr, f, v) * pr.J + j) * 2;
    x = (double)p[0];
    y = (double)p[1];
}

// DLT over the views of `mask` in ascending order
ET_TRI_HD void solve_views(const Problem &pr, int f, int j, int mask, double (&X)[3])
{
    double R[4][4] = {};
    for (int v = 0; v < pr.V; ++v)
        if (mask >> v & 1) {
            double x, y;
            detection(pr, f, v, j, x, y);
            add_view(R, pr.krt + view_row(pr, f, v) * 12, x, y);
        }
    smallest_right_vector(R, X);
}

// The source-view pixel (ox, oy), in image coordinates, that the layer found for the feature-map pixel under the detection
// (x, y) of view v.  Returns kInfoClamped when that pixel lies outside the map (it is then clamped into it), else 0.
ET_TRI_HD int correspondence(const Problem &pr, int f, int v, double x, double y, double &ox, double &oy)
{
    const double qx = (x / pr.resize + 0.5 - pr.ds / 2.0) / pr.ds;
    const double qy = (y / pr.resize + 0.5 - pr.ds / 2.0) / pr.ds;
    int ix, iy, flag = 0;
    // int() truncates toward zero: (-1, 0) is pixel 0.  (The comparisons also send a NaN into the map.)
    if (qx < (double)pr.W && qx > -1.0) ix = (int)qx;
    else {
        ix = qx < (double)pr.W ? 0 : pr.W - 1;
        flag = kInfoClamped;
    }
    if (qy < (double)pr.H && qy > -1.0) iy = (int)qy;
    else {
        iy = qy < (double)pr.H ? 0 : pr.H - 1;
        flag = kInfoClamped;
    }
    const float *c = pr.corr_pos + ((view_row(pr, f, v) * pr.H + iy) * pr.W + ix) * 2;
    ox = ((double)c[0] * pr.ds + pr.ds / 2.0 - 0.5) * pr.resize;
    oy = ((double)c[1] * pr.ds + pr.ds / 2.0 - 0.5) * pr.resize;
    return flag;
}

// Branches 1 and 2: view v with its correspondence in the source view.  Returns correspondence()'s flag.
ET_TRI_HD int solve_single(const Problem &pr, int f, int j, int v, double (&X)[3])
{
    double x, y, ox, oy;
    detection(pr, f, v, j, x, y);
    const int flag = correspondence(pr, f, v, x, y, ox, oy);
    double R[4][4] = {};
    add_view(R, pr.krt + view_row(pr, f, v) * 12, x, y);
    add_view(R, pr.other_krt + view_row(pr, f, v) * 12, ox, oy);
    smallest_right_vector(R, X);
    return flag;
}

// distance of p from the ray of view v through its detection (point2line of triangulation.py:87-95)
ET_TRI_HD double ray_distance(const Problem &pr, int f, int j, int v, const double (&p)[3])
{
    const float *M = pr.krt + view_row(pr, f, v) * 12;
    const double a00 = M[0], a01 = M[1], a02 = M[2], a10 = M[4], a11 = M[5], a12 = M[6], a20 = M[8], a21 = M[9], a22 = M[10];
    const double t[3] = {(double)M[3], (double)M[7], (double)M[11]};
    double inv[3][3] = {{a11 * a22 - a12 * a21, a02 * a21 - a01 * a22, a01 * a12 - a02 * a11},
                        {a12 * a20 - a10 * a22, a00 * a22 - a02 * a20, a02 * a10 - a00 * a12},
                        {a10 * a21 - a11 * a20, a01 * a20 - a00 * a21, a00 * a11 - a01 * a10}};
    const double det = a00 * inv[0][0] + a01 * inv[1][0] + a02 * inv[2][0];
    double x, y;
    detection(pr, f, v, j, x, y);
    double c[3], x1[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) inv[i][k] /= det;
        c[i] = -(inv[i][0] * t[0] + inv[i][1] * t[1] + inv[i][2] * t[2]);
        x1[i] = (inv[i][0] * x + inv[i][1] * y + inv[i][2]) + c[i];
    }
    const double d1[3] = {x1[0] - p[0], x1[1] - p[1], x1[2] - p[2]};
    const double d2[3] = {c[0] - p[0], c[1] - p[1], c[2] - p[2]};
    const double d3[3] = {x1[0] - c[0], x1[1] - c[1], x1[2] - c[2]};
    const double cr[3] = {d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]};
    return sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]) / sqrt(d3[0] * d3[0] + d3[1] * d3[1] + d3[2] * d3[2]);
}

// Hypothesis h: the h-th pair a < b of ALL views in lexicographic order -- restricted to the selected views that is the
// reference's enumeration without its mirrored (b, a) twins, which give the same point.
ET_TRI_HD Hypothesis evaluate_hypothesis(const Problem &pr, int f, int j, int selected, int h)
{
    Hypothesis hy{-1, 0, 0, {0.0, 0.0, 0.0}};
    int a = 0, b = 0, n = 0;
    bool found = false;
    for (int u = 0; u < pr.V; ++u)
        for (int w = u + 1; w < pr.V; ++w)
            if (n++ == h) {
                a = u;
                b = w;
                found = true;
            }
    hy.pair = (1 << a) | (1 << b);
    if (!found || (selected & hy.pair) != hy.pair) return hy;
    solve_views(pr, f, j, hy.pair, hy.p);
    hy.count = 0;
    for (int v = 0; v < pr.V; ++v)
        if ((selected >> v & 1) && ray_distance(pr, f, j, v, hy.p) < pr.ransac_thres) {
            ++hy.count;
            hy.inliers |= 1 << v;
        }
    return hy;
}

// What the best hypothesis returns; the bits 8.. of the info word.
ET_TRI_HD int finish_hypothesis(const Problem &pr, int f, int j, const Hypothesis &best, double (&X)[3])
{
    if (best.count <= 0) {
        X[0] = X[1] = X[2] = 0.0;
        return kInfoNoInlier;
    }
    if (best.count > 2) {
        solve_views(pr, f, j, best.inliers, X);
        return best.inliers << 8;
    }
    X[0] = best.p[0];
    X[1] = best.p[1];
    X[2] = best.p[2];
    return best.pair << 8;
}

ET_TRI_HD void store(const Problem &pr, int f, int j, const double (&X)[3], int info)
{
    double *o = pr.out + ((size_t)f * pr.J + j) * 3;
    o[0] = X[0];
    o[1] = X[1];
    o[2] = X[2];
    if (pr.info) pr.info[(size_t)f * pr.J + j] = info;
}

// The joints that need no hypothesis search: one view and its correspondence, or epipolar_dlt.  Returns false for the others.
ET_TRI_HD bool solve_direct(const Problem &pr, int f, int j, const Selection &s)
{
    double X[3];
    if (s.branch != 0) {
        const int flag = solve_single(pr, f, j, s.single, X);
        store(pr, f, j, X, s.mask | s.mask << 8 | s.branch << 16 | flag);
        return true;
    }
    if (pr.dlt) {
        solve_views(pr, f, j, s.mask, X);
        store(pr, f, j, X, s.mask | s.mask << 8);
        return true;
    }
    return false;
}

// the whole joint, hypotheses one after the other (the host hook)
inline void joint_serial(const Problem &pr, int f, int j)
{
    const Selection s = select(pr, f, j);
    if (solve_direct(pr, f, j, s)) return;
    Hypothesis best{-1, 0, 0, {0.0, 0.0, 0.0}};
    for (int h = 0; h < pr.V * (pr.V - 1) / 2; ++h) {
        const Hypothesis hy = evaluate_hypothesis(pr, f, j, s.mask, h);
        if (hy.count > best.count) best = hy;
    }
    double X[3];
    const int bits = finish_hypothesis(pr, f, j, best, X);
    store(pr, f, j, X, s.mask | bits);
}

// ---- KEYPOINT.TRIANGULATION pymvg / naive / refine (vision/triangulation.py:425-441, 99-154, 162-232) ----------------------------
// The methods that need only detections, scores and projections.  They share solve_views / evaluate_hypothesis with the epipolar
// method above (a Problem without corr_pos) and add the two selection rules and a finish of their own.  The info word has its
// own layout:
//   bits 0-7  : views selected                bits 8-15 : the views the returned point was computed from (none: 0)
//   bit 18    : zeros written (no hypothesis had an inlier, or fewer than two views were selected)
//   bits 24-30: threshold steps taken (pymvg)
constexpr int kMethodPymvg = 0, kMethodNaive = 1, kMethodRefine = 2;
constexpr int kInfoZeros = kInfoNoInlier;
constexpr int kInfoStepsShift = 24;
constexpr double kMaxConfThres = 2.0;    // bounds the lowering loop of pymvg: (2 + 1) / 0.05 + 1 = 61 steps

struct ViewsProblem {
    Problem pr;          // H, W, other_krt, corr_pos, ds, resize, dlt unused
    double conf_thres;   // pymvg lowers it in float64 and compares in float32
    int method;
};

ET_TRI_HD void store_zeros(const Problem &pr, int f, int j, int info)
{
    const double Z[3] = {0.0, 0.0, 0.0};
    store(pr, f, j, Z, info | kInfoZeros);
}

// pymvg: the views with conf > float32(t), t lowered by 0.05 (repeated float64 subtraction: the rounding of the sequence is part
// of the rule) while at most one view is selected and t >= -1; then the DLT over them.  The reference fails or returns a
// rank-deficient vector when the loop ends with fewer than two views (V = 1, NaN scores, scores <= -1): zeros and the flag here.
ET_TRI_HD void pymvg_joint(const ViewsProblem &vp, int f, int j)
{
    const Problem &pr = vp.pr;
    float c[kMaxViews];
#pragma unroll
    for (int v = 0; v < kMaxViews; ++v) c[v] = v < pr.V ? pr.conf[view_row(pr, f, v) * pr.J + j] : -INFINITY;
    double t = vp.conf_thres;
    int mask, n, steps = 0;
    for (;;) {
        const float tf = (float)t;
        mask = 0;
        n = 0;
#pragma unroll
        for (int v = 0; v < kMaxViews; ++v)
            if (c[v] > tf) {
                mask |= 1 << v;
                ++n;
            }
        if (t < -1.0 || n > 1) break;
        t -= 0.05;
        ++steps;
    }
    const int word = mask | steps << kInfoStepsShift;
    if (n < 2) {
        store_zeros(pr, f, j, word);
        return;
    }
    double X[3];
    solve_views(pr, f, j, mask, X);
    store(pr, f, j, X, word | mask << 8);
}

// naive / refine: the views above float32(conf_thres), no lowering
ET_TRI_HD int select_above(const Problem &pr, int f, int j, int &n)
{
    int mask = 0;
    n = 0;
    for (int v = 0; v < pr.V; ++v)
        if (pr.conf[view_row(pr, f, v) * pr.J + j] > pr.conf_thres) {
            mask |= 1 << v;
            ++n;
        }
    return mask;
}

// What the best hypothesis returns.  naive: its own point.  refine: the DLT over its inliers when it has MORE THAN ONE
// (triangulation.py:226; the epipolar method's finish_hypothesis asks for more than two).
ET_TRI_HD void finish_views(const ViewsProblem &vp, int f, int j, int selected, const Hypothesis &best)
{
    const Problem &pr = vp.pr;
    if (best.count <= 0) {
        store_zeros(pr, f, j, selected);
        return;
    }
    if (vp.method == kMethodRefine && best.count > 1) {
        double X[3];
        solve_views(pr, f, j, best.inliers, X);
        store(pr, f, j, X, selected | best.inliers << 8);
        return;
    }
    store(pr, f, j, best.p, selected | best.pair << 8);
}

// the whole joint of any of the three methods, hypotheses one after the other (the host hook)
inline void views_joint_serial(const ViewsProblem &vp, int f, int j)
{
    const Problem &pr = vp.pr;
    if (vp.method == kMethodPymvg) {
        pymvg_joint(vp, f, j);
        return;
    }
    int n;
    const int selected = select_above(pr, f, j, n);
    if (n < 2) {
        store_zeros(pr, f, j, selected);
        return;
    }
    Hypothesis best{-1, 0, 0, {0.0, 0.0, 0.0}};
    for (int h = 0; h < pr.V * (pr.V - 1) / 2; ++h) {
        const Hypothesis hy = evaluate_hypothesis(pr, f, j, selected, h);
        if (hy.count > best.count) best = hy;
    }
    finish_views(vp, f, j, selected, best);
}

// ---- the gradient of every lifting above in its detections (et_triangulate_bwd) ----------------------------------------------------
// The info word of the forward names the rows A of the DLT that produced the point: the views of bits 8-15, or -- bits 16-17 set,
// the epipolar method's single-view branches -- that one view and its correspondence in the source view.  With A fixed at that
// decision, v the unit right singular vector of the smallest singular value s4 and X = v[:3] / v[3]:
//   gv = (gX / v3, -(gX . v[:3]) / v3^2)
//   w  = - sum over the other three right vectors v_k of v_k (v_k . gv) / (s_k^2 - s4^2)      (pinv(A^T A - s4^2 I) applied to gv)
//   gA = (A w) v^T + (A v) w^T ;  the detection (x, y) of a used view receives gA[row_x] . P[2] and gA[row_y] . P[2]
// R is rebuilt by the forward's own routines in the forward's order, so v IS the forward's vector.  A vanishing gap s3^2 - s4^2
// is not guarded: the result is then what float64 autograd through an SVD gives as well (inf or NaN).
struct BackwardProblem {
    Problem pr;                // conf, ransac_thres, conf_thres, dlt, out, info unused; other_krt and corr_pos both given or both NULL
    const int32_t *word;       // (F, J) the forward's info
    const double *grad_out;    // (F, J, 3)
    float *grad_pts;           // (F, V, J, 2), every element written
};

// Writes all 2 V values of the joint: rounded once to float32, exactly 0 for a view that was not used.
ET_TRI_HD void backward_joint(const BackwardProblem &bp, int f, int j)
{
    const Problem &pr = bp.pr;
    const int word = bp.word[(size_t)f * pr.J + j];
    const int branch = word >> 16 & 3;
    int used = word >> 8 & 0xff & ((1 << pr.V) - 1);
    double R[4][4] = {};
    bool solved = false;
    if (branch != 0) {
        // (branch bits without the two arrays -- a word of the epipolar method handed to the backward of the views -- are not followed)
        if (used != 0 && pr.other_krt && pr.corr_pos) {
            int v = 0;
            while (!(used >> v & 1)) ++v;
            used = 1 << v;
            double x, y, ox, oy;
            detection(pr, f, v, j, x, y);
            correspondence(pr, f, v, x, y, ox, oy);
            add_view(R, pr.krt + view_row(pr, f, v) * 12, x, y);
            add_view(R, pr.other_krt + view_row(pr, f, v) * 12, ox, oy);
            solved = true;
        }
    } else if ((used & (used - 1)) != 0) {             // two views or more
        for (int v = 0; v < pr.V; ++v)
            if (used >> v & 1) {
                double x, y;
                detection(pr, f, v, j, x, y);
                add_view(R, pr.krt + view_row(pr, f, v) * 12, x, y);
            }
        solved = true;
    }
    double vec[4] = {0.0, 0.0, 0.0, 0.0}, w[4] = {0.0, 0.0, 0.0, 0.0};
    if (solved) {
        double Vm[4][4], n[4];
        const int least = right_vectors(R, Vm, n);
        double n4 = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k == least) {
                n4 = n[k];
#pragma unroll
                for (int i = 0; i < 4; ++i) vec[i] = Vm[i][k];
            }
        const double *g = bp.grad_out + ((size_t)f * pr.J + j) * 3;
        const double gv[4] = {g[0] / vec[3], g[1] / vec[3], g[2] / vec[3],
                              -(g[0] * vec[0] + g[1] * vec[1] + g[2] * vec[2]) / (vec[3] * vec[3])};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k != least) {
                double d = 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i) d += Vm[i][k] * gv[i];
                const double c = d / (n[k] - n4);
#pragma unroll
                for (int i = 0; i < 4; ++i) w[i] -= Vm[i][k] * c;
            }
    }
    for (int v = 0; v < pr.V; ++v) {
        float gx = 0.f, gy = 0.f;
        if (solved && (used >> v & 1)) {
            const float *P = pr.krt + view_row(pr, f, v) * 12;
            double x, y;
            detection(pr, f, v, j, x, y);
            double aw0 = 0.0, av0 = 0.0, aw1 = 0.0, av1 = 0.0, pw = 0.0, pv = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double p2 = (double)P[8 + i];
                const double r0 = x * p2 - (double)P[i], r1 = y * p2 - (double)P[4 + i];
                aw0 += r0 * w[i];
                av0 += r0 * vec[i];
                aw1 += r1 * w[i];
                av1 += r1 * vec[i];
                pw += p2 * w[i];
                pv += p2 * vec[i];
            }
            gx = (float)(aw0 * pv + av0 * pw);
            gy = (float)(aw1 * pv + av1 * pw);
        }
        float *o = bp.grad_pts + (view_row(pr, f, v) * pr.J + j) * 2;
        o[0] = gx;
        o[1] = gy;
    }
}

#undef ET_TRI_HD

}  // namespace et_tri
