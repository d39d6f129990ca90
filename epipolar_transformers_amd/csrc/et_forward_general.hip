// libepipolar_amd.so: the operator's parameterised / pooled / prior branches as ONE kernel (et_epipolar_forward_general).
// ----------------------------------------------------------------------------
// SURVEY.md row N4.  The reference applies its optional 1x1 convolutions to the MAPS before sampling
// (epipolar.py:138-153: other1 = phi(feat2), feat1 = theta(feat1), other2 = g(feat2)), so these branches are the
// headline operator with three differences:
//   * the query rows, the similarity map and the value map are three tensors (C/BOTTLENECK and C/BOTTLENECK channels);
//   * POOLING (epipolar.py:200-202, 211-213): `view(2, K/2, C, H, W).max(0)` -- the per-channel maximum of samples k and
//     k + K/2, on both sampled maps, before the dot product: K/2 similarities / attention weights per pixel;
//   * PRIOR (epipolar.py:300-301, 308-309): a learned (K', H, W) map per camera pair added to the masked similarity, or
//     multiplied onto the soft-max output (PRIORMUL).
// The reference (and the torch restatement Epipolar._attend_general_chunk) materialises the sampled K x C x H x W tensor
// per pair; here one wave owns one reference pixel and nothing but the outputs is written:
//   lanes <-> samples : epipolar segment, the K samples' four taps and bilinear weights -> LDS (36 bytes per sample)
//   lanes <-> channels: sim[k'] = sum_c q[c] * pooled sample of the similarity map   (wave reduction per sample)
//   lanes <-> samples : `== 0 -> -1e10` mask, prior, soft-max (or / K'), first arg-max -> attn, corr_pos
//   lanes <-> channels: out[c] = sum_k' attn[k'] * pooled sample of the value map
// HBM/L2-bound gather like the per-pixel headline kernel (algorithmic bytes per pixel: K x 4 taps x (Cs + Cv) x 4 B);
// not tuned further -- these modes are not on BASELINE.json's metric.  et_epipolar_backward_general (below) is its
// backward, for every branch (round 5: cosine similarity, ATTENTION max, additive / multiplicative prior incl. the prior
// tables' own gradient, SIMILARITY prior).
#include "et_common.h"

namespace {
#include "et_wave_reduce.h"

struct GeneralParams {
    EtLayerDesc d;          // geometry, K, soft-max switches (d.C is not used)
    const float *xs, *ys, *steps, *cam;
    const float *q;         // (N, H*W, cs)   query rows: feat1 or theta(feat1), channels last
    const float *m_sim;     // (N, H*W, cs)   similarity map: feat2 or phi(feat2)
    const float *m_val;     // (N, H*W, cv)   value map: feat2 or g(feat2)
    const float *prior;     // (N, K', H*W) or NULL
    float *out;             // (N, H*W, cv)
    float *attn;            // (N, K', H*W) or NULL
    float *corr;            // (N, H*W, 2) or NULL
    int cs, cv, prior_mul;
    int cosine;             // similarity = cosine of q and the (pooled) sample (F.cosine_similarity, eps 1e-8) instead of the dot product
    int attn_max;           // ATTENTION max: raw cosine similarity, no mask / soft-max; out = the arg-max sample's values
    int sim_prior;          // SIMILARITY prior (epipolar.py:288-289): the prior table IS the attention -- no similarity, mask or soft-max
};

constexpr int kGenWaves = 4;        // waves (= reference pixels) per block
constexpr int kGenMaxQ = 8;         // query channels a lane keeps in registers: cs <= 512
constexpr int gen_wave_floats(int K) { return (K * 9 + 3) & ~3; }   // 36 bytes per sample, 16-byte aligned per wave
constexpr int gen_bwd_wave_floats(int K) { return (K * 11 + 3) & ~3; }   // + a second and a third [K'] array
constexpr size_t gen_lds_bytes(int K) { return (size_t)kGenWaves * gen_wave_floats(K) * sizeof(float); }

// one channel of one bilinear sample: tap[r] < 0 <=> outside the image (weight 0, zero padding)
__device__ __forceinline__ float gen_sample(const float *map, int ch, int c, const int4 t, const float4 w)
{
    float v = 0.f;
    if (t.x >= 0) v = fmaf(map[(size_t)t.x * ch + c], w.x, v);
    if (t.y >= 0) v = fmaf(map[(size_t)t.y * ch + c], w.y, v);
    if (t.z >= 0) v = fmaf(map[(size_t)t.z * ch + c], w.z, v);
    if (t.w >= 0) v = fmaf(map[(size_t)t.w * ch + c], w.w, v);
    return v;
}

// ---- the phases the forward and the backward kernel share ------------------------------------------------------------
// Where a wave stands: its reference pixel, the pixel's epipolar segment, and the wave's arrays in LDS.
struct GenPixel {
    int n, pix;
    et::Segment seg;
    float4 *s_w;            // [K] bilinear weights
    int4 *s_tap;            // [K] taps
    float *s_sim;           // [K'] arrays from here on: one in the forward, three in the backward
};

// Wave -> (n, pix, h, w); lanes <-> samples: the epipolar segment, then every sample's taps and weights into LDS, fenced.
// False for the waves behind the last pixel (wave-uniform: the kernels have no block-wide barrier).
__device__ __forceinline__ bool gen_pixel(const GeneralParams &p, float *s_dyn, int wave_floats, int lane, GenPixel &px)
{
    const EtLayerDesc &d = p.d;
    const int W = d.W, K = d.K, HW = d.H * W;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long gp = (long long)blockIdx.x * kGenWaves + wave;
    px.n = (int)(gp / HW);
    if (px.n >= d.N) return false;
    px.pix = (int)(gp - (long long)px.n * HW);
    const int h = px.pix / W, w = px.pix - h * W;
    px.s_w = reinterpret_cast<float4 *>(s_dyn + (size_t)wave * wave_floats);
    px.s_tap = reinterpret_cast<int4 *>(px.s_w + K);
    px.s_sim = reinterpret_cast<float *>(px.s_tap + K);
    px.seg = et::epipolar_segment(d, p.cam + (size_t)px.n * ET_CAM_STRIDE, p.xs[w], p.ys[h]);
    for (int k = lane; k < K; k += kWave) {
        const et::SampleSetup su = et::sample_setup(d, px.seg, p.steps[k]);
        px.s_w[k] = make_float4(su.weight[0], su.weight[1], su.weight[2], su.weight[3]);
        px.s_tap[k] = make_int4(su.tap[0], su.tap[1], su.tap[2], su.tap[3]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return true;
}

// lanes <-> channels: the pixel's query row into registers; returns |q|^2 under the cosine similarity (else 0)
__device__ __forceinline__ float gen_query(const GeneralParams &p, const float *qrow, int lane, float (&qv)[kGenMaxQ])
{
#pragma unroll
    for (int i = 0; i < kGenMaxQ; ++i) qv[i] = (lane + i * kWave < p.cs) ? qrow[lane + i * kWave] : 0.f;
    float qq = 0.f;
    if (p.cosine) {
#pragma unroll
        for (int i = 0; i < kGenMaxQ; ++i) qq = fmaf(qv[i], qv[i], qq);
        qq = wave_all_sum(qq);
    }
    return qq;
}

// taps and weights of similarity k': sample k, and under POOLING its partner k + K' (else sample k again)
template <bool POOL>
__device__ __forceinline__ void gen_taps(const int4 *s_tap, const float4 *s_w, int k, int Ks, int4 &t0, float4 &w0,
                                         int4 &t1, float4 &w1)
{
    t0 = s_tap[k];
    w0 = s_w[k];
    t1 = t0;
    w1 = w0;
    if (POOL) {
        t1 = s_tap[k + Ks];
        w1 = s_w[k + Ks];
    }
}

// one channel of the pooled sample: the maximum of the two samples (epipolar.py:200-202, 211-213), and which sample won it --
// torch.max's rule: a NaN is above every value (fmaxf would return the other operand and lose it), else the second only when
// strictly larger (the first on a tie, and of two NaNs)
template <bool POOL>
__device__ __forceinline__ float gen_pooled_argwin(const float *map, int ch, int c, const int4 t0, const float4 w0,
                                                   const int4 t1, const float4 w1, bool &second)
{
    const float v0 = gen_sample(map, ch, c, t0, w0);
    second = false;
    float v = v0;
    if (POOL) {
        const float v1 = gen_sample(map, ch, c, t1, w1);
        second = (v1 > v0) | ((v1 != v1) & (v0 == v0));
        v = second ? v1 : v0;
    }
    return v;
}

// the value alone
template <bool POOL>
__device__ __forceinline__ float gen_pooled(const float *map, int ch, int c, const int4 t0, const float4 w0, const int4 t1,
                                            const float4 w1)
{
    bool second;
    return gen_pooled_argwin<POOL>(map, ch, c, t0, w0, t1, w1, second);
}

// lanes <-> channels: dot = q . P_k' over the wave, and vv = |P_k'|^2 (summed over the wave under the cosine similarity only)
template <bool POOL>
__device__ __forceinline__ void gen_similarity(const GeneralParams &p, const float *m1, int lane, const float (&qv)[kGenMaxQ],
                                               const int4 t0, const float4 w0, const int4 t1, const float4 w1, float &dot,
                                               float &vv)
{
    dot = 0.f;
    vv = 0.f;
#pragma unroll
    for (int i = 0; i < kGenMaxQ; ++i) {
        const int c = lane + i * kWave;
        if (c < p.cs) {
            const float v = gen_pooled<POOL>(m1, p.cs, c, t0, w0, t1, w1);
            dot = fmaf(qv[i], v, dot);
            vv = fmaf(v, v, vv);
        }
    }
    dot = wave_all_sum(dot);
    if (p.cosine) vv = wave_all_sum(vv);
}

// lanes <-> samples: kGenKPL slots of 64 hold the K' <= K values of a pixel, and validate() admits K <= 256
constexpr int kGenKPL = 4;
static_assert(kGenKPL * kWave == 256, "the lanes <-> samples phases must hold validate()'s largest K");

// first maximum over k' (torch.argmax) of a[s] = value of k' = s * 64 + lane: a NaN above every value, then the largest value,
// then the lowest index (argmax_key); always one of 0 .. K'-1
__device__ __forceinline__ int gen_first_argmax(const float (&a)[kGenKPL], int Ks, int lane)
{
    unsigned bestk = 0u;
    int besti = 0x7fffffff;
#pragma unroll
    for (int s = 0; s < kGenKPL; ++s) {
        const int k = s * kWave + lane;
        const unsigned key = argmax_key(a[s]);
        if (k < Ks && key > bestk) {
            bestk = key;
            besti = k;
        }
    }
    return wave_first_argmax(bestk, besti);
}

template <bool POOL>
__global__ __launch_bounds__(kWave *kGenWaves) void epipolar_fwd_general_kernel(const GeneralParams p)
{
    extern __shared__ float s_dyn[];
    const EtLayerDesc &d = p.d;
    const int H = d.H, W = d.W, K = d.K, HW = H * W;
    const int Ks = POOL ? K / 2 : K;          // similarities per pixel
    const int lane = threadIdx.x & (kWave - 1);
    const float neg_inf = -__builtin_huge_valf();

    // ---- lanes <-> samples: the epipolar segment and every sample's taps ------------------------------------------
    GenPixel px;
    if (!gen_pixel(p, s_dyn, gen_wave_floats(K), lane, px)) return;
    const int n = px.n, pix = px.pix;
    const float4 *s_w = px.s_w;
    const int4 *s_tap = px.s_tap;
    float *s_sim = px.s_sim;                  // [K'] similarity, then attention

    // ---- lanes <-> channels: similarities (epipolar.py:294-295 on the pooled samples) -----------------------------
    if (!p.sim_prior) {
        const float *qrow = p.q + ((size_t)n * HW + pix) * p.cs;
        const float *m1 = p.m_sim + (size_t)n * HW * p.cs;
        float qv[kGenMaxQ];
        const float qq = gen_query(p, qrow, lane, qv);
        for (int k = 0; k < Ks; ++k) {
            int4 t0, t1;
            float4 w0, w1;
            gen_taps<POOL>(s_tap, s_w, k, Ks, t0, w0, t1, w1);
            float dot, vv;
            gen_similarity<POOL>(p, m1, lane, qv, t0, w0, t1, w1, dot, vv);
            // epipolar.py:282-286 / :290-293: x1 . x2 / (max(|x1|, eps) max(|x2|, eps)), eps = 1e-8
            if (p.cosine) dot = dot / (fmaxf(sqrtf(qq), 1e-8f) * fmaxf(sqrtf(vv), 1e-8f));
            if (lane == 0) s_sim[k] = dot;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // ---- lanes <-> samples: mask, prior, soft-max, arg-max (epipolar.py:298-311, :237-241) -------------------------
    {
        constexpr int KPL = kGenKPL;
        float l[KPL], a[KPL], pr[KPL];
        float vmax = neg_inf;
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            const int k = s * kWave + lane;
            const bool in = k < Ks;
            float v = (in && !p.sim_prior) ? s_sim[k] : 0.f;
            pr[s] = (in && p.prior) ? p.prior[((size_t)n * Ks + k) * HW + pix] : 0.f;
            if (p.sim_prior) {
                v = pr[s];                                                        // :288-289: returned as is
            } else if (!p.attn_max) {                                             // (ATTENTION max: the raw cosine, :282-286)
                v = (v == 0.f) ? -1e10f : v;                                      // epipolar.py:298
                if (p.prior && !p.prior_mul) v += pr[s];                          // :300-301
                v = d.softmax_enabled ? v * d.softmax_scale : v / (float)Ks;      // :306 / :311
            }
            l[s] = v;
            if (in) vmax = fmaxf(vmax, v);      // (the soft-max's maximum: a NaN it drops comes back as expf(NaN - vmax))
        }
        if (d.softmax_enabled && !p.attn_max && !p.sim_prior) {
            vmax = wave_all_max(vmax);
            float sum = 0.f;
#pragma unroll
            for (int s = 0; s < KPL; ++s) {
                a[s] = (s * kWave + lane < Ks) ? expf(l[s] - vmax) : 0.f;
                sum += a[s];
            }
            sum = wave_all_sum(sum);
#pragma unroll
            for (int s = 0; s < KPL; ++s) {
                a[s] = a[s] / sum;
                if (p.prior && p.prior_mul) a[s] *= pr[s];                        // :308-309
            }
        } else {
#pragma unroll
            for (int s = 0; s < KPL; ++s) a[s] = (s * kWave + lane < Ks) ? l[s] : 0.f;
        }
        const int besti = gen_first_argmax(a, Ks, lane);
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            const int k = s * kWave + lane;
            if (k < Ks) {
                // ATTENTION max gathers the arg-max sample (epipolar.py:232-235): a one-hot weight for the sum below
                s_sim[k] = p.attn_max ? (k == besti ? 1.f : 0.f) : a[s];
                if (p.attn) p.attn[((size_t)n * Ks + k) * HW + pix] = a[s];
            }
        }
        if (p.corr && lane == 0 && besti < Ks) {
            // the location of sample `besti` of the UNPOOLED list: sample_locs[idx], idx < K' (epipolar.py:239)
            const et::SampleSetup su = et::sample_setup(d, px.seg, p.steps[besti]);
            float *o = p.corr + ((size_t)n * HW + pix) * 2;
            o[0] = et::de_normalize(d, su.nx, W);
            o[1] = et::de_normalize(d, su.ny, H);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // ---- lanes <-> channels: the weighted sum of the pooled value samples (epipolar.py:243) ------------------------
    {
        const float *m2 = p.m_val + (size_t)n * HW * p.cv;
        float *orow = p.out + ((size_t)n * HW + pix) * p.cv;
        for (int c0 = 0; c0 < p.cv; c0 += 4 * kWave) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < Ks; ++k) {
                const float ak = s_sim[k];
                if (p.attn_max && ak == 0.f) continue;      // wave-uniform (the one-hot weights of ATTENTION max)
                int4 t0, t1;
                float4 w0, w1;
                gen_taps<POOL>(s_tap, s_w, k, Ks, t0, w0, t1, w1);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = c0 + lane + i * kWave;
                    if (c < p.cv) acc[i] = fmaf(ak, gen_pooled<POOL>(m2, p.cv, c, t0, w0, t1, w1), acc[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = c0 + lane + i * kWave;
                if (c < p.cv) orow[c] = acc[i];
            }
        }
    }
}

// ---- backward of the same branches: d q, d map_sim, d map_val, d prior from d out -----------------------------------
// One wave per reference pixel again.  With P_k' / V_k' the pooled samples of the similarity / value map, g = d out:
//     s_k'  = q . P_k'            (dot)      or   q . P_k' / (max(|q|, eps) max(|P_k'|, eps))     (cosine, eps = 1e-8)
//     v_k'  = mask(s_k') [+ prior_k']                          (`== 0 -> -1e10`, epipolar.py:298, 300-301)
//     sm    = soft-max(scale v)   a = sm [* prior]             (:303-309)        or   a = v / K'   (:310-311)
//     out   = sum_k' a_k' V_k'                                 (:243)
//  =>  d a_k' = g . V_k'      d sm = d a [* prior]      d v = scale sm (d sm - sum_j sm_j d sm_j)     (or d a / K')
//      d prior_k' = d v_k' (added) | sm_k' d a_k' (multiplied)          d s_k' = d v_k', 0 under the mask
//      dot:     d q = sum d s_k' P_k'                       d P_k' = d s_k' q
//      cosine:  d q = sum alpha_k' P_k' - (sum gamma_k') q  d P_k' = alpha_k' q - beta_k' P_k'
//               alpha = d s / (|q| |P|),  beta = d s s / |P|^2,  gamma = d s s / |q|^2  (torch's cosine_similarity divides by the
//               clamped norms but differentiates the unclamped ones; a norm below eps only occurs at s = 0: masked)
//      d V_k' = a_k' g
//  ATTENTION max (:222-235, 282-286): out = V of the first arg-max of the raw cosine -- a one-hot a, no gradient through the
//  similarity.  SIMILARITY prior (:288-289): a = the prior table itself: d prior_k' = d a_k', nothing through q / P.
//  A gradient through the returned attention, ga = d loss / d attn (nullable), joins d a: every line above holds with
//  d a_k' = g . V_k' + ga_k'.  ATTENTION max returns the raw cosine as its attention: d s_k' = ga_k' (no mask), through the cosine
//  derivative above; with SIMILARITY prior beside it the returned weights are the table: d prior_k' = ga_k'.
//  d P / d V go through the per-channel maximum to the sample that won (the first on a tie, as torch.max), times the four
//  bilinear weights onto the taps of the maps: float atomics (the sums over pixels arrive in any order: reproducible to
//  rounding only, like the tile backward).  The similarities are recomputed (nothing but the inputs is saved by the forward).
struct GeneralBwdParams {
    GeneralParams f;        // inputs as in the forward (out / attn / corr unused)
    const float *gout;      // (N, H*W, cv)
    const float *gattn;     // (N, K', H*W)  nullable: d loss / d attn, joins d a_k' = g . V_k'
    float *gq;              // (N, H*W, cs)  written
    float *gsim;            // (N, H*W, cs)  nullable, accumulated with atomics: zero it first
    float *gval;            // (N, H*W, cv)  nullable, accumulated with atomics: zero it first
    float *gprior;          // (N, K', H*W)  nullable, written (one wave owns a pixel's K' entries)
};

__device__ __forceinline__ void gen_scatter(float *gmap, int ch, int c, const int4 t, const float4 w, float g)
{
    if (t.x >= 0) unsafeAtomicAdd(gmap + (size_t)t.x * ch + c, g * w.x);
    if (t.y >= 0) unsafeAtomicAdd(gmap + (size_t)t.y * ch + c, g * w.y);
    if (t.z >= 0) unsafeAtomicAdd(gmap + (size_t)t.z * ch + c, g * w.z);
    if (t.w >= 0) unsafeAtomicAdd(gmap + (size_t)t.w * ch + c, g * w.w);
}

template <bool POOL>
__global__ __launch_bounds__(kWave *kGenWaves) void epipolar_bwd_general_kernel(const GeneralBwdParams bp)
{
    extern __shared__ float s_dyn[];
    const GeneralParams &p = bp.f;
    const EtLayerDesc &d = p.d;
    const int H = d.H, W = d.W, K = d.K, HW = H * W;
    const int Ks = POOL ? K / 2 : K;
    const int lane = threadIdx.x & (kWave - 1);
    const float neg_inf = -__builtin_huge_valf();
    const float kEps = 1e-8f;

    GenPixel px;
    if (!gen_pixel(p, s_dyn, gen_bwd_wave_floats(K), lane, px)) return;
    const int n = px.n, pix = px.pix;
    const float4 *s_w = px.s_w;
    const int4 *s_tap = px.s_tap;
    float *s_sim = px.s_sim;                                // [K'] q . P, then alpha
    float *s_a = s_sim + K;                                 // [K'] d a, then a
    float *s_b = s_a + K;                                   // [K'] |P|^2 (cosine), then beta

    const float *qrow = p.q + ((size_t)n * HW + pix) * p.cs;
    const float *grow = bp.gout + ((size_t)n * HW + pix) * p.cv;
    const float *m1 = p.m_sim + (size_t)n * HW * p.cs;
    const float *m2 = p.m_val + (size_t)n * HW * p.cv;
    float qv[kGenMaxQ];
    const float qq = gen_query(p, qrow, lane, qv);

    // ---- lanes <-> channels: q . P_k' (and |P_k'|^2)  and  d a_k' = g . V_k' ------------------------------------------
    for (int k = 0; k < Ks; ++k) {
        int4 t0, t1;
        float4 w0, w1;
        gen_taps<POOL>(s_tap, s_w, k, Ks, t0, w0, t1, w1);
        float dot = 0.f, vv = 0.f, da = 0.f;
        if (!p.sim_prior) gen_similarity<POOL>(p, m1, lane, qv, t0, w0, t1, w1, dot, vv);
        if (!p.attn_max) {
            for (int c = lane; c < p.cv; c += kWave) da = fmaf(grow[c], gen_pooled<POOL>(m2, p.cv, c, t0, w0, t1, w1), da);
            da = wave_all_sum(da);
        }
        if (lane == 0) {
            s_sim[k] = dot;
            s_a[k] = da;
            s_b[k] = vv;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // ---- lanes <-> samples: a (recomputed), d prior, and the coefficients alpha / beta / gamma of the maps' gradients ----
    float gamma = 0.f;
    {
        constexpr int KPL = kGenKPL;
        const float nq = fmaxf(sqrtf(qq), kEps);
        float sim[KPL], da[KPL], pr[KPL], np_[KPL], aout[KPL], alpha[KPL], beta[KPL], dprior[KPL];
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            const int k = s * kWave + lane;
            const bool in = k < Ks;
            const float raw = in ? s_sim[k] : 0.f;
            np_[s] = p.cosine ? fmaxf(sqrtf(in ? s_b[k] : 1.f), kEps) : 1.f;
            sim[s] = p.cosine ? raw / (nq * np_[s]) : raw;           // (the forward's expression)
            da[s] = in ? s_a[k] : 0.f;
            if (bp.gattn && in) da[s] += bp.gattn[((size_t)n * Ks + k) * HW + pix];     // (block-uniform pointer test)
            pr[s] = (in && p.prior) ? p.prior[((size_t)n * Ks + k) * HW + pix] : 0.f;
            if (p.sim_prior) sim[s] = pr[s];
            aout[s] = alpha[s] = beta[s] = dprior[s] = 0.f;
        }
        // d s_k' -> the coefficients of the maps' gradients (dot: alpha; cosine: alpha, beta, gamma)
        auto through_similarity = [&](int s, float ds) {
            if (p.cosine) {
                alpha[s] = ds / (nq * np_[s]);
                beta[s] = (np_[s] > kEps) ? ds * sim[s] / (np_[s] * np_[s]) : 0.f;
                gamma += (nq > kEps) ? ds * sim[s] / (nq * nq) : 0.f;
            } else {
                alpha[s] = ds;
            }
        };
        if (p.attn_max) {
            // first maximum over k' (torch.argmax): a one-hot weight, nothing flows from `out` through the similarity
            const int besti = gen_first_argmax(sim, Ks, lane);
#pragma unroll
            for (int s = 0; s < KPL; ++s) aout[s] = (s * kWave + lane == besti) ? 1.f : 0.f;
            if (bp.gattn) {
                // ... but the returned attention is the raw cosine (or the given weights) itself: d s_k' = ga_k' (da holds it:
                // no g . V_k' in this mode), no mask
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    if (p.sim_prior) dprior[s] = da[s];
                    else through_similarity(s, (s * kWave + lane < Ks) ? da[s] : 0.f);
                }
            }
        } else if (p.sim_prior) {
#pragma unroll
            for (int s = 0; s < KPL; ++s) {
                aout[s] = pr[s];
                dprior[s] = da[s];
            }
        } else {
            bool masked[KPL];
            float v[KPL], dv[KPL];
            const bool padd = p.prior && !p.prior_mul, pmul = p.prior && p.prior_mul;
#pragma unroll
            for (int s = 0; s < KPL; ++s) {
                masked[s] = (sim[s] == 0.f);
                v[s] = masked[s] ? -1e10f : sim[s];
                if (padd) v[s] += pr[s];
            }
            if (d.softmax_enabled) {
                float l[KPL], sm[KPL], dsm[KPL];
                float vmax = neg_inf;
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    l[s] = v[s] * d.softmax_scale;
                    if (s * kWave + lane < Ks) vmax = fmaxf(vmax, l[s]);
                }
                vmax = wave_all_max(vmax);
                float sum = 0.f;
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    sm[s] = (s * kWave + lane < Ks) ? expf(l[s] - vmax) : 0.f;
                    sum += sm[s];
                }
                sum = wave_all_sum(sum);
                float ada = 0.f;
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    sm[s] = sm[s] / sum;
                    dsm[s] = pmul ? pr[s] * da[s] : da[s];
                    ada = fmaf(sm[s], dsm[s], ada);
                }
                ada = wave_all_sum(ada);
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    dv[s] = d.softmax_scale * sm[s] * (dsm[s] - ada);
                    aout[s] = pmul ? sm[s] * pr[s] : sm[s];
                    dprior[s] = pmul ? sm[s] * da[s] : (padd ? dv[s] : 0.f);
                }
            } else {
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    const bool in = s * kWave + lane < Ks;
                    aout[s] = in ? v[s] / (float)Ks : 0.f;
                    dv[s] = da[s] / (float)Ks;
                    dprior[s] = padd ? dv[s] : 0.f;                       // (PRIORMUL only acts behind the soft-max, :308-309)
                }
            }
#pragma unroll
            for (int s = 0; s < KPL; ++s) {
                through_similarity(s, (masked[s] || s * kWave + lane >= Ks) ? 0.f : dv[s]);
            }
        }
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            const int k = s * kWave + lane;
            if (k < Ks) {
                s_sim[k] = alpha[s];
                s_b[k] = beta[s];
                s_a[k] = aout[s];
                if (bp.gprior) bp.gprior[((size_t)n * Ks + k) * HW + pix] = dprior[s];
            }
        }
        gamma = wave_all_sum(gamma);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // ---- lanes <-> channels: d q, and the scatter of d P / d V through the maximum onto the maps ------------------------
    {
        float dq[kGenMaxQ];
#pragma unroll
        for (int i = 0; i < kGenMaxQ; ++i) dq[i] = 0.f;
        float *g1 = bp.gsim ? bp.gsim + (size_t)n * HW * p.cs : nullptr;
        float *g2 = bp.gval ? bp.gval + (size_t)n * HW * p.cv : nullptr;
        for (int k = 0; k < Ks; ++k) {
            const float al = s_sim[k], be = s_b[k], ak = s_a[k];
            int4 t0, t1;
            float4 w0, w1;
            gen_taps<POOL>(s_tap, s_w, k, Ks, t0, w0, t1, w1);
            if (al != 0.f || be != 0.f) {    // wave-uniform
#pragma unroll
                for (int i = 0; i < kGenMaxQ; ++i) {
                    const int c = lane + i * kWave;
                    if (c < p.cs) {
                        bool second;
                        const float v = gen_pooled_argwin<POOL>(m1, p.cs, c, t0, w0, t1, w1, second);
                        dq[i] = fmaf(al, v, dq[i]);
                        if (g1) gen_scatter(g1, p.cs, c, second ? t1 : t0, second ? w1 : w0, al * qv[i] - be * v);
                    }
                }
            }
            if (g2 && ak != 0.f) {
                for (int c = lane; c < p.cv; c += kWave) {
                    bool second;   // only the winner is needed here: without POOL the unused sample is dead code, no load
                    gen_pooled_argwin<POOL>(m2, p.cv, c, t0, w0, t1, w1, second);
                    gen_scatter(g2, p.cv, c, second ? t1 : t0, second ? w1 : w0, ak * grow[c]);
                }
            }
        }
        float *gqrow = bp.gq + ((size_t)n * HW + pix) * p.cs;
#pragma unroll
        for (int i = 0; i < kGenMaxQ; ++i)
            // (gamma == 0 -- every similarity but the cosine, and ATTENTION max without a gradient through the attention --: q does
            //  not enter its own gradient, and 0 x q must not either: a NaN or an Inf in q stays out, as in the reference's graph)
            if (lane + i * kWave < p.cs) gqrow[lane + i * kWave] = gamma != 0.f ? dq[i] - gamma * qv[i] : dq[i];
    }
}

// SIMILARITY prior: the prior table is the attention (needs one; excludes the other similarity / prior switches)
int check_sim_prior(const char *who, int flags, bool has_prior)
{
    if (!(flags & ET_GENERAL_SIM_PRIOR)) return 0;
    if (!has_prior) return fail("%s: SIM_PRIOR without a prior", who);
    if (flags & (ET_GENERAL_PRIOR_MUL | ET_GENERAL_COSINE))
        return fail("%s: SIM_PRIOR excludes PRIOR_MUL / COSINE (flags=%d)", who, flags);
    return 0;
}

// The argument checks of both entry points, then the inputs of the parameter block (out / attn / corr are the caller's) and
// the grid.  `written` is the output every call writes: the forward's out, the backward's grad_q.  `backward`: grad_out is
// required too, and a grad_prior needs a prior.
int general_params(const char *who, bool backward, const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                   const float *cam, const float *q, const float *map_sim, const float *map_val, const float *prior, int c_sim,
                   int c_val, int flags, const float *written, const float *grad_out, const float *grad_prior, GeneralParams &p,
                   unsigned &blocks)
{
    if (!desc) return fail("%s: desc is NULL", who);
    EtLayerDesc chk = *desc;
    chk.C = 4;                                   // (the channel counts of these entry points are c_sim / c_val)
    if (int e = validate(&chk)) return e;        // K <= 256, so K' fits the kernels' kGenKPL lane slots
    if (!xs || !ys || !steps || !cam || !q || !map_sim || !map_val || !written || (backward && !grad_out))
        return fail("%s: NULL pointer", who);
    if (c_sim <= 0 || c_sim > kGenMaxQ * kWave) return fail("%s: c_sim=%d outside [1, %d]", who, c_sim, kGenMaxQ * kWave);
    if (c_val <= 0 || c_val > 4096) return fail("%s: c_val=%d outside [1, 4096]", who, c_val);
    if (flags & ~(ET_GENERAL_POOLING | ET_GENERAL_PRIOR_MUL | ET_GENERAL_COSINE | ET_GENERAL_ATTENTION_MAX | ET_GENERAL_SIM_PRIOR))
        return fail("%s: unknown flag bits %d", who, flags);
    if ((flags & ET_GENERAL_ATTENTION_MAX) && prior && !(flags & ET_GENERAL_SIM_PRIOR))
        return fail("%s: ATTENTION max takes no prior", who);
    if (int e = check_sim_prior(who, flags, prior != nullptr)) return e;
    if ((flags & ET_GENERAL_POOLING) && (desc->K & 1)) return fail("%s: POOLING needs an even K (K=%d)", who, desc->K);
    if ((flags & ET_GENERAL_PRIOR_MUL) && !prior) return fail("%s: PRIOR_MUL without a prior", who);
    if (backward && grad_prior && !prior) return fail("%s: grad_prior without a prior", who);
    const long long hw = (long long)desc->H * desc->W;
    if (hw * (c_sim > c_val ? c_sim : c_val) * 4 >= (1LL << 31)) return fail("one feature map must stay below 2 GiB");
    p.d = *desc;
    p.xs = xs; p.ys = ys; p.steps = steps; p.cam = cam;
    p.q = q; p.m_sim = map_sim; p.m_val = map_val; p.prior = prior;
    p.cs = c_sim; p.cv = c_val; p.prior_mul = (flags & ET_GENERAL_PRIOR_MUL) ? 1 : 0;
    p.attn_max = (flags & ET_GENERAL_ATTENTION_MAX) ? 1 : 0;
    p.cosine = (flags & (ET_GENERAL_COSINE | ET_GENERAL_ATTENTION_MAX)) ? 1 : 0;   // (ATTENTION max is always cosine, epipolar.py:282)
    p.sim_prior = (flags & ET_GENERAL_SIM_PRIOR) ? 1 : 0;
    const long long nblocks = (hw * desc->N + kGenWaves - 1) / kGenWaves;
    if (nblocks > 0x7fffffffLL) return fail("grid too large");
    blocks = (unsigned)nblocks;
    return 0;
}

// one wave per reference pixel; the POOLING switch is a template parameter of the kernels
template <class P>
int launch_general(const char *who, bool pool, void (*pooled)(P), void (*plain)(P), unsigned blocks, size_t lds, void *stream,
                   const P &p)
{
    void (*kernel)(P) = pool ? pooled : plain;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kWave * kGenWaves), lds, (hipStream_t)stream, p);
    return check_launch(who);
}
}  // namespace

extern "C" {

int et_epipolar_forward_general(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                const float *cam, const float *q, const float *map_sim, const float *map_val,
                                const float *prior, int c_sim, int c_val, int flags, float *out, float *attn,
                                float *corr_pos, void *stream)
{
    const char *who = "et_epipolar_forward_general";
    GeneralParams p;
    unsigned blocks;
    if (int e = general_params(who, false, desc, xs, ys, steps, cam, q, map_sim, map_val, prior, c_sim, c_val, flags, out, nullptr,
                               nullptr, p, blocks))
        return e;
    p.out = out; p.attn = attn; p.corr = corr_pos;
    return launch_general(who, flags & ET_GENERAL_POOLING, epipolar_fwd_general_kernel<true>, epipolar_fwd_general_kernel<false>,
                          blocks, gen_lds_bytes(desc->K), stream, p);
}

int et_epipolar_backward_general(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                 const float *cam, const float *q, const float *map_sim, const float *map_val,
                                 const float *prior, const float *grad_out, int c_sim, int c_val, int flags, float *grad_q,
                                 float *grad_map_sim, float *grad_map_val, float *grad_prior, void *stream)
{
    return et_epipolar_backward_general_ga(desc, xs, ys, steps, cam, q, map_sim, map_val, prior, grad_out, nullptr, c_sim, c_val, flags,
                                           grad_q, grad_map_sim, grad_map_val, grad_prior, stream);
}

int et_epipolar_backward_general_ga(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                    const float *cam, const float *q, const float *map_sim, const float *map_val,
                                    const float *prior, const float *grad_out, const float *grad_attn, int c_sim, int c_val,
                                    int flags, float *grad_q, float *grad_map_sim, float *grad_map_val, float *grad_prior,
                                    void *stream)
{
    const char *who = "et_epipolar_backward_general";
    GeneralBwdParams bp;
    unsigned blocks;
    if (int e = general_params(who, true, desc, xs, ys, steps, cam, q, map_sim, map_val, prior, c_sim, c_val, flags, grad_q, grad_out,
                               grad_prior, bp.f, blocks))
        return e;
    bp.f.out = nullptr; bp.f.attn = nullptr; bp.f.corr = nullptr;
    bp.gout = grad_out; bp.gattn = grad_attn; bp.gq = grad_q; bp.gsim = grad_map_sim; bp.gval = grad_map_val; bp.gprior = grad_prior;
    const size_t lds = (size_t)kGenWaves * gen_bwd_wave_floats(desc->K) * sizeof(float);
    return launch_general(who, flags & ET_GENERAL_POOLING, epipolar_bwd_general_kernel<true>, epipolar_bwd_general_kernel<false>,
                          blocks, lds, stream, bp);
}

}  // extern "C"
