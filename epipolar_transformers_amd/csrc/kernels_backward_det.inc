// Part of et_backward_tile.hip (one translation unit, one anonymous namespace): what the deterministic tile backward
// (et_epipolar_backward_tiled_det, the DET instances of kernels_backward_tile.inc) needs around the tile kernel.  Not a
// stand-alone header.
// ----------------------------------------------------------------------------
// d(feat_src) is a sum over the tiles that touch a source row.  The default form adds the tiles' fp32 results with float
// atomics: the order, and with it the rounding, changes from run to run.  Here every contribution is converted to 64-bit fixed
// point under ONE power-of-two quantum q per pair and added with integer atomics: integer addition is associative, the sum
// does not depend on the order, and one pass converts it to fp32 at the end (one rounding per element).
//
// The quantum comes from a BOUND on a contribution, not from an estimate.  One group run (at most 32 pixels p) adds
//     c[u, ch] = sum_p  Bs[p, u] F1[p, ch]  +  B[p, u] G[p, ch]
// into source row u.  With the soft-max on:  B[p, u] = sum_k a_k w_ku, a >= 0, sum_k a_k = 1, 0 <= w <= 1  ->  |B| <= 1;
// Bs[p, u] = sum_k ds_k w_ku, ds_k = scale a_k (e_k - sum_j a_j e_j)  ->  |Bs| <= 2 |scale| max_k |e_k|;  e_k = g . S_k with S_k a
// convex combination of source rows  ->  |e_k| <= 256 M_g M_src.  So
//     |c| <= 32 (2 |scale| 256 M_g M_src M_ref + M_g) = bound        (M_* = max |.| of the pair's three maps; x (1 + 1/64) for
// the rounding of the split-fp16 products).  With a gradient ga = d loss / d attn the soft-max gradient is formed from e_k + ga_k,
// |e_k + ga_k| <= 256 M_g M_src + M_ga (M_ga = max |ga| of the pair), and the bound becomes
//     32 (2 |scale| (256 M_g M_src + M_ga) M_ref + M_g)              -- the same bits as above for M_ga = 0, and a proper bound
// (not 0) for a loss on the attention alone (M_g = 0).  The forms the tile path admits: merged and the half-array form add c once per group
// run and (row, channel); a single source role adds one of the two terms; the two-round form of the 256-row kernel (one
// role, or ET_VARIANT_TILE_CLASSIC) adds the Bs term and the B term SEPARATELY -- two additions per group run, each bounded by its
// own term, their magnitudes together by `bound`.  What counts is the sum of magnitudes: a group run of m pixels is bounded by
// (m / 32) bound, the group runs of a pair partition its H W pixels, so every partial sum of a row, in any order and any form,
// stays below (H W / 32) bound <= 2^9 bound -- the 2^14 below (one run per pixel, each charged the full bound) has 5 bits to spare.
// A source row receives at most H W <= 2^14 group runs per pair (single-pixel groups), so with
//     q = 2^(floor(log2 bound) + 1 + 14 - 62)
// every partial sum stays below 2^62 and every contribution below 2^48 quanta, and a contribution AT the bound keeps 47 bits.
// q is clamped to >= 2^-100 so that 1 / q and acc * q are exact normal fp32 arithmetic.  With the soft-max off the
// "attention" is sim / K (-1e10 / K under the mask): no useful bound -- the entry point refuses that case.
// A finite contribution of 2^48 quanta or more cannot happen under the bound; the tile kernel checks it all the same, ORs
// kDetGuardMask (bit 2) into the workspace's sticky error word and does not add it.  A contribution that is NaN or infinite -- the
// pair holds a non-finite input; the maxima above skip such values -- marks its element instead, and the element comes out NaN.

// (kDetMaxBlocks, the blocks per pair of det_maxima_kernel -- one partial result each: et_tile_layout.h)
constexpr int kDetQuantumMinExp = -100;     // (an fp32 bound gives at most 2^81: no upper clamp is needed)

struct DetQuantum {
    float q, invq, bound;
};

__host__ __device__ inline DetQuantum det_quantum(float softmax_scale, float m_ref, float m_src, float m_g, float m_ga = 0.f)
{
    // (the M_ga term is a separate addend: with M_ga = 0 the sum is the expression without it, bit for bit -- whatever M_ref is)
    const double s2 = 2.0 * fabs((double)softmax_scale);
    const double ga_term = m_ga > 0.f ? s2 * (double)m_ga * (double)m_ref : 0.0;
    const double b = 32.0 * ((s2 * 256.0 * (double)m_g * (double)m_src * (double)m_ref + ga_term) + (double)m_g) * (1.0 + 1.0 / 64.0);
    DetQuantum r;
    r.bound = (float)b;                 // (the exponent is taken from the fp32 value: what the caller is told is what q is made for)
    r.q = r.invq = 1.f;
    if (!(r.bound > 0.f)) {             // all-zero gradients (or a NaN maximum): nothing to scale
        r.bound = 0.f;
        return r;
    }
    int e = 129;                        // bound = m 2^e, 0.5 <= m < 1: floor(log2 bound) = e - 1   (inf: beyond the clamp)
    if (r.bound <= 3.402823466e38f) frexpf(r.bound, &e);
    int qe = (e - 1) + 1 + 14 - 62;
    qe = qe < kDetQuantumMinExp ? kDetQuantumMinExp : qe;
    r.q = ldexpf(1.f, qe);
    r.invq = ldexpf(1.f, -qe);
    return r;
}

// max |.| of the three maps of every pair (and of its rows of gattn = d loss / d attn, nullable: K H W floats per pair): block
// (b, n) takes every gridDim.x-th run of 256 float4 of pair n and leaves { M_ref, M_src, M_g, M_ga } in
// partial[(n * gridDim.x + b) * 4 ..] (finite values only)
__global__ __launch_bounds__(256) void det_maxima_kernel(const float4 *__restrict__ fref, const float4 *__restrict__ fsrc,
                                                         const float4 *__restrict__ gout, unsigned vec4_per_pair,
                                                         const float *__restrict__ gattn, unsigned ga_per_pair,
                                                         float *__restrict__ partial)
{
    __shared__ float s_m[4][4];
    const int n = blockIdx.y;
    const size_t base = (size_t)n * vec4_per_pair;
    // (a NaN or an Inf counts as 0: the quantum is made for the pair's FINITE values, which then keep their accuracy; what a
    //  non-finite value contributes is non-finite and is marked, not scaled: det_add)
    auto mag = [](float x) { const float a = fabsf(x); return a <= kLargestFinite ? a : 0.f; };
    auto amax4 = [&](float m, const float4 &v) { return fmaxf(fmaxf(m, fmaxf(mag(v.x), mag(v.y))), fmaxf(mag(v.z), mag(v.w))); };
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;
    if (gattn) {    // (scalar loads: K H W need not be a multiple of four)
        const float *ga = gattn + (size_t)n * ga_per_pair;
        for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < ga_per_pair; i += gridDim.x * blockDim.x) m3 = fmaxf(m3, mag(ga[i]));
    }
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < vec4_per_pair; i += gridDim.x * blockDim.x) {
        const float4 a = fref[base + i], b = fsrc[base + i], c = gout[base + i];
        m0 = amax4(m0, a);
        m1 = amax4(m1, b);
        m2 = amax4(m2, c);
    }
    m0 = wave_max(m0);
    m1 = wave_max(m1);
    m2 = wave_max(m2);
    m3 = wave_max(m3);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_m[0][wave] = m0;
        s_m[1][wave] = m1;
        s_m[2][wave] = m2;
        s_m[3][wave] = m3;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int t = threadIdx.x;
        partial[((size_t)n * gridDim.x + blockIdx.x) * 4 + t] = fmaxf(fmaxf(s_m[t][0], s_m[t][1]), fmaxf(s_m[t][2], s_m[t][3]));
    }
}

// one thread per pair: the pair's maxima from the partial results, its quantum -> quanta[n] = { q, 1 / q, bound, 0 }
__global__ __launch_bounds__(64) void det_quantum_kernel(int N, int blocks_per_pair, float softmax_scale,
                                                         const float *__restrict__ partial, float *__restrict__ quanta)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float m[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < blocks_per_pair; ++b)
        for (int t = 0; t < 4; ++t) m[t] = fmaxf(m[t], partial[((size_t)n * blocks_per_pair + b) * 4 + t]);
    const DetQuantum r = det_quantum(softmax_scale, m[0], m[1], m[2], m[3]);
    *reinterpret_cast<float4 *>(quanta + (size_t)n * 4) = make_float4(r.q, r.invq, r.bound, 0.f);
}

// grad_src = (float)acc * q: the conversion rounds once, the product with a power of two is exact.  Four channels per thread:
// two 16-byte loads, one 16-byte store, consecutive threads along the row.
__global__ __launch_bounds__(256) void det_finish_kernel(const long long *__restrict__ acc, const float *__restrict__ quanta,
                                                         float4 *__restrict__ gsrc, unsigned vec4_per_pair)
{
    typedef long long i64x2 __attribute__((ext_vector_type(2)));
    const size_t base = (size_t)blockIdx.y * vec4_per_pair;          // (blockIdx.y: the pair)
    const i64x2 *a = reinterpret_cast<const i64x2 *>(acc) + 2 * base;
    gsrc += base;
    const float q = quanta[blockIdx.y * 4];
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < vec4_per_pair; i += gridDim.x * blockDim.x) {
        const i64x2 lo = __builtin_nontemporal_load(a + 2 * i), hi = __builtin_nontemporal_load(a + 2 * i + 1);
        // (an element beyond 2^61 was marked non-finite by det_add: NaN)
        auto val = [q](long long a) { return (a < kDetPoisonFloor && a > -kDetPoisonFloor) ? (float)a * q : __builtin_nanf(""); };
        gsrc[i] = make_float4(val(lo.x), val(lo.y), val(hi.x), val(hi.y));
    }
}
