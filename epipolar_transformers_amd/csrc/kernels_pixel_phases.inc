// Part of et_forward.hip and et_backward.hip (inside the unit's anonymous namespace, after et_common.h /
// kernels_sample_table.inc): the phases the per-pixel kernels share, one definition each.  Not a stand-alone header.
// The inner sample loops are NOT here: they differ between the kernels (channel mapping, tap cache, batching).

// ----------------------------------------------------------------------------
// backward: the tail of a pass-A batch, and the soft-max gradient
// ----------------------------------------------------------------------------
// Batch kb .. kb+7 of lane slot s: sum the eight partial pairs (p1: S_k . f, p2: S_k . g) over the wave, apply the
// `== 0 -> -1e10` mask (epipolar.py:298) and the logit scale, and hand the three values of sample kb + j to the lane
// that owns it (lane kb + j of slot s).
template <int KPL>
__device__ __forceinline__ void keep_batch(const EtLayerDesc &d, int K, int lane, int s, int kb, const float (&p1)[8],
                                           const float (&p2)[8], float (&v_logit)[KPL], float (&v_da)[KPL],
                                           bool (&v_masked)[KPL])
{
    const float u1 = reduce8(p1, lane);
    const float u2 = reduce8(p2, lane);
    const bool masked = (u1 == 0.f);
    float sv = masked ? -1e10f : u1;
    sv = d.softmax_enabled ? sv * d.softmax_scale : sv / (float)K;
    const int srcl = lane_of_sample<8>(lane & 7);
    const float mine_l = __shfl(sv, srcl);
    const float mine_d = __shfl(u2, srcl);
    const int mine_m = __shfl((int)masked, srcl);
    if ((lane >> 3) == (kb >> 3)) {
        v_logit[s] = mine_l;
        v_da[s] = mine_d;
        v_masked[s] = mine_m != 0;
    }
}

// Lanes <-> samples: from the logits and da_k = g . S_k (+ d loss / d attn_k) to the attention a_k and d s_k.
template <int KPL>
__device__ __forceinline__ void softmax_grad(const BwdParams &p, int n, int pix, int lane, const float (&v_logit)[KPL],
                                             float (&v_da)[KPL], const bool (&v_masked)[KPL], float (&v_a)[KPL],
                                             float (&v_ds)[KPL])
{
    const EtLayerDesc &d = p.d;
    const int K = d.K, HW = d.H * d.W;
    const float neg_inf = -__builtin_huge_valf();
    if (p.gattn) {  // block-uniform: d loss / d attn_k reaches a_k beside e_k = g . S_k (include/epipolar_amd.h)
        const float *ga = p.gattn + (size_t)n * K * HW + pix;
#pragma unroll
        for (int s = 0; s < KPL; ++s)
            if (s * kWave + lane < K) v_da[s] += ga[(size_t)(s * kWave + lane) * HW];
    }
    if (d.softmax_enabled) {
        float mx = neg_inf;      // (fmaxf drops a NaN logit; expf(NaN - mx) below is NaN and reaches the sum and every weight)
#pragma unroll
        for (int s = 0; s < KPL; ++s) mx = fmaxf(mx, (s * kWave + lane < K) ? v_logit[s] : neg_inf);
        mx = wave_max(mx);
        float lsum = 0.f;
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            v_a[s] = (s * kWave + lane < K) ? expf(v_logit[s] - mx) : 0.f;
            lsum += v_a[s];
        }
        const float denom = wave_sum(lsum);
        float dsum = 0.f;
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            v_a[s] = v_a[s] / denom;
            dsum = fmaf(v_a[s], v_da[s], dsum);
        }
        const float dot = wave_sum(dsum);
#pragma unroll
        for (int s = 0; s < KPL; ++s)
            v_ds[s] = v_masked[s] ? 0.f : d.softmax_scale * v_a[s] * (v_da[s] - dot);
    } else {
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            const bool in = s * kWave + lane < K;
            v_a[s] = in ? v_logit[s] : 0.f;  // already sim / K
            v_ds[s] = (in && !v_masked[s]) ? v_da[s] / (float)K : 0.f;
        }
    }
}

// ----------------------------------------------------------------------------
// forward: the outputs beside `out`
// ----------------------------------------------------------------------------
// Additive term of the residual fusion, feat_ref + res_bias, while the reference row is still in registers.  A lane's
// c-th float4 group of the pixel row is first + c * STRIDE; groups from nvec on do not exist.
template <int N, int STRIDE>
__device__ __forceinline__ void write_res_base(const FwdParams &p, size_t row, int first, int nvec, const float4 (&f1)[N])
{
    float4 *b4 = reinterpret_cast<float4 *>(p.res_base + row * p.d.C);
    const float4 *bias4 = reinterpret_cast<const float4 *>(p.res_bias);
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int v = first + c * STRIDE;
        if (v < nvec) {
            float4 r = f1[c];
            if (bias4) {
                const float4 bb = bias4[v];
                r = make_float4(r.x + bb.x, r.y + bb.y, r.z + bb.z, r.w + bb.w);
            }
            b4[v] = r;
        }
    }
}

// First maximum over k (torch.argmax) of a[s] = value of sample s * 64 + lane: a NaN above every value, then the value, then
// the lowest index (argmax_key).  Always one of the samples 0 .. K-1: the callers read a lane and p.steps[] with it.
template <int KPL>
__device__ __forceinline__ int first_argmax(const float (&a)[KPL], int K, int lane)
{
    unsigned bestk = 0u;
    int besti = 0x7fffffff;
#pragma unroll
    for (int s = 0; s < KPL; ++s) {
        const int k = s * kWave + lane;
        const unsigned key = argmax_key(a[s]);
        if (k < K && key > bestk) {      // (ascending k: an equal key keeps the lower index)
            bestk = key;
            besti = k;
        }
    }
    return wave_first_argmax(bestk, besti);
}

// The block's [K][16] attention tile in LDS -> (N,K,H,W): for a fixed k the 16 pixels of this block are contiguous.
// Called by the whole block once every wave has written its pixels' columns.
__device__ __forceinline__ void store_attn_tile(const FwdParams &p, const float *s_attn, int n, int pix_base)
{
    const int K = p.d.K, HW = p.d.H * p.d.W;
    __syncthreads();
    const int npix = min(kPixPerBlock, HW - pix_base);
    float *dst = p.attn + (size_t)n * K * HW + pix_base;
    if (npix == kPixPerBlock && (HW & 3) == 0) {
        for (int t = threadIdx.x; t < K * 4; t += blockDim.x) {
            const int k = t >> 2, q = t & 3;
            const float4 v = *reinterpret_cast<const float4 *>(&s_attn[k * kPixPerBlock + q * 4]);
            *reinterpret_cast<float4 *>(dst + (size_t)k * HW + q * 4) = v;
        }
    } else {
        for (int t = threadIdx.x; t < K * kPixPerBlock; t += blockDim.x) {
            const int k = t / kPixPerBlock, i = t % kPixPerBlock;
            if (i < npix) dst[(size_t)k * HW + i] = s_attn[k * kPixPerBlock + i];
        }
    }
}
