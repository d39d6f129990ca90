// Part of et_backward.hip (inside its anonymous namespace, after et_common.h / kernels_sample_table.inc /
// kernels_pixel_phases.inc): the backward kernels (atomic scatter, and emit / scan / bucket / gather).  Not a stand-alone header.
// ----------------------------------------------------------------------------
// backward
// ----------------------------------------------------------------------------
// Same walk, twice.  Pass A recomputes the logits and da_k = g . S_k; the
// soft-max gradient is formed with lanes <-> samples; pass B accumulates
// d(feat_ref) and scatters d(feat_src) through a gradient twin of the tap
// cache: a tap's gradient row is flushed with float atomics only when the tap
// is evicted, i.e. once per (pixel, source row) instead of once per sample.
// Channel mapping here is lane + 64*i (dword-strided) so that each atomic
// instruction of a flush covers 256 contiguous bytes.
template <int CPD /*dwords per lane: C <= 64*CPD*/, int KPL>
__global__ __launch_bounds__(kWave *kWavesPerBlock) void epipolar_bwd_kernel(const BwdParams p)
{
    // Float-atomic scatter form (no workspace needed); the default is the gather form below.
    const EtLayerDesc &d = p.d;
    const int H = d.H, W = d.W, C = d.C, K = d.K;
    const int HW = H * W;

    const int vb = xcd_remap(blockIdx.x, p.total_blocks);
    const int n = vb / p.blocks_per_pair;
    const int pb = vb - n * p.blocks_per_pair;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pix_base = pb * kPixPerBlock;

    const float *cam = p.cam + (size_t)n * ET_CAM_STRIDE;
    const __amdgpu_buffer_rsrc_t src = make_rsrc(p.fsrc + (size_t)n * HW * C, (unsigned)HW * C * 4u);
    const __amdgpu_buffer_rsrc_t gsrc = make_rsrc(p.gsrc + (size_t)n * HW * C, (unsigned)HW * C * 4u);
    const int row_bytes = C * 4;
    const float neg_inf = -__builtin_huge_valf();
    // lanes beyond C (only when C < 64*CPD) point past the buffer: their loads return zeros and their atomics are dropped
    // (the range check of a raw buffer looks at the vector offset alone), so they contribute zero to every dot product.
    // (They used to alias the last channel and add 0.0f to it: 0 x Inf = NaN, once a weight was infinite.)
    int voff[CPD];
    bool live[CPD];
#pragma unroll
    for (int c = 0; c < CPD; ++c) {
        live[c] = (lane + c * kWave) < C;
        voff[c] = live[c] ? (lane + c * kWave) * 4 : 0x7ffff000;
    }

    for (int pp = 0; pp < kPixPerWave; ++pp) {
        const int pix = pix_base + wave * kPixPerWave + pp;
        if (pix >= HW) break;
        const int h = pix / W, w = pix - h * W;

        const et::Segment seg = et::epipolar_segment(d, cam, p.xs[w], p.ys[h]);
        SampleTable<KPL> tb;
        build_sample_table<KPL>(d, seg, p.steps, lane, row_bytes, tb);
        float v_logit[KPL], v_da[KPL];
        bool v_masked[KPL];
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            v_logit[s] = neg_inf;
            v_da[s] = 0.f;
            v_masked[s] = false;
        }

        float f1[CPD], g[CPD], R[4][CPD];
        const float *ref = p.fref + ((size_t)n * HW + pix) * C;
        const float *go = p.gout + ((size_t)n * HW + pix) * C;
#pragma unroll
        for (int c = 0; c < CPD; ++c) {
            const int ch = lane + c * kWave;
            f1[c] = live[c] ? ref[ch] : 0.f;
            g[c] = live[c] ? go[ch] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) R[r][c] = 0.f;
        }

        // ---------------- pass A: logits and da ---------------------------------
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            const int kcount = min(kWave, K - s * kWave);
            for (int kb = 0; kb < kcount; kb += 8) {
                float p1[8], p2[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int kk = kb + j;
                    p1[j] = 0.f;
                    p2[j] = 0.f;
                    if (kk < kcount) {
                        const int need = __builtin_amdgcn_readlane(tb.need[s], kk);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            if (need & (1 << r)) {
                                const int off = __builtin_amdgcn_readlane(tb.off[s][r], kk);
#pragma unroll
                                for (int c = 0; c < CPD; ++c) R[r][c] = tap_row_f1(src, voff[c], off);
                            }
                        }
                        const float w0 = lane_bcast(tb.w[s][0], kk), w1 = lane_bcast(tb.w[s][1], kk);
                        const float w2 = lane_bcast(tb.w[s][2], kk), w3 = lane_bcast(tb.w[s][3], kk);
#pragma unroll
                        for (int c = 0; c < CPD; ++c) {
                            float sv = w0 * R[0][c];
                            sv = fmaf(w1, R[1][c], sv);
                            sv = fmaf(w2, R[2][c], sv);
                            sv = fmaf(w3, R[3][c], sv);
                            p1[j] = fmaf(sv, f1[c], p1[j]);
                            p2[j] = fmaf(sv, g[c], p2[j]);
                        }
                    }
                }
                keep_batch<KPL>(d, K, lane, s, kb, p1, p2, v_logit, v_da, v_masked);
            }
        }

        // ---------------- soft-max gradient, lanes <-> samples -----------------
        float v_a[KPL], v_ds[KPL];
        softmax_grad<KPL>(p, n, pix, lane, v_logit, v_da, v_masked, v_a, v_ds);

        // ---------------- pass B: d(feat_ref) and scatter of d(feat_src) --------
        float d1[CPD], G[4][CPD];
#pragma unroll
        for (int c = 0; c < CPD; ++c) {
            d1[c] = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                G[r][c] = 0.f;
                R[r][c] = 0.f;
            }
        }
        int tag[4] = {-1, -1, -1, -1};  // byte offset of the row whose gradient G[r] holds (scalar)

#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            const int kcount = min(kWave, K - s * kWave);
            for (int kk = 0; kk < kcount; ++kk) {
                const int need = __builtin_amdgcn_readlane(tb.need[s], kk);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (need & (1 << r)) {
                        const int off = __builtin_amdgcn_readlane(tb.off[s][r], kk);
                        // (what an absent tap gathered -- weight 0 times dS, NaN once dS is infinite -- belongs to no row: dropped)
#pragma unroll
                        for (int c = 0; c < CPD; ++c) {
                            if (tag[r] >= 0) __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(G[r][c], gsrc, voff[c], tag[r], 0);
                            G[r][c] = 0.f;
                        }
#pragma unroll
                        for (int c = 0; c < CPD; ++c) R[r][c] = tap_row_f1(src, voff[c], off);
                        tag[r] = off;
                    }
                }
                const float w0 = lane_bcast(tb.w[s][0], kk), w1 = lane_bcast(tb.w[s][1], kk);
                const float w2 = lane_bcast(tb.w[s][2], kk), w3 = lane_bcast(tb.w[s][3], kk);
                const float ak = lane_bcast(v_a[s], kk), dsk = lane_bcast(v_ds[s], kk);
                // OTHER_GRAD (epipolar.py:141-153): which of the two uses of feat_src carry gradient
                const float ak_src = (d.src_grad_mask & 2) ? ak : 0.f;
                const float dsk_src = (d.src_grad_mask & 1) ? dsk : 0.f;
#pragma unroll
                for (int c = 0; c < CPD; ++c) {
                    float sv = w0 * R[0][c];
                    sv = fmaf(w1, R[1][c], sv);
                    sv = fmaf(w2, R[2][c], sv);
                    sv = fmaf(w3, R[3][c], sv);
                    d1[c] = fmaf(dsk, sv, d1[c]);
                    const float dS = fmaf(dsk_src, f1[c], ak_src * g[c]);
                    G[0][c] = fmaf(w0, dS, G[0][c]);
                    G[1][c] = fmaf(w1, dS, G[1][c]);
                    G[2][c] = fmaf(w2, dS, G[2][c]);
                    G[3][c] = fmaf(w3, dS, G[3][c]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (tag[r] >= 0) {
#pragma unroll
                for (int c = 0; c < CPD; ++c)
                    __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(G[r][c], gsrc, voff[c], tag[r], 0);
            }
        }
        float *gr = p.gref + ((size_t)n * HW + pix) * C;
#pragma unroll
        for (int c = 0; c < CPD; ++c) {
            const int ch = lane + c * kWave;
            if (live[c]) gr[ch] = d1[c];
        }
    }
}

// ----------------------------------------------------------------------------
// backward, emit form with the forward's channel mapping (float4 per lane):
// d(feat_ref) + per-(pixel, source row) coefficients for the gather pass
// ----------------------------------------------------------------------------
template <int CPL, int KPL>
__global__ __launch_bounds__(kWave *kWavesPerBlock) void epipolar_bwd_emit_kernel(const BwdParams p)
{
    extern __shared__ float s_dyn[];  // per wave: [KPL*64] float4 weights, then [cap] u, [cap] alpha, [cap] beta
    const EtLayerDesc &d = p.d;
    const int H = d.H, W = d.W, C = d.C, K = d.K;
    const int HW = H * W;
    const int nvec = C >> 2;

    const int vb = xcd_remap(blockIdx.x, p.total_blocks);
    const int n = vb / p.blocks_per_pair;
    const int pb = vb - n * p.blocks_per_pair;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pix_base = pb * kPixPerBlock;
    char *wbase = reinterpret_cast<char *>(s_dyn) + (size_t)wave * (KPL * kWave * 16 + 3 * p.cap * 4);
    float4 *s_wt = reinterpret_cast<float4 *>(wbase);
    int *s_eu = reinterpret_cast<int *>(wbase + KPL * kWave * 16);
    float *s_ea = reinterpret_cast<float *>(s_eu) + p.cap;
    float *s_eb = s_ea + p.cap;

    const float *cam = p.cam + (size_t)n * ET_CAM_STRIDE;
    const __amdgpu_buffer_rsrc_t src = make_rsrc(p.fsrc + (size_t)n * HW * C, (unsigned)HW * C * 4u);
    const int row_bytes = C * 4;
    const float neg_inf = -__builtin_huge_valf();
    int voff[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) voff[c] = (lane + c * kWave < nvec) ? (lane + c * kWave) * 16 : 0x7ffff000;   // (idle lanes: zeros, as in the forward)

    for (int pp = 0; pp < kPixPerWave; ++pp) {
        const int pix = pix_base + pp * kWavesPerBlock + wave;  // waves of a block on neighbouring pixels
        if (pix >= HW) continue;
        const int h = pix / W, w = pix - h * W;
        const et::Segment seg = et::epipolar_segment(d, cam, p.xs[w], p.ys[h]);
        SampleTable<KPL> tb;
        build_sample_table<KPL>(d, seg, p.steps, lane, row_bytes, tb);
        float v_logit[KPL], v_da[KPL];
        bool v_masked[KPL];
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            v_logit[s] = neg_inf;
            v_da[s] = 0.f;
            v_masked[s] = false;
            s_wt[s * kWave + lane] = make_float4(tb.w[s][0], tb.w[s][1], tb.w[s][2], tb.w[s][3]);
        }
        __builtin_amdgcn_wave_barrier();

        float4 f1[CPL], g[CPL], R[4][CPL];
        const float4 *ref = reinterpret_cast<const float4 *>(p.fref + ((size_t)n * HW + pix) * C);
        const float4 *go = reinterpret_cast<const float4 *>(p.gout + ((size_t)n * HW + pix) * C);
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int v = lane + c * kWave;
            f1[c] = (v < nvec) ? ref[v] : f4_zero();
            g[c] = (v < nvec) ? go[v] : f4_zero();
#pragma unroll
            for (int r = 0; r < 4; ++r) R[r][c] = f4_zero();
        }

        // ---------------- pass A: logits and da -----------------------------------
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            const int kcount = min(kWave, K - s * kWave);
            for (int kb = 0; kb < kcount; kb += 8) {
                float p1[8], p2[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int kk = kb + j;
                    p1[j] = 0.f;
                    p2[j] = 0.f;
                    if (kk < kcount) {
                        const int need = __builtin_amdgcn_readlane(tb.need[s], kk);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            if (need & (1 << r)) {
                                const int off = __builtin_amdgcn_readlane(tb.off[s][r], kk);
#pragma unroll
                                for (int c = 0; c < CPL; ++c) R[r][c] = tap_row_f4(src, voff[c], off);
                            }
                        }
                        const float4 wv = s_wt[s * kWave + kk];
#pragma unroll
                        for (int c = 0; c < CPL; ++c) {
                            float4 sv = f4_mul(wv.x, R[0][c]);
                            sv = f4_fma(wv.y, R[1][c], sv);
                            sv = f4_fma(wv.z, R[2][c], sv);
                            sv = f4_fma(wv.w, R[3][c], sv);
                            p1[j] += f4_dot(sv, f1[c]);
                            p2[j] += f4_dot(sv, g[c]);
                        }
                    }
                }
                keep_batch<KPL>(d, K, lane, s, kb, p1, p2, v_logit, v_da, v_masked);
            }
        }

        // ---------------- soft-max gradient, lanes <-> samples -----------------------
        float v_a[KPL], v_ds[KPL];
        softmax_grad<KPL>(p, n, pix, lane, v_logit, v_da, v_masked, v_a, v_ds);

        // ---------------- pass B: d(feat_ref) and the coefficient entries ----------------
        float4 d1[CPL];
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            d1[c] = f4_zero();
#pragma unroll
            for (int r = 0; r < 4; ++r) R[r][c] = f4_zero();
        }
        int tag[4] = {-1, -1, -1, -1};
        float ea[4] = {0.f, 0.f, 0.f, 0.f}, eb[4] = {0.f, 0.f, 0.f, 0.f};
        // A pixel whose grad_out / feat_ref row holds an Inf: the gather pass multiplies the SUMS alpha_u, beta_u with that row,
        // the reference multiplies term by term -- w a_k g with terms of both signs (or a zero one) is Inf - Inf (0 x Inf) = NaN
        // there, alpha_u x Inf = +-Inf here.  So such a pixel (wave-uniform, rare) also records, per entry, whether its terms are
        // of one strict sign (bit 0: positive, 1: negative, 2: zero or NaN seen), and the entry carries "mixed" flags in the
        // upper bits of its row index (bit 24: alpha, bit 25: beta) for the gather pass, which turns Inf factors into NaN then.
        bool odd_row = false;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            auto odd = [](float x) { return !(fabsf(x) <= kLargestFinite); };
            odd_row |= odd(f1[c].x) | odd(f1[c].y) | odd(f1[c].z) | odd(f1[c].w) | odd(g[c].x) | odd(g[c].y) | odd(g[c].z) | odd(g[c].w);
        }
        const bool odd_pixel = __builtin_amdgcn_ballot_w64(odd_row) != 0;
        int fa[4] = {0, 0, 0, 0}, fb[4] = {0, 0, 0, 0};
        auto sign_bits = [](float t) { return t > 0.f ? 1 : t < 0.f ? 2 : 4; };
        auto mixed = [](int f) { return (f & 4) != 0 || (f & 3) == 3; };
        int ecount = 0;
        auto emit = [&](int r) {  // wave-uniform call
            if (lane == 0) {
                s_eu[ecount] = (tag[r] / row_bytes) | (mixed(fa[r]) ? 1 << 24 : 0) | (mixed(fb[r]) ? 1 << 25 : 0);
                s_ea[ecount] = ea[r];
                s_eb[ecount] = eb[r];
            }
            ++ecount;
            ea[r] = 0.f;
            eb[r] = 0.f;
        };
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            const int kcount = min(kWave, K - s * kWave);
            for (int kk = 0; kk < kcount; ++kk) {
                const int need = __builtin_amdgcn_readlane(tb.need[s], kk);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (need & (1 << r)) {
                        const int off = __builtin_amdgcn_readlane(tb.off[s][r], kk);
                        if (tag[r] >= 0) emit(r);
                        ea[r] = 0.f;      // (what an absent tap gathered, weight 0 times a_k / ds_k, belongs to no row: dropped)
                        eb[r] = 0.f;
                        fa[r] = 0;
                        fb[r] = 0;
#pragma unroll
                        for (int c = 0; c < CPL; ++c) R[r][c] = tap_row_f4(src, voff[c], off);
                        tag[r] = off;
                    }
                }
                const float4 wv = s_wt[s * kWave + kk];
                const float ak = lane_bcast(v_a[s], kk), dsk = lane_bcast(v_ds[s], kk);
                // OTHER_GRAD (epipolar.py:141-153): which of the two uses of feat_src carry gradient
                const float ak_src = (d.src_grad_mask & 2) ? ak : 0.f;
                const float dsk_src = (d.src_grad_mask & 1) ? dsk : 0.f;
                ea[0] = fmaf(wv.x, ak_src, ea[0]); eb[0] = fmaf(wv.x, dsk_src, eb[0]);
                ea[1] = fmaf(wv.y, ak_src, ea[1]); eb[1] = fmaf(wv.y, dsk_src, eb[1]);
                ea[2] = fmaf(wv.z, ak_src, ea[2]); eb[2] = fmaf(wv.z, dsk_src, eb[2]);
                ea[3] = fmaf(wv.w, ak_src, ea[3]); eb[3] = fmaf(wv.w, dsk_src, eb[3]);
                if (odd_pixel) {  // wave-uniform
                    const float w4[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        fa[r] |= sign_bits(w4[r] * ak_src);
                        fb[r] |= sign_bits(w4[r] * dsk_src);
                    }
                }
#pragma unroll
                for (int c = 0; c < CPL; ++c) {
                    float4 sv = f4_mul(wv.x, R[0][c]);
                    sv = f4_fma(wv.y, R[1][c], sv);
                    sv = f4_fma(wv.z, R[2][c], sv);
                    sv = f4_fma(wv.w, R[3][c], sv);
                    d1[c] = f4_fma(dsk, sv, d1[c]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (tag[r] >= 0) emit(r);
        __builtin_amdgcn_wave_barrier();
        const size_t ebase = ((size_t)n * HW + pix) * p.cap;
        for (int i = lane; i < ecount; i += kWave) {
            const int u = s_eu[i] & 0xffffff;      // (the flags travel in ent_u)
            p.ent_u[ebase + i] = s_eu[i];
            p.ent_a[ebase + i] = s_ea[i];
            p.ent_b[ebase + i] = s_eb[i];
            atomicAdd(&p.row_count[(size_t)n * HW + u], 1);
        }
        if (lane == 0) p.ent_count[(size_t)n * HW + pix] = ecount;
        float4 *gr = reinterpret_cast<float4 *>(p.gref + ((size_t)n * HW + pix) * C);
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int v = lane + c * kWave;
            if (v < nvec) gr[v] = d1[c];
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ----------------------------------------------------------------------------
// gather-form backward of d(feat_src): scan, bucket, gather
// ----------------------------------------------------------------------------
// Per pair: exclusive prefix sum of row_count[HW] -> row_base[HW] (one block per pair).
__global__ __launch_bounds__(256) void bwd_scan_kernel(int HW, const int *row_count, int *row_base, int *row_cursor)
{
    __shared__ int s_part[256];
    const int n = blockIdx.x, t = threadIdx.x;
    const int *cnt = row_count + (size_t)n * HW;
    int *base = row_base + (size_t)n * HW;
    int *cur = row_cursor + (size_t)n * HW;
    const int per = (HW + 255) / 256;
    const int lo = t * per, hi = min(HW, lo + per);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += cnt[i];
    s_part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) {
            const int v = s_part[i];
            s_part[i] = run;
            run += v;
        }
    }
    __syncthreads();
    int run = s_part[t];
    for (int i = lo; i < hi; ++i) {
        base[i] = run;
        cur[i] = 0;
        run += cnt[i];
    }
}

// One wave per reference pixel: move its entries to their source rows' segments.
__global__ __launch_bounds__(256) void bwd_bucket_kernel(int HW, int cap, int total_rows, const int *ent_count,
                                                          const int *ent_u, const float *ent_a, const float *ent_b,
                                                          const int *row_base, int *row_cursor, int4 *csr)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wave_global = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * kWavesPerBlock;
    for (int gp = wave_global; gp < total_rows; gp += nwaves) {  // global reference pixel n*HW + p
        const int cnt = ent_count[gp];
        const int n = gp / HW;
        const int pidx = gp - n * HW;
        const size_t ebase = (size_t)gp * cap;
        const size_t pair_rows = (size_t)n * HW;
        for (int slot = lane; slot < cnt; slot += kWave) {
            const int eu = ent_u[ebase + slot];
            const int u = eu & 0xffffff;
            const size_t gu = pair_rows + u;
            const int pos = row_base[gu] + atomicAdd(&row_cursor[gu], 1);
            const size_t o = pair_rows * cap + pos;     // per-pair CSR region of HW*cap slots
            // one 16-byte record per entry (a single scattered store): {ordering key, alpha, beta, mixed-sign flags}
            csr[o] = make_int4(pidx * cap + slot, __float_as_int(ent_a[ebase + slot]),
                               __float_as_int(ent_b[ebase + slot]), eu >> 24);
        }
    }
}

// One wave per source pixel u: d feat_src[u] = sum_e alpha_e * g[p_e] + beta_e * f[p_e].
// Entries are ordered by reference pixel index first (bitonic sort in LDS) so the float32 sum has a
// fixed order: the result is bit-reproducible, unlike the atomic scatter.
template <int CPL>
__global__ __launch_bounds__(256) void epipolar_bwd_gather_kernel(int HW, int C, int cap, int total_rows, int mask,
                                                                   const int *row_count, const int *row_base,
                                                                   const int4 *csr, const float *fref,
                                                                   const float *gout, float *gsrc, int max_sort)
{
    extern __shared__ int s_sort[];  // per wave: max_sort keys + max_sort CSR indices
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gu = xcd_remap(blockIdx.x, gridDim.x) * kWavesPerBlock + wave;  // global source pixel n*HW + u
    if (gu >= total_rows) return;
    const int n = gu / HW;
    const int cnt = row_count[gu];
    const size_t seg = (size_t)n * HW * cap + row_base[gu];
    const int nvec = C >> 2;
    float4 acc[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) acc[c] = f4_zero();
    int voff[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) voff[c] = min(lane + c * kWave, nvec - 1);

    // order of summation: ascending (reference pixel, emission slot) -- a key that does not depend on
    // the arrival order of the bucket pass.  Keys are unique, so an entry's place in that order is the
    // number of smaller keys: a rank sort (every lane compares its keys against all keys, read as LDS
    // broadcasts, no dependent passes) is cheaper here than a bitonic network (n ~ 140).
    int *keys = s_sort + wave * 2 * max_sort;
    int *vals = keys + max_sort;
    const __amdgpu_buffer_rsrc_t G4 = make_rsrc(gout + (size_t)n * HW * C, (unsigned)HW * C * 4u);
    const __amdgpu_buffer_rsrc_t F4 = make_rsrc(fref + (size_t)n * HW * C, (unsigned)HW * C * 4u);
    const int row_bytes = C * 4;
    // keys[0 .. count) (padded to a multiple of four with INT_MAX) -> vals[rank] = index_of(position)
    auto rank_sort = [&](int count, auto index_of) {
        const int cnt4 = (count + 3) & ~3;
        for (int base = 0; base < count; base += kWave) {
            const int mine = (base + lane < count) ? keys[base + lane] : 0x7fffffff;
            int rank = 0;
            for (int j = 0; j < cnt4; j += 4) {
                const int4 kq = *reinterpret_cast<const int4 *>(&keys[j]);  // same address in every lane
                rank += (kq.x < mine) + (kq.y < mine) + (kq.z < mine) + (kq.w < mine);
            }
            if (base + lane < count) vals[rank] = index_of(base + lane);
        }
        __builtin_amdgcn_wave_barrier();
    };
    // entries index_of(0 .. count) of the row's CSR segment, in that order, onto the accumulators
    auto accumulate = [&](int count, auto index_of) {
        for (int e0 = 0; e0 < count; e0 += kWave) {
            const int m = min(kWave, count - e0);
            int pp = 0, ff = 0;
            float aa = 0.f, bb = 0.f;
            if (lane < m) {
                const int4 rec = csr[seg + index_of(e0 + lane)];
                pp = rec.x / cap;
                aa = __int_as_float(rec.y);
                bb = __int_as_float(rec.z);
                ff = rec.w;
            }
            for (int j = 0; j < m; ++j) {
                const int pj = __builtin_amdgcn_readlane(pp, j) * row_bytes;  // scalar row offset
                const float aj = lane_bcast(aa, j), bj = lane_bcast(bb, j);
                const int fj = __builtin_amdgcn_readlane(ff, j);              // (0 unless the pixel's row holds an Inf: emit kernel)
#pragma unroll
                for (int c = 0; c < CPL; ++c) {
                    if (mask & 2) acc[c] = f4_fma(aj, buf_load_f4(G4, voff[c] * 16, pj), acc[c]);
                    if (mask & 1) acc[c] = f4_fma(bj, buf_load_f4(F4, voff[c] * 16, pj), acc[c]);
                }
                if (fj != 0) {  // wave-uniform: terms of mixed sign times an infinite factor are NaN in the reference
                    auto nan_of_inf = [](float4 v) {
                        auto h = [](float x) { return fabsf(x) == __builtin_huge_valf() ? __builtin_nanf("") : 0.f; };
                        return make_float4(h(v.x), h(v.y), h(v.z), h(v.w));
                    };
                    auto f4_add = [](const float4 &a, const float4 &b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); };
#pragma unroll
                    for (int c = 0; c < CPL; ++c) {
                        if ((mask & 2) && (fj & 1)) acc[c] = f4_add(acc[c], nan_of_inf(buf_load_f4(G4, voff[c] * 16, pj)));
                        if ((mask & 1) && (fj & 2)) acc[c] = f4_add(acc[c], nan_of_inf(buf_load_f4(F4, voff[c] * 16, pj)));
                    }
                }
            }
        }
    };
    if (max_sort <= 0) {                       // ET_VARIANT_BWD_UNSORTED: arrival order
        accumulate(cnt, [&](int i) { return i; });
    } else if (cnt <= max_sort) {
        const int cnt4 = (cnt + 3) & ~3;
        for (int i = lane; i < cnt4; i += kWave) keys[i] = (i < cnt) ? csr[seg + i].x : 0x7fffffff;
        __builtin_amdgcn_wave_barrier();
        rank_sort(cnt, [&](int i) { return i; });
        accumulate(cnt, [&](int i) { return vals[i]; });
    } else {
        // More entries than the LDS sort holds -- a source pixel next to an epipole INSIDE the map, which every epipolar
        // line of the pair passes (thousands of entries; the ring rig's rows have ~140).  Rounds 1-4 summed such a row in
        // arrival order: not reproducible, found by the epipole-inside fixtures of round 5.  Same fixed order here, range by
        // range of the key: scan the row's entries, collect those with klo <= key < khi (at most half the LDS arrays: the
        // other half of `keys` holds their positions), rank-sort, accumulate, next range; a range that holds too many is
        // halved (keys are unique: a range of one key always fits), a sparse one lets the next grow.
        const int half = max_sort >> 1;
        int *pos = keys + half;
        const long long kend = (long long)HW * cap;      // (< 2^31: checked by the host wrapper)
        long long klo = 0;
        long long span = kend * (half / 2) / cnt;
        if (span < 1) span = 1;
        while (klo < kend) {
            const long long khi = (klo + span < kend) ? klo + span : kend;
            int got = 0;
            bool over = false;
            for (int e0 = 0; e0 < cnt; e0 += kWave) {
                const int i = e0 + lane;
                const int key = (i < cnt) ? csr[seg + i].x : -1;
                const bool in = key >= klo && key < khi;
                const unsigned long long bal = __builtin_amdgcn_ballot_w64(in);
                const int nin = __popcll(bal);
                if (got + nin > half) {
                    over = true;
                    break;
                }
                if (in) {
                    const int at = got + __popcll(bal & ((1ull << lane) - 1ull));
                    keys[at] = key;
                    pos[at] = i;
                }
                got += nin;
            }
            if (over) {
                span = (span + 1) >> 1;
                continue;
            }
            if (got > 0) {
                if (lane < ((got + 3) & ~3) - got) keys[got + lane] = 0x7fffffff;
                __builtin_amdgcn_wave_barrier();
                rank_sort(got, [&](int i) { return pos[i]; });
                accumulate(got, [&](int i) { return vals[i]; });
                __builtin_amdgcn_wave_barrier();
            }
            klo = khi;
            if (got < half / 4) span *= 2;
        }
    }
    float4 *o4 = reinterpret_cast<float4 *>(gsrc) + (size_t)gu * nvec;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int v = lane + c * kWave;
        if (v < nvec) o4[v] = acc[c];
    }
}

