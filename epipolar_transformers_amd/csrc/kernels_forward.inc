// Part of et_forward.hip (inside its anonymous namespace, after et_common.h / kernels_sample_table.inc /
// kernels_pixel_phases.inc): the fused forward kernels.  Not a stand-alone header.
// ----------------------------------------------------------------------------
// forward: fused epipolar sample + dot + masked softmax + weighted sum
// ----------------------------------------------------------------------------
// CPL: float4 channel groups per lane (C <= 256*CPL); KPL: samples per lane
// (K <= 64*KPL); RAGGED: the last batch of samples may be short, so batches
// carry per-sample validity logic.  Tuned on MI355X (profiles/r01_variant_sweep_last.json):
// cross-lane reductions per kBatch = 4 samples, and room for 5 waves per SIMD (<= 96 VGPRs).
constexpr int kBatch = 4;
template <int CPL, int KPL, bool RAGGED>
__global__ __launch_bounds__(kWave *kWavesPerBlock, 5) void epipolar_fwd_kernel(const FwdParams p)
{
    // dynamic LDS: [K][16] attention tile (only when attn is requested), then one
    // [KPL*64] float4 table of bilinear weights per wave
    extern __shared__ float s_dyn[];
    const EtLayerDesc &d = p.d;
    const int H = d.H, W = d.W, C = d.C, K = d.K;
    const int HW = H * W;
    const int nvec = C >> 2;  // float4 groups per pixel row

    const int vb = xcd_remap(blockIdx.x, p.total_blocks);
    const int n = vb / p.blocks_per_pair;
    const int pb = vb - n * p.blocks_per_pair;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pix_base = pb * kPixPerBlock;
    float *s_attn = s_dyn;
    float4 *s_wt = reinterpret_cast<float4 *>(s_dyn + (p.attn ? K * kPixPerBlock : 0)) + wave * (KPL * kWave);

    const float *cam = p.cam + (size_t)n * ET_CAM_STRIDE;
    const __amdgpu_buffer_rsrc_t src = make_rsrc(p.fsrc + (size_t)n * HW * C, (unsigned)HW * C * 4u);
    const int row_bytes = C * 4;
    const float neg_inf = -__builtin_huge_valf();
    // Lanes beyond C/4 (only when C < 256*CPL) point past the buffer: their loads return zeros (the range check of a raw
    // buffer looks at the vector offset alone, whatever row the scalar offset selects), their reference features are
    // zeroed and their results never stored, so the hot loop carries no per-lane predicate and stays on scalar branches.
    // (They used to re-read the last channel group: 0 x Inf = NaN then turned an infinite logit into a NaN.)
    constexpr int kOob = 0x7ffff000;
    int voff[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) voff[c] = (lane + c * kWave < nvec) ? (lane + c * kWave) * 16 : kOob;

    for (int pp = 0; pp < kPixPerWave; ++pp) {
        // pixels interleaved across the block's waves (wave w takes pixels w, w+4, ..), which keeps the
        // four waves on neighbouring epipolar lines at the same time (shared rows hit in the CU's L1)
        const int slot_in_block = pp * kWavesPerBlock + wave;
        const int pix = pix_base + slot_in_block;
        if (pix >= HW) break;  // wave-uniform
        const int h = pix / W, w = pix - h * W;

        // ---- lanes <-> samples: geometry and tap table ----------------------
        const et::Segment seg = et::epipolar_segment(d, cam, p.xs[w], p.ys[h]);
        SampleTable<KPL> tb;
        build_sample_table<KPL>(d, seg, p.steps, lane, row_bytes, tb);
        float v_sim[KPL];
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            v_sim[s] = neg_inf;
            // a sample's four weights come back as ONE broadcast ds_read_b128 (same address in
            // every lane) instead of four v_readlane
            s_wt[s * kWave + lane] = make_float4(tb.w[s][0], tb.w[s][1], tb.w[s][2], tb.w[s][3]);
        }
        __builtin_amdgcn_wave_barrier();

        // ---- lanes <-> channels -------------------------------------------
        float4 f1[CPL], acc[CPL], R[4][CPL];
        const float4 *ref = reinterpret_cast<const float4 *>(p.fref + ((size_t)n * HW + pix) * C);
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int v = lane + c * kWave;
            f1[c] = (v < nvec) ? ref[v] : f4_zero();
            acc[c] = f4_zero();
#pragma unroll
            for (int r = 0; r < 4; ++r) R[r][c] = f4_zero();
        }
        if (p.res_base) write_res_base<CPL, kWave>(p, (size_t)n * HW + pix, lane, nvec, f1);
        float m_run = neg_inf;

#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            const int kcount = min(kWave, K - s * kWave);  // samples held in this slot (uniform)
            for (int kb = 0; kb < kcount; kb += kBatch) {
                float4 S[kBatch][CPL];
                float part[kBatch];
#pragma unroll
                for (int j = 0; j < kBatch; ++j) {
                    const int kk = kb + j;
                    if (RAGGED) {
                        part[j] = 0.f;
#pragma unroll
                        for (int c = 0; c < CPL; ++c) S[j][c] = f4_zero();
                    }
                    // (the branch is kept even when it is always taken: per-sample basic blocks stop the
                    //  compiler from renaming the tap registers across samples, which costs ~100 VGPRs)
                    if (kk < kcount) {  // wave-uniform
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
                        const float w0 = wv.x, w1 = wv.y, w2 = wv.z, w3 = wv.w;
#pragma unroll
                        for (int c = 0; c < CPL; ++c) {
                            float4 sv = f4_mul(w0, R[0][c]);
                            sv = f4_fma(w1, R[1][c], sv);
                            sv = f4_fma(w2, R[2][c], sv);
                            sv = f4_fma(w3, R[3][c], sv);
                            S[j][c] = sv;
                            part[j] = (c == 0) ? f4_dot(sv, f1[c]) : part[j] + f4_dot(sv, f1[c]);
                        }
                    }
                }
                // four dot products -> 16-lane rows
                const float u = reduce4(part, lane);
                const bool jvalid = !RAGGED || (kb + sample_of_lane(lane)) < kcount;
                float sv = (u == 0.f) ? -1e10f : u;  // epipolar.py:298
                float e;
                if (d.softmax_enabled) {
                    sv = sv * d.softmax_scale;  // epipolar.py:306
                    const float bm = group_max(jvalid ? sv : neg_inf);
                    // (fmaxf drops a NaN logit from the running maximum; it is not lost: exp(NaN - m) below is NaN, and so
                    //  are the sum and every weight, as in torch's soft-max)
                    const float m_new = fmaxf(m_run, bm);
                    // accumulator weights only need ~1e-6 relative accuracy (the returned attention is
                    // recomputed with expf in the final pass): hardware exp2
                    const float alpha = __expf(m_run - m_new);
                    e = jvalid ? __expf(sv - m_new) : 0.f;
#pragma unroll
                    for (int c = 0; c < CPL; ++c) acc[c] = f4_mul(alpha, acc[c]);
                    m_run = m_new;
                } else {
                    sv = sv / (float)K;  // epipolar.py:311
                    e = jvalid ? sv : 0.f;
                }
                // keep the logit of sample (kb + j) in lane (kb + j) for the final pass
                const float mine = __shfl(sv, lane_of_sample<kBatch>(lane & (kBatch - 1)));
                if ((lane / kBatch) == (kb / kBatch)) v_sim[s] = mine;
#pragma unroll
                for (int j = 0; j < kBatch; ++j) {
                    const float ej = lane_bcast(e, lane_of_sample<kBatch>(j));
#pragma unroll
                    for (int c = 0; c < CPL; ++c) acc[c] = f4_fma(ej, S[j][c], acc[c]);
                }
            }
        }

        // ---- lanes <-> samples: exact soft-max, arg-max, outputs ------------
        float a[KPL];
        float denom = 1.f;
        if (d.softmax_enabled) {
            float lsum = 0.f;
#pragma unroll
            for (int s = 0; s < KPL; ++s) {
                const int k = s * kWave + lane;
                a[s] = (k < K) ? expf(v_sim[s] - m_run) : 0.f;  // m_run == max_k logit
                lsum += a[s];
            }
            denom = wave_sum(lsum);
#pragma unroll
            for (int s = 0; s < KPL; ++s) a[s] = a[s] / denom;
        } else {
#pragma unroll
            for (int s = 0; s < KPL; ++s) a[s] = v_sim[s];
        }
        const int besti = first_argmax<KPL>(a, K, lane);
        if (p.corr) {
            float bx = 0.f, by = 0.f;
#pragma unroll
            for (int s = 0; s < KPL; ++s) {
                const float tx = __shfl(tb.nx[s], besti & (kWave - 1));
                const float ty = __shfl(tb.ny[s], besti & (kWave - 1));
                if ((besti >> 6) == s) {
                    bx = tx;
                    by = ty;
                }
            }
            if (lane == 0) {
                float *o = p.corr + ((size_t)n * HW + pix) * 2;
                o[0] = et::de_normalize(d, bx, W);
                o[1] = et::de_normalize(d, by, H);
            }
        }
        if (p.attn) {
#pragma unroll
            for (int s = 0; s < KPL; ++s) {
                const int k = s * kWave + lane;
                if (k < K) s_attn[k * kPixPerBlock + slot_in_block] = a[s];
            }
        }
        float4 *o4 = reinterpret_cast<float4 *>(p.out + ((size_t)n * HW + pix) * C);
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int v = lane + c * kWave;
            float4 r = acc[c];
            if (d.softmax_enabled) r = make_float4(r.x / denom, r.y / denom, r.z / denom, r.w / denom);
            if (v < nvec) o4[v] = r;
        }
    }

    if (p.attn) store_attn_tile(p, s_attn, n, pix_base);
}

// ----------------------------------------------------------------------------
// forward, four pixels per wave ("multi", C == 256): PPW = 4 neighbouring pixels advance
// in lockstep, LPP = 16 lanes each, CQ = 4 float4 channel groups per lane.
// ----------------------------------------------------------------------------
// Why: in the one-pixel-per-wave kernel only ~13 of ~36 VALU instructions per sample
// are arithmetic; the rest is per-sample bookkeeping (lane broadcasts, 64-lane
// reductions, soft-max updates) that here is issued once per step for PPW pixels:
// the per-step record (tap offsets, weights, need bits) is read from LDS by each
// lane group, tap loads are exec-masked per group, the dot product reduces over
// LPP lanes only, and the online soft-max runs one sample per step (no batching).
// Requires C == 4 * LPP * CQ == 256 exactly, and K <= 64 (one sample slot per lane).
__global__ __launch_bounds__(kWave *kWavesPerBlock) void epipolar_fwd_multi_kernel(const FwdParams p)
{
    constexpr int PPW = 4, CQ = 4, KPL = 1;
    constexpr int LPP = kWave / PPW;
    constexpr int ROUNDS = kPixPerWave / PPW;
    constexpr int KP = KPL * kWave;  // padded samples per pixel
    extern __shared__ float s_dyn[];
    const EtLayerDesc &d = p.d;
    const int H = d.H, W = d.W, C = d.C, K = d.K;
    const int HW = H * W;

    const int vb = xcd_remap(blockIdx.x, p.total_blocks);
    const int n = vb / p.blocks_per_pair;
    const int pb = vb - n * p.blocks_per_pair;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pix_base = pb * kPixPerBlock;
    const int g = lane / LPP, li = lane % LPP;

    // LDS carve-up: attention tile, then per wave 32-byte records {tap offsets | need bits, weights} and the
    // segments.  Row offsets are multiples of 16, so the four need bits ride in the low bits of the first
    // offset; a step's logit overwrites its (consumed) first weight -- 37 KB per block = 4 blocks per CU.
    float *s_attn = s_dyn;
    char *wbase = reinterpret_cast<char *>(s_dyn + (p.attn ? K * kPixPerBlock : 0)) +
                  (size_t)wave * (PPW * KP * 32 + PPW * 16);
    int4 *s_off = reinterpret_cast<int4 *>(wbase);                       // [PPW][KP]
    float4 *s_wt = reinterpret_cast<float4 *>(wbase + PPW * KP * 16);    // [PPW][KP]
    float4 *s_seg = reinterpret_cast<float4 *>(wbase + PPW * KP * 32);   // [PPW]

    const float *cam = p.cam + (size_t)n * ET_CAM_STRIDE;
    const __amdgpu_buffer_rsrc_t src = make_rsrc(p.fsrc + (size_t)n * HW * C, (unsigned)HW * C * 4u);
    const int row_bytes = C * 4;
    const float neg_inf = -__builtin_huge_valf();
    const int lane_off = li * 16;  // + c * LPP * 16 as the instruction's immediate offset

    for (int round = 0; round < ROUNDS; ++round) {
        const int first = pix_base + wave * kPixPerWave + round * PPW;  // first pixel of this wave's group
        if (first >= HW) break;                                         // wave-uniform
        // ---- the PPW epipolar segments at once: lane group g evaluates pixel g's ------------
        {
            const int pixg = min(first + g, HW - 1);
            const int hg = pixg / W, wg = pixg - hg * W;
            const et::Segment sg = et::epipolar_segment(d, cam, p.xs[wg], p.ys[hg]);
            if (li == 0) s_seg[g] = make_float4(sg.sx, sg.sy, sg.vx, sg.vy);
        }
        __builtin_amdgcn_wave_barrier();
        // ---- lanes <-> samples, one pixel after the other: records into LDS ----
#pragma unroll
        for (int gg = 0; gg < PPW; ++gg) {
            const bool live = first + gg < HW;
            const float4 sq = s_seg[gg];
            et::Segment seg;
            seg.sx = sq.x; seg.sy = sq.y; seg.vx = sq.z; seg.vy = sq.w;
            SampleTable<KPL> tb;
            build_sample_table<KPL>(d, seg, p.steps, lane, row_bytes, tb);
#pragma unroll
            for (int s = 0; s < KPL; ++s) {
                const int k = s * kWave + lane;
                // an absent tap (-1) points past the buffer: when the step needs it (the register held a row before) the
                // load returns zeros, so a stale row never meets its weight 0 (0 x NaN)
                constexpr int kAbsent = 0x7ffff000;
                auto offv = [&](int r) { return tb.off[s][r] < 0 ? kAbsent : tb.off[s][r]; };
                s_off[gg * KP + k] = make_int4((offv(0) & ~15) | (live ? tb.need[s] : 0), offv(1), offv(2), offv(3));
                s_wt[gg * KP + k] = make_float4(tb.w[s][0], tb.w[s][1], tb.w[s][2], tb.w[s][3]);
            }
        }
        __builtin_amdgcn_wave_barrier();

        // ---- lanes <-> (pixel, channels) ------------------------------------------
        const int mypix = first + g;
        const bool mylive = mypix < HW;
        float4 f1[CQ], acc[CQ], R[4][CQ];
        const float4 *ref = reinterpret_cast<const float4 *>(p.fref + ((size_t)n * HW + (mylive ? mypix : 0)) * C);
#pragma unroll
        for (int c = 0; c < CQ; ++c) {
            f1[c] = mylive ? ref[c * LPP + li] : f4_zero();
            acc[c] = f4_zero();
#pragma unroll
            for (int r = 0; r < 4; ++r) R[r][c] = f4_zero();
        }
        if (p.res_base && mylive) write_res_base<CQ, LPP>(p, (size_t)n * HW + mypix, li, LPP * CQ, f1);
        float m_run = neg_inf;
        const int rec0 = g * KP;

        // request (exec-masked per lane group) the tap rows step k does not have yet
        auto issue_step = [&](int k) {
            int4 off = s_off[rec0 + k];
            const int need = off.x & 15;
            off.x &= ~15;
            if (need & 1) {
#pragma unroll
                for (int c = 0; c < CQ; ++c) R[0][c] = buf_load_f4(src, off.x + lane_off, c * LPP * 16);
            }
            if (need & 2) {
#pragma unroll
                for (int c = 0; c < CQ; ++c) R[1][c] = buf_load_f4(src, off.y + lane_off, c * LPP * 16);
            }
            if (need & 4) {
#pragma unroll
                for (int c = 0; c < CQ; ++c) R[2][c] = buf_load_f4(src, off.z + lane_off, c * LPP * 16);
            }
            if (need & 8) {
#pragma unroll
                for (int c = 0; c < CQ; ++c) R[3][c] = buf_load_f4(src, off.w + lane_off, c * LPP * 16);
            }
        };
        for (int k = 0; k < K; ++k) {
            issue_step(k);
            const float4 wv = s_wt[rec0 + k];
            float4 S[CQ];
            float part = 0.f;
#pragma unroll
            for (int c = 0; c < CQ; ++c) {
                float4 sv = f4_mul(wv.x, R[0][c]);
                sv = f4_fma(wv.y, R[1][c], sv);
                sv = f4_fma(wv.z, R[2][c], sv);
                sv = f4_fma(wv.w, R[3][c], sv);
                S[c] = sv;
            }
#pragma unroll
            for (int c = 0; c < CQ; ++c) part = (c == 0) ? f4_dot(S[c], f1[c]) : part + f4_dot(S[c], f1[c]);
            // all-reduce over the LPP lanes of the pixel
            part += dpp<0x128>(part);  // row_ror:8
            part += dpp<0x124>(part);  // row_ror:4
            part += dpp<0x122>(part);  // row_ror:2
            part += dpp<0x121>(part);  // row_ror:1
            float sv = (part == 0.f) ? -1e10f : part;  // epipolar.py:298
            float e;
            if (d.softmax_enabled) {
                sv = sv * d.softmax_scale;  // epipolar.py:306
                const float m_new = fmaxf(m_run, sv);
                // rescale every step (alpha == 1 when the maximum did not move): a voted lazy rescale
                // costs more in branch + register copies than these 2*CQ packed multiplies
                const float alpha = __expf(m_run - m_new);
#pragma unroll
                for (int c = 0; c < CQ; ++c) acc[c] = f4_mul(alpha, acc[c]);
                m_run = m_new;
                e = __expf(sv - m_new);
            } else {
                sv = sv / (float)K;  // epipolar.py:311
                e = sv;
            }
            reinterpret_cast<float *>(&s_wt[rec0 + k])[0] = sv;  // the step's weights are consumed: keep its logit there
#pragma unroll
            for (int c = 0; c < CQ; ++c) acc[c] = f4_fma(e, S[c], acc[c]);
        }
        __builtin_amdgcn_wave_barrier();

        // ---- lanes <-> samples per pixel: exact soft-max, arg-max, outputs ----------
        float my_scale = 1.f;
#pragma unroll
        for (int gg = 0; gg < PPW; ++gg) {
            const int pix = first + gg;
            if (pix >= HW) break;  // wave-uniform
            const float m_g = lane_bcast(m_run, gg * LPP);
            float a[KPL];
            float denom = 1.f;
            if (d.softmax_enabled) {
                float lsum = 0.f;
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    const int k = s * kWave + lane;
                    a[s] = (k < K) ? expf(s_wt[gg * KP + k].x - m_g) : 0.f;
                    lsum += a[s];
                }
                denom = wave_sum(lsum);
#pragma unroll
                for (int s = 0; s < KPL; ++s) a[s] = a[s] / denom;
                if (g == gg) my_scale = 1.f / denom;
            } else {
#pragma unroll
                for (int s = 0; s < KPL; ++s) a[s] = (s * kWave + lane < K) ? s_wt[gg * KP + s * kWave + lane].x : 0.f;
            }
            const int besti = first_argmax<KPL>(a, K, lane);
            if (p.corr && lane == 0) {
                const float4 sg = s_seg[gg];
                et::Segment seg;
                seg.sx = sg.x; seg.sy = sg.y; seg.vx = sg.z; seg.vy = sg.w;
                const et::SampleSetup su = et::sample_setup(d, seg, p.steps[besti]);
                float *o = p.corr + ((size_t)n * HW + pix) * 2;
                o[0] = et::de_normalize(d, su.nx, W);
                o[1] = et::de_normalize(d, su.ny, H);
            }
            if (p.attn) {
                const int slot_in_block = wave * kPixPerWave + round * PPW + gg;
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    const int k = s * kWave + lane;
                    if (k < K) s_attn[k * kPixPerBlock + slot_in_block] = a[s];
                }
            }
        }
        if (mylive) {
            float4 *o4 = reinterpret_cast<float4 *>(p.out + ((size_t)n * HW + mypix) * C);
#pragma unroll
            for (int c = 0; c < CQ; ++c) o4[c * LPP + li] = f4_mul(my_scale, acc[c]);
        }
        __builtin_amdgcn_wave_barrier();
    }

    if (p.attn) store_attn_tile(p, s_attn, n, pix_base);
}

