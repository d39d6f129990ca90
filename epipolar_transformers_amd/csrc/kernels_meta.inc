// ----------------------------------------------------------------------------
// The Meta fusion layer (modeling/layers/meta.py:27-50 + the hourglass caller's `ret + feat`, ProHG.py:219-220,239) for C = 256:
//
//     x[n, m, :] = [feat[n, m, :] +] [bias +] src[n, m, :] . W_n^T,        W_n = weight[n] + share        (pair n, row m < HW)
//
// -- the reference's loop of N conv2d calls, the shared 1x1 convolution and two adds (four passes over N HW 256 floats) as one.  It is
// residual_gemm_kernel's GEMM (kernels_residual_gemm.inc, included in front of this file: its constants, fragment layout, stage and
// scale are used as they stand) with ONE difference: the B operand changes with the pair.  So
//   * meta_pack_kernel lays W_n (or W_n^T, for d src = g . W_n) out per pair, each pair under a scale from ITS OWN largest magnitude;
//   * meta_gemm_kernel takes its 64-row tiles PER PAIR -- ceil(HW / 64) each, none spans two pairs: a block reads one pack (256 KB,
//     from L2), and what a pair's rows come out as does not depend on where the pair sits in a batch.  The last tile of a pair is cut
//     by its buffer resources: rows at or beyond HW load as zeros and their stores are dropped;
//   * meta_wgrad_kernel is z_wgrad_bf16x3_kernel's contraction over rows (three bf16 terms per value) per pair:
//     grad_w[n] = g[n]^T . src[n], a pair's rows split over a number of blocks that depends on HW alone, partials summed in a fixed
//     order by meta_wgrad_finish_kernel (which also sums the bias gradient over every block of the call).
// No atomics anywhere: the same inputs give the same bits, and a pair's rows of x / d src / grad_w are the same bits alone or in a batch.
// ----------------------------------------------------------------------------

constexpr int kMetaPackWords = kRgPackedWords + 64;      // uint32 words per pair: et_residual_gemm_packed_bytes() / 4
constexpr int kMetaWgRowsPerBlock = 2048;                // rows of a pair one weight-gradient block contracts, at the most

// grid = N * kRgPackBlocks blocks of 1024 threads: as residual_gemm_pack_kernel, every block finds the largest magnitude of its pair's
// sum for itself and packs its share of the pair's 8192 fragments.
__global__ __launch_bounds__(1024) void meta_pack_kernel(const float *__restrict__ weight, const float *__restrict__ share, int transpose,
                                                         unsigned *__restrict__ packed)
{
    __shared__ float s_red[16];
    __shared__ float s_sc[2];
    const int n = blockIdx.x / kRgPackBlocks, part = blockIdx.x % kRgPackBlocks;
    const float *w = weight + (size_t)n * 65536;
    unsigned *out = packed + (size_t)n * kMetaPackWords;
    float m = 0.f;
    if (((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(share)) & 15) == 0) {
        for (int i = threadIdx.x; i < 65536 / 4; i += 1024) {
            float4 v = reinterpret_cast<const float4 *>(w)[i];
            if (share) {
                const float4 s = reinterpret_cast<const float4 *>(share)[i];
                v.x += s.x; v.y += s.y; v.z += s.z; v.w += s.w;
            }
            m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
        }
    } else {                                  // (views at an odd offset)
        for (int i = threadIdx.x; i < 65536; i += 1024) m = fmaxf(m, fabsf(w[i] + (share ? share[i] : 0.f)));
    }
    m = wave_all_max(m);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float mx = 0.f;
        for (int k = 0; k < 16; ++k) mx = fmaxf(mx, s_red[k]);
        float sc = 1.f, inv = 1.f;
        if (mx > 0.f && mx < 3e38f) rg_scale_of(mx, sc, inv);
        s_sc[0] = sc;
        s_sc[1] = inv;
        if (part == 0) reinterpret_cast<float *>(out)[kRgPackedWords] = inv;
    }
    __syncthreads();
    const float sc = s_sc[0];
    // fragment (ks, nb, term, lane): B[k][o] = W_n[o][k] (transpose: W_n[k][o]), lane (o = 32 nb + (lane & 31), kg = lane >> 5) holds
    // k = 16 ks + 8 kg .. + 7
    for (int f = part * 1024 + threadIdx.x; f < 16 * 8 * 64; f += kRgPackBlocks * 1024) {
        const int lane = f & 63, nb = (f >> 6) & 7, ks = f >> 9;
        const int o = nb * 32 + (lane & 31), k0 = ks * 16 + (lane >> 5) * 8;
        rg_f16x8 hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int at = transpose ? (k0 + j) * 256 + o : o * 256 + k0 + j;
            const float v = (w[at] + (share ? share[at] : 0.f)) * sc;
            const float h = __uint_as_float(__float_as_uint(v) & 0xFFFFE000u);
            hi[j] = (_Float16)h;
            lo[j] = (_Float16)(v - h);
        }
        rg_f16x8 *dst = reinterpret_cast<rg_f16x8 *>(out) + ((size_t)(ks * 8 + nb) * 2) * 64 + lane;
        dst[0] = hi;
        dst[64] = lo;
    }
}

// One block = one 64-row tile of one pair, 4 waves, two blocks per CU: the stage / MFMA / epilogue phases of residual_gemm_kernel.
// Blocks are numbered so that each XCD walks whole pairs (its L2 keeps the pack of the pair it is working on).
template <bool HAS_FEAT>
__global__ __launch_bounds__(256, 2) void meta_gemm_kernel(const float *__restrict__ src, const float *__restrict__ feat,
                                                           const unsigned *__restrict__ packed, const float *__restrict__ bias,
                                                           float *__restrict__ x, int HW, int tiles_per_pair)
{
    extern __shared__ char s_rg[];
    char *s_hi = s_rg;
    char *s_lo = s_rg + kRgRows * kRgStageRow;
    float *s_unscale = reinterpret_cast<float *>(s_rg + 2 * kRgRows * kRgStageRow);
    float *s_out = reinterpret_cast<float *>(s_rg);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int blk = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int pair = blk / tiles_per_pair, tile = blk - pair * tiles_per_pair;
    const long long row0 = (long long)pair * HW + (long long)tile * kRgRows;
    const unsigned nrows = (unsigned)min(kRgRows, HW - tile * kRgRows);          // (>= 1: tiles_per_pair = ceil(HW / 64))
    const unsigned span = nrows * 1024u;                                         // rows at or beyond HW: outside every resource
    const __amdgpu_buffer_rsrc_t r_src = make_rsrc(src + row0 * 256, span);
    const __amdgpu_buffer_rsrc_t r_feat = make_rsrc(HAS_FEAT ? feat + row0 * 256 : src, HAS_FEAT ? span : 0u);
    const __amdgpu_buffer_rsrc_t r_x = make_rsrc(x + row0 * 256, span);
    const unsigned *pack = packed + (size_t)pair * kMetaPackWords;
    const __amdgpu_buffer_rsrc_t r_w = make_rsrc(pack, (unsigned)kRgPackedWords * 4u);
    const float inv_w = reinterpret_cast<const float *>(pack)[kRgPackedWords];

    // ---- stage: rows 16 wave .. + 15 of the tile (rows past the pair's end: zeros) ----
    float4 fr[16];     // the feat rows the epilogue adds: requested right behind the src rows, used behind the MFMA loop
    {
        float4 a[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = buf_load_f4_nt(r_src, (wave * 16 + r) * 1024 + lane * 16, 0);
        if (HAS_FEAT) {
#pragma unroll
            for (int r = 0; r < 16; ++r) fr[r] = buf_load_f4_nt(r_feat, (wave * 16 + r) * 1024 + lane * 16, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += 4) {
            float m[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                m[j] = fmaxf(fmaxf(fabsf(a[r0 + j].x), fabsf(a[r0 + j].y)), fmaxf(fabsf(a[r0 + j].z), fabsf(a[r0 + j].w)));
            wave_all_max4(m);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = wave * 16 + r0 + j;
                float sc, inv;
                rg_scale_of(m[j], sc, inv);
                const float v[4] = {a[r0 + j].x * sc, a[r0 + j].y * sc, a[r0 + j].z * sc, a[r0 + j].w * sc};
                rg_f16x4 hi, lo;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float h = __uint_as_float(__float_as_uint(v[c]) & 0xFFFFE000u);
                    hi[c] = (_Float16)h;
                    lo[c] = (_Float16)(v[c] - h);
                }
                *reinterpret_cast<rg_f16x4 *>(s_hi + row * kRgStageRow + lane * 8) = hi;
                *reinterpret_cast<rg_f16x4 *>(s_lo + row * kRgStageRow + lane * 8) = lo;
                if (lane == 0) s_unscale[row] = inv * inv_w;
            }
        }
    }
    const float4 b4 = bias ? *reinterpret_cast<const float4 *>(bias + lane * 4) : f4_zero();
    __syncthreads();

    // ---- MFMA: all 64 rows x channels 64 wave .. + 63, B fragments of THIS pair straight from L2 ----
    rg_f32x16 acc[2][2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t >> 1][t & 1][r] = 0.f;
    constexpr int kRing = 3;
    u32x4 bq[kRing][4];      // [k-step mod kRing][2 nb + term]
    const int woff = (wave * 2) * 2 * 1024 + lane * 16;     // fragment (ks, nb = 2 wave, hi) of this lane, bytes
    auto wload = [&](int ks, u32x4 (&dst)[4]) {
#pragma unroll
        for (int t = 0; t < 4; ++t) dst[t] = __builtin_amdgcn_raw_buffer_load_b128(r_w, woff + ks * 8 * 2 * 1024 + t * 1024, 0, 0);
    };
#pragma unroll
    for (int ks = 0; ks < kRing; ++ks) wload(ks, bq[ks]);
    const char *ahp = s_hi + li * kRgStageRow + lh * 16, *alp = s_lo + li * kRgStageRow + lh * 16;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
        rg_f16x8 ahi[2], alo[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            ahi[mt] = *reinterpret_cast<const rg_f16x8 *>(ahp + mt * 32 * kRgStageRow + ks * 32);
            alo[mt] = *reinterpret_cast<const rg_f16x8 *>(alp + mt * 32 * kRgStageRow + ks * 32);
        }
        u32x4(&bb)[4] = bq[ks % kRing];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const rg_f16x8 bhi = __builtin_bit_cast(rg_f16x8, bb[2 * nb]);
            const rg_f16x8 blo = __builtin_bit_cast(rg_f16x8, bb[2 * nb + 1]);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                acc[mt][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo[mt], bhi, acc[mt][nb], 0, 0, 0);
                acc[mt][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi[mt], blo, acc[mt][nb], 0, 0, 0);
                acc[mt][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi[mt], bhi, acc[mt][nb], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (ks + kRing < 16) wload(ks + kRing, bq[ks % kRing]);
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();      // every wave is done with the stage

    // ---- epilogue: accumulators -> LDS (row-major), then whole rows ----
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                s_out[m * kRgOutStride + wave * 64 + nb * 32 + li] = acc[mt][nb][r] * s_unscale[m];
            }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = wave * 16 + r;
        float4 v = *reinterpret_cast<const float4 *>(s_out + row * kRgOutStride + lane * 4);
        v.x += b4.x; v.y += b4.y; v.z += b4.z; v.w += b4.w;
        if (HAS_FEAT) { v.x += fr[r].x; v.y += fr[r].y; v.z += fr[r].z; v.w += fr[r].w; }
        const u32x4 o = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
        __builtin_amdgcn_raw_buffer_store_b128(o, r_x, row * 1024 + lane * 16, 0, 2);      // (streaming; rows past the pair's end: dropped)
    }
}

// grad_w[n] = g[n]^T . src[n]: z_wgrad_bf16x3_kernel's step (16 rows, three bf16 terms per value, the six cross terms, two stages)
// with a block's rows taken from ONE pair -- block (pair, part) owns rows part * rows_per_block .. of the pair's HW and the whole
// 256 x 256 partial result; the dy threads' running sums are the bias gradient's partials.
__global__ __launch_bounds__(512, 1) void meta_wgrad_kernel(const float *__restrict__ g, const float *__restrict__ src, int HW,
                                                            int blocks_per_pair, int rows_per_block, float *__restrict__ partial_w,
                                                            float *__restrict__ partial_b)
{
    extern __shared__ char s_wgb[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int pair = blockIdx.x / blocks_per_pair, part = blockIdx.x - pair * blocks_per_pair;
    const long long row0 = (long long)pair * HW + (long long)part * rows_per_block;
    const int nrows = max(0, min(rows_per_block, HW - part * rows_per_block));
    const unsigned bytes = (unsigned)nrows * 1024u;
    const int steps = (nrows + kWgRows - 1) / kWgRows;
    // staging role: operand `sop` (0: g, 1: src), channel `sch`
    const int sop = __builtin_amdgcn_readfirstlane(tid >> 8), sch = tid & 255;
    const __amdgpu_buffer_rsrc_t r_in = make_rsrc((sop ? src : g) + row0 * 256, bytes);
    char *s_mine = s_wgb + sop * 3 * kWgbTerm + sch * kWgbChan;
    float ld[kWgRows];
    auto load = [&](int k) {
#pragma unroll
        for (int r = 0; r < kWgRows; ++r) ld[r] = buf_load_f1_nt(r_in, (k * kWgRows + r) * 1024 + sch * 4, 0);   // (rows past the end: zeros)
    };
    float bsum = 0.f;
    auto store = [&](int stage) {
        char *s_to = s_mine + stage * kWgbStage;
        unsigned t1[kWgRows / 2], t2[kWgRows / 2], t3[kWgRows / 2];
#pragma unroll
        for (int r = 0; r < kWgRows; r += 2) {
            unsigned hi[2][3];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float v = ld[r + e];
                bsum += v;                                                          // (the g threads': the bias gradient, rows in order)
                const unsigned u1 = __float_as_uint(v) & 0xFFFF0000u;
                const float r1 = v - __uint_as_float(u1);
                const unsigned u2 = __float_as_uint(r1) & 0xFFFF0000u;
                const float r2 = r1 - __uint_as_float(u2);
                hi[e][0] = u1;
                hi[e][1] = u2;
                hi[e][2] = __float_as_uint(r2);                                     // (its upper half: truncated)
            }
            // rows r (low half) and r + 1 (high half) of one dword
            t1[r / 2] = __builtin_amdgcn_perm(hi[1][0], hi[0][0], 0x07060302u);
            t2[r / 2] = __builtin_amdgcn_perm(hi[1][1], hi[0][1], 0x07060302u);
            t3[r / 2] = __builtin_amdgcn_perm(hi[1][2], hi[0][2], 0x07060302u);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<u32x4 *>(s_to + 0 * kWgbTerm + h * 16) = u32x4{t1[4 * h], t1[4 * h + 1], t1[4 * h + 2], t1[4 * h + 3]};
            *reinterpret_cast<u32x4 *>(s_to + 1 * kWgbTerm + h * 16) = u32x4{t2[4 * h], t2[4 * h + 1], t2[4 * h + 2], t2[4 * h + 3]};
            *reinterpret_cast<u32x4 *>(s_to + 2 * kWgbTerm + h * 16) = u32x4{t3[4 * h], t3[4 * h + 1], t3[4 * h + 2], t3[4 * h + 3]};
        }
    };
    rg_f32x16 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    if (steps > 0) {
        load(0);
        store(0);
    }
    __syncthreads();
    // A = g^T: lane (co = 32 wave + li, k-group lh); B = src: lane (ci = 32 t + li, k-group lh)
    const char *a_at = s_wgb + (wave * 32 + li) * kWgbChan + lh * 16;
    const char *b_at = s_wgb + 3 * kWgbTerm + li * kWgbChan + lh * 16;
    for (int k = 0; k < steps; ++k) {
        if (k + 1 < steps) load(k + 1);
        const char *ap = a_at + (k & 1) * kWgbStage;
        const wg_bf16x8 a1 = *reinterpret_cast<const wg_bf16x8 *>(ap), a2 = *reinterpret_cast<const wg_bf16x8 *>(ap + kWgbTerm);
        const wg_bf16x8 a3 = *reinterpret_cast<const wg_bf16x8 *>(ap + 2 * kWgbTerm);
#pragma unroll
        for (int t0 = 0; t0 < 8; t0 += 4) {
            wg_bf16x8 b1[4], b2[4], b3[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const char *bp = b_at + (k & 1) * kWgbStage + (t0 + u) * 32 * kWgbChan;
                b1[u] = *reinterpret_cast<const wg_bf16x8 *>(bp);
                b2[u] = *reinterpret_cast<const wg_bf16x8 *>(bp + kWgbTerm);
                b3[u] = *reinterpret_cast<const wg_bf16x8 *>(bp + 2 * kWgbTerm);
            }
            // (small terms first; four independent accumulators per term)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[t0 + u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b2[u], acc[t0 + u], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[t0 + u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b3[u], acc[t0 + u], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[t0 + u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, b1[u], acc[t0 + u], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[t0 + u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b2[u], acc[t0 + u], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[t0 + u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b1[u], acc[t0 + u], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[t0 + u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1[u], acc[t0 + u], 0, 0, 0);
        }
        // (the other stage was last read in step k - 1: every wave has passed that step's barrier)
        if (k + 1 < steps) store((k + 1) & 1);
        __syncthreads();
    }
    // accumulator t, register r  <->  co = 32 wave + (r & 3) + 8 (r >> 2) + 4 lh,  ci = 32 t + li
    float *pw = partial_w + (size_t)blockIdx.x * 65536;
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * lh;
            pw[co * 256 + 32 * t + li] = acc[t][r];
        }
    if (sop == 0) partial_b[(size_t)blockIdx.x * 256 + sch] = bsum;
}

// Blocks 0 .. 256 N - 1: element (blockIdx & 255) * 256 + thread of pair blockIdx >> 8 -- the pair's partials in part order.  Block
// 256 N (launched when the bias gradient is asked for): the bias partials of all N * blocks_per_pair blocks in block order, four
// running sums as z_wgrad_finish_kernel.
__global__ __launch_bounds__(256) void meta_wgrad_finish_kernel(const float *__restrict__ partial_w, const float *__restrict__ partial_b,
                                                                int N, int blocks_per_pair, float *__restrict__ grad_w,
                                                                float *__restrict__ grad_b)
{
    const int pair = blockIdx.x >> 8;
    if (pair < N) {
        const int idx = (blockIdx.x & 255) * 256 + threadIdx.x;
        const float *p = partial_w + (size_t)pair * blocks_per_pair * 65536 + idx;
        float s = p[0];
        for (int b = 1; b < blocks_per_pair; ++b) s += p[(size_t)b * 65536];
        grad_w[(size_t)pair * 65536 + idx] = s;
        return;
    }
    const long long blocks = (long long)N * blocks_per_pair;
    const float *p = partial_b + threadIdx.x;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    long long b = 0;
#pragma unroll 4
    for (; b + 4 <= blocks; b += 4) {
        s0 += p[(size_t)b * 256];
        s1 += p[(size_t)(b + 1) * 256];
        s2 += p[(size_t)(b + 2) * 256];
        s3 += p[(size_t)(b + 3) * 256];
    }
    for (; b < blocks; ++b) s0 += p[(size_t)b * 256];
    grad_b[threadIdx.x] = (s0 + s1) + (s2 + s3);
}
