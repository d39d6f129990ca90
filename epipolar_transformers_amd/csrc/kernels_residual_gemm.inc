// ----------------------------------------------------------------------------
// The eval-mode residual fusion as one hand-written GEMM (C = 256):
//
//     x[m, :] = [feat[m, :] +] bias + out[m, :] . Wf^T            (epipolar.py:250-253 folded, resnet.py:388)
//
// M = N H W rows of 1 KB, Wf 256 x 256.  The arithmetic (68.7 GFLOP at Config 2) is small next to the traffic --
// out and feat read once, x written once: 1.6 GB -- so the kernel is laid out for HBM, and the products run as
// split-fp16 MFMAs (x s = hi + lo in fp16, hi lo' + lo hi' + hi hi' accumulated in fp32: fp32-level error at a
// third of the fp32 matrix time, see kernels_forward_tile_ws.inc) so the matrix pipe is never the limit.
//
//   * One block = 64 rows, 4 waves, two blocks per CU (67.6 KB of LDS each): the load / MFMA / store phases of the
//     two overlap.
//   * Stage: wave w reads rows 16 w .. 16 w + 15 (a lane = four channels: whole 1 KB rows per instruction), scales
//     every row by a power of two of its own (largest magnitude -> [2^10, 2^11): no estimate, no overflow), splits
//     and writes the fp16 hi / lo tiles to LDS in A-fragment order.
//   * MFMA: wave w owns output channels 64 w .. 64 w + 63 of all 64 rows (2 x 2 accumulators of
//     v_mfma_f32_32x32x16_f16).  The B operand -- Wf split and laid out fragment by fragment by
//     residual_gemm_pack_kernel, 1 KB contiguous per instruction -- comes straight from L2: 64 KB per wave.
//   * Epilogue: the accumulators go through the (now dead) stage so that a lane again owns four channels of a
//     row: + bias, + the feat row (loaded before the MFMA loop), whole-row stores.
// ----------------------------------------------------------------------------

constexpr int kRgRows = 64;                 // rows per block
constexpr int kRgStageRow = 528;            // bytes per row of an fp16 stage (512 + 16: conflict-free b128 fragment reads)
constexpr int kRgOutStride = 260;           // floats per row of the epilogue array
// (kRgPackedWords, the size of the packed weight [k-step][n-block][hi|lo][lane][16 B], lives in et_common.h)
constexpr size_t kRgLdsBytes = (size_t)2 * kRgRows * kRgStageRow + kRgRows * 4;
static_assert((size_t)kRgRows * kRgOutStride * 4 <= (size_t)2 * kRgRows * kRgStageRow, "the epilogue array reuses the stage");

typedef _Float16 rg_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 rg_f16x4 __attribute__((ext_vector_type(4)));
typedef float rg_f32x16 __attribute__((ext_vector_type(16)));

// power of two that puts a value of biased exponent E (1 .. 254) into [2^10, 2^11), and its inverse
__device__ __forceinline__ void rg_scale_of(float mx, float &sc, float &inv)
{
    int E = (int)((__float_as_uint(mx) >> 23) & 255u);
    E = min(max(E, 12), 250);
    sc = __uint_as_float((unsigned)(264 - E) << 23);      // 2^(137 - E)
    inv = __uint_as_float((unsigned)(E - 10) << 23);      // 2^(E - 137)
}

// Wf (256 out x 256 in, row-major) -> fragments.  kRgPackBlocks blocks of 1024 threads: every block finds the weight's largest
// magnitude for itself (256 KB from L2) and packs its share of the 8192 fragments -- the training step packs two weights per step,
// and one block took 25 us for each.
constexpr int kRgPackBlocks = 8;
__global__ __launch_bounds__(1024) void residual_gemm_pack_kernel(const float *__restrict__ wf, unsigned *__restrict__ packed)
{
    __shared__ float s_red[16];
    __shared__ float s_sc[2];
    float m = 0.f;
    if ((reinterpret_cast<uintptr_t>(wf) & 15) == 0) {
        for (int i = threadIdx.x; i < 256 * 256 / 4; i += 1024) {
            const float4 v = reinterpret_cast<const float4 *>(wf)[i];
            m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
        }
    } else {                                  // (a weight that is a view at an odd offset)
        for (int i = threadIdx.x; i < 256 * 256; i += 1024) m = fmaxf(m, fabsf(wf[i]));
    }
    m = wave_all_max(m);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float mx = 0.f;
        for (int w = 0; w < 16; ++w) mx = fmaxf(mx, s_red[w]);
        float sc = 1.f, inv = 1.f;
        if (mx > 0.f && mx < 3e38f) rg_scale_of(mx, sc, inv);
        s_sc[0] = sc;
        s_sc[1] = inv;
        if (blockIdx.x == 0) reinterpret_cast<float *>(packed)[kRgPackedWords] = inv;
    }
    __syncthreads();
    const float sc = s_sc[0];
    // fragment (ks, nb, term, lane): B[k][n] = Wf[n][k], lane (n = lane & 31, kg = lane >> 5) holds k = 16 ks + 8 kg .. + 7
    for (int f = blockIdx.x * 1024 + threadIdx.x; f < 16 * 8 * 64; f += gridDim.x * 1024) {
        const int lane = f & 63, nb = (f >> 6) & 7, ks = f >> 9;
        const float *src = wf + (size_t)(nb * 32 + (lane & 31)) * 256 + ks * 16 + (lane >> 5) * 8;
        rg_f16x8 hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = src[j] * sc;
            const float h = __uint_as_float(__float_as_uint(v) & 0xFFFFE000u);
            hi[j] = (_Float16)h;
            lo[j] = (_Float16)(v - h);
        }
        rg_f16x8 *dst = reinterpret_cast<rg_f16x8 *>(packed) + ((size_t)(ks * 8 + nb) * 2) * 64 + lane;
        dst[0] = hi;
        dst[64] = lo;
    }
}

// STATS = true is the first pass of the TRAINING-mode epilogue (batch statistics, modeling/layers/BN.py:59-82 with
// training = True): the same GEMM with the RAW z weight, y = out . Wz^T + bz written out (the batch norm's input: autograd
// keeps it, as it does in the reference) and, per block, the mean and the centred sum of squares of its 64 rows per channel
// -- partial[block][0 | 1][256], merged by z_stats_finish_kernel with Chan's update.  (One-pass sums of y and y^2 would
// cancel: a channel of z(out) can vary by 6e-3 around 0.2.)  The second pass is this kernel again, STATS = false, with
// the statistics folded into the weight (Epipolar._train_epilogue).
// DY = true is the BACKWARD of that epilogue w.r.t. `out` (z_bwd_*): the A rows are not read but formed on the fly,
//     dy = ca g + cb (y - mean) + cc        (the batch norm's input gradient, per-channel coefficients from z_bwd_finish_kernel)
// from the rows of g = d loss / d x (`feat` pointer) and of the saved y (`out` pointer), written out on request (the weight
// gradient dy^T out is a library GEMM), and the product runs against the TRANSPOSED z weight:  x = dy . Wz  [+ g: ZRESIDUAL].
// LIST = true (round 6) is the same GEMM over the pixel rows of a LIST of tiles: the x rows of the tiles the fused persistent forward
// left to the one-block-per-tile kernel (et_forward_tile.hip).  A block takes two tiles of the list at a time (64 rows, found through
// `perm`; padding pixels and a missing second tile are rows past the buffers: loaded as zeros, stores dropped).
template <bool HAS_FEAT, bool STATS = false, bool DY = false, bool LIST = false>
__global__ __launch_bounds__(256, 2) void residual_gemm_kernel(const float *__restrict__ out, const float *__restrict__ feat,
                                                               const unsigned *__restrict__ packed,
                                                               const float *__restrict__ bias, float *__restrict__ x,
                                                               long long rows, float *__restrict__ partial = nullptr,
                                                               const float *__restrict__ coef = nullptr, int add_rows = 1,
                                                               const int *__restrict__ perm = nullptr,
                                                               const int *__restrict__ tile_list = nullptr,
                                                               const int *__restrict__ tile_count = nullptr, int tiles_per_pair = 0,
                                                               int HW = 0, const int *__restrict__ ref_index = nullptr, int M_ref = 0)
{
    static_assert(!LIST || (!STATS && !DY), "the list form is the plain epilogue");
    extern __shared__ char s_rg[];
    char *s_hi = s_rg;
    char *s_lo = s_rg + kRgRows * kRgStageRow;
    float *s_unscale = reinterpret_cast<float *>(s_rg + 2 * kRgRows * kRgStageRow);
    float *s_out = reinterpret_cast<float *>(s_rg);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int list_count = LIST ? *tile_count : 0;
    const int trips = LIST ? (list_count + 1) / 2 : 1;
#pragma unroll 1
    for (int trip = LIST ? (int)blockIdx.x : 0; trip < trips; trip += LIST ? (int)gridDim.x : 1) {
    // (LIST: a wave's 16 rows belong to ONE tile -- waves 0, 1 the first tile of the trip, waves 2, 3 the second -- so its buffers are
    //  the maps of that tile's pair and the row offsets stay inside one map)
    const int list_slot = LIST ? 2 * trip + (wave >> 1) : 0;
    const int list_tile = (LIST && list_slot < list_count) ? tile_list[list_slot] : -1;
    const long long row0 = LIST ? (long long)max(list_tile, 0) / tiles_per_pair * HW : (long long)blockIdx.x * kRgRows;
    const unsigned nrows = LIST ? (unsigned)kRgRows : (unsigned)min((long long)kRgRows, rows - row0);
    const unsigned span = LIST ? (unsigned)HW * 1024u : nrows * 1024u;
    const __amdgpu_buffer_rsrc_t r_out = make_rsrc(out + row0 * 256, span);
    // (LIST: `feat` may be a pool of M_ref maps, the tile's pair reading map ref_index[pair]: pair_map, et_common.h)
    const long long feat_row0 = LIST ? (long long)pair_map(ref_index, max(list_tile, 0) / tiles_per_pair, M_ref) * HW : row0;
    const __amdgpu_buffer_rsrc_t r_feat = make_rsrc(HAS_FEAT ? feat + feat_row0 * 256 : out, HAS_FEAT ? span : 0u);
    const __amdgpu_buffer_rsrc_t r_x = make_rsrc(x + row0 * 256, span);
    const __amdgpu_buffer_rsrc_t r_w = make_rsrc(packed, (unsigned)kRgPackedWords * 4u);
    const float inv_w = reinterpret_cast<const float *>(packed)[kRgPackedWords];
    // byte offset of row 16 wave + r of the block inside the buffers
    int roff[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if constexpr (LIST) {
            roff[r] = 0x7ffff000;                                       // (past the buffers)
            if (list_tile >= 0) {
                const int pix = perm[(size_t)list_tile * 32 + (wave & 1) * 16 + r];
                if (pix >= 0) roff[r] = pix * 1024;
            }
        } else {
            roff[r] = (wave * 16 + r) * 1024;
        }
    }

    // ---- stage: rows 16 wave .. + 15 (rows past the end: zeros) ----
    float4 fr[16];     // the rows the epilogue adds: requested right behind the `out` rows, used behind the MFMA loop
    {
        float4 a[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = buf_load_f4_nt(r_out, roff[r] + lane * 16, 0);
        if (HAS_FEAT) {
#pragma unroll
            for (int r = 0; r < 16; ++r) fr[r] = buf_load_f4_nt(r_feat, roff[r] + lane * 16, 0);
        }
        if constexpr (DY) {
            // coef: [ca | cb | cc | mean][256]; `partial` (nullable) receives the dy rows
            const float4 ca = *reinterpret_cast<const float4 *>(coef + lane * 4), cb = *reinterpret_cast<const float4 *>(coef + 256 + lane * 4);
            const float4 cc = *reinterpret_cast<const float4 *>(coef + 512 + lane * 4), mu = *reinterpret_cast<const float4 *>(coef + 768 + lane * 4);
            const __amdgpu_buffer_rsrc_t r_dy = make_rsrc(partial ? partial + row0 * 256 : out, partial ? nrows * 1024u : 0u);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float4 v;
                v.x = fmaf(ca.x, fr[r].x, fmaf(cb.x, a[r].x - mu.x, cc.x));
                v.y = fmaf(ca.y, fr[r].y, fmaf(cb.y, a[r].y - mu.y, cc.y));
                v.z = fmaf(ca.z, fr[r].z, fmaf(cb.z, a[r].z - mu.z, cc.z));
                v.w = fmaf(ca.w, fr[r].w, fmaf(cb.w, a[r].w - mu.w, cc.w));
                // (rows past the end were loaded as zeros and would become cc: their stores are dropped, their GEMM rows unused)
                a[r] = v;
                const u32x4 o4 = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
                __builtin_amdgcn_raw_buffer_store_b128(o4, r_dy, roff[r] + lane * 16, 0, 2);
            }
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
    const float4 b4 = DY ? f4_zero() : *reinterpret_cast<const float4 *>(bias + lane * 4);      // (DY: no bias behind the product)
    __syncthreads();

    // ---- MFMA: all 64 rows x channels 64 wave .. + 63 ----
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
    if constexpr (STATS) {
        // thread <-> channel: mean and centred sum of squares of the block's rows of out . Wz^T (without the bias: it shifts
        // the mean only), two passes over the 64 values in LDS
        const int n = (int)nrows;
        float sum = 0.f;
        for (int m = 0; m < n; ++m) sum += s_out[m * kRgOutStride + tid];
        const float mean = sum / (float)n;
        float m2 = 0.f;
        for (int m = 0; m < n; ++m) {
            const float dv = s_out[m * kRgOutStride + tid] - mean;
            m2 = fmaf(dv, dv, m2);
        }
        partial[(size_t)blockIdx.x * 512 + tid] = mean;
        partial[(size_t)blockIdx.x * 512 + 256 + tid] = m2;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = wave * 16 + r;
        float4 v = *reinterpret_cast<const float4 *>(s_out + row * kRgOutStride + lane * 4);
        v.x += b4.x; v.y += b4.y; v.z += b4.z; v.w += b4.w;
        if (HAS_FEAT && (!DY || add_rows)) { v.x += fr[r].x; v.y += fr[r].y; v.z += fr[r].z; v.w += fr[r].w; }
        const u32x4 o = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
        __builtin_amdgcn_raw_buffer_store_b128(o, r_x, roff[r] + lane * 16, 0, 2);      // (streaming)
    }
    if constexpr (LIST) __syncthreads();      // (the next trip restages over the epilogue array)
    }
}

// Merge the per-block (count, mean, M2) of residual_gemm_kernel<false, true> into the batch statistics of z(out): one block
// per channel, a thread takes every 256th partial (Chan et al.'s pairwise update, in double), then a tree over the threads.
// mean_y = mean + z bias;  var = M2 / n (biased: what batch norm normalises with, BN.py:71-76).
__global__ __launch_bounds__(256) void z_stats_finish_kernel(const float *__restrict__ partial, long long blocks, long long rows,
                                                             const float *__restrict__ zbias, float *__restrict__ mean_out,
                                                             float *__restrict__ var_out)
{
    __shared__ double s_n[256], s_mean[256], s_m2[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (long long b = tid; b < blocks; b += 256) {
        const long long left = rows - b * kRgRows;
        const double nb = (double)(left < kRgRows ? left : kRgRows);
        const double mb = (double)partial[(size_t)b * 512 + c], qb = (double)partial[(size_t)b * 512 + 256 + c];
        const double tot = n + nb, delta = mb - mean;
        mean += delta * nb / tot;
        m2 += qb + delta * delta * n * nb / tot;
        n = tot;
    }
    s_n[tid] = n; s_mean[tid] = mean; s_m2[tid] = m2;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) {
            const double na = s_n[tid], nb = s_n[tid + o];
            if (nb > 0.0) {
                const double tot = na + nb, delta = s_mean[tid + o] - s_mean[tid];
                s_m2[tid] = s_m2[tid] + s_m2[tid + o] + delta * delta * na * nb / tot;
                s_mean[tid] = s_mean[tid] + delta * nb / tot;
                s_n[tid] = tot;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        mean_out[c] = (float)(s_mean[0] + (double)zbias[c]);
        var_out[c] = (float)(s_m2[0] / s_n[0]);
    }
}

// ---- backward of the training-mode epilogue: the per-channel sums of the batch norm's backward -----------------------------
// sum_rows g  and  sum_rows g (y - mean)  over all rows (g = d loss / d x, y = the saved batch-norm input): one block per 256 rows,
// a lane owns four channels of whole rows (1 KB per wave instruction), per-block partials [2][256], merged in double by
// z_bwd_finish_kernel -- which also forms the coefficients of dy = ca g + cb (y - mean) + cc  (BN.py:59-82 differentiated):
//     d beta = sum g      d gamma = invstd sum g (y - mean)      k = gamma invstd
//     ca = k      cb = - k invstd^2 sum g (y - mean) / M      cc = - k sum g / M
constexpr int kZbRows = 256;
__global__ __launch_bounds__(256) void z_bwd_sums_kernel(const float *__restrict__ g, const float *__restrict__ y,
                                                         const float *__restrict__ mean, long long rows, float *__restrict__ partial)
{
    __shared__ float s_red[2][4][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * kZbRows;
    const unsigned nrows = (unsigned)min((long long)kZbRows, rows - row0);
    const __amdgpu_buffer_rsrc_t r_g = make_rsrc(g + row0 * 256, nrows * 1024u), r_y = make_rsrc(y + row0 * 256, nrows * 1024u);
    const float4 mu = *reinterpret_cast<const float4 *>(mean + lane * 4);
    float4 sg = f4_zero(), sgy = f4_zero();
    for (int r0 = wave * 8; r0 < (int)nrows; r0 += 32) {
        float4 gv[8], yv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {           // (rows past the end: zeros for g -- nothing is added)
            gv[j] = buf_load_f4_nt(r_g, (r0 + j) * 1024 + lane * 16, 0);
            yv[j] = buf_load_f4_nt(r_y, (r0 + j) * 1024 + lane * 16, 0);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sg.x += gv[j].x; sg.y += gv[j].y; sg.z += gv[j].z; sg.w += gv[j].w;
            sgy.x = fmaf(gv[j].x, yv[j].x - mu.x, sgy.x);
            sgy.y = fmaf(gv[j].y, yv[j].y - mu.y, sgy.y);
            sgy.z = fmaf(gv[j].z, yv[j].z - mu.z, sgy.z);
            sgy.w = fmaf(gv[j].w, yv[j].w - mu.w, sgy.w);
        }
    }
    *reinterpret_cast<float4 *>(&s_red[0][wave][lane * 4]) = sg;
    *reinterpret_cast<float4 *>(&s_red[1][wave][lane * 4]) = sgy;
    __syncthreads();
    for (int w = 0; w < 2; ++w)
        partial[(size_t)blockIdx.x * 512 + w * 256 + tid] = (s_red[w][0][tid] + s_red[w][1][tid]) + (s_red[w][2][tid] + s_red[w][3][tid]);
}

__global__ __launch_bounds__(256) void z_bwd_finish_kernel(const float *__restrict__ partial, long long blocks, long long rows,
                                                           const float *__restrict__ gamma, const float *__restrict__ mean,
                                                           const float *__restrict__ invstd, float *__restrict__ coef,
                                                           float *__restrict__ dgamma, float *__restrict__ dbeta)
{
    __shared__ double s_a[256], s_b[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (long long k = tid; k < blocks; k += 256) {
        a += (double)partial[(size_t)k * 512 + c];
        b += (double)partial[(size_t)k * 512 + 256 + c];
    }
    s_a[tid] = a; s_b[tid] = b;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) {
            s_a[tid] += s_a[tid + o];
            s_b[tid] += s_b[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double sg = s_a[0], sgy = s_b[0], is = (double)invstd[c], k = (double)gamma[c] * is, m = (double)rows;
        dbeta[c] = (float)sg;
        dgamma[c] = (float)(sgy * is);
        coef[c] = (float)k;
        coef[256 + c] = (float)(-k * is * is * sgy / m);
        coef[512 + c] = (float)(-k * sg / m);
        coef[768 + c] = mean[c];
    }
}

// ---- the weight gradient of the training-mode epilogue:  d Wz = dy^T . out,  d bz = sum_rows dy -----------------------------------
// A 256 x 256 x M GEMM contracted over the M = N H W rows (524 288 at Config 2): 68.7 GFLOP over 1 GB of operands.  MIOpen's 1x1
// weight-gradient kernel takes 1.47 ms for it; the bound is the fp32 matrix rate (0.44 ms), since here the products run as EXACT
// fp32 MFMAs (v_mfma_f32_32x32x2_f32): contracted over rows, the operands cannot be scaled row by row into fp16's range the way
// the other GEMMs of this file do, and the fp32 fragment layout needs no transposition either -- lane (i, k) supplies
// A[i][k] = dy[row 2 q + k][co0 + i] and B[k][n] = out[row 2 q + k][ci0 + n], i.e. 32 consecutive channels of a ROW-major stage.
//   * grid = one block per CU, 8 waves; a block owns a contiguous range of rows and the whole 256 x 256 result: wave w the
//     output rows (co) 32 w .. 32 w + 31 against all eight 32-column blocks (ci): 8 accumulators of 16 registers;
//   * rows go through LDS 16 at a time (both operands, row-major, 288-float rows: the two half-waves of a fragment read hit
//     disjoint banks), double buffered: the loads of step k + 1 are in flight while step k multiplies; one barrier per step;
//   * per-block partial results (plain stores) are summed in block order by z_wgrad_finish_kernel: no float atomics,
//     bit-reproducible.
constexpr int kWgRows = 16;                   // rows per step
constexpr int kWgStride = 288;                // floats per staged row
constexpr size_t kWgLdsBytes = (size_t)2 * 2 * kWgRows * kWgStride * 4;
__global__ __launch_bounds__(512, 1) void z_wgrad_kernel(const float *__restrict__ dy, const float *__restrict__ out, long long rows,
                                                         long long rows_per_block, float *__restrict__ partial_w,
                                                         float *__restrict__ partial_b)
{
    extern __shared__ float s_wg[];           // [2 stages][dy | out][16][288]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const long long row0 = (long long)blockIdx.x * rows_per_block;
    long long nrows = rows - row0;
    if (nrows > rows_per_block) nrows = rows_per_block;
    if (nrows < 0) nrows = 0;
    const unsigned bytes = (unsigned)(nrows * 1024);
    const __amdgpu_buffer_rsrc_t r_dy = make_rsrc(dy + row0 * 256, bytes), r_o = make_rsrc(out + row0 * 256, bytes);
    const int steps = (int)((nrows + kWgRows - 1) / kWgRows);
    // thread t stages row t >> 5 of a step, 16-byte chunks (t & 31) and 32 + (t & 31) of both operands (rows past the end: zeros)
    const int srow = tid >> 5, sc = (tid & 31) * 4;
    float4 ld[4];
    auto load = [&](int k) {
        const int off = (k * kWgRows + srow) * 1024 + sc * 4;
        ld[0] = buf_load_f4_nt(r_dy, off, 0);
        ld[1] = buf_load_f4_nt(r_dy, off + 512, 0);
        ld[2] = buf_load_f4_nt(r_o, off, 0);
        ld[3] = buf_load_f4_nt(r_o, off + 512, 0);
    };
    auto store = [&](int stage) {
        float *base = s_wg + stage * 2 * kWgRows * kWgStride + srow * kWgStride + sc;
        *reinterpret_cast<float4 *>(base) = ld[0];
        *reinterpret_cast<float4 *>(base + 128) = ld[1];
        *reinterpret_cast<float4 *>(base + kWgRows * kWgStride) = ld[2];
        *reinterpret_cast<float4 *>(base + kWgRows * kWgStride + 128) = ld[3];
    };
    rg_f32x16 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float bsum = 0.f;
    if (steps > 0) {
        load(0);
        store(0);
    }
    __syncthreads();
    for (int k = 0; k < steps; ++k) {
        if (k + 1 < steps) load(k + 1);
        const float *sd = s_wg + (k & 1) * 2 * kWgRows * kWgStride + lh * kWgStride + wave * 32 + li;
        const float *so = s_wg + (k & 1) * 2 * kWgRows * kWgStride + kWgRows * kWgStride + lh * kWgStride + li;
#pragma unroll
        for (int q = 0; q < kWgRows / 2; ++q) {
            const float a = sd[2 * q * kWgStride];
            bsum += a;
            float b[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) b[t] = so[2 * q * kWgStride + 32 * t];
#pragma unroll
            for (int t = 0; t < 8; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[t], acc[t], 0, 0, 0);
        }
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
    bsum += __shfl_xor(bsum, 32);
    if (lh == 0) partial_b[(size_t)blockIdx.x * 256 + 32 * wave + li] = bsum;
}

// ---- the same product on the bf16 matrix cores (round 6, the default): each fp32 value as THREE bf16 terms -----------------------
// v = b1 + b2 + b3 with b1 = the upper 16 bits of v, b2 those of v - b1, b3 those of v - b1 - b2 (every remainder exact in fp32): 24
// significant bits, and bf16 keeps fp32's exponent -- so, unlike the fp16 splits of the other GEMMs, no scale is needed and nothing can
// overflow, which is what a contraction over ROWS wants (there is no per-row scale to factor out of a sum over rows).  A product is the
// six terms b1 b1' + b1 b2' + b2 b1' + b1 b3' + b3 b1' + b2 b2' (what is dropped is 2^-24 relative) on v_mfma_f32_32x32x16_bf16 with
// fp32 accumulation: 6 MFMAs of 16 rows against 8 fp32 MFMAs of 2 rows each -- a fifth of the matrix time (0.59 -> see DESIGN 4.5).
//   * grid, ownership of rows and of the result, partial sums, finish kernel: as z_wgrad_kernel above (bit-reproducible);
//   * a step is 16 rows.  Thread t <-> (operand t >> 8, channel t & 255): it loads its channel's 16 row values (a wave's load
//     covers 256 contiguous bytes of a row), splits them and writes, per term, the 16 rows as 32 contiguous bytes: [term][channel]
//     [16 rows], 48 bytes per channel (12-dword stride: the 16-byte accesses of 16 neighbouring channels hit distinct banks) -- which
//     IS the MFMA fragment layout: lane (channel i, k-group g) reads rows 8 g .. 8 g + 7 of its channel with one ds_read_b128;
//   * two stages: the loads of step k + 1 are in flight while step k multiplies, a wave splits and stores them behind its own
//     MFMAs (in the shadow of the other waves'); one barrier per step.  Four accumulators at a time take the six terms in turn, so
//     consecutive MFMAs never wait for each other's result.
typedef __bf16 wg_bf16x8 __attribute__((ext_vector_type(8)));
constexpr int kWgbChan = 48;                                   // bytes per (term, channel): 32 of rows + 16 of padding
constexpr int kWgbTerm = 256 * kWgbChan;                       // bytes per term
constexpr int kWgbStage = 2 * 3 * kWgbTerm;                    // [operand][term][channel]
constexpr size_t kWgbLdsBytes = (size_t)2 * kWgbStage;         // two stages
__global__ __launch_bounds__(512, 1) void z_wgrad_bf16x3_kernel(const float *__restrict__ dy, const float *__restrict__ out, long long rows,
                                                                long long rows_per_block, float *__restrict__ partial_w,
                                                                float *__restrict__ partial_b)
{
    extern __shared__ char s_wgb[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const long long row0 = (long long)blockIdx.x * rows_per_block;
    long long nrows = rows - row0;
    if (nrows > rows_per_block) nrows = rows_per_block;
    if (nrows < 0) nrows = 0;
    const unsigned bytes = (unsigned)(nrows * 1024);
    const int steps = (int)((nrows + kWgRows - 1) / kWgRows);
    // staging role: operand `sop` (0: dy, 1: out), channel `sch`
    const int sop = __builtin_amdgcn_readfirstlane(tid >> 8), sch = tid & 255;
    const __amdgpu_buffer_rsrc_t r_in = make_rsrc((sop ? out : dy) + row0 * 256, bytes);
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
                bsum += v;                                                          // (the dy threads': the bias gradient, rows in order)
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
    // A = dy^T: lane (co = 32 wave + li, k-group lh); B = out: lane (ci = 32 t + li, k-group lh)
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

__global__ __launch_bounds__(256) void z_wgrad_finish_kernel(const float *__restrict__ partial_w, const float *__restrict__ partial_b,
                                                             int blocks, float *__restrict__ grad_w, float *__restrict__ grad_b)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;       // element of the 256 x 256 result; block 256: the bias row
    // four running sums over the blocks b = 0, 1, 2, 3 (mod 4), added pairwise at the end: a fixed order (bit-reproducible) with
    // sixteen loads in flight instead of a chain of `blocks` dependent additions behind one load each (65 -> 20 us at 256 blocks)
    const float *src = blockIdx.x < 256 ? partial_w + idx : partial_b + threadIdx.x;
    const size_t stride = blockIdx.x < 256 ? 65536 : 256;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int b = 0;
#pragma unroll 4
    for (; b + 4 <= blocks; b += 4) {
        s0 += src[(size_t)b * stride];
        s1 += src[(size_t)(b + 1) * stride];
        s2 += src[(size_t)(b + 2) * stride];
        s3 += src[(size_t)(b + 3) * stride];
    }
    for (; b < blocks; ++b) s0 += src[(size_t)b * stride];
    const float s = (s0 + s1) + (s2 + s3);
    if (blockIdx.x < 256) grad_w[idx] = s;
    else grad_b[threadIdx.x] = s;
}
