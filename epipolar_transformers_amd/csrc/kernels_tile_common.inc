// Included inside the anonymous namespace of a tile translation unit: the device helpers the one-block-per-tile forward
// (kernels_forward_tile.inc) and the tiled backward (kernels_backward_tile.inc) share -- a sample's taps, building an array
// row without LDS atomics, and the tile GEMMs (exact fp32 and split fp16).

#pragma once
#include "kernels_tile_order.inc"   // kTilePix, kTileRows*
#include "et_wave_reduce.h"
#include "et_split_f16.h"

// Row index that pads a tile's row list up to the GEMMs' step: its byte offset, kTilePadRow * 1024 (+ the lane's channels), lies
// past every map, so the raw buffer loads of a pad row return zeros.  (The forward's lists used to be padded with source row 0
// against zero B columns: 0 x a NaN or an Inf in source pixel (0, 0) is NaN, in every pixel of the tile.)
constexpr int kTilePadRow = 0x7ffff000 / 1024;

// The four bilinear taps of a sample from its normalised location: the same arithmetic (and
// rounding) as the tail of et::sample_setup, in plain nw / ne / sw / se order.
struct TapSet {
    int tap[4];     // linear source pixel index, -1 outside the image
    float w[4];     // bilinear weight, 0 outside the image
    int cell;       // id of the sample's 2x2 cell (same id <=> same four taps); unique per lane when !in
};
__device__ __forceinline__ TapSet taps_of(const EtLayerDesc &d, float nx, float ny, bool in)
{
    const float x = et::unnormalize(nx, d.W, d.align_corners);
    const float y = et::unnormalize(ny, d.H, d.align_corners);
    const float xw = floorf(x), yn = floorf(y);
    const float w = x - xw, e = 1.f - w, n = y - yn, so = 1.f - n;
    const int x0 = (int)fminf(fmaxf(xw, -2.f), (float)d.W);
    const int y0 = (int)fminf(fmaxf(yn, -2.f), (float)d.H);
    TapSet o;
    o.cell = in ? y0 * 32768 + x0 : -(1 << 30) - (int)(threadIdx.x & 63);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int tx = t & 1, ty = t >> 1;
        const int xx = x0 + tx, yy = y0 + ty;
        const bool ok = in && ((unsigned)xx < (unsigned)d.W) && ((unsigned)yy < (unsigned)d.H);
        o.w[t] = ok ? (ty ? n : so) * (tx ? w : e) : 0.f;
        o.tap[t] = ok ? yy * d.W + xx : -1;
    }
    return o;
}

// Building a B row (array row of one pixel := sum over its samples of coef_k * w_kt on the row slots) without
// LDS atomics.  Consecutive samples that fall into the same 2x2 cell share all four taps, and a cell is never
// revisited along the line, so within one tap stream equal slots only occur in runs of neighbouring lanes.
// RowRuns holds the run structure (shared by the four streams); for runs of at most two samples each stream
// is one DPP add + a plain read-modify-write by the last lane of every run (distinct slots, no conflicts).
// ds_add_f32 costs ~70 clocks of the CU-wide LDS pipe per wave instruction; pixels with longer runs (short
// epipolar segments) keep the atomic form.
struct RowRuns {
    bool same;   // this lane's cell == the previous lane's
    bool end;    // last lane of its run
    bool longer; // wave-uniform: some run has three or more samples
};
__device__ __forceinline__ RowRuns row_runs(int cell)
{
    const int p1 = __builtin_amdgcn_update_dpp(-1, cell, 0x138, 0xf, 0xf, false);  // wave_shr:1
    const int p2 = __builtin_amdgcn_update_dpp(-1, p1, 0x138, 0xf, 0xf, false);
    const int n1 = __builtin_amdgcn_update_dpp(-1, cell, 0x130, 0xf, 0xf, false);  // wave_shl:1
    RowRuns r;
    r.same = p1 == cell;
    r.end = n1 != cell;
    r.longer = __builtin_amdgcn_ballot_w64(r.same && p2 == cell) != 0;
    return r;
}
__device__ __forceinline__ void scatter_row(float *drow, const int (&sl)[4], const float (&val)[4], const RowRuns &rr, int pad)
{
    if (rr.longer) {
#pragma unroll
        for (int r = 0; r < 4; ++r) atomicAdd(&drow[sl[r]], val[r]);
        return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float pv = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(val[r]), 0x138, 0xf, 0xf, false));
        const float sum = rr.same ? val[r] + pv : val[r];
        if (rr.end && sl[r] != pad) drow[sl[r]] += sum;
    }
}

// ---- the D-type GEMM of a tile: array = A_t . F2_U^T --------------------------------------------------------
// A_t = the tile's 32 rows of `abuf` (feat_ref for the similarity, grad_out for the backward's g . S_k), F2_U the
// tile's U source rows.  Fragment layout of v_mfma_f32_32x32x2_f32: lane l supplies A[m = l & 31][k = l >> 5] and
// B[k = l >> 5][n = l & 31].  The k order is ours to choose as long as A and B agree: MFMA number 4q + t contracts
// channels 8q + t (lanes 0-31) and 8q + 4 + t (lanes 32-63), so each lane feeds four MFMAs from ONE 16-byte load,
// straight from global memory (no LDS staging).  Loads run kStages ahead of the MFMAs; sched_barriers pin the
// order (left alone, the scheduler sinks every load next to its use and the matrix pipe waits a full memory
// latency per 8 MFMAs).
//
// Work split over the block's four waves (one per SIMD): whole 32-row blocks, two at a time per wave (shared A
// fragment, two independent accumulators).  With U ~ 155 that is five blocks for four waves -- one SIMD idle, one
// padded block -- but the phase is bound by operand traffic from L2 (every wave re-reads the 32 KB A tile), not by
// the MFMA makespan: dealing the blocks out evenly (whole block + a channel half of a fifth/sixth block per wave,
// the halves meeting in spare array columns) was measured and changed nothing; (row block, channel half) units
// meeting through ds_add_f32 cost +0.7 ms; 16 x 16 x 4 MFMA blocks +0.16 ms (1.7x the operand traffic).
// When every wave has at most one pair of row blocks (nb <= 8) the A tile is first staged ONCE in LDS -- in the
// D/B array itself, which is idle until the results are written -- and the waves read their A fragments from
// there: the tile then pulls ~190 KB instead of ~290 KB from L2 in this phase.
// (kAStride floats per staged A row, tile_array_floats: et_tile_layout.h)

// on_a_ready(staged): called once by every thread when the A tile can be read (staged = true: from LDS, row i at
// s_D + i * kAStride), before any MFMA -- the forward copies its res_base rows there.
template <int STRIDE, class OnAReady>
__device__ __forceinline__ void tile_gemm_rows(const __amdgpu_buffer_rsrc_t abuf, const __amdgpu_buffer_rsrc_t src,
                                               int abase, int stage_off, const int *s_rows, float *s_D, int U, int nb,
                                               int tid, int wave, int li, int lh, OnAReady &&on_a_ready)
{
    constexpr int kRowBytes = 1024, kStages = 4;
    if (nb <= 2 * kWavesPerBlock) {
        // thread t stages 128 bytes of A row t >> 3 (stage_off: its byte offset in `abuf`, past the end for a pixel
        // outside the group: zeros)
        {
            float4 st[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) st[k] = buf_load_f4(abuf, stage_off + k * 16, 0);
            float *arow = s_D + (tid >> 3) * kAStride + (tid & 7) * 32;
#pragma unroll
            for (int k = 0; k < 8; ++k) *reinterpret_cast<float4 *>(arow + k * 4) = st[k];
        }
        __syncthreads();
        on_a_ready(true);
        // Wave w: the 32-row blocks 2 w, 2 w + 1 = four 16-row quarters, each against the two 16-pixel halves of the
        // tile (v_mfma_f32_16x16x4_f32).  The load path merges the addresses of a lane QUAD only
        // (scripts/micro/load_patterns.hip: an instruction whose quads read 64 contiguous bytes runs at 32-40 B/clk per
        // CU; in operand order -- lane n = row n, neighbouring lanes 1 KB apart -- at 15 B/clk, which is what bounded
        // this phase): a lane LOADS 16 bytes of row (lane >> 2), chunk (lane & 3) of a 64-byte segment, and
        // ds_bpermute (the LDS crossbar, no LDS memory) hands lane (n, kg) = (lane & 15, lane >> 4) the registers of
        // lane 4 n + kg: chunk kg of row n = the operand of the four MFMAs of the segment (k = kg <-> channel
        // 16 seg + 4 kg + w in MFMA w; the A fragment is the matching 16 bytes of the staged tile).
        typedef float f32x4_t __attribute__((ext_vector_type(4)));
        const int jb = 2 * wave;
        const bool work = jb < nb;
        f32x4_t acc[2][4];     // [pixel half][row quarter]
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t >> 2][t & 3] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        const int ln = (li & 15), lk = (lh << 1) | (li >> 4);      // lane & 15, lane >> 4
        if (work) {
            const int lane_ = li + 32 * lh;
            const int paddr = (4 * ln + lk) * 4;
            int offh[4];
#pragma unroll
            for (int hh = 0; hh < 4; ++hh)
                offh[hh] = s_rows[min(jb * 32 + hh * 16 + (lane_ >> 2), U - 1)] * kRowBytes + (lane_ & 3) * 16;
            const float *afrag = s_D + ln * kAStride + lk * 4;
            constexpr int kSegStages = 2;
            float4 b[kSegStages][4];
#pragma unroll
            for (int q = 0; q < kSegStages; ++q)
#pragma unroll
                for (int hh = 0; hh < 4; ++hh) b[q][hh] = buf_load_f4(src, offh[hh] + q * 64, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float4 xa0 = *reinterpret_cast<const float4 *>(afrag + q * 16);
                const float4 xa1 = *reinterpret_cast<const float4 *>(afrag + 16 * kAStride + q * 16);
#pragma unroll
                for (int hh = 0; hh < 4; ++hh) {
                    const float4 x = b[q % kSegStages][hh];
                    const float px = __int_as_float(__builtin_amdgcn_ds_bpermute(paddr, __float_as_int(x.x)));
                    const float py = __int_as_float(__builtin_amdgcn_ds_bpermute(paddr, __float_as_int(x.y)));
                    const float pz = __int_as_float(__builtin_amdgcn_ds_bpermute(paddr, __float_as_int(x.z)));
                    const float pw = __int_as_float(__builtin_amdgcn_ds_bpermute(paddr, __float_as_int(x.w)));
                    acc[0][hh] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa0.x, px, acc[0][hh], 0, 0, 0);
                    acc[1][hh] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa1.x, px, acc[1][hh], 0, 0, 0);
                    acc[0][hh] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa0.y, py, acc[0][hh], 0, 0, 0);
                    acc[1][hh] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa1.y, py, acc[1][hh], 0, 0, 0);
                    acc[0][hh] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa0.z, pz, acc[0][hh], 0, 0, 0);
                    acc[1][hh] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa1.z, pz, acc[1][hh], 0, 0, 0);
                    acc[0][hh] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa0.w, pw, acc[0][hh], 0, 0, 0);
                    acc[1][hh] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa1.w, pw, acc[1][hh], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (q + kSegStages < 16) {
#pragma unroll
                    for (int hh = 0; hh < 4; ++hh) b[q % kSegStages][hh] = buf_load_f4(src, offh[hh] + (q + kSegStages) * 64, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();  // every wave is done with the staged A tile: the array may take the results
        if (work) {
            const bool has1 = jb + 1 < nb;
            float *drow = s_D + (4 * lk) * STRIDE + jb * 32 + ln;
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int hh = 0; hh < 4; ++hh) {
                    if (hh >= 2 && !has1) continue;
#pragma unroll
                    for (int r = 0; r < 4; ++r) drow[(16 * g + r) * STRIDE + 16 * hh] = acc[g][hh][r];
                }
        }
        return;
    }
    on_a_ready(false);
    for (int jb = 2 * wave; jb < nb; jb += 2 * kWavesPerBlock) {
        const int off0 = s_rows[min(jb * 32 + li, U - 1)] * kRowBytes + lh * 16;
        const int off1 = s_rows[min(jb * 32 + 32 + li, U - 1)] * kRowBytes + lh * 16;
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc0[r] = 0.f;
            acc1[r] = 0.f;
        }
        float4 av[kStages], b0[kStages], b1[kStages];
#pragma unroll
        for (int q = 0; q < kStages; ++q) {
            av[q] = buf_load_f4(abuf, abase + q * 32, 0);
            b0[q] = buf_load_f4(src, off0 + q * 32, 0);
            b1[q] = buf_load_f4(src, off1 + q * 32, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 32; ++q) {
            const float4 x0 = b0[q % kStages], x1 = b1[q % kStages];
            const float4 xa = av[q % kStages];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(xa.x, x0.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(xa.x, x1.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(xa.y, x0.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(xa.y, x1.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(xa.z, x0.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(xa.z, x1.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(xa.w, x0.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(xa.w, x1.w, acc1, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (q + kStages < 32) {
                av[q % kStages] = buf_load_f4(abuf, abase + (q + kStages) * 32, 0);
                b0[q % kStages] = buf_load_f4(src, off0 + (q + kStages) * 32, 0);
                b1[q % kStages] = buf_load_f4(src, off1 + (q + kStages) * 32, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const bool has1 = jb + 1 < nb;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = (r & 3) + 8 * (r >> 2) + 4 * lh;
            s_D[m * STRIDE + jb * 32 + li] = acc0[r];
            if (has1) s_D[m * STRIDE + jb * 32 + 32 + li] = acc1[r];
        }
    }
}

// ---- the D-type GEMM (array = A_t . F2_U^T) as split-fp16 products ------------------------------------------------
// Same work split and load scheme as tile_gemm_rows (wave w: the 32-row blocks 2 w, 2 w + 1 of every pass of eight blocks,
// as four 16-row quarters; quad-contiguous loads rearranged by ds_bpermute) on v_mfma_f32_16x16x32_f16: 24 MFMAs of 16
// cycles per 32 channels instead of 64 fp32 MFMAs of 32.  The A tile is staged ONCE as fp16 hi | lo (in the k order of the
// B operand), every row under the power of two of its own exact maximum (1 / scale -> s_red[32]); the source rows are scaled by the
// per-pair ESTIMATE `s_src` (tile_order_kernel) and every converted value is checked: the function returns true (for this
// wave) if one is beyond fp16's range -- the caller then redoes the tile with the exact fp32 tile_gemm_rows.  Needs
// 2 x 32 x 528 bytes of stage at the start of the array (the results replace it at the end: no trailing barrier, like
// tile_gemm_rows).  PASSES = passes of eight 32-row blocks (1: U <= 256; 2: U <= 512); the accumulators of all passes
// stay in registers until every wave is done with the stage.
template <int STRIDE, int PASSES>
__device__ __forceinline__ bool tile_gemm_rows_split(const __amdgpu_buffer_rsrc_t abuf, const __amdgpu_buffer_rsrc_t src,
                                                     int stage_off, const int *s_rows, float *s_D, float *s_red, int U, int nb,
                                                     int tid, int wave, int lane, float s_src, float inv_src)
{
    constexpr int kRowBytes = 1024, kStageRow = 528;
    char *s_hi = reinterpret_cast<char *>(s_D), *s_lo = s_hi + kTilePix * kStageRow;
    {
        float4 st[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) st[k] = buf_load_f4(abuf, stage_off + k * 16, 0);
        float m = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) m = fmaxf(m, fmaxf(fmaxf(fabsf(st[k].x), fabsf(st[k].y)), fmaxf(fabsf(st[k].z), fabsf(st[k].w))));
        // every A row under the power of two of ITS OWN maximum (the eight threads of a row: lanes t & 7): exact, and a
        // row that is tiny next to its neighbours keeps its bits (a flushed reference row would mask all its samples)
        m = fmaxf(m, dpp<0xB1>(m));      // quad_perm [1,0,3,2]
        m = fmaxf(m, dpp<0x4E>(m));      // quad_perm [2,3,0,1]
        m = fmaxf(m, dpp<0x141>(m));     // row_half_mirror: the other quad of the eight
        float sa, sa_inv;
        pow2_scale_of(m, sa, sa_inv);
        if ((tid & 7) == 0) s_red[tid >> 3] = sa_inv;
        // thread t holds channels 32 ks .. + 31 (ks = t & 7) of row t >> 3: channel 32 ks + 16 e + 4 kg + w -> fp16
        // position 32 ks + 8 kg + 4 e + w (the k order of the B operand below)
        char *hrow = s_hi + (tid >> 3) * kStageRow + (tid & 7) * 64, *lrow = s_lo + (tid >> 3) * kStageRow + (tid & 7) * 64;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = k >> 2, kg = k & 3;
            unsigned h0, l0, h1, l1;
            split_f16_pair(st[k].x * sa, st[k].y * sa, h0, l0);
            split_f16_pair(st[k].z * sa, st[k].w * sa, h1, l1);
            typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
            *reinterpret_cast<u32x2_t *>(hrow + kg * 16 + e * 8) = u32x2_t{h0, h1};
            *reinterpret_cast<u32x2_t *>(lrow + kg * 16 + e * 8) = u32x2_t{l0, l1};
        }
    }
    __syncthreads();
    const int ln = lane & 15, lk = lane >> 4;
    f32x4 acc[PASSES][2][4];     // [pass][pixel half][row quarter]
#pragma unroll
    for (int q = 0; q < PASSES; ++q)
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[q][t >> 2][t & 3] = f32x4{0.f, 0.f, 0.f, 0.f};
    float amax = 0.f;
    const int paddr = (4 * ln + lk) * 4;
    const char *ahp = s_hi + ln * kStageRow + lk * 16, *alp = s_lo + ln * kStageRow + lk * 16;
#pragma unroll
    for (int q = 0; q < PASSES; ++q) {
        const int jb = 8 * q + 2 * wave;
        if (jb >= nb) break;                                 // wave-uniform, forward exit
        const bool has1 = jb + 1 < nb;
        int offh[4];
#pragma unroll
        for (int hh = 0; hh < 4; ++hh)
            offh[hh] = (hh < 2 || has1) ? s_rows[min(jb * 32 + hh * 16 + (lane >> 2), U - 1)] * kRowBytes + (lane & 3) * 16
                                        : 0x7ffff000;                       // (no second block: zeros, no traffic)
        constexpr int kSt = 2;
        float4 b[kSt][4][2];
#pragma unroll
        for (int qq = 0; qq < kSt; ++qq)
#pragma unroll
            for (int hh = 0; hh < 4; ++hh)
#pragma unroll
                for (int e = 0; e < 2; ++e) b[qq][hh][e] = buf_load_f4(src, offh[hh] + qq * 128 + e * 64, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            f16x8 ahi[2], alo[2];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                ahi[g] = *reinterpret_cast<const f16x8 *>(ahp + g * 16 * kStageRow + ks * 64);
                alo[g] = *reinterpret_cast<const f16x8 *>(alp + g * 16 * kStageRow + ks * 64);
            }
#pragma unroll
            for (int hh = 0; hh < 4; ++hh) {
                if (hh >= 2 && !has1) continue;              // wave-uniform
                float v[8];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const float4 x = b[ks % kSt][hh][e];
                    v[4 * e + 0] = __int_as_float(__builtin_amdgcn_ds_bpermute(paddr, __float_as_int(x.x))) * s_src;
                    v[4 * e + 1] = __int_as_float(__builtin_amdgcn_ds_bpermute(paddr, __float_as_int(x.y))) * s_src;
                    v[4 * e + 2] = __int_as_float(__builtin_amdgcn_ds_bpermute(paddr, __float_as_int(x.z))) * s_src;
                    v[4 * e + 3] = __int_as_float(__builtin_amdgcn_ds_bpermute(paddr, __float_as_int(x.w))) * s_src;
                }
                f16x8 bhi, blo;
                split_f16x8<true>(v, bhi, blo, amax);
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    acc[q][g][hh] = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo[g], bhi, acc[q][g][hh], 0, 0, 0);
                    acc[q][g][hh] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi[g], blo, acc[q][g][hh], 0, 0, 0);
                    acc[q][g][hh] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi[g], bhi, acc[q][g][hh], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (ks + kSt < 8) {
#pragma unroll
                for (int hh = 0; hh < 4; ++hh)
#pragma unroll
                    for (int e = 0; e < 2; ++e) b[ks % kSt][hh][e] = buf_load_f4(src, offh[hh] + (ks + kSt) * 128 + e * 64, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();  // every wave is done with the stage: the array may take the results
    const f32x4 ai[2] = {*reinterpret_cast<const f32x4 *>(s_red + 4 * lk), *reinterpret_cast<const f32x4 *>(s_red + 16 + 4 * lk)};
#pragma unroll
    for (int q = 0; q < PASSES; ++q) {
        const int jb = 8 * q + 2 * wave;
        if (jb >= nb) break;
        const bool has1 = jb + 1 < nb;
        float *drow = s_D + (4 * lk) * STRIDE + jb * 32 + ln;
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int hh = 0; hh < 4; ++hh) {
                if (hh >= 2 && !has1) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) drow[(16 * g + r) * STRIDE + 16 * hh] = (acc[q][g][hh][r] * ai[g][r]) * inv_src;
            }
    }
    // (an Inf trips this; a NaN is dropped by the running fmaxf and comes back as a NaN logit, which splits the tile down to
    //  single pixels: fwd_tile_body, behind phase 2)
    return !(amax < kF16GuardLimit);
}

// ---- the second GEMM of a tile (out_t = B . F2_U) as split-fp16 products ---------------------------------------------
// B rows: finished in LDS by the soft-max phase, then (tile_convert_b_rows) scaled by 2^10 and split to fp16 hi | lo in
// place per group of eight columns -- two plain 16-byte reads per fragment.  Needs attention x weights <= 1, i.e. the
// soft-max on.  Source rows: quarter-row loads (a lane LOADS 16 bytes of row 16 ks + 8 lh + 4 s + q: four instructions of
// 4 rows x 256 B per step), halves traded with lane ^ 16 (v_permlane16_swap), scaled by the per-pair estimate and split on
// the register pairs the loads leave (the same rows passed the guard of the first GEMM).  Wave w: channels 64 w .. + 63.
// The scheme of the warp-specialised kernel's G2 (kernels_forward_tile_ws.inc), inside the one-block-per-tile kernel.
__device__ __forceinline__ void tile_convert_b_rows(float *row_a, float *row_b, int ucols, int lane)
{
    for (int g0 = 0; g0 < ucols / 8; g0 += 32) {
        const int grp = g0 + (lane & 31);
        if (grp >= ucols / 8) continue;
        float *gp = (lane < 32 ? row_a : row_b) + grp * 8;
        const float4 x0 = *reinterpret_cast<const float4 *>(gp), x1 = *reinterpret_cast<const float4 *>(gp + 4);
        const float bv[8] = {x0.x * 1024.f, x0.y * 1024.f, x0.z * 1024.f, x0.w * 1024.f,
                             x1.x * 1024.f, x1.y * 1024.f, x1.z * 1024.f, x1.w * 1024.f};
        f16x8 bhi8, blo8;
        float bdummy = 0.f;
        split_f16x8<false>(bv, bhi8, blo8, bdummy);      // (values <= 2^10 by construction: soft-max on)
        *reinterpret_cast<f16x8 *>(gp) = bhi8;
        *reinterpret_cast<f16x8 *>(gp + 4) = blo8;
    }
}

// A_F32 (the backward's d feat_ref = Bs . F2_U): the A rows are plain fp32 in LDS (any row stride) and are scaled by the
// power of two s_a (the caller's exact block maximum -> [2^10, 2^11)) and split on the fly, eight values per k-step and lane.
template <int STRIDE, bool A_F32 = false, class Store>
__device__ __forceinline__ void tile_gemm_out_split(const float *srcp, unsigned map_bytes, const int *s_rows, const float *s_B,
                                                    int upad, int wave, int lane, float s_src, float inv_src, Store &&store,
                                                    float s_a = 1024.f)
{
    constexpr int kRowBytes = 1024, kD2 = 4;
    const int li = lane & 31, lh = lane >> 5;
    const int nks = upad >> 4;
    const int c0 = wave * 64;
    const int voff = (c0 + 4 * (lane & 15)) * 4;
    float4 xring[kD2][4];
    int ridx[4];
    auto g2_rows = [&](int ks) {   // row indices of this lane's four loads of step ks (past the list: whatever LDS holds, never used)
        const int4 a = *reinterpret_cast<const int4 *>(s_rows + min(ks, nks - 1) * 16 + (lane >> 4) * 4);
        ridx[0] = a.x; ridx[1] = a.y; ridx[2] = a.z; ridx[3] = a.w;
    };
    if (nks == 0) {   // no source row in reach of the tile (every sample outside the image): out = 0, like the exact form
        const int chan0 = c0 + 4 * (lane & 15) + 2 * ((lane >> 4) & 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) store((r & 3) + 8 * (r >> 2) + 4 * lh, chan0, f32x2{0.f, 0.f});
        return;
    }
#pragma unroll
    for (int ks = 0; ks < kD2; ++ks) {
        g2_rows(ks);
        unsigned nbytes = ks < nks ? map_bytes : 0u;
        asm volatile("" : "+s"(nbytes));
        const __amdgpu_buffer_rsrc_t srck = make_rsrc(srcp, nbytes);
#pragma unroll
        for (int q = 0; q < 4; ++q) xring[ks][q] = buf_load_f4(srck, ridx[q] * kRowBytes + voff, 0);
    }
    g2_rows(kD2);
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
    const float *arow = s_B + li * STRIDE + lh * 8;
    auto kstep = [&](int ks, float4 (&xr)[4]) {
        f16x8 ahi, alo;
        if constexpr (A_F32) {
            float av[8], unused = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) av[e] = arow[ks * 16 + e] * s_a;
            split_f16x8<false>(av, ahi, alo, unused);
        } else {
            ahi = *reinterpret_cast<const f16x8 *>(arow + ks * 16);
            alo = *reinterpret_cast<const f16x8 *>(arow + ks * 16 + 4);
        }
        f32x2 v[8];
        const f32x2 s2 = {s_src, s_src};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            auto r0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(xr[q].x), __float_as_uint(xr[q].z), false, false);
            auto r1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(xr[q].y), __float_as_uint(xr[q].w), false, false);
            v[q] = f32x2{__uint_as_float(r0[0]), __uint_as_float(r1[0])} * s2;
            v[4 + q] = f32x2{__uint_as_float(r0[1]), __uint_as_float(r1[1])} * s2;
        }
        f16x8 ehi, elo, ohi, olo;
        split_f16x8_pairs(v, ehi, elo, ohi, olo);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, ehi, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, elo, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, ehi, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, ohi, acc1, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, olo, acc1, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, ohi, acc1, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        {
            unsigned nbytes = ks + kD2 < nks ? map_bytes : 0u;
            asm volatile("" : "+s"(nbytes));
            const __amdgpu_buffer_rsrc_t srck = make_rsrc(srcp, nbytes);
#pragma unroll
            for (int q = 0; q < 4; ++q) xr[q] = buf_load_f4(srck, ridx[q] * kRowBytes + voff, 0);
        }
        g2_rows(ks + kD2 + 1);
        __builtin_amdgcn_sched_barrier(0);
    };
#pragma unroll 1
    for (int ks0 = 0; ks0 < nks; ks0 += kD2) {
#pragma unroll
        for (int q = 0; q < kD2; ++q)
            if (ks0 + q < nks) kstep(ks0 + q, xring[q]);
    }
    // accumulator t, column n = 16 s + cq  <->  channel c0 + 4 cq + 2 s + t ; register r <-> pixel (r & 3) + 8 (r >> 2) + 4 lh
    const float inv = inv_src * (1.f / s_a);            // (s_a: 2^10 for the pre-converted B rows of the forward)
    const int chan = c0 + 4 * (lane & 15) + 2 * ((lane >> 4) & 1);
#pragma unroll
    for (int r = 0; r < 16; ++r) store((r & 3) + 8 * (r >> 2) + 4 * lh, chan, f32x2{acc0[r] * inv, acc1[r] * inv});
}
