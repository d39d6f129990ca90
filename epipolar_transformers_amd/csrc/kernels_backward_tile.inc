// Part of epipolar_kernels.hip (one translation unit, one anonymous namespace): the MFMA tile
// formulation of the backward.  Not a stand-alone header.
// ----------------------------------------------------------------------------
// Same tiles, same row sets, same one 32 x (ROWS+1) LDS array as the forward (kernels_forward_tile.inc),
// which is reused four times.  With g = d(out), f = feat_ref rows, F2_U the tile's source rows:
//
//   D = F1_t . F2_U^T          -> sim[p,k]   (resampled, kept in registers)
//   E = G_t  . F2_U^T          -> e[p,k] = g . S_k    (the array now holds E)  [+ ga[p,k] = d loss / d attn, where given]
//   soft-max forward + backward, lanes <-> samples:  a[p,k],  ds[p,k] = d(sim)
//   Bs[p,u] = sum ds w   (array)  -> d(feat_ref)_t  = Bs . F2_U            (as the forward's second GEMM)
//                                   d(feat_src)_U += Bs^T . F1_t           ('other1', similarity path)
//   B [p,u] = sum a  w   (array)  -> d(feat_src)_U += B^T  . G_t           ('other2', value path)
//
// The two transposed GEMMs contract over the tile's 32 PIXELS (16 MFMAs of k = 2 per 32 x 32 block) and
// their U x C result is added into grad_src with float atomics: ~5 tiles touch a source pixel, against
// 4K = 256 bilinear-transpose contributions per reference pixel in the scatter form, so the atomic count
// drops ~50x.  The summation order across tiles is not fixed: results are reproducible to rounding only
// (the gather form, et_epipolar_backward with a workspace, stays the bit-reproducible path).
// K <= 256: KPL = ceil(K / 64) samples per lane.  K <= 64 keeps the normalised sample locations in an LDS table; beyond
// that (the table would be 64 KB and up) a sample's location is re-derived from the pixel's segment where needed.
//
// Forms of the last two steps (one round of grad_src atomics per tile wherever it is possible):
//   * merged (two arrays, Bs and B at once; 192 / 288 columns: K <= 64 on maps up to 96 x 96): both transposed products
//     are added in registers before the atomic add;
//   * one array, 384 / 512 rows (K > 64, large maps): the array is used as two half-width arrays over half the row slots at
//     a time -- the same single round of atomics, the scatters run per half;
//   * one array, 256 rows (ET_VARIANT_TILE_CLASSIC, or a gradient for one of the two source roles only): Bs^T . F1, then the
//     array is rebuilt as B and B^T . G follows -- two rounds.
// GEMMs: the transposed ones are split-fp16 products under exact scales; the D-type ones and d(feat_ref) too wherever the
// array holds their fp16 stage (SPLIT_D: merged kernels and 384 rows up), with the exact-fp32 forms as the fallback of a
// tile whose source rows fail the fp16 guard.

#pragma once
#include "kernels_tile_common.inc"   // taps_of, row_runs / scatter_row, tile_gemm_* (and et_split_f16.h)

template <int ROWS> struct kArrayFloatsOf { static constexpr int value = bwd_tile_array_floats(ROWS); };
// dynamic LDS of a block of ROWS = rows and KPL = kpl: et_tile_layout.h's layout, which bwd_tile_body's pointers are asserted
// against
constexpr size_t bwd_tile_lds_bytes(int rows, int hw_words, int kpl) { return (size_t)bwd_tile_lds(rows, hw_words, kpl).end; }

struct BwdTileParams {
    BwdParams b;
    const int *perm;     // (N, tiles_per_pair * 32) reference pixels in epipolar-line order, -1 = padding
    int tiles_per_pair;
    int hw_words;        // ceil(H*W / 32)
    int rows_cap;        // overflow threshold (ROWS; smaller only to test the splitting)
    const float *scales; // nullable: per pair { ., ., s_src, 1 / s_src } (tile_order_kernel): the D-type GEMMs and d(feat_ref)
                         // then run as split-fp16 products where SPLIT_D holds (exact-fp32 redo of a tile whose rows overflow)
    const float *attn;   // nullable: the forward's attention (N,K,H,W).  Given, the soft-max is not recomputed -- the
                         // kernel skips the D = F1 . F2_U^T GEMM, its resampling and the soft-max forward
    // Round 5: a tile whose row set exceeds the merged kernel's 192 (288) columns is not split there any more but handed to the
    // one-array kernel of 256 (384) rows through a list -- with the epipole inside the map most tiles have 190-240 rows, every
    // second one was split in two and the call took 8.3 ms instead of 2.3 (profiles/r05_bwd_rigs.txt).
    int *ovf_count;         // merged launch: tiles deferred to the second launch are counted here ...
    int *ovf_list;          // ... and listed here (NULL: split in place, as before)
    const int *tile_list;   // second launch: block b takes tile tile_list[b] while b < *tile_count
    const int *tile_count;
    // The deterministic instances (DET, kernels_backward_det.inc): d(feat_src) is not added into grad_src with float atomics but,
    // as 64-bit fixed point under the pair's quantum, into an int64 accumulator with integer atomics -- an order-free sum.
    long long *det_acc;     // (N, H, W, 256) int64, cleared beside the ordering kernel's sort
    const float *det_q;     // per pair { q, 1 / q, bound, 0 } (det_quantum_kernel)
    int *det_err;           // the workspace's sticky error word (bit kDetGuardMask: a contribution beyond the bound)
    int list_cap;           // merged launch: row capacity of the second launch's kernel (a deferred tile beyond it is shared by
                            // kDetHardParts blocks there)
};

constexpr long long kDetPoison = 1LL << 62, kDetPoisonFloor = 1LL << 61;   // an accumulator element marked non-finite (det_add)
constexpr int kDetGuardMask = 1 << 2;   // sticky error word, bit 2: a fixed-point contribution of the deterministic backward was out of range
constexpr int kDetHardParts = 8;    // blocks of the second launch that share a deferred tile beyond that launch's own capacity

#ifndef ET_BWD_NO_ATOMICS
#define ET_BWD_NO_ATOMICS 0
#endif
constexpr int kBwdMergedBlocks = 3;     // blocks per CU the 64 x 64 kernels are compiled for
// over-capacity tiles of a merged launch that are still searched / split in place (the ring has a few dozen per call, the room rig
// ~150); beyond that count the call is one of MANY such tiles and they go to the second launch without a search
constexpr int kBwdInPlaceTiles = 256;
// Blocks of the merged launch that start during one pixel-group run of a split tile (~100 us beside the CU's other blocks;
// the launch retires ~7 tiles per us with 192 columns at 64 x 64, ~5.3 with 288 at 96 x 96): see the over-capacity policy below.
constexpr int bwd_blocks_per_group(int rows) { return rows == kTileRowsMergedLarge ? 550 : 700; }
// one tile (`vb`: its index, pair-major) by one block -- or, in a short list of deferred tiles, by `nparts` blocks: pixel
// groups are independent (grad_src is added with atomics, every other output is per pixel), so block `part` takes the
// `part`-th run of kTilePix / nparts pixels.
// DET (ET_VARIANT_BWD_DETERMINISTIC, et_epipolar_backward_tiled_det): the same five GEMMs; the U x C results are scaled by the
// pair's 1 / q (a power of two: exact), rounded to int64 and added with 64-bit integer atomics -- integer addition is
// associative, so the sum does not depend on the arrival order -- and the way a tile is grouped (which decides how its fp32
// partial sums are rounded) is a pure function of the tile: no counters, no block indices.
template <int KPL, int ROWS, bool DET = false>
__device__ __forceinline__ void bwd_tile_body(const BwdTileParams &tp, const int vb, const int part = 0, const int nparts = 1)
{
    // ROWS == kTileRowsMerged / kTileRowsMergedLarge (192 columns: 99.5 % of the 64 x 64 tiles; the rest are split into
    // pixel groups): TWO arrays,
    // Bs and B at once, so both transposed products are added in registers and grad_src sees ONE round of atomics
    // per tile -- the atomics, not the arithmetic, bound this kernel (4.2 ms with both rounds, 2.9 ms with one, 2.8 ms
    // with none).  The second array takes the place of the sample-location table (locations are re-derived from the
    // segments, as for K > 64), which keeps three blocks per CU.
    constexpr bool MERGED = bwd_rows_merged(ROWS);
    constexpr bool TAB = (KPL == 1) && !MERGED;
    // the D-type GEMMs (and d feat_ref) as split-fp16 products: wherever the array holds their 2 x 32 x 528-byte fp16 stage --
    // the merged kernels (two arrays) and the one-array kernels from 384 rows up; in one pass of eight 32-row blocks, or two
    constexpr bool SPLIT_D = MERGED || ROWS >= kTileRowsLarge;
    constexpr int kSplitPasses = (!MERGED && ROWS > 256) ? 2 : 1;
    static_assert(!SPLIT_D || kArrayFloatsOf<ROWS>::value * 4 >= 2 * kTilePix * 528, "the fp16 stage must fit the array");
    constexpr int kTileRowsMax = ROWS, kTileStride = ROWS + 1;
    constexpr int kArrayFloats = bwd_tile_array_floats(ROWS);
    extern __shared__ float s_dyn[];
    const BwdParams &p = tp.b;
    const EtLayerDesc &d = p.d;
    constexpr int C = 256;
    constexpr int kRowBytes = C * 4;
    constexpr int PW = kTilePix / kWavesPerBlock;  // pixels per wave
    constexpr int PB = 4;                          // pixels per batch of the lanes <-> samples stages
    const int H = d.H, W = d.W, K = d.K;
    const int HW = H * W;

    float *s_D = s_dyn;                                                  // [32][ROWS+1]  D, E, Bs, B in turn
    float *s_D2 = s_D + kTilePix * kTileStride;                          // MERGED: [32][ROWS+1]  B beside Bs
    int *s_rows = reinterpret_cast<int *>(s_D + kArrayFloats);           // [ROWS] slot -> source pixel
    int *s_pix = s_rows + kTileRowsMax;                                  // [32]  tile pixel ids
    int *s_misc = s_pix + kTilePix;                                      // BwdTileLds' U .. ainv, at the word indices below
    // The regions of et_tile_layout.h's BwdTileLds.  The pointers are kept as this chain (written from the layout's offsets the
    // backend fails to compile this kernel: "illegal VGPR to SGPR copy") and asserted against the layout instead: its constant
    // part at hw_words = 0, and at hw_words = 7 the terms that bitmap | prefix | nxy add behind it.
    constexpr BwdTileLds L = bwd_tile_lds(ROWS, 0, KPL), L7 = bwd_tile_lds(ROWS, 7, KPL);
    constexpr int kMiscU = 0, kMiscGroupRows = (L.group_rows - L.U) / 4, kMiscDrawn = (L.drawn - L.U) / 4, kMiscRed2 = (L.red2 - L.U) / 4,
                  kMiscRed1 = (L.red1 - L.U) / 4, kMiscAinv = (L.ainv - L.U) / 4, kMiscWords = (L.seg - L.U) / 4;
    static_assert(L.arr == 0 && L.rows == kArrayFloats * 4 && L.pix == L.rows + kTileRowsMax * 4 && L.U == L.pix + kTilePix * 4 &&
                      L.bitmap == L.seg + kTilePix * 16 && L.prefix == L.bitmap && L.nxy == L.prefix &&
                      L.end == L.nxy + (TAB ? kTileNxyBytes : 0),
                  "bwd_tile_body's pointers follow et_tile_layout.h");
    static_assert(L7.bitmap == L.bitmap && L7.prefix == L7.bitmap + 7 * 4 && L7.nxy == L7.prefix + 7 * 4 &&
                      L7.end == L7.nxy + (TAB ? kTileNxyBytes : 0),
                  "bitmap, prefix: hw_words words each, then the table");
    float *s_seg = reinterpret_cast<float *>(s_misc + kMiscWords);       // [32][4] epipolar segments
    unsigned *s_bitmap = reinterpret_cast<unsigned *>(s_seg + kTilePix * 4);  // [hw_words]
    int *s_prefix = reinterpret_cast<int *>(s_bitmap + tp.hw_words);     // [hw_words] exclusive popcount prefix
    f32x2 *s_nxy = reinterpret_cast<f32x2 *>(s_prefix + tp.hw_words);    // TAB: [32][64] normalised sample locations

    const int n = vb / tp.tiles_per_pair;
    const int tile = vb - n * tp.tiles_per_pair;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;

    const float *cam = p.cam + (size_t)n * ET_CAM_STRIDE;
    const unsigned map_bytes = (unsigned)HW * C * 4u;
    // the pair's maps inside the pools (NULL index: map n); grad_src is the source pool's gradient, so several pairs add into one map
    const int n_ref = pair_map(p.ref_index, n, p.M_ref), n_src = pair_map(p.src_index, n, p.M_src);
    const __amdgpu_buffer_rsrc_t src = make_rsrc(p.fsrc + (size_t)n_src * HW * C, map_bytes);
    const __amdgpu_buffer_rsrc_t ref = make_rsrc(p.fref + (size_t)n_ref * HW * C, map_bytes);
    const __amdgpu_buffer_rsrc_t gout = make_rsrc(p.gout + (size_t)n * HW * C, map_bytes);
    const __amdgpu_buffer_rsrc_t gsrc = make_rsrc(p.gsrc + (size_t)n_src * HW * C, map_bytes);
    const float neg_inf = -__builtin_huge_valf();
    // DET: the pair's int64 accumulator and 1 / q; a FINITE contribution of 2^48 quanta or more -- impossible under the
    // bound q is made from (kernels_backward_det.inc) -- is reported in the sticky error word and not added
    long long *det_pair = nullptr;
    float det_invq = 0.f;
    if constexpr (DET) {
        det_pair = tp.det_acc + (size_t)n * HW * C;
        det_invq = tp.det_q[n * 4 + 1];
    }
    // A contribution that is itself NaN or infinite (a non-finite input of this pair) is no error: the element is MARKED, set to
    // kDetPoison once (compare-and-swap; later additions, each below 2^48 quanta and fewer than 2^14, leave it beyond 2^61, and a
    // marked element is not marked again), and det_finish_kernel writes NaN for it -- whatever the order of arrival, so the call
    // stays bit-reproducible, and never lost.
    auto det_add = [&](float v, long long *dst) {
        const float s = v * det_invq;
        if (fabsf(s) < 0x1p48f) {
            __hip_atomic_fetch_add(dst, __float2ll_rn(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (!(fabsf(v) <= kLargestFinite)) {
            long long cur = __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            while (cur < kDetPoisonFloor && cur > -kDetPoisonFloor &&
                   !__hip_atomic_compare_exchange_strong(dst, &cur, kDetPoison, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            }
        } else {
            atomicOr(tp.det_err, kDetGuardMask);
        }
    };

    // ---- geometry, once per tile (as the forward) ----
    if (tid < kTilePix) {
        const int pix = tp.perm[((size_t)n * tp.tiles_per_pair + tile) * kTilePix + tid];
        et::Segment sg;
        sg.sx = sg.sy = sg.vx = sg.vy = 0.f;
        if (pix >= 0) {
            const int h = pix / W, w = pix - h * W;
            sg = et::epipolar_segment(d, cam, p.xs[w], p.ys[h]);
        }
        s_pix[tid] = pix;
        *reinterpret_cast<float4 *>(s_seg + tid * 4) = make_float4(sg.sx, sg.sy, sg.vx, sg.vy);
    }
    for (int t = tid; t < tp.hw_words; t += blockDim.x) s_bitmap[t] = 0u;
    __syncthreads();
    // sample k = s * 64 + lane of tile pixel i: taps / weights / cell (lanes <-> samples).  Without the table the location
    // is re-derived from the pixel's segment every time it is needed (three times per sample): with power-of-two resize
    // factors (every reference config) the divisions of coord2pix are exact multiplications -- same bits, ~30 fewer
    // instructions per evaluation (et::Pow2Recips).
    const et::Pow2Recips pr_t = et::pow2_recips(d);
    float step_t[KPL];
#pragma unroll
    for (int s = 0; s < KPL; ++s) step_t[s] = p.steps[min(s * kWave + lane, K - 1)];
    auto taps_at = [&](int i, int s, bool on) {
        if constexpr (TAB) {
            const f32x2 nxy = s_nxy[i * kWave + lane];
            return taps_of(d, nxy.x, nxy.y, lane < K && on);
        } else {
            const float4 v = *reinterpret_cast<const float4 *>(s_seg + i * 4);  // same address in every lane
            et::Segment sg;
            sg.sx = lane_bcast(v.x, 0);
            sg.sy = lane_bcast(v.y, 0);
            sg.vx = lane_bcast(v.z, 0);
            sg.vy = lane_bcast(v.w, 0);
            const int k = s * kWave + lane;
            float nx, ny;
            if constexpr (KPL == 1) {          // (K > 64: the second code path costs the larger kernels their registers)
                if (pr_t.ok) et::sample_location<true>(d, sg, step_t[s], pr_t, nx, ny);
                else et::sample_location<false>(d, sg, step_t[s], pr_t, nx, ny);
            } else {
                et::sample_location<false>(d, sg, step_t[s], pr_t, nx, ny);
            }
            return taps_of(d, nx, ny, k < K && on);
        }
    };
    if constexpr (TAB) {
        const float step = p.steps[min(lane, K - 1)];
        const et::Pow2Recips pr = et::pow2_recips(d);
        auto tabulate = [&](auto p2) {
#pragma unroll 1
            for (int ii = 0; ii < PW; ++ii) {
                const int i = wave * PW + ii;
                const float4 v = *reinterpret_cast<const float4 *>(s_seg + i * 4);  // same address in every lane
                et::Segment sg;
                sg.sx = lane_bcast(v.x, 0);
                sg.sy = lane_bcast(v.y, 0);
                sg.vx = lane_bcast(v.z, 0);
                sg.vy = lane_bcast(v.w, 0);
                float nx, ny;
                et::sample_location<decltype(p2)::value>(d, sg, step, pr, nx, ny);
                s_nxy[i * kWave + lane] = f32x2{nx, ny};
            }
        };
        if (pr.ok) tabulate(std::true_type());
        else tabulate(std::false_type());
    }
    // the row-set bitmap of the whole tile
#pragma unroll 1
    for (int ii = 0; ii < PW; ++ii) {
        const int i = wave * PW + ii;
        if (__builtin_amdgcn_readfirstlane(s_pix[i]) < 0) continue;  // wave-uniform
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            const TapSet ts = taps_at(i, s, true);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int prev = __builtin_amdgcn_update_dpp(-2, ts.tap[r], 0x111, 0xf, 0xf, false);  // row_shr:1
                if (ts.tap[r] >= 0 && ts.tap[r] != prev) atomicOr(&s_bitmap[ts.tap[r] >> 5], 1u << (ts.tap[r] & 31));
            }
        }
    }

    auto run_group = [&](int g, int gsize, auto first_pass) __attribute__((always_inline)) -> bool {
        auto active = [&](int i) { return __builtin_amdgcn_readfirstlane(s_pix[i]) >= 0 && i / gsize == g; };
        // ================= phase 0: the row set of this (sub)tile =================
        if constexpr (!decltype(first_pass)::value) {
            for (int t = tid; t < tp.hw_words; t += blockDim.x) s_bitmap[t] = 0u;
            __syncthreads();
#pragma unroll 1
            for (int ii = 0; ii < PW; ++ii) {
                const int i = wave * PW + ii;
                if (!active(i)) continue;  // wave-uniform
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    const TapSet ts = taps_at(i, s, true);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int prev = __builtin_amdgcn_update_dpp(-2, ts.tap[r], 0x111, 0xf, 0xf, false);
                        if (ts.tap[r] >= 0 && ts.tap[r] != prev) atomicOr(&s_bitmap[ts.tap[r] >> 5], 1u << (ts.tap[r] & 31));
                    }
                }
            }
        }
        __syncthreads();
        if (wave == 0) {
            int carry = 0;
            for (int base = 0; base < tp.hw_words; base += kWave) {
                const int t = base + lane;
                const int c = (t < tp.hw_words) ? __popc(s_bitmap[t]) : 0;
                int incl = c;
#pragma unroll
                for (int m = 1; m < kWave; m <<= 1) {
                    const int o = __shfl_up(incl, m);
                    if (lane >= m) incl += o;
                }
                if (t < tp.hw_words) s_prefix[t] = carry + incl - c;
                carry += __shfl(incl, kWave - 1);
            }
            if (lane == 0) s_misc[kMiscU] = carry;
        }
        __syncthreads();
        const int U = s_misc[kMiscU];
        if (U > tp.rows_cap) return false;  // block-uniform: split the tile further
        for (int t = tid; t < tp.hw_words; t += blockDim.x) {
            unsigned m = s_bitmap[t];
            int slot = s_prefix[t];
            while (m) {
                const int b = __ffs(m) - 1;
                s_rows[slot++] = t * 32 + b;
                m &= m - 1;
            }
        }
        const int nb = (U + 31) >> 5;
        const int ucols = nb * 32;  // columns the GEMMs below read: pad the row list, keep those columns defined
        if (tid < ucols - U) s_rows[U + tid] = kTilePadRow;      // (a row past the map: its loads return zeros)
        __syncthreads();

        // ---- D-type GEMM (the forward's phase 1, tile_gemm_rows): array = A_t . F2_U^T, A_t = the tile's rows of `abuf` ----
        // (returns true when the split-fp16 form was used and every converted source value passed the fp16 guard)
        auto gemm_rows = [&](const __amdgpu_buffer_rsrc_t abuf) -> bool {
            const int pix = s_pix[li];
            const bool act = pix >= 0 && li / gsize == g;
            const int abase = act ? pix * kRowBytes + lh * 16 : 0x7ffff000;  // past the buffer: loads return zeros
            const int spix = s_pix[tid >> 3];
            const int stage_off = (spix >= 0 && (tid >> 3) / gsize == g) ? spix * kRowBytes + (tid & 7) * 128 : 0x7ffff000;
            if constexpr (SPLIT_D) {
                if (tp.scales && nb <= 2 * kWavesPerBlock * kSplitPasses) {
                    const bool ovf = tile_gemm_rows_split<kTileStride, kSplitPasses>(abuf, src, stage_off, s_rows, s_D,
                                                                       reinterpret_cast<float *>(s_misc + kMiscAinv), U, nb, tid, wave,
                                                                       lane, tp.scales[n * 4 + 2], tp.scales[n * 4 + 3]);
                    if (!__syncthreads_or(ovf)) return true;      // (a value beyond fp16's range: the tile again, in exact fp32)
                }
            }
            tile_gemm_rows<kTileStride>(abuf, src, abase, stage_off, s_rows, s_D, U, nb, tid, wave, li, lh, [](bool) {});
            return false;
        };
        // ---- lanes <-> samples: slots and weights of sample `lane` of pixel i (re-derived from s_nxy) ----
        auto derive = [&](int i, int s, bool act, int (&sl)[4], float (&wt)[4]) {
            const TapSet ts = taps_at(i, s, act);
            const int cell = ts.cell;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = ts.tap[r] >= 0;
                const int u = ok ? ts.tap[r] : 0;
                const int word = u >> 5;
                const int rank = s_prefix[word] + __popc(s_bitmap[word] & ((1u << (u & 31)) - 1u));
                sl[r] = ok ? rank : kTileRowsMax;  // no tap: the pad column, with weight 0
                wt[r] = ts.w[r];
            }
            return cell;
        };
        auto resample = [&](const float *drow, const int (&sl)[4], const float (&wt)[4]) {
            float acc = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = drow[sl[r]];
                acc = fmaf(wt[r], (sl[r] != kTileRowsMax) ? v : 0.f, acc);
            }
            return acc;
        };
        // ---- array rows of this wave's pixels := sum_k coef[k] * w[k,t] on the row slots (zeros elsewhere) ----
        // (slot window [lo, lo + width): only those slots are written, at column colbase + slot - lo of `arr`'s rows; the others
        //  go to the row's pad column)
        auto scatter_rows = [&](const float (&coef)[PW][KPL], float *arr, int lo = 0, int width = ROWS, int colbase = 0) {
            const int wcols = min(width, ucols - lo);
            const int pad = kTileRowsMax - colbase;          // the row's pad column, seen from column colbase
#pragma unroll
            for (int ii = 0; ii < PW; ++ii) {
                const int i = wave * PW + ii;
                float *drow = arr + i * kTileStride + colbase;
                for (int c = lane; c < wcols; c += kWave) drow[c] = 0.f;
                const bool act = active(i);
                if (!act) continue;  // wave-uniform: a pixel outside the group contributes nothing (k of the transposed GEMMs)
#pragma unroll
                for (int s = 0; s < KPL; ++s) {   // (a sample set at a time: LDS operations of one wave stay in order)
                    int sl[4];
                    float wt[4];
                    const RowRuns rr = row_runs(derive(i, s, act, sl, wt));
#pragma unroll
                    for (int r = 0; r < 4; ++r) sl[r] = (sl[r] != kTileRowsMax && sl[r] >= lo && sl[r] < lo + width) ? sl[r] - lo : pad;
                    const float val[4] = {coef[ii][s] * wt[0], coef[ii][s] * wt[1], coef[ii][s] * wt[2], coef[ii][s] * wt[3]};
                    scatter_row(drow, sl, val, rr, pad);
                }
            }
        };
        // the merged form's two arrays at once: ONE derivation of the sample's slots and weights, two scatters
        auto scatter_rows2 = [&](const float (&coefA)[PW][KPL], float *arrA, const float (&coefB)[PW][KPL], float *arrB) {
#pragma unroll
            for (int ii = 0; ii < PW; ++ii) {
                const int i = wave * PW + ii;
                float *rowA = arrA + i * kTileStride, *rowB = arrB + i * kTileStride;
                for (int c = lane; c < ucols; c += kWave) {
                    rowA[c] = 0.f;
                    rowB[c] = 0.f;
                }
                const bool act = active(i);
                if (!act) continue;  // wave-uniform
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    int sl[4];
                    float wt[4];
                    const RowRuns rr = row_runs(derive(i, s, act, sl, wt));
                    const float valA[4] = {coefA[ii][s] * wt[0], coefA[ii][s] * wt[1], coefA[ii][s] * wt[2], coefA[ii][s] * wt[3]};
                    const float valB[4] = {coefB[ii][s] * wt[0], coefB[ii][s] * wt[1], coefB[ii][s] * wt[2], coefB[ii][s] * wt[3]};
                    scatter_row(rowA, sl, valA, rr, kTileRowsMax);
                    scatter_row(rowB, sl, valB, rr, kTileRowsMax);
                }
            }
        };
        // ---- transposed GEMM: grad_src[rows of U] += X^T . Y_t, X = the array (32 x U), Y_t = the tile's rows of `ybuf` ----
        // As split-fp16 products (et_split_f16.h) on v_mfma_f32_32x32x16_f16: the contraction runs over the tile's 32
        // PIXELS = two k-steps of 16, i.e. 12 MFMAs of 32 cycles per 32-slot block and accumulator pair instead of 32
        // fp32 MFMAs of 64.  Both operands are scaled by powers of two of exact maxima -- X over the tile (a block
        // reduction), Y per wave and accumulator -- so there is no estimate and no overflow path.  A[m = row slot][k = pixel]: a lane reads its slot's column of
        // the array (eight LDS reads per k-step, lanes along the slots: conflict-free); B[k = pixel][n = channel]:
        // loaded and split once, reused for every slot block.  Accumulator t holds channels c0 + 32 t + n, so every
        // atomic instruction covers two full 128-byte runs.
        // Up to two products into the same accumulators: X1^T . Y1 (+ X2^T . Y2 when X2 is given: the merged form).
        // The two terms then share ONE total scale (the smaller of the two: neither can overflow; the smaller term
        // loses low bits only relative to the larger one).
        // (slot0, nbk: the arrays hold the slots slot0 .. slot0 + 32 nbk - 1 in their columns 0 ..)
        auto gemm_transposed = [&](const float *X1, const __amdgpu_buffer_rsrc_t y1buf, const float *X2,
                                   const __amdgpu_buffer_rsrc_t y2buf, int slot0 = 0, int nbk = -1) {
            if (nbk < 0) nbk = nb;
            const int xcols = nbk * 32;
            const int c0 = wave * 64;
            const bool two = X2 != nullptr;
            // largest |X| of the arrays (row tid >> 3, every eighth column): one scale per array for the block
            float xm1 = 0.f, xm2 = 0.f;
            {
                const float *xr = X1 + (tid >> 3) * kTileStride;
                for (int c = tid & 7; c < xcols; c += 8) xm1 = fmaxf(xm1, fabsf(xr[c]));
                if (two) {
                    const float *xq = X2 + (tid >> 3) * kTileStride;
                    for (int c = tid & 7; c < xcols; c += 8) xm2 = fmaxf(xm2, fabsf(xq[c]));
                }
            }
            xm1 = wave_all_max(xm1);
            xm2 = wave_all_max(xm2);
            float *s_red = reinterpret_cast<float *>(s_misc + kMiscRed2);
            if (lane == 0) {                                  // (block barriers separate the uses of s_red)
                s_red[wave] = xm1;
                s_red[4 + wave] = xm2;
            }
            // Y: accumulator t = channels c0 + 32 t + li, k-step s2, j: pixel 16 s2 + 8 lh + j; one scale per wave
            auto load_y = [&](const __amdgpu_buffer_rsrc_t ybuf, float (&yv)[2][2][8]) {
                float ym = 0.f;
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                        for (int jj = 0; jj < 8; ++jj) {
                            const int pix = s_pix[16 * s2 + 8 * lh + jj];
                            // (padding pixel: its X row is zero; last use of these rows: streaming)
                            yv[t][s2][jj] = buf_load_f1_nt(ybuf, max(pix, 0) * kRowBytes + (c0 + 32 * t + li) * 4, 0);
                        }
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                        for (int jj = 0; jj < 8; ++jj) ym = fmaxf(ym, fabsf(yv[t][s2][jj]));
                return wave_all_max(ym);
            };
            auto split_y = [&](const float (&yv)[2][2][8], float sy, f16x8 (&yhi)[2][2], f16x8 (&ylo)[2][2]) {
                float dummy = 0.f;
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        float v[8];
#pragma unroll
                        for (int jj = 0; jj < 8; ++jj) v[jj] = yv[t][s2][jj] * sy;
                        split_f16x8<false>(v, yhi[t][s2], ylo[t][s2], dummy);
                    }
            };
            f16x8 y1hi[2][2], y1lo[2][2], y2hi[2][2], y2lo[2][2];
            float sy1, sy2 = 1.f;
            {
                float yv[2][2][8];
                sy1 = pow2_scale_capped(load_y(y1buf, yv));
                split_y(yv, sy1, y1hi, y1lo);
            }
            if (two) {
                float yv[2][2][8];
                sy2 = pow2_scale_capped(load_y(y2buf, yv));
                split_y(yv, sy2, y2hi, y2lo);
            }
            __syncthreads();
            float sx1 = pow2_scale_capped(fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3])));
            float sx2 = pow2_scale_capped(fmaxf(fmaxf(s_red[4], s_red[5]), fmaxf(s_red[6], s_red[7])));
            float total = sx1 * sy1;                          // the scale both terms are accumulated under
            if (two) {
                const float t2 = sx2 * sy2;
                total = fminf(total, t2);
                sx2 *= total / t2;                            // (powers of two: exact)
            }
            sx1 *= total / (sx1 * sy1);
            const float inv = 1.f / total;
            float dummy = 0.f;
            for (int mb = 0; mb < nbk; ++mb) {
                f32x16 acc0, acc1;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    acc0[r] = 0.f;
                    acc1[r] = 0.f;
                }
                auto product = [&](const float *X, float sx, const f16x8 (&yhi)[2][2], const f16x8 (&ylo)[2][2]) {
                    const float *xcol = X + (8 * lh) * kTileStride + mb * 32 + li;
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        float v[8];
#pragma unroll
                        for (int jj = 0; jj < 8; ++jj) v[jj] = xcol[(16 * s2 + jj) * kTileStride] * sx;
                        f16x8 xhi, xlo;
                        split_f16x8<false>(v, xhi, xlo, dummy);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xlo, yhi[0][s2], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xlo, yhi[1][s2], acc1, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xhi, ylo[0][s2], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xhi, ylo[1][s2], acc1, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xhi, yhi[0][s2], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xhi, yhi[1][s2], acc1, 0, 0, 0);
                    }
                };
                product(X1, sx1, y1hi, y1lo);
                if (two) product(X2, sx2, y2hi, y2lo);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int u = slot0 + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
#if ET_BWD_NO_ATOMICS     // (development: what the kernel costs WITHOUT its atomics -- wrong results; the products stay alive)
                    if (u < U && acc0[r] == 1.2345e-33f) {
#else
                    if (u < U) {
#endif
                        if constexpr (DET) {
                            // fixed point under the pair's quantum: v / q is exact (q a power of two), one rounding to int64;
                            // a lane covers 8 bytes, a half-wave 256 bytes of the row's accumulator
                            long long *dst = det_pair + (size_t)s_rows[u] * C + c0 + li;
                            det_add(acc0[r] * inv, dst);
                            det_add(acc1[r] * inv, dst + 32);
                        } else {
                            const int off = s_rows[u] * kRowBytes + (c0 + li) * 4;
                            __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(acc0[r] * inv, gsrc, off, 0, 0);
                            __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(acc1[r] * inv, gsrc, off + 128, 0, 0);
                        }
                    }
                }
            }
        };

        // ================= 1. D = F1 . F2_U^T, sim = resample(D) -- or the attention the forward returned =================
        // With the forward's attention a (what autograd saves in the reference too) the soft-max backward needs no
        // logits: ds_k = scale a_k (e_k - sum_j a_j e_j) is already zero where the mask put -1e10 (a_k = 0 exactly);
        // only a pixel whose samples are ALL masked (an all-zero reference row: uniform attention) has to be told
        // apart -- every a_k the same value 1 / K.  (All logits equal without a mask also gives that.  Without grad_attn
        // e_k - dot = 0 then, unless the samples differ while their logits agree to the last bit.  With grad_attn the true
        // ds_k = scale / K (ga_k - mean ga) of such an unmasked pixel is NOT zero and this branch drops it, where the
        // recomputed-attention branch, which sees the mask itself, keeps it: a documented limit of the saved-attention
        // form, include/epipolar_amd.h.)
        const bool have_attn = tp.attn != nullptr;
        float simv[PW][KPL];       // recomputed logits, or the forward's attention
        if (!have_attn) {
            gemm_rows(ref);
            __syncthreads();
#pragma unroll
            for (int ii = 0; ii < PW; ++ii) {
                const int i = wave * PW + ii;
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    int sl[4];
                    float wt[4];
                    derive(i, s, active(i), sl, wt);
                    simv[ii][s] = resample(s_D + i * kTileStride, sl, wt);
                }
            }
            __syncthreads();
        } else {
            const __amdgpu_buffer_rsrc_t abuf = make_rsrc(tp.attn + (size_t)n * K * HW, (unsigned)K * HW * 4u);
#pragma unroll
            for (int ii = 0; ii < PW; ++ii) {
                const int i = wave * PW + ii;
                const int pix = __builtin_amdgcn_readfirstlane(s_pix[i]);
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    const int k = s * kWave + lane;
                    simv[ii][s] = buf_load_f1(abuf, (active(i) && k < K) ? (k * HW + pix) * 4 : 0x7ffff000, 0);   // (else: zeros)
                }
            }
        }
        // ================= 2. E = G . F2_U^T, e = resample(E); soft-max forward and backward =================
        const bool rows_passed_guard = gemm_rows(gout);      // block-uniform
        __syncthreads();
        // d loss / d attn (nullable, (N,K,H,W) as the saved attention): it reaches a_k beside e_k, so e_k + ga_k takes e_k's place
        // in the soft-max gradient below -- one load per (pixel, sample), added where e is produced
        const bool have_ga = p.gattn != nullptr;             // block-uniform
        auto ga_at = [&](int i, int k) {
            const __amdgpu_buffer_rsrc_t gbuf = make_rsrc(p.gattn + (size_t)n * K * HW, (unsigned)K * HW * 4u);
            const int pix = __builtin_amdgcn_readfirstlane(s_pix[i]);
            return buf_load_f1(gbuf, (active(i) && k < K) ? (k * HW + pix) * 4 : 0x7ffff000, 0);   // (else: zeros)
        };
        float av[PW][KPL], dsv[PW][KPL];
        if constexpr (KPL == 1) {   // four pixels at a time: interleaved wave reductions
#pragma unroll
        for (int i0 = 0; i0 < PW; i0 += PB) {
            float lg[PB], ev[PB];
            bool masked[PB];
            const bool in = lane < K;
#pragma unroll
            for (int j = 0; j < PB; ++j) {
                const int i = wave * PW + i0 + j;
                int sl[4];
                float wt[4];
                derive(i, 0, active(i), sl, wt);
                ev[j] = resample(s_D + i * kTileStride, sl, wt);
                if (have_ga) ev[j] += ga_at(i, lane);
                masked[j] = simv[i0 + j][0] == 0.f;
                const float l = masked[j] ? -1e10f : simv[i0 + j][0];               // epipolar.py:298
                lg[j] = d.softmax_enabled ? l * d.softmax_scale : l / (float)K;   // epipolar.py:306 / 311
            }
            if (have_attn) {
#pragma unroll
                for (int j = 0; j < PB; ++j) {
                    const float a = simv[i0 + j][0];
                    if (d.softmax_enabled) {
                        const float a0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a)));
                        const bool all_masked = __builtin_amdgcn_ballot_w64(in && a != a0) == 0 && fabsf(a0 * (float)K - 1.f) < 1e-6f;
                        const float dot = wave_all_sum(a * ev[j]);
                        av[i0 + j][0] = a;
                        dsv[i0 + j][0] = all_masked ? 0.f : d.softmax_scale * a * (ev[j] - dot);
                    } else {
                        av[i0 + j][0] = a;                                        // (= sim / K, or -1e10 / K under the mask)
                        dsv[i0 + j][0] = (in && a != -1e10f / (float)K) ? ev[j] / (float)K : 0.f;
                    }
                }
            } else if (d.softmax_enabled) {
                float m[PB];
#pragma unroll
                for (int j = 0; j < PB; ++j) m[j] = in ? lg[j] : neg_inf;
                wave_all_max4(m);
#pragma unroll
                for (int j = 0; j < PB; ++j) {
                    const float e = in ? expf(lg[j] - m[j]) : 0.f;
                    const float a = e / wave_all_sum(e);
                    const float dot = wave_all_sum(a * ev[j]);
                    av[i0 + j][0] = a;
                    dsv[i0 + j][0] = masked[j] ? 0.f : d.softmax_scale * a * (ev[j] - dot);
                }
            } else {
#pragma unroll
                for (int j = 0; j < PB; ++j) {
                    av[i0 + j][0] = in ? lg[j] : 0.f;
                    dsv[i0 + j][0] = (in && !masked[j]) ? ev[j] / (float)K : 0.f;
                }
            }
        }
        } else {
#pragma unroll
        for (int ii = 0; ii < PW; ++ii) {
            const int i = wave * PW + ii;
            float lg[KPL], ev[KPL];
            bool masked[KPL];
            float vmax = neg_inf;
#pragma unroll
            for (int s = 0; s < KPL; ++s) {
                const bool in = s * kWave + lane < K;
                int sl[4];
                float wt[4];
                derive(i, s, active(i), sl, wt);
                ev[s] = resample(s_D + i * kTileStride, sl, wt);
                if (have_ga) ev[s] += ga_at(i, s * kWave + lane);
                masked[s] = simv[ii][s] == 0.f;
                const float l = masked[s] ? -1e10f : simv[ii][s];                  // epipolar.py:298
                lg[s] = d.softmax_enabled ? l * d.softmax_scale : l / (float)K;   // epipolar.py:306 / 311
                if (in) vmax = fmaxf(vmax, lg[s]);
            }
            if (have_attn) {
                if (d.softmax_enabled) {
                    const float a0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(simv[ii][0])));
                    bool differs = false;
                    float dotl = 0.f;
#pragma unroll
                    for (int s = 0; s < KPL; ++s) {
                        differs = differs || (s * kWave + lane < K && simv[ii][s] != a0);
                        dotl += simv[ii][s] * ev[s];
                    }
                    const bool all_masked = __builtin_amdgcn_ballot_w64(differs) == 0 && fabsf(a0 * (float)K - 1.f) < 1e-6f;
                    const float dot = wave_all_sum(dotl);
#pragma unroll
                    for (int s = 0; s < KPL; ++s) {
                        av[ii][s] = simv[ii][s];
                        dsv[ii][s] = all_masked ? 0.f : d.softmax_scale * simv[ii][s] * (ev[s] - dot);
                    }
                } else {
#pragma unroll
                    for (int s = 0; s < KPL; ++s) {
                        const bool in = s * kWave + lane < K;
                        av[ii][s] = simv[ii][s];
                        dsv[ii][s] = (in && simv[ii][s] != -1e10f / (float)K) ? ev[s] / (float)K : 0.f;
                    }
                }
            } else if (d.softmax_enabled) {
                vmax = wave_all_max(vmax);
                float e[KPL], lsum = 0.f;
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    e[s] = (s * kWave + lane < K) ? expf(lg[s] - vmax) : 0.f;
                    lsum += e[s];
                }
                const float denom = wave_all_sum(lsum);
                float dotl = 0.f;
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    av[ii][s] = e[s] / denom;
                    dotl += av[ii][s] * ev[s];
                }
                const float dot = wave_all_sum(dotl);
#pragma unroll
                for (int s = 0; s < KPL; ++s)
                    dsv[ii][s] = masked[s] ? 0.f : d.softmax_scale * av[ii][s] * (ev[s] - dot);
            } else {
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    const bool in = s * kWave + lane < K;
                    av[ii][s] = in ? lg[s] : 0.f;
                    dsv[ii][s] = (in && !masked[s]) ? ev[s] / (float)K : 0.f;
                }
            }
        }
        }
        // ================= 3. Bs: d(feat_ref) = Bs . F2_U, d(feat_src) += Bs^T . F1 =================
        if constexpr (MERGED) {
            if (d.src_grad_mask & 2) scatter_rows2(dsv, s_D, av, s_D2);
            else scatter_rows(dsv, s_D);
        } else {
            scatter_rows(dsv, s_D);
        }
        __syncthreads();
        bool dref_done = false;
        if constexpr (SPLIT_D) {
            // d(feat_ref) = Bs . F2_U as split-fp16 products (the forward's second GEMM, tile_gemm_out_split): the source rows
            // under the per-pair estimate -- the same rows, under the same scale, passed the guard of the E GEMM above --,
            // the Bs rows under the power of two of their EXACT block maximum, split on the fly (Bs stays fp32 in LDS: the
            // transposed GEMM below reads it again).  A fifth of the fp32 form's matrix time.
            if (rows_passed_guard) {
                float xm = 0.f;
                const float *xr = s_D + (tid >> 3) * kTileStride;
                for (int c = tid & 7; c < ucols; c += 8) xm = fmaxf(xm, fabsf(xr[c]));
                xm = wave_all_max(xm);
                float *s_red = reinterpret_cast<float *>(s_misc + kMiscRed1);
                if (lane == 0) s_red[wave] = xm;
                __syncthreads();
                const float sa = pow2_scale_capped(fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3])));
                tile_gemm_out_split<kTileStride, true>(p.fsrc + (size_t)n_src * HW * C, map_bytes, s_rows, s_D, ucols, wave, lane,
                                                       tp.scales[n * 4 + 2], tp.scales[n * 4 + 3], [&](int m, int chan, f32x2 v) {
                                                           const int pix = s_pix[m];
                                                           if (pix >= 0 && m / gsize == g)
                                                               __builtin_nontemporal_store(v, reinterpret_cast<f32x2 *>(p.gref + ((size_t)n * HW + pix) * C + chan));
                                                       }, sa);
                dref_done = true;
            }
        }
        if (!dref_done) {
            const int c0 = wave * 64;
            f32x16 acc0, acc1;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc0[r] = 0.f;
                acc1[r] = 0.f;
            }
            constexpr int kG = 8;
            const int ngrp = ucols / (2 * kG);
            const int voff = (c0 + 2 * li) * 4;
            const float *bcol = s_D + li * kTileStride + lh;
            const int *rcol = s_rows + lh;
            auto fetch = [&](int grp, float (&xa)[kG], f32x2 (&x)[kG]) {
#pragma unroll
                for (int j = 0; j < kG; ++j) {
                    xa[j] = bcol[grp * 2 * kG + 2 * j];
                    x[j] = buf_load_f2(src, rcol[grp * 2 * kG + 2 * j] * kRowBytes + voff, 0);
                }
            };
            auto contract = [&](const float (&xa)[kG], const f32x2 (&x)[kG]) {
#pragma unroll
                for (int j = 0; j < kG; ++j) {
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[j], x[j].x, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[j], x[j].y, acc1, 0, 0, 0);
                }
            };
            float xaA[kG], xaB[kG];
            f32x2 xA[kG], xB[kG];
            if (ngrp > 0) fetch(0, xaA, xA);
            for (int grp = 0; grp < ngrp; grp += 2) {
                __builtin_amdgcn_sched_barrier(0);
                if (grp + 1 < ngrp) fetch(grp + 1, xaB, xB);
                __builtin_amdgcn_sched_barrier(0);
                contract(xaA, xA);
                __builtin_amdgcn_sched_barrier(0);
                if (grp + 2 < ngrp) fetch(grp + 2, xaA, xA);
                __builtin_amdgcn_sched_barrier(0);
                if (grp + 1 < ngrp) contract(xaB, xB);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int pix = s_pix[m];
                if (pix >= 0 && m / gsize == g)
                    __builtin_nontemporal_store(f32x2{acc0[r], acc1[r]}, reinterpret_cast<f32x2 *>(p.gref + ((size_t)n * HW + pix) * C + c0 + 2 * li));
            }
        }
        if constexpr (MERGED) {
            // ================= 4. d(feat_src) += Bs^T . F1 + B^T . G, one round of atomics =================
            const int mask = d.src_grad_mask & 3;            // OTHER_GRAD 'other1' | 'other2' (epipolar.py:141-153)
            if (mask == 3) gemm_transposed(s_D, ref, s_D2, gout);
            else if (mask == 1) gemm_transposed(s_D, ref, nullptr, gout);
            else if (mask == 2) gemm_transposed(s_D2, gout, nullptr, gout);
        } else if ((d.src_grad_mask & 3) == 3) {
            // ================= 4'. one round of atomics in the one-array kernels too (256, 384 and 512 rows) =================
            // (Round 6: the 256-row kernel as well -- it takes the tiles the merged kernel defers, every fifth one when the epipole
            //  lies inside the map.  The call is bound by the RATE of float atomics, 1.31 TB/s on this chip whatever their scope
            //  (scripts/micro/atomic_scopes.hip; bench.py extra.box.atomic_probe): 1 KB per (tile, row) and round.)
            // The array is used as TWO half-width arrays: columns [0, H) take Bs and columns [H, 2 H) take B of the row
            // slots [h H, h H + H), h = 0, 1 -- both transposed products of a half are added in registers, then the
            // second half.  The scatters run per half (twice the lanes <-> samples work of this phase), the atomics -- what
            // this kernel is bound by -- once per tile instead of twice.
            constexpr int kHalf = ROWS / 2;
            for (int lo = 0; lo < ucols; lo += kHalf) {
                __syncthreads();                              // (the array is free: d feat_ref / the previous half are done)
                scatter_rows(dsv, s_D, lo, kHalf);
                scatter_rows(av, s_D, lo, kHalf, kHalf);
                __syncthreads();
                gemm_transposed(s_D, ref, s_D + kHalf, gout, lo, min(kHalf, ucols - lo) / 32);
            }
        } else {
            if (d.src_grad_mask & 1) gemm_transposed(s_D, ref, nullptr, ref);   // OTHER_GRAD 'other1' (epipolar.py:141-153)
            __syncthreads();
            // ================= 4. B: d(feat_src) += B^T . G =================
            if (d.src_grad_mask & 2) {                        // 'other2'
                scatter_rows(av, s_D);
                __syncthreads();
                gemm_transposed(s_D, gout, nullptr, gout);
            }
        }
        if constexpr (!decltype(first_pass)::value) __syncthreads();
        return true;
    };
    auto rows_of_group = [&](int g, int gsize) {
        __syncthreads();
        for (int t = tid; t < tp.hw_words; t += blockDim.x) s_bitmap[t] = 0u;
        if (tid == 0) s_misc[kMiscGroupRows] = 0;
        __syncthreads();
#pragma unroll 1
        for (int ii = 0; ii < PW; ++ii) {
            const int i = wave * PW + ii;
            if (__builtin_amdgcn_readfirstlane(s_pix[i]) < 0 || i / gsize != g) continue;  // wave-uniform
#pragma unroll
            for (int s = 0; s < KPL; ++s) {
                const TapSet ts = taps_at(i, s, true);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (ts.tap[r] >= 0) atomicOr(&s_bitmap[ts.tap[r] >> 5], 1u << (ts.tap[r] & 31));
            }
        }
        __syncthreads();
        int cnt = 0;
        for (int t = tid; t < tp.hw_words; t += blockDim.x) cnt += __popc(s_bitmap[t]);
        if (cnt) atomicAdd(&s_misc[kMiscGroupRows], cnt);
        __syncthreads();
        return s_misc[kMiscGroupRows];
    };
    const bool whole = nparts == 1 && run_group(0, kTilePix, std::true_type());
    if (!whole) {
        // The tile's row set does not fit.  grad_src is accumulated with atomics, so (unlike the forward) a group
        // must never run twice: first find the number of groups whose row sets all fit (bitmap + popcount only),
        // then run them.
        int ngroups = 2, g_first = 0, g_end = -1;
        bool found = false;     // (ngroups has been settled before the plain search)
        if constexpr (DET && MERGED) {
            // Deterministic merged launch: EVERY tile that does not fit whole goes to the second launch -- no counter, no block
            // index decides.  One that fits that launch's kernel whole (U <= list_cap) is listed from the front (count: header
            // word kTileHdrCount); a larger one from the back (count: kTileHdrDetHard, cleared by the ordering kernel) and is shared there by
            // kDetHardParts blocks, each splitting its own pixels by the plain search.  Both are functions of the tile alone; only
            // the order of the entries varies.  Nothing has been added yet.
            if (tp.ovf_list) {
                if (tid == 0) {
                    if (s_misc[kMiscU] <= tp.list_cap) tp.ovf_list[atomicAdd(tp.ovf_count, 1)] = vb;
                    else tp.ovf_list[tp.b.total_blocks - 1 - atomicAdd(tp.ovf_count + kTileHdrDetHard, 1)] = vb;
                }
                return;
            }
        }
        if (nparts > 1) {
            // A tile shared by `nparts` blocks: this one owns the `part`-th run of kTilePix / nparts pixels and splits them only as
            // far as THEIR row sets need (usually not at all: one search pass, one group run -- no block waits for a search over
            // the whole tile).
            int per = 1;
#pragma unroll 1
            for (;; per *= 2) {
                ngroups = nparts * per;
                if (ngroups >= kTilePix) break;     // (single pixels always fit)
                bool ok = true;
#pragma unroll 1
                for (int g = part * per; g < (part + 1) * per && ok; ++g) ok = rows_of_group(g, kTilePix / ngroups) <= tp.rows_cap;
                if (ok) break;
            }
            g_first = part * per;
            g_end = g_first + per;
            found = true;
        }
        if (!DET && MERGED && tp.ovf_list) {     // (MERGED: a compile-time constant -- the other kernels carry none of this)
            // Merged launch with a second launch behind it (round 5).  Splitting a tile in place is a serial chain of group runs
            // inside one block, and a tile's lines overlap -- half the pixels still touch two thirds to nine tenths of the rows:
            //   * two groups that fit (the ring rig's over-capacity tiles: lines side by side): ~2 x a tile, hidden beside the
            //     other blocks of the CU -- split in place;
            //   * four groups: ~100 us in one block.  A few per call are hidden (the ring has a few dozen; a second launch for
            //     those alone is a pure tail of one tile's latency, +2-4 % of the call), so the first 128 of a call stay in place;
            //     with the epipole inside the map every second tile is one of these (8.3 ms instead of 2.3) -- the rest go to
            //     the one-array kernel of 256 (384) rows;
            //   * eight or more (lines fanning out from an epipole near the map: the room rig has a few dozen, each a
            //     0.5-1 ms chain that ends up as the main launch's tail: 3.6 ms instead of 2.3) -- deferred, except early in the
            //     launch (below).
            // Nothing has been added to grad_src yet.
            // Round 6: all of that is for calls with FEW such tiles.  With the epipole inside the map every fifth tile is one
            // (3 229 of 16 384), the searches and the in-place halves cost the merged launch 0.7 ms beyond its fitting tiles
            // (2.92 against 2.21 ms) -- and the second launch is now a merged kernel of 288 columns (64 x 64 maps), which takes a
            // 193..288-row tile whole at 0.18 us against two group runs of 0.135 here.  So beyond the first kBwdInPlaceTiles
            // over-capacity tiles of a call nothing is searched or split: deferred at once.
            if (tid == 0) s_misc[kMiscDrawn] = atomicAdd(tp.ovf_count + kTileHdrBwdOverCap, 1);   // (cleared by the ordering kernel)
            __syncthreads();
            if (s_misc[kMiscDrawn] >= kBwdInPlaceTiles) {
                if (tid == 0) tp.ovf_list[atomicAdd(tp.ovf_count, 1)] = vb;
                return;
            }
            constexpr int kHalf = kTilePix / 2, kQuarter = kTilePix / 4;
            if (rows_of_group(0, kHalf) <= tp.rows_cap && rows_of_group(1, kHalf) <= tp.rows_cap) {
                run_group(0, kHalf, std::false_type());
                run_group(1, kHalf, std::false_type());
                return;
            }
            bool quarters = true;
#pragma unroll 1
            for (int g = 0; g < 4 && quarters; ++g) quarters = rows_of_group(g, kQuarter) <= tp.rows_cap;
            if (quarters) {
                if (tid == 0) s_misc[kMiscDrawn] = atomicAdd(tp.ovf_count + kTileHdrBwdQuads, 1);   // (cleared by the ordering kernel)
                __syncthreads();
                if (s_misc[kMiscDrawn] < 128) {
#pragma unroll 1
                    for (int g = 0; g < 4; ++g) run_group(g, kQuarter, std::false_type());
                    return;
                }
            }
            // eight or more groups: a serial chain of ~100 us per group (a group run costs a whole tile's GEMMs whatever its pixel
            // count, at a tile's latency beside the CU's other blocks): 0.8 ms for eight, 3 ms for thirty-two single pixels (the
            // room rig).  Started here it is hidden only while the launch still has that much work ahead of it -- blocks start in
            // index order, so a group is worth bwd_blocks_per_group later blocks -- and never many of them; otherwise deferred.
            // (A deferred tile is not free either: a list of one or two is a ~0.1 ms tail, one group run with nothing beside it,
            // which is why the ring's one or two hard tiles are worth keeping here when they come early enough.)
            bool in_place = false;
#pragma unroll 1
            for (ngroups = 8; ngroups <= kTilePix && (long long)blockIdx.x + ngroups * bwd_blocks_per_group(ROWS) < (long long)gridDim.x; ngroups *= 2) {
                bool ok = true;
#pragma unroll 1
                for (int g = 0; g < ngroups && ok; ++g) ok = rows_of_group(g, kTilePix / ngroups) <= tp.rows_cap;
                if (!ok) continue;
                if (tid == 0) s_misc[kMiscDrawn] = atomicAdd(tp.ovf_count + kTileHdrBwdEarly, 1);   // (cleared by the ordering kernel)
                __syncthreads();
                in_place = s_misc[kMiscDrawn] < 32;
                break;
            }
            if (!in_place) {
                if (tid == 0) tp.ovf_list[atomicAdd(tp.ovf_count, 1)] = vb;
                return;
            }
            found = true;
        }
#pragma unroll 1
        for (; !found && ngroups < kTilePix; ngroups *= 2) {  // (32 groups = single pixels always fit: host-side eligibility)
            bool ok = true;
#pragma unroll 1
            for (int g = 0; g < ngroups && ok; ++g) ok = rows_of_group(g, kTilePix / ngroups) <= tp.rows_cap;
            if (ok) break;
        }
        if (g_end < 0) g_end = ngroups;
#pragma unroll 1
        for (int g = g_first; g < g_end; ++g) run_group(g, kTilePix / ngroups, std::false_type());
    }
}

// The kernel: one tile per block (the launch covers every tile) ...
template <int KPL, int ROWS, bool DET = false>
__global__ __launch_bounds__(256, ((ROWS == kTileRowsSmall || ROWS == kTileRowsMerged) && KPL == 1) ? kBwdMergedBlocks : 2) void epipolar_bwd_tile_kernel(const BwdTileParams tp)
{
    bwd_tile_body<KPL, ROWS, DET>(tp, xcd_remap(blockIdx.x, tp.b.total_blocks));
}

// ... and its list form, the second launch of a merged call: a few blocks per compute unit walk the list of deferred tiles (a
// launch of one block per tile that finds the list almost empty costs 0.08 ms in block dispatch alone at Config 2).
template <int KPL, int ROWS, bool DET = false>
__global__ __launch_bounds__(256, 2) void epipolar_bwd_tile_list_kernel(const BwdTileParams tp)
{
    if constexpr (DET) {
        // The deterministic form: how many blocks share a tile depends on the tile alone -- kDetHardParts for the tiles listed from
        // the back (beyond this kernel's capacity: chains of group runs, started first), one for those listed from the front.
        const int easy = tp.tile_count[kTileHdrCount], hard = tp.tile_count[kTileHdrDetHard] * kDetHardParts;
#pragma unroll 1
        for (int idx = blockIdx.x; idx < hard + easy; idx += gridDim.x) {
            const bool h = idx < hard;
            const int vb = tp.tile_list[h ? tp.b.total_blocks - 1 - idx / kDetHardParts : idx - hard];
            bwd_tile_body<KPL, ROWS, true>(tp, vb, h ? idx % kDetHardParts : 0, h ? kDetHardParts : 1);
            __syncthreads();
        }
        return;
    }
    // A short list (the ring's one or two tiles, the room rig's two dozen) is a tail of whole group chains, one block each: eight
    // blocks share a tile then.  A long one (epipole inside the map: thousands) fills the chip as it is.
    const int count = *tp.tile_count;
    const int nparts = count * 8 <= (int)gridDim.x ? 8 : 1;
#pragma unroll 1
    for (int idx = blockIdx.x; idx < count * nparts; idx += gridDim.x) {
        bwd_tile_body<KPL, ROWS>(tp, tp.tile_list[idx / nparts], idx % nparts, nparts);
        __syncthreads();
    }
}
