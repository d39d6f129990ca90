// Included inside the anonymous namespace of et_forward_tile.hip: the MFMA tile
// formulation of the fused forward, one block per tile.
// ----------------------------------------------------------------------------
// Idea.  The per-pixel kernels are bound by VALU issue and by L1/TA bandwidth: every
// reference pixel drags its ~220 source rows (1 KB each) through the vector pipeline on its
// own, although reference pixels whose epipolar lines (nearly) coincide touch the SAME rows.
// Here 32 reference pixels with neighbouring epipolar lines form a tile, the union of the
// source rows their samples touch (U rows, typically 200-260) is the tile's row set, and the
// bilinear resampling commutes with both contractions:
//
//   sim[p,k]  = sum_t w[p,k,t] * D[p, row(p,k,t)]          D = F1_tile (32 x C) . F2_U^T (C x U)
//   out[p,:]  = sum_u B[p,u] * F2_U[u,:]                    B[p,u] = sum_{k,t: row = u} a[p,k] w[p,k,t]
//
// so the C-long work is two fp32 GEMMs on the matrix cores (v_mfma_f32_32x32x2_f32, operands
// straight from global memory into the MFMA fragment layout, no LDS staging), each source row
// is fetched twice per TILE instead of once per pixel, and the VALU only does the K-long
// geometry / soft-max work.  D and B share one 32 x 257 LDS array.
//
//   tile_order_kernel        one block per pair: key = (line angle, line offset) of every
//                            reference pixel's epipolar line, bitonic sort in LDS -> perm   (kernels_tile_order.inc)
//   epipolar_fwd_tile_kernel one block (4 waves) per tile
//
// Correctness never depends on the ordering: a tile whose row set exceeds the LDS array is
// split into 2, 4, .. 32 pixel groups that are processed one after the other.
#pragma once
#include "kernels_tile_common.inc"   // taps_of, row_runs / scatter_row, tile_gemm_*

struct TileParams {
    FwdParams f;
    const int *perm;     // (N, tiles_per_pair * 32) reference pixels in epipolar-line order, -1 = padding
    int tiles_per_pair;
    int hw_words;        // ceil(H*W / 32): words of the source-pixel bitmap
    int *stats;          // workspace: per tile  U | ngroups << 16
    int rows_cap;        // row-set capacity used by the overflow test (ROWS; smaller only to test the splitting)
    const int *tile_list;   // list form (epipolar_fwd_tile_list_kernel): the tiles to process ...
    const int *tile_count;  // ... and how many (device memory: written by the warp-specialised kernel)
    const float *scales;    // workspace, nullable: per pair { ., ., s_src, 1 / s_src } (tile_order_kernel): both GEMMs of a
                            // tile then run as split-fp16 products (exact-fp32 redo of a tile whose rows overflow)
};

// dynamic LDS of a block of ROWS = rows and KPL = kpl: the layout fwd_tile_body takes its pointers from (et_tile_layout.h)
constexpr size_t fwd_tile_lds_bytes(int rows, int hw_words, int kpl) { return (size_t)fwd_tile_lds(rows, hw_words, kpl).end; }

// ---- the tile kernel -------------------------------------------------------------------------
// C == 256 exactly.  Each wave owns 8 of the tile's 32 pixels for the K-long work (lanes <-> samples);
// with K <= 64 (KPL == 1) their tap tables stay in registers from the row-set phase to the soft-max phase.
// In a SHORT list of left-over tiles (list kernel) `nparts` blocks share a tile: pixel groups are independent, so block `part`
// takes the `part`-th run of kTilePix / nparts pixels and splits only those as far as their rows need -- a tile that must be
// split into eight groups is otherwise a serial chain in one block with the rest of the chip idle (epipole inside the map: 11
// tiles, 0.15 ms behind a 1.07 ms layer kernel).
template <int KPL, int ROWS>
__device__ __forceinline__ void fwd_tile_body(const TileParams &tp, const int vb, float *s_dyn, const int part = 0, const int nparts = 1)
{
    constexpr int kTileRowsMax = ROWS, kTileStride = ROWS + 4;
    constexpr int kPasses = ROWS / 256;      // passes of eight 32-row blocks of the split first GEMM (256: 1; 384, 512: 2)
    const FwdParams &p = tp.f;
    const EtLayerDesc &d = p.d;
    constexpr int C = 256;
    constexpr int kRowBytes = C * 4;
    constexpr int PW = kTilePix / kWavesPerBlock;  // pixels per wave
    constexpr bool TAB = (KPL == 1);
    constexpr unsigned kNone = 0xFFFFu;
    const int H = d.H, W = d.W, K = d.K;
    const int HW = H * W;

    const FwdTileLds L = fwd_tile_lds(ROWS, tp.hw_words, KPL);
    char *const s_base = reinterpret_cast<char *>(s_dyn);
    float *s_D = reinterpret_cast<float *>(s_base + L.arr);              // [32][ROWS+4]  D, then B
    int *s_rows = reinterpret_cast<int *>(s_base + L.rows);              // [ROWS] slot -> source pixel
    int *s_pix = reinterpret_cast<int *>(s_base + L.pix);                // [32]  tile pixel ids
    int *s_U = reinterpret_cast<int *>(s_base + L.U);                    // rows of the tile's row set
    float *s_ainv = reinterpret_cast<float *>(s_base + L.ainv);          // [32] 1 / scale of the A rows
    float *s_seg = reinterpret_cast<float *>(s_base + L.seg);            // [32][4] epipolar segments
    unsigned *s_bitmap = reinterpret_cast<unsigned *>(s_base + L.bitmap);  // [hw_words]
    int *s_prefix = reinterpret_cast<int *>(s_base + L.prefix);          // [hw_words] exclusive popcount prefix
    f32x2 *s_nxy = reinterpret_cast<f32x2 *>(s_base + L.nxy);            // TAB: [32][64] normalised sample locations

    const int n = vb / tp.tiles_per_pair;
    const int tile = vb - n * tp.tiles_per_pair;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;

    const float *cam = p.cam + (size_t)n * ET_CAM_STRIDE;
    const __amdgpu_buffer_rsrc_t src = make_rsrc(p.fsrc + (size_t)pair_map(p.src_index, n, p.M_src) * HW * C, (unsigned)HW * C * 4u);
    const __amdgpu_buffer_rsrc_t ref = make_rsrc(p.fref + (size_t)pair_map(p.ref_index, n, p.M_ref) * HW * C, (unsigned)HW * C * 4u);
    const float neg_inf = -__builtin_huge_valf();
    // outputs through raw buffers: 32-bit offsets, and a store whose offset is past the end is dropped, so
    // "lane >= K", "not lane 0/1" and "output not requested" (empty buffer) need no branches
    const __amdgpu_buffer_rsrc_t attn_buf =
        make_rsrc(p.attn ? p.attn + (size_t)n * K * HW : nullptr, p.attn ? (unsigned)K * HW * 4u : 0u);
    const __amdgpu_buffer_rsrc_t corr_buf =
        make_rsrc(p.corr ? p.corr + (size_t)n * HW * 2 : nullptr, p.corr ? (unsigned)HW * 8u : 0u);
    constexpr int kDropped = 0x7ffffff0;
    // (Plain cache policy on purpose: with the non-temporal hint the small scattered output stores are not merged in
    //  L2 any more and the launch takes 2.3-3.0 ms instead of 1.5-1.65 -- measured.)

    // ---- geometry, once per tile: thread i < 32 evaluates the segment of tile pixel i ----
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
    auto segment_of = [&](int i) {
        const float4 v = *reinterpret_cast<const float4 *>(s_seg + i * 4);  // same address in every lane
        et::Segment sg;
        sg.sx = lane_bcast(v.x, 0);
        sg.sy = lane_bcast(v.y, 0);
        sg.vx = lane_bcast(v.z, 0);
        sg.vy = lane_bcast(v.w, 0);
        return sg;
    };
    // TAB: each wave tabulates the normalised sample locations of its 8 pixels (lanes <-> samples); taps,
    // weights and row slots are re-derived from them where needed instead of being held in registers.
    // While a location is in registers its taps also go into the row-set bitmap of the whole-tile pass.
    if constexpr (TAB) {
        const float step = p.steps[min(lane, K - 1)];
        const et::Pow2Recips pr = et::pow2_recips(d);
        auto tabulate = [&](auto p2) {
#pragma unroll 1
            for (int ii = 0; ii < PW; ++ii) {
                const int i = wave * PW + ii;
                float nx, ny;
                et::sample_location<decltype(p2)::value>(d, segment_of(i), step, pr, nx, ny);
                s_nxy[i * kWave + lane] = f32x2{nx, ny};
                if (__builtin_amdgcn_readfirstlane(s_pix[i]) < 0) continue;  // wave-uniform
                const TapSet ts = taps_of(d, nx, ny, lane < K);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // neighbouring samples share taps: only the first lane of a run sets the bit
                    const int prev = __builtin_amdgcn_update_dpp(-2, ts.tap[r], 0x111, 0xf, 0xf, false);  // row_shr:1
                    if (ts.tap[r] >= 0 && ts.tap[r] != prev) atomicOr(&s_bitmap[ts.tap[r] >> 5], 1u << (ts.tap[r] & 31));
                }
            }
        };
        if (pr.ok) tabulate(std::true_type());
        else tabulate(std::false_type());
    }

    // One pass over the pixels of group g (gsize pixels each); returns false when their row set does not
    // fit the LDS array.  The whole tile is group 0 of 1: that call is straight-line code (kept out of any
    // loop so that nothing is hoisted across the phases and held in registers); only a tile that overflows
    // takes the loop below, which splits it into 2, 4, .. 32 groups.
    auto run_group = [&](int g, int gsize, auto first_pass) __attribute__((always_inline)) -> bool {
        constexpr bool kBitmapDone = TAB && decltype(first_pass)::value;  // the tabulation above filled it
        auto active = [&](int i) { return __builtin_amdgcn_readfirstlane(s_pix[i]) >= 0 && i / gsize == g; };
        // ================= phase 0: the row set of this (sub)tile =================
        if constexpr (!kBitmapDone) {
            for (int t = tid; t < tp.hw_words; t += blockDim.x) s_bitmap[t] = 0u;
            __syncthreads();
    #pragma unroll 1
            for (int ii = 0; ii < PW; ++ii) {
                const int i = wave * PW + ii;
                if (!active(i)) continue;  // wave-uniform
                if constexpr (TAB) {
                    const f32x2 nxy = s_nxy[i * kWave + lane];
                    const TapSet ts = taps_of(d, nxy.x, nxy.y, lane < K);
    #pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        // neighbouring samples share taps: only the first lane of a run sets the bit
                        const int prev = __builtin_amdgcn_update_dpp(-2, ts.tap[r], 0x111, 0xf, 0xf, false);  // row_shr:1
                        if (ts.tap[r] >= 0 && ts.tap[r] != prev) atomicOr(&s_bitmap[ts.tap[r] >> 5], 1u << (ts.tap[r] & 31));
                    }
                } else {
                    const et::Segment sg = segment_of(i);
    #pragma unroll
                    for (int s = 0; s < KPL; ++s) {
                        const int k = s * kWave + lane;
                        const et::SampleSetup su = et::sample_setup(d, sg, p.steps[min(k, K - 1)]);   // (every lane: the DPP below reads neighbours)
    #pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            // neighbouring samples in one 2x2 cell have the same tap in the same (parity) position: only the
                            // first lane of such a run sets the bit (fewer LDS atomics, far fewer same-word conflicts)
                            const int tapv = k < K ? su.tap[r] : -1;
                            const int prev = __builtin_amdgcn_update_dpp(-2, tapv, 0x111, 0xf, 0xf, false);  // row_shr:1
                            if (tapv >= 0 && tapv != prev) atomicOr(&s_bitmap[tapv >> 5], 1u << (tapv & 31));
                        }
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
            if (lane == 0) *s_U = carry;
        }
        __syncthreads();
        const int U = *s_U;
        if (U > tp.rows_cap) {  // block-uniform: split the tile further
            return false;
        }
        for (int t = tid; t < tp.hw_words; t += blockDim.x) {
            unsigned m = s_bitmap[t];
            int slot = s_prefix[t];
            while (m) {
                const int b = __ffs(m) - 1;
                s_rows[slot++] = t * 32 + b;
                m &= m - 1;
            }
        }
        // phase 3 walks the rows in groups of 16: pad the list with a row past the map (loads return zeros; the matching
        // B columns are zero too)
        const int upad = (U + 15) & ~15;
        if (tid < upad - U) s_rows[U + tid] = kTilePadRow;
        __syncthreads();

        bool split_ok = false;           // block-uniform: this (sub)tile's GEMMs run as split-fp16 products
        bool odd_logit = false;          // per lane: a logit of this group is NaN or infinite (see behind phase 2)
        // ================= phase 1: D = F1_tile . F2_U^T on the matrix cores =================
        // fragment layout of v_mfma_f32_32x32x2_f32: lane l supplies A[m = l & 31][k = l >> 5] and
        // B[k = l >> 5][n = l & 31].  The k order is ours to choose as long as A and B agree: MFMA
        // number 4q + t contracts channels 8q + t (lanes 0-31) and 8q + 4 + t (lanes 32-63), so each
        // lane feeds four MFMAs from ONE 16-byte load.
        {
            const int pix = s_pix[li];
            const bool act = pix >= 0 && li / gsize == g;
            // (a pixel outside this group points past the buffer: raw buffer loads return zeros there)
            const int abase = act ? pix * kRowBytes + lh * 16 : 0x7ffff000;
            const int nb = (U + 31) >> 5;
            // additive term of the residual fusion, res_base = feat_ref + bias (a 1 KB row copy per pixel): wave w
            // copies channel groups 8w .. 8w+7 of every pixel, from the A tile staged in LDS when there is one.
            // (Measured alternatives, all slower: the whole copy on the wave that has no row blocks; loads first and
            //  stores after the MFMA loop; stores from the A fragments inside the MFMA loop.)
            auto copy_base = [&](bool staged) {
                if (!(p.res_base && act)) return;
#pragma unroll
                for (int qq = 0; qq < 8; ++qq) {
                    const int q = wave * 8 + qq;
                    float4 r = staged ? *reinterpret_cast<const float4 *>(s_D + li * kAStride + q * 8 + lh * 4)
                                      : buf_load_f4(ref, abase + q * 32, 0);
                    if (p.res_bias) {
                        const float4 bb = *reinterpret_cast<const float4 *>(p.res_bias + q * 8 + lh * 4);
                        r = make_float4(r.x + bb.x, r.y + bb.y, r.z + bb.z, r.w + bb.w);
                    }
                    *reinterpret_cast<float4 *>(p.res_base + ((size_t)n * HW + pix) * C + q * 8 + lh * 4) = r;
                }
            };
            const int spix = s_pix[tid >> 3];
            const int stage_off = (spix >= 0 && (tid >> 3) / gsize == g) ? spix * kRowBytes + (tid & 7) * 128 : 0x7ffff000;
            // split-fp16 products (fp32 accumulate, ~22 significant bits per product) under the per-pair scale estimate;
            // a tile with a source value beyond fp16's range (checked on every converted value) is redone in exact fp32
            if (tp.scales && nb <= 8 * kPasses) {
                const bool ovf = tile_gemm_rows_split<kTileStride, kPasses>(ref, src, stage_off, s_rows, s_D,
                                                                            s_ainv, U, nb, tid, wave,
                                                                            lane, tp.scales[n * 4 + 2], tp.scales[n * 4 + 3]);
                split_ok = !__syncthreads_or(ovf);
                __syncthreads();
                if (split_ok) copy_base(false);
            }
            if (!split_ok)
                tile_gemm_rows<kTileStride>(ref, src, abase, stage_off, s_rows, s_D, U, nb, tid, wave, li, lh, copy_base);
        }
        __syncthreads();

        // ================= phase 2: resample D, masked soft-max, build B in place =================
        {
            const int ucols = upad;  // columns phase 3 reads
            if constexpr (TAB) {
                // the wave's pixels advance four at a time: independent dependency chains per stage
                constexpr int PB = 4;
#pragma unroll 1
                for (int i0 = 0; i0 < PW; i0 += PB) {
                    float lg[PB], a[PB], wt[PB][4];
                    int sl[PB][4], best[PB];
                    RowRuns runs[PB];
                    float mynx[PB], myny[PB];
                    bool act[PB];
#pragma unroll
                    for (int j = 0; j < PB; ++j) {
                        const f32x2 nxy = s_nxy[(wave * PW + i0 + j) * kWave + lane];
                        mynx[j] = nxy.x;
                        myny[j] = nxy.y;
                        act[j] = active(wave * PW + i0 + j);
                    }
#pragma unroll
                    for (int j = 0; j < PB; ++j) {
                        const float *drow = s_D + (wave * PW + i0 + j) * kTileStride;
                        const TapSet ts = taps_of(d, mynx[j], myny[j], lane < K && act[j]);
                        runs[j] = row_runs(ts.cell);
                        float acc = 0.f;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const bool ok = ts.tap[r] >= 0;
                            const int u = ok ? ts.tap[r] : 0;
                            const int word = u >> 5;
                            const int rank = s_prefix[word] + __popc(s_bitmap[word] & ((1u << (u & 31)) - 1u));
                            sl[j][r] = ok ? rank : kTileRowsMax;  // (no tap: the pad column, with weight 0)
                            wt[j][r] = ts.w[r];
                            const float v = drow[sl[j][r]];
                            acc = fmaf(ts.w[r], ok ? v : 0.f, acc);
                        }
                        float l = (acc == 0.f) ? -1e10f : acc;           // epipolar.py:298
                        if (d.softmax_enabled) l = l * d.softmax_scale;  // epipolar.py:306
                        else l = l / (float)K;                           // epipolar.py:311
                        lg[j] = l;
                        odd_logit |= !(fabsf(l) <= kLargestFinite);      // (lanes without a sample: -1e10 x scale, finite)
                    }
                    {
                        static_assert(PB == 4, "the wave reductions below are four wide");
                        const bool in = lane < K;
                        float amax[PB], idx[PB];
                        if (d.softmax_enabled) {
                            // hardware exp2 / reciprocal: ~1e-6 relative on the returned attention (tolerance 1e-5)
                            float m[PB];
#pragma unroll
                            for (int j = 0; j < PB; ++j) m[j] = in ? lg[j] : neg_inf;
                            wave_all_max4(m);
#pragma unroll
                            for (int j = 0; j < PB; ++j) {
                                const float e = in ? __expf(lg[j] - m[j]) : 0.f;
                                const float rdn = __builtin_amdgcn_rcpf(wave_all_sum(e));
                                a[j] = e * rdn;
                                amax[j] = rdn;  // the largest logit has e == 1
                            }
                        } else {
#pragma unroll
                            for (int j = 0; j < PB; ++j) {
                                a[j] = in ? lg[j] : 0.f;
                                amax[j] = in ? a[j] : neg_inf;
                            }
                            wave_all_max4(amax);
                        }
                        // first maximum over k (torch.argmax): a NaN is above every value -- the first NaN where there is one (v_max
                        // dropped it from amax; behind the soft-max one NaN makes every weight NaN: sample 0) --, else the lowest
                        // lane that holds the maximum.  No hit at all cannot address anything: masked to a lane where it is used.
#pragma unroll
                        for (int j = 0; j < PB; ++j) idx[j] = (in && a[j] == amax[j]) ? (float)lane : 1e9f;
                        wave_all_min4(idx);
#pragma unroll
                        for (int j = 0; j < PB; ++j) {
                            const unsigned long long nans = __builtin_amdgcn_ballot_w64(in && a[j] != a[j]);
                            best[j] = nans ? (int)__builtin_ctzll(nans) : (int)idx[j];
                        }
                    }
#pragma unroll
                    for (int j = 0; j < PB; ++j) {
                        if (!act[j]) continue;  // wave-uniform
                        const int i = wave * PW + i0 + j;
                        const int pix = __builtin_amdgcn_readfirstlane(s_pix[i]);
                        float *drow = s_D + i * kTileStride;
                        {
                            const int bi = __builtin_amdgcn_readfirstlane(best[j]) & (kWave - 1);
                            const float bx = lane_bcast(mynx[j], bi), by = lane_bcast(myny[j], bi);
                            const float cv = (lane == 0) ? et::de_normalize(d, bx, W) : et::de_normalize(d, by, H);
                            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(cv), corr_buf,
                                                                  lane < 2 ? (pix * 2 + lane) * 4 : kDropped, 0, 0);
                        }
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(a[j]), attn_buf, (lane * HW + pix) * 4, 0, 0);
                        // B row: zero, then scatter a_k * w_kt onto the row slots (same wave: LDS ops stay in order)
                        for (int c = lane; c < ucols; c += kWave) drow[c] = 0.f;
                        const float val[4] = {a[j] * wt[j][0], a[j] * wt[j][1], a[j] * wt[j][2], a[j] * wt[j][3]};
                        scatter_row(drow, sl[j], val, runs[j], kTileRowsMax);
                    }
                }
            } else {
#pragma unroll 1
                for (int ii = 0; ii < PW; ++ii) {
                    const int i = wave * PW + ii;
                    if (!active(i)) continue;  // wave-uniform
                    const int pix = __builtin_amdgcn_readfirstlane(s_pix[i]);
                    const et::Segment sg = segment_of(i);
                    float *drow = s_D + i * kTileStride;
                    int slot[KPL][4];
                    float wt[KPL][4], nx[KPL], ny[KPL], sv[KPL];
                    float vmax = neg_inf;
#pragma unroll
                    for (int s = 0; s < KPL; ++s) {
                        const int k = s * kWave + lane;
                        const bool in = k < K;
                        const et::SampleSetup su = et::sample_setup(d, sg, in ? p.steps[k] : 0.f);
                        nx[s] = su.nx;
                        ny[s] = su.ny;
                        float acc = 0.f;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const bool ok = in && su.tap[r] >= 0;
                            const int u = ok ? su.tap[r] : 0;
                            const int word = u >> 5;
                            const int sl = s_prefix[word] + __popc(s_bitmap[word] & ((1u << (u & 31)) - 1u));
                            slot[s][r] = ok ? sl : -1;
                            wt[s][r] = ok ? su.weight[r] : 0.f;
                            const float v = ok ? drow[sl] : 0.f;
                            acc = fmaf(wt[s][r], v, acc);
                        }
                        float l = (acc == 0.f) ? -1e10f : acc;           // epipolar.py:298
                        if (d.softmax_enabled) l = l * d.softmax_scale;  // epipolar.py:306
                        else l = l / (float)K;                           // epipolar.py:311
                        sv[s] = l;
                        odd_logit |= !(fabsf(l) <= kLargestFinite);
                        if (in) vmax = fmaxf(vmax, l);      // (a NaN it drops comes back as expf(NaN - vmax) below)
                    }
                    float a[KPL];
                    if (d.softmax_enabled) {
                        vmax = wave_all_max(vmax);
                        float lsum = 0.f;
#pragma unroll
                        for (int s = 0; s < KPL; ++s) {
                            a[s] = (s * kWave + lane < K) ? expf(sv[s] - vmax) : 0.f;
                            lsum += a[s];
                        }
                        const float denom = wave_all_sum(lsum);
#pragma unroll
                        for (int s = 0; s < KPL; ++s) a[s] = a[s] / denom;
                    } else {
#pragma unroll
                        for (int s = 0; s < KPL; ++s) a[s] = (s * kWave + lane < K) ? sv[s] : 0.f;
                    }
                    // first maximum over k (torch.argmax): a NaN above every value, then the largest value, then the lowest
                    // index (argmax_key); always one of the samples
                    unsigned bestk = 0u;
                    int bestl = 0x7fffffff;
#pragma unroll
                    for (int s = 0; s < KPL; ++s) {
                        const int k = s * kWave + lane;
                        const unsigned key = argmax_key(a[s]);
                        if (k < K && key > bestk) {
                            bestk = key;
                            bestl = k;
                        }
                    }
                    const int besti = wave_first_argmax(bestk, bestl);
                    if (p.corr) {
                        float bx = 0.f, by = 0.f;
#pragma unroll
                        for (int s = 0; s < KPL; ++s) {
                            const float tx = __shfl(nx[s], besti & (kWave - 1));
                            const float ty = __shfl(ny[s], besti & (kWave - 1));
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
                            if (k < K) p.attn[((size_t)n * K + k) * HW + pix] = a[s];
                        }
                    }
                    for (int c = lane; c < ucols; c += kWave) drow[c] = 0.f;
                    // scatter a_k * w_kt onto the row slots, 64 samples at a time: runs of neighbouring samples in one 2x2
                    // cell are combined by DPP and written by the run's last lane (scatter_row: no LDS atomics unless a run
                    // is longer than two); the slots of one pixel are visited in sample order by ONE wave, so the passes of
                    // the KPL groups cannot race
#pragma unroll
                    for (int s = 0; s < KPL; ++s) {
                        const bool in = s * kWave + lane < K;
                        const float px = et::unnormalize(nx[s], d.W, d.align_corners), py = et::unnormalize(ny[s], d.H, d.align_corners);
                        const int x0 = (int)fminf(fmaxf(floorf(px), -2.f), (float)d.W), y0 = (int)fminf(fmaxf(floorf(py), -2.f), (float)d.H);
                        const int cell = in ? y0 * 32768 + x0 : -(1 << 30) - lane;     // (same id <=> same four taps)
                        // et::sample_setup keeps the taps by coordinate PARITY (tap (x, y) in position 2 (y & 1) + (x & 1)): in that
                        // order neighbouring cells share a tap within one position, and two runs would write one slot in the
                        // same instruction.  scatter_row needs them by CORNER (nw, ne, sw, se): then equal slots within a
                        // position <=> same cell.
                        int sl4[4];
                        float val[4];
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const int pos = (((y0 + (t >> 1)) & 1) << 1) | ((x0 + (t & 1)) & 1);
                            const int sl_p = pos == 0 ? slot[s][0] : pos == 1 ? slot[s][1] : pos == 2 ? slot[s][2] : slot[s][3];
                            const float w_p = pos == 0 ? wt[s][0] : pos == 1 ? wt[s][1] : pos == 2 ? wt[s][2] : wt[s][3];
                            sl4[t] = sl_p >= 0 ? sl_p : kTileRowsMax;
                            val[t] = a[s] * w_p;
                        }
                        scatter_row(drow, sl4, val, row_runs(cell), kTileRowsMax);
                    }
                }
            }
        }
        // the finished B rows of this wave's pixels -> fp16 hi | lo (x 2^10) for the split second GEMM (same wave as the
        // scatter: LDS operations stay in order); needs attention x weight <= 1: the soft-max on
        const bool split_out = split_ok && d.softmax_enabled;
        if (split_out) {
#pragma unroll
            for (int ii = 0; ii < PW; ii += 2)
                tile_convert_b_rows(s_D + (wave * PW + ii) * kTileStride, s_D + (wave * PW + ii + 1) * kTileStride, upad, lane);
        }
        // A logit that is not finite means a source row of this group (or a reference pixel) holds a NaN or an Inf.  The GEMM
        // below multiplies EVERY pixel of the group with EVERY row of the group's row set -- B is 0 for a row the pixel does not
        // tap, and 0 x NaN = NaN --, so the value would reach pixels whose samples never touch it; the reference confines it to
        // the pixels that tap it (include/epipolar_amd.h, "Non-finite values").  Such a group is split like one whose row set
        // overflows, down to single pixels: a pixel's row set is its own taps, B has no zeros against foreign rows.  Every row
        // of the row set is tapped by some pixel of the group (zero weights included: their products are in the logit), so no
        // non-finite row escapes the test.  Block-uniform; the outputs this pass has already stored are stored again.
        if (__syncthreads_or(odd_logit) && gsize > 1) return false;

        // ================= phase 3: out = B . F2_U on the matrix cores =================
        if (split_out) {
            tile_gemm_out_split<kTileStride>(p.fsrc + (size_t)pair_map(p.src_index, n, p.M_src) * HW * C, (unsigned)HW * C * 4u, s_rows, s_D, upad, wave, lane,
                                             tp.scales[n * 4 + 2], tp.scales[n * 4 + 3], [&](int m, int chan, f32x2 v) {
                                                 const int pix = s_pix[m];
                                                 if (pix >= 0 && m / gsize == g)
                                                     *reinterpret_cast<f32x2 *>(p.out + ((size_t)n * HW + pix) * C + chan) = v;
                                             });
        } else {
            const int c0 = wave * 64;
            f32x16 acc0, acc1;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc0[r] = 0.f;
                acc1[r] = 0.f;
            }
            // K loop over pairs of rows, in groups of kG pairs; a group's operands (one LDS read and one
            // 8-byte load per MFMA pair) are requested a whole group (2 * kG MFMAs) ahead of their use.
            // Output column n of accumulator t is channel c0 + 2n + t: one float2 feeds both MFMAs.
            // Columns U .. upad-1 of the B rows are zero and s_rows is padded up to upad with a row that reads zeros, so
            // the loop needs no bounds logic; rows of pixels outside this group hold stale values, but their
            // accumulator rows are never stored.
            constexpr int kG = 8;
            const int ngrp = upad / (2 * kG);
            const int voff = (c0 + 2 * li) * 4;
            const float *bcol = s_D + li * kTileStride + lh;
            const int *rcol = s_rows + lh;
            auto fetch = [&](int grp, float (&av)[kG], f32x2 (&x)[kG]) {
#pragma unroll
                for (int j = 0; j < kG; ++j) {
                    av[j] = bcol[grp * 2 * kG + 2 * j];
                    x[j] = buf_load_f2(src, rcol[grp * 2 * kG + 2 * j] * kRowBytes + voff, 0);
                }
            };
            auto contract = [&](const float (&av)[kG], const f32x2 (&x)[kG]) {
#pragma unroll
                for (int j = 0; j < kG; ++j) {
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], x[j].x, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], x[j].y, acc1, 0, 0, 0);
                }
            };
            float avA[kG], avB[kG];
            f32x2 xA[kG], xB[kG];
            if (ngrp > 0) fetch(0, avA, xA);
            for (int grp = 0; grp < ngrp; grp += 2) {
                __builtin_amdgcn_sched_barrier(0);
                if (grp + 1 < ngrp) fetch(grp + 1, avB, xB);
                __builtin_amdgcn_sched_barrier(0);
                contract(avA, xA);
                __builtin_amdgcn_sched_barrier(0);
                if (grp + 2 < ngrp) fetch(grp + 2, avA, xA);
                __builtin_amdgcn_sched_barrier(0);
                if (grp + 1 < ngrp) contract(avB, xB);
            }
    #pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int pix = s_pix[m];
                if (pix >= 0 && m / gsize == g)
                    *reinterpret_cast<f32x2 *>(p.out + ((size_t)n * HW + pix) * C + c0 + 2 * li) = f32x2{acc0[r], acc1[r]};
            }
        }
        // (the next group reuses the LDS arrays; the whole-tile pass just ends here, stores still in flight)
        if constexpr (!decltype(first_pass)::value) __syncthreads();
        return true;
    };
    int ngroups = 1;
    if (nparts > 1 || !run_group(0, kTilePix, std::true_type())) {
#pragma unroll 1
        for (ngroups = nparts > 1 ? nparts : 2; ngroups <= kTilePix; ngroups *= 2) {  // host-side eligibility: one pixel alone always fits
            const int per = ngroups / nparts;       // (this block's groups: all of them unless the tile is shared)
            bool ok = true;
#pragma unroll 1
            for (int g = part * per; g < (part + 1) * per && ok; ++g) ok = run_group(g, kTilePix / ngroups, std::false_type());
            if (ok) break;
        }
    }

    if (tp.stats && tid == 0 && part == 0) tp.stats[vb] = *s_U | (ngroups << 16);
}

// one block per tile, XCD-remapped so that an XCD walks whole pairs
template <int KPL, int ROWS>
// (blocks per CU the register allocation aims at; ET_TILE_HUGE_MIN_BLOCKS: a development define for the 512-row instances --
//  measured in round 5, profiles/r05_config5_ab.txt)
#ifndef ET_TILE_HUGE_MIN_BLOCKS
#define ET_TILE_HUGE_MIN_BLOCKS 2
#endif
#ifndef ET_TILE_SMALL_MIN_BLOCKS     // (256-row instances; 1: the spill-free build of the packed-fp32 experiment, scripts/dev/README.md)
#define ET_TILE_SMALL_MIN_BLOCKS 3
#endif
__global__ __launch_bounds__(256, ROWS == kTileRowsSmall ? ET_TILE_SMALL_MIN_BLOCKS : (ROWS == kTileRowsHuge ? ET_TILE_HUGE_MIN_BLOCKS : 2)) void epipolar_fwd_tile_kernel(const TileParams tp)
{
    extern __shared__ float s_dyn[];
    fwd_tile_body<KPL, ROWS>(tp, xcd_remap(blockIdx.x, tp.f.total_blocks), s_dyn);
}

// list form: the tiles the warp-specialised kernel left over (row sets that overflow its arrays)
template <int KPL, int ROWS>
__global__ __launch_bounds__(256, 2) void epipolar_fwd_tile_list_kernel(const TileParams tp)
{
    extern __shared__ float s_dyn[];
    const int count = *tp.tile_count;
    // (a short list: eight blocks per tile, see fwd_tile_body.  Round 6 measured the alternatives -- three blocks per compute unit
    //  for the 256-row instance, 2 / 4 / 8 blocks per tile by the list's length -- and none moves a call on any rig:
    //  profiles/r06_fwd_ab.txt, block 15)
    const int nparts = count * 8 <= (int)gridDim.x ? 8 : 1;
#pragma unroll 1
    for (int idx = blockIdx.x; idx < count * nparts; idx += gridDim.x) {
        fwd_tile_body<KPL, ROWS>(tp, tp.tile_list[idx / nparts], s_dyn, idx % nparts, nparts);
        __syncthreads();
    }
}
