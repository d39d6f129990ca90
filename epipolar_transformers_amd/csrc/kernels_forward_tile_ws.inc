// Part of et_forward_tile.hip (inside its anonymous namespace): the warp-specialised, persistent form of the MFMA
// tile forward (kernels_forward_tile.inc explains the tile formulation itself).
// ----------------------------------------------------------------------------
// The one-block-per-tile kernel runs a tile's stages one after the other (set-up -> GEMM 1 -> soft-max ->
// GEMM 2) and relies on three co-resident blocks per CU to overlap them: every block is a serial, latency-bound
// chain of ~147 k cycles for 20 k cycles of matrix work, and the matrix pipes sit at 38 %.  Here ONE block per
// CU stays resident and walks a list of tiles with its waves split into two roles:
//
//   matrix waves (4, one per SIMD)   only MFMA work:  G1(t) D = F1_t . F2_U^T   and   G2(t) out = B . F2_U
//   vector waves (NV = 8)            everything else: S1 geometry (segments, sample cells -> column masks + per-sample
//                                    (x, y) table), S2 row list + pixel -> slot table (the wave that finishes S1
//                                    last), SM resample / masked soft-max / B rows (split to fp16 in place), the
//                                    reference rows -> fp16 A stage (+ res_base on request)
//
// in a software pipeline over the block's tile sequence T_0, T_1, ... with two block barriers per step i:
//
//   phase A(i):   matrix  G1(T_i), prefetch G2(T_{i-1})     | vector  S1(T_{i+1}), last wave to finish: S2(T_{i+1})
//   phase B(i):   matrix  G2(T_{i-1}), prefetch G1(T_{i+1}) | vector  [row loads of T_{i+1}], SM(T_i), A stage(T_{i+1})
//
// so the operands of G1(T_{i+1}) (the fp16 A stage in LDS and the first ring of B loads) are ready or in flight
// when the barrier before phase A(i+1) falls.  Which role does what was settled with per-phase cycle counters
// (-DET_WS_PROFILE=2, scripts/ws_profile.py): the two roles are within 10 % of each other in both phases.
//
// The vector side is bound by instruction issue (one VALU instruction per ~4 cycles and SIMD, shared with the
// matrix wave), so the per-sample geometry is evaluated ONCE: S1 leaves every sample's un-normalised tap-space
// location (x, y) in an LDS table (8 bytes per sample; samples without any tap inside the image are parked at
// (-2, -2)), and S2 turns the tile's row set into the row list AND into a pixel -> slot table over the
// map padded by two pixels on every side, whose border entries permanently name the pad column (an always-zero
// column of D).
//
// The row set.  The 32 lines of a tile nearly coincide (tile_order_kernel sorts the pixels by line), so every source
// pixel the tile touches lies within a few rows of ONE line: tile_order_kernel leaves that base line per tile
// (minor = a + b * major along the axis it mostly runs, |b| <= 1), and the set is kept as one 16-bit mask per column u
// of the major axis: bit i <-> minor coordinate floor(a + b u) - 1 + i.  S1 ORs two masks per sample (its 2 x 2 taps =
// two rows in each of two columns) into a 68-word LDS array -- neighbouring samples sit in neighbouring columns, i.e. in
// different words and banks.  (Rounds 1-3 kept a bitmap over the whole map: four ds_or per sample, and the 64 samples of
// a line along a map row fall into TWO words of it -- the atomics serialised, S1 alone took 5-7 k of the tile's 35 k
// cycles, every wave then prefix-scanned all 128 words behind a spinning barrier.)  The wave that finishes S1 last
// (a counter in LDS tells it) runs S2 alone, lanes <-> columns: mask & in-image rows, one wave prefix sum of the
// popcounts, <= 16 rows per column written out -- a few hundred cycles, nobody waits in a spin loop.  A tile with a tap
// outside its 16-row window (three in a thousand: the tiles where the sort order wraps) goes to the overflow list.  SM then needs no validity tests and no popcount ranks: two floors, one address, four 16-bit slot
// reads, four D reads, four FMAs.  (Entries of the slot table are only ever read at taps of the tile that wrote
// them, so it is never cleared.)
//
// The matrix work itself: on gfx950 an MFMA and the VALU instructions of ANY wave of the same SIMD exclude each other
// (measured, scripts/micro/mfma_valu_*.hip: co-resident MFMA-only and VALU-only waves take the SUM of their times,
// s_setprio changes nothing), and v_mfma_f32_32x32x2_f32 runs at the fp32 VECTOR rate -- 64 cycles per MFMA, 20.5 k
// cycles per tile and SIMD, more than everything else together.  The fp16 matrix cores are 16x faster per product,
// so both GEMMs run as SPLIT-fp16 products with fp32 accumulation:
//
//     x * s = hi + lo exactly,  hi = the top 11 significant bits of x * s (round-toward-zero conversion: exact),
//     lo = fp16(x * s - hi) (the next 11 bits),        a . b  ~=  (ahi . bhi + ahi . blo + alo . bhi) / (sa sb)
//
// three fp16 MFMAs (v_mfma_f32_32x32x16_f16 / 16x16x32) per 16 channels instead of eight fp32 MFMAs: 5.3x less matrix
// time (et_split_f16.h).  The dropped
// lo . lo term and the rounding of lo are 2^-21 relative per product -- the same size as the rounding of the fp32
// accumulation itself (measured on the CPU against float64: 2.8e-5 vs 2.2e-5 for a plain fp32 GEMM at |D| = 72).
// s is a power of two per pair and map (tile_order_kernel places an estimate of the map's largest magnitude at
// 2^10); every converted value is checked, and a tile that meets a value beyond fp16's range is handed to the
// exact-fp32 one-block-per-tile kernel through the overflow list.  The reference tile A (32 x 256) is converted once
// per tile by the vector waves (they read those rows anyway, for res_base) into an fp16 hi / lo stage in LDS.
//
// A tile whose row set exceeds the array is not split here: it is appended to an overflow list in the
// workspace and the one-block-per-tile kernel (which knows how to split) runs over that list afterwards.
// K <= 64 only (lanes <-> samples).  Two instances: maps up to 64 x 64 (256-row arrays; lanes <-> columns in S2; the slot
// table over the whole map) and, BT = true, maps up to 96 x 96 (288-row arrays -- every tile of a 96 x 96 map has at most 280
// rows --, two columns per lane in S2, and the slot table over the tile's band only: 16 entries per column, rewritten whole by S2
// for every tile; the whole-map table would be 2 x 20 KB there and the block is at the LDS limit).  On small maps the second
// returns what the first returns bit for bit (tests/test_gpu_band.py) and is 10 % slower.

#include "et_lds_layout.h"     // where the fp16 MFMA operands sit in LDS; G1's lane trade

struct TileWsParams {
    FwdParams f;
    const int *perm;     // (total_tiles * 32) reference pixels in epipolar-line order, -1 = padding
    int tiles_per_pair;
    int total_tiles;
    int rows_cap;        // row-set capacity (ROWS; smaller only to test the overflow path)
    int *ovf_count;      // workspace: number of overflow tiles (zeroed by tile_order_kernel)
    int *ovf_list;       // workspace: their tile ids
    int *stats;          // workspace: per tile  U | 1 << 16  (0 for overflow tiles until the second kernel fills it)
    int setprio;         // tuning: raise the priority of the matrix waves
    const float4 *segs;  // workspace: (total_tiles * 32) epipolar segments in the same order (tile_order_kernel)
    const float *scales; // workspace: per pair { s_ref, 1 / s_ref, s_src, 1 / s_src } (tile_order_kernel)
    const float4 *band;  // workspace: per tile { a, b, x-major ? 1 : 0, - }: the tile's base line (tile_order_kernel)
    // FUSED kernel only (et_epipolar_forward_fused): x = feat_ref + bias + out . Wf^T as a third GEMM behind G2
    const unsigned *packed_w;   // Wf as residual_gemm_pack_kernel lays it out (+ 1 / its scale behind the fragments)
    const float *bias;          // (256)
    float *x;                   // (N, H, W, 256)
    int *err;                   // workspace: sticky error word (bit 1: a matrix wave gave up at the barrier in front of G3)
    int *tile_ctr;              // workspace: one tile counter per XCD (zeroed by tile_order_kernel): the blocks of an XCD draw
                                // their tiles from it
    long long *prof;     // ET_WS_PROFILE builds only: per (block, wave) cycle totals of the pipeline segments
};

constexpr unsigned kWsColOvf = 0x80000000u;   // a tap outside the column's 16-row window
// dynamic LDS of a block: the layout the kernel takes its pointers from (et_tile_layout.h, with the slot tables, the column
// masks and the A stages it places)
constexpr size_t tile_ws_lds_bytes(int rows, int H, int W, bool band_table = false)
{
    return (size_t)tile_ws_lds(rows, H, W, band_table).bytes;
}

#include "et_split_f16.h"

constexpr float kF16Guard = 32768.f;   // |x * s| must stay below this (fp16 max 65504)
constexpr float kF16ResultGuard = 3.0e38f;   // G1's guard on its results: a finite accumulator (see g1_main)

// Block barrier that orders LDS traffic only.  Everything the waves of a block hand each other lives in LDS;
// __syncthreads() would also drain the vector-memory counter, i.e. make the matrix waves wait for their `out`
// stores and for the operand loads they issue ahead of the barrier on purpose.
__device__ __forceinline__ void lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// The vector waves count themselves in when their share of S1 is done (a monotonic LDS counter, one increment per wave
// and step); the wave that brings the count to `target` knows every other wave's column masks are in LDS -- each wave
// releases its LDS traffic before it increments -- and runs S2.  Nobody waits: the others go on to the block barrier.
__device__ __forceinline__ bool vector_arrive_last(int *counter, int target, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    int old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    old = __builtin_amdgcn_readfirstlane(old);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    return old == target - 1;
}

// Barrier among the four matrix waves (the hardware barrier counts every wave of the block): a monotonic LDS counter, one
// increment per wave, polled with s_sleep.  The four waves run the same straight-line code on the same tile, so the wait is
// short; the spin is bounded all the same, and a wave that gives up says so in the workspace's sticky error word (the results
// of that call are invalid; ops.check_tile_errors raises) instead of hanging the device.
__device__ __forceinline__ void matrix_barrier(int *counter, int target, int lane, int *err)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    if (lane == 0) __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    bool ok = false;
    for (int spin = 0; spin < (1 << 18); ++spin) {
        if (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= target) {
            ok = true;
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    if (!ok && lane == 0) atomicOr(err, 2);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// inclusive prefix sum over the 64 lanes on DPP (row shifts, then the two row broadcasts)
__device__ __forceinline__ int wave_scan_incl(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2 and 3
    return v;
}

// KH = 2 (round 6): 64 < K <= 128 as TWO passes of 64 samples per tile with an online soft-max.  A step of the pipeline is then a
// HALF tile -- step i = half (i & 1) of the block's tile number i >> 1: samples 64 h .. 64 h + 63 of the tile's 32 pixels, with a
// row set, a D / B array and a G1 / G2 of its own (half a segment touches about half the rows: the 288-row arrays hold it where the
// one-block-per-tile kernel needs 512).  What couples the halves is the soft-max (epipolar.py:303-307 over all K samples):
//   SM(h = 0):  m0 = max logit, p_k = exp(l_k - m0), s0 = sum p_k;  B rows from the UNNORMALISED p_k;  logits kept in registers
//   G2(h = 0):  O0 = B . F2_U, stashed in LDS (the wave's own accumulators: no exchange)
//   SM(h = 1):  m = max(m0, max logit), alpha = exp(m0 - m), s = s0 alpha + sum p_k;  B rows from p_k = exp(l_k - m);
//               attention of BOTH halves (exp(l - m) / s), arg-max over all K, corr_pos;  alpha and 1 / s per pixel -> LDS
//   G2(h = 1):  out = (O0 alpha + B . F2_U) / s        -- the flash-attention recurrence with two blocks.
// The A stage (one, not two: the second stage's bytes are the stash) is written once per tile, behind the second half's SM.
template <int ROWS, int NV, bool FUSED = false, bool BT = false, int KH = 1>
__global__ __launch_bounds__((kWsMatrixWaves + NV) * kWave) void epipolar_fwd_tile_ws_kernel(const TileWsParams tp)
{
    static_assert(KH == 1 || (KH == 2 && BT && !FUSED), "two sample passes: the band-table instance, sample + attention only");
    constexpr int kColWords = BT ? kWsColWordsBand : kWsColWords;
    constexpr int STRIDE = ROWS + 4;    // 16-byte aligned rows (G2 reads the B rows as b128); pad column = ROWS
    constexpr int C = 256, kRowBytes = C * 4;
    constexpr int PW = kTilePix / NV;   // pixels per vector wave
    constexpr int PB = 4;               // pixels per batch of the lanes <-> samples stages
    constexpr int kArr = kTilePix * STRIDE;
    constexpr int kOob = 0x7ffff000;    // past every buffer: raw buffer loads return zeros, stores are dropped
    constexpr int kDropped = 0x7ffffff0;
    constexpr int kPad = ROWS;          // the pad column of the D/B arrays: always zero when SM reads D
    static_assert(PW % PB == 0, "vector waves own a multiple of four pixels");
    static_assert(NV == 8, "the A stage scales four rows per wave at a time");
    extern __shared__ float s_dyn[];
    const FwdParams &p = tp.f;
    const EtLayerDesc &d = p.d;
    const int H = d.H, W = d.W, K = d.K;
    const int HW = H * W;
    const int PWD = tile_ws_slot_width(W);       // width of the padded pixel -> slot table
    const int slot_entries = tile_ws_slot_table_entries(H, W, BT);

    const TileWsLds L = tile_ws_lds_of(ROWS, slot_entries, BT);
    char *const s_base = reinterpret_cast<char *>(s_dyn);
    float *s_arr = reinterpret_cast<float *>(s_base + L.arr);               // [2][32][STRIDE]
    int *s_rows = reinterpret_cast<int *>(s_base + L.rows);                 // [3][ROWS]
    int *s_pix = reinterpret_cast<int *>(s_base + L.pix);                   // [3][32]
    float *s_seg = reinterpret_cast<float *>(s_base + L.seg);               // [3][32][4]
    int *s_U = reinterpret_cast<int *>(s_base + L.U);                       // [3] U (or -1: overflow tile, skipped); [4] barrier counter of the vector waves
    int *s_tq = reinterpret_cast<int *>(s_base + L.tq);                     // [8] ring of this block's tile ids (-1: none left)
    float *s_ainv = reinterpret_cast<float *>(s_base + L.ainv);             // [2][32] 1 / scale of the rows of the A stages
    float *s_band = reinterpret_cast<float *>(s_base + L.band);             // [3][4] base line of the slot's tile (SM of the band-table kernel)
    int *s_dead = reinterpret_cast<int *>(s_base + L.dead);                 // [4] KH == 2: tile (sequence number & 3) left to the list kernels
    float *s_alpha = reinterpret_cast<float *>(s_base + L.alpha);           // [32] KH == 2: exp(m0 - m) per pixel of the tile (SM of half 1 -> G2)
    float *s_rinv = reinterpret_cast<float *>(s_base + L.rinv);             // [32]          1 / (sum over all K samples)
    unsigned *s_col = reinterpret_cast<unsigned *>(s_base + L.col);         // [kColWords] column masks of the tile in S1 / S2
    unsigned short *s_slot = reinterpret_cast<unsigned short *>(s_base + L.slot);  // [2][slot_entries]
    // (an offset of the layout, not a rounded pointer, and a multiple of 256 bytes: see TileWsLds::astage)
    const int ahi_off = L.astage;
    // TWO A stages (tile j uses stage j & 1) since round 6: the (x, y) sample table that used to take these 32 KB is in registers,
    // and with a stage of its own the A tile of T_{i+1} can be written while G1(T_i) reads the other one -- see kCopyInA.
    constexpr int kAStageBytes = kWsAStageBytes;
    char *s_ahi = s_base + ahi_off;                                     // [2] x { [32][512 B] fp16 hi of the scaled A tile,
    char *s_alo = s_ahi + kTilePix * kWsAStageRow;                          //         [32][512 B] fp16 lo }
    // KH == 2: ONE A stage (both halves of a tile multiply the same reference rows); the second stage's bytes are the stash of
    // the first half's G2 accumulators: 8 KB per matrix wave, a lane's registers at lane-private addresses (no exchange)
    auto astage_of = [&](int j) { return KH == 2 ? 0 : (j & 1); };
    float *s_stash = reinterpret_cast<float *>(s_base + L.stash);          // (kWsStashBytes: fits the second stage, et_tile_layout.h)

    // ---- this block's tile sequence: XCD x (hardware: block b -> XCD b % 8) owns a contiguous chunk of the
    // tile list and its blocks walk it side by side, so the tiles in flight on an XCD belong to one or two
    // pairs whose source maps stay in its L2 ----
    const int b = blockIdx.x;
    const int xcd = b % kXcds;
    const int cq = tp.total_tiles / kXcds, cr = tp.total_tiles % kXcds;
    const int cstart = xcd * cq + min(xcd, cr), clen = cq + (xcd < cr ? 1 : 0);
    // The blocks of an XCD DRAW their tiles from one counter: one returning atomic per block and step, issued at the start of a
    // step and consumed at its end, a step before the tile is first needed -- its latency is never waited for.  Rounds 2-4 gave
    // block jx of the XCD the tiles jx, jx + nbx, ..: every block had its 64 tiles whatever they cost (a tile's row set is
    // 48 .. 238 rows), the blocks of an XCD drifted apart, and the rows a tile shares with its neighbours (70 %) were asked for
    // at different times and fetched from HBM more than once: 2.87 GB per launch against 1.75 GB algorithmic.  Drawn: 1.91 GB
    // (L2 hit rate 73 -> 83 %), and no block waits for the slowest at the end: the forward call 0.99 -> 0.915 ms, the one-kernel
    // layer 1.23 -> 1.16 ms (profiles/r04_fwd_ab.txt).  Tile ids travel through a ring of eight in LDS: step i reads the tiles
    // of steps i - 1 .. i + 2 and writes that of step i + 3.
    // (KH == 2: steps 2 q and 2 q + 1 are the two halves of the block's q-th tile)
    auto seq_of = [&](int j) { return KH == 2 ? j >> 1 : j; };
    auto half_of = [&](int j) { return KH == 2 ? j & 1 : 0; };
    auto tile_of = [&](int j) { return __builtin_amdgcn_readfirstlane(s_tq[seq_of(j) & 7]); };
    auto has_tile = [&](int j) { return j >= 0 && __builtin_amdgcn_readfirstlane(s_tq[seq_of(j) & 7]) >= 0; };
    int drawn = 0;
#ifdef ET_WS_PROFILE
    int drawn_static = b / kXcds;           // (experiment bit 2: block jx of the XCD takes tiles jx, jx + nbx, .. -- no atomic)
    const int nbx = ((int)gridDim.x - xcd + kXcds - 1) / kXcds;
#endif
    auto draw_issue = [&](bool who) {       // (one lane of one wave)
#ifdef ET_WS_PROFILE
        if (tp.setprio & 2) {
            if (who) {
                drawn = drawn_static;
                drawn_static += nbx;
            }
            return;
        }
#endif
        if (who) drawn = __hip_atomic_fetch_add(tp.tile_ctr + xcd, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto draw_commit = [&](int q, bool who) {      // q: the tile's sequence number in this block
        if (who) s_tq[q & 7] = drawn < clen ? cstart + drawn : -1;
    };

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool is_matrix = wave < kWsMatrixWaves;
    const int li = lane & 31, lh = lane >> 5;
    const unsigned map_bytes = (unsigned)HW * C * 4u;
    const float neg_inf = -__builtin_huge_valf();

    if (tid < kColWords) s_col[tid] = 0u;
    for (int t = tid; t < slot_entries; t += blockDim.x)   // both tables: every entry names the pad column
        reinterpret_cast<unsigned *>(s_slot)[t] = (unsigned)kPad | ((unsigned)kPad << 16);
    if (tid < 8) s_U[tid] = tid < kWsSlots ? -1 : 0;
    if (tid < 4) s_dead[tid] = 0;
    if (tid == kWsMatrixWaves * kWave) {     // (lane 0 of the first vector wave: the one that draws)
        for (int j = 0; j < 2; ++j) {       // (tiles 0 and 1; step i commits the tile of step i + 3, starting with i = -1 --
            draw_issue(true);               //  KH == 2: an even step i commits tile i / 2 + 2, the tile of steps i + 4 and i + 5)
            draw_commit(j, true);
        }
        for (int j = 2; j < 8; ++j) s_tq[j] = -1;
    }
    __syncthreads();
    if (!has_tile(0)) return;

    // =====================================================================================================
    // matrix waves
    // =====================================================================================================
    // G1(T_j): D = (F1_t . F2_U^T) as split-fp16 products on v_mfma_f32_16x16x32_f16 (16 pixels x 16 rows x 32 channels).
    //   * Loads.  The load path merges the addresses of a lane QUAD only (scripts/micro/load_patterns.hip: an
    //     instruction whose quads each read 64 contiguous bytes runs at 32-40 B/clk per CU; in operand order -- lane
    //     n = row n, so neighbouring lanes are 1 KB apart -- it is 15 B/clk, and G1 was bound by exactly that:
    //     192 KB per tile = 12 k cycles).  So a lane LOADS 16 bytes of row (lane >> 2), one chunk of a 64-byte segment
    //     (chunk lane & 3 for rows 0-7 of the unit, (lane & 3) ^ 2 for rows 8-15: et_g1_loaded_chunk): two instructions
    //     (segments e = 0, 1) per 16-row unit and 32-channel k-step.
    //   * Operand order.  The MFMA wants lane (n, kg) = (lane & 15, lane >> 4) to hold eight k-values of row n: the
    //     loaded registers are rearranged with ds_bpermute (the LDS crossbar, no LDS memory; lane (n, kg) takes the
    //     registers of the lane that loaded chunk kg of row n, et_g1_source_lane: ONE address for all sixteen registers
    //     of a k-step.  The chunk order of rows 8-15 makes the 32 sources of a half-wave distinct mod 32: with 4 n + kg
    //     throughout they were two to a residue, which SQ_LDS_BANK_CONFLICT counts -- 2.2e7 per launch of the headline
    //     shape, profiles/lds_layout_ab.txt -- although the instruction takes the same time for every pattern,
    //     scripts/micro/bpermute_patterns.hip).  Lane (n, kg) then holds
    //     channels 32 ks + 16 e + 4 kg + w (e, w = segment, word); the k order is ours to choose -- the fp16 A stage
    //     is written in the same order (copy_finish), so the A fragments stay single 16-byte LDS reads.
    //   * B rows go through a ring of kD1 k-steps of registers that runs across the wave's units; the first ring
    //     fill is issued one phase early (g1_prefetch).
    //   * Work split: 16-row UNITS dealt out round robin (wave w: units w, w + 4, w + 8, w + 12), each against both
    //     16-pixel halves of the tile.  With U ~ 165 that is 11 units: 3 + 3 + 3 + 2 (whole 32-row blocks gave
    //     2 + 2 + 1 + 1 blocks: two waves idle for a third of the phase).
    //   * Round 6 tried the LAST units of a tile on the vector waves, which wait for G1 in every phase A: the call got 4-9 %
    //     slower, because G1 is bound by the CU's LDS pipe whoever issues its work (profiles/r06_fwd_ab.txt, call 11).
    constexpr int kD1 = 6;      // ring depth in 32-channel k-steps
    constexpr int kUnits = (ROWS + 63) / 64;          // units per wave at most
    float4 bring[kD1][2];        // [flat k-step mod kD1][segment e]
    int boff[kUnits];
    auto g1_prefetch = [&](int j, bool valid) {
        const int slot = j % kWsSlots;
        const int U = valid ? s_U[slot] : 0;
#pragma unroll
        for (int ui = 0; ui < kUnits; ++ui) {
            const int unit = wave + 4 * ui;
            boff[ui] = kOob;
            if (U > 0 && unit < ((U + 15) >> 4))
                boff[ui] = s_rows[slot * ROWS + min(unit * 16 + (lane >> 2), U - 1)] * kRowBytes + et_g1_loaded_chunk(lane) * 16;
        }
        const int n = valid ? tile_of(j) / tp.tiles_per_pair : 0;
        const __amdgpu_buffer_rsrc_t src = make_rsrc(p.fsrc + (size_t)pair_map(p.src_index, n, p.M_src) * HW * C, map_bytes);
#pragma unroll
        for (int ks = 0; ks < kD1; ++ks)
#pragma unroll
            for (int e = 0; e < 2; ++e)             // (offsets past the map: zeros, no traffic)
                bring[ks][e] = buf_load_f4(src, boff[0] + ks * 128 + e * 64, 0);
    };
    auto g1_main = [&](int j) {
        const int slot = j % kWsSlots;
        const int U = s_U[slot];
        if (U <= 0) return;
        const int n = tile_of(j) / tp.tiles_per_pair;
        const __amdgpu_buffer_rsrc_t src = make_rsrc(p.fsrc + (size_t)pair_map(p.src_index, n, p.M_src) * HW * C, map_bytes);
        const float s_src = tp.scales[n * 4 + 2];
        const float inv = tp.scales[n * 4 + 3];          // 1 / s_src; the A rows carry their own scales (s_ainv)
        const int nunits = (U + 15) >> 4;                // 16-row units of the tile
        if (wave >= nunits) return;
        float *dst = s_arr + (j & 1) * kArr;
        float amax = 0.f;
        const int paddr = et_g1_source_lane(lane & 15, lane >> 4) * 4;
        // this lane's chunk (k-step 0, k-group lane >> 4) of pixel row lane & 15, as an offset into the block's LDS; the chunk of
        // k-step ks is at that offset ^ et_astage_kstep_xor(ks) (one XOR per k-step; rows + 16 and the lo stage: constants)
        const int aoff = ahi_off + astage_of(j) * kAStageBytes + et_astage_off(lane & 15, 0, lane >> 4);
        constexpr int kALo = kTilePix * kWsAStageRow;
        // straight-line over the units and their k-steps, forward exits only (exact vmcnt waits, see G2)
        // Round 6: the LDS stage of a k-step -- eight ds_bpermute of the loaded B registers, four fragment reads of the A stage --
        // is issued ONE k-step ahead, into a second set of registers (24 more).  Until then every k-step began with those twelve
        // LDS operations and waited for them (~200 cycles with nothing else to issue: the matrix wave is alone on its SIMD for
        // most of phase A), 24-30 times per tile and wave: about half of G1's 10 k cycles.
        float pv[2][8];
        f16x8 afh[2][2], afl[2][2];
        auto lds_stage = [&](int t, float (&pvd)[8], f16x8 (&ah)[2], f16x8 (&al)[2]) {      // k-step t (flat): permute + A fragments
            const int ks = t & 7;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float4 x = bring[t % kD1][e];
                pvd[4 * e + 0] = __int_as_float(__builtin_amdgcn_ds_bpermute(paddr, __float_as_int(x.x)));
                pvd[4 * e + 1] = __int_as_float(__builtin_amdgcn_ds_bpermute(paddr, __float_as_int(x.y)));
                pvd[4 * e + 2] = __int_as_float(__builtin_amdgcn_ds_bpermute(paddr, __float_as_int(x.z)));
                pvd[4 * e + 3] = __int_as_float(__builtin_amdgcn_ds_bpermute(paddr, __float_as_int(x.w)));
            }
            const char *ap = reinterpret_cast<const char *>(s_dyn) + (aoff ^ et_astage_kstep_xor(ks));
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                ah[g] = *reinterpret_cast<const f16x8 *>(ap + g * 16 * kWsAStageRow);
                al[g] = *reinterpret_cast<const f16x8 *>(ap + g * 16 * kWsAStageRow + kALo);
            }
        };
        lds_stage(0, pv[0], afh[0], afl[0]);
#pragma unroll
        for (int ui = 0; ui < kUnits; ++ui) {
            if (ui > 0 && wave + 4 * ui >= nunits) break;
            f32x4 acc[2];                             // [pixel half]
            acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int t = ui * 8 + ks;            // flat k-step
                const int slot_r = t % kD1;
                // the LDS stage of the NEXT k-step (past the wave's last unit: zeros from beyond the map, never used)
                if (t + 1 < kUnits * 8) lds_stage(t + 1, pv[(t + 1) & 1], afh[(t + 1) & 1], afl[(t + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                f16x8(&ahi)[2] = afh[t & 1];
                f16x8(&alo)[2] = afl[t & 1];
                float v[8];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    // (packed multiplies: two values per instruction -- 1.5 % of the forward call, profiles/r04_fwd_ab.txt)
                    const f32x2 s2 = {s_src, s_src};
                    const f32x2 p0 = f32x2{pv[t & 1][4 * e + 0], pv[t & 1][4 * e + 1]} * s2;
                    const f32x2 p1 = f32x2{pv[t & 1][4 * e + 2], pv[t & 1][4 * e + 3]} * s2;
                    v[4 * e + 0] = p0.x;
                    v[4 * e + 1] = p0.y;
                    v[4 * e + 2] = p1.x;
                    v[4 * e + 3] = p1.y;
                }
                f16x8 bhi, blo;
                split_f16x8<false>(v, bhi, blo, amax);
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo[g], bhi, acc[g], 0, 0, 0);
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi[g], blo, acc[g], 0, 0, 0);
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi[g], bhi, acc[g], 0, 0, 0);
                }
                // (pinned: left alone, the scheduler converts a ring entry right behind its load and every k-step
                //  waits a memory latency)
                __builtin_amdgcn_sched_barrier(0);
                if (t + kD1 < kUnits * 8) {               // (a unit the wave does not have: past the map, zeros)
                    const int tn = t + kD1;
#pragma unroll
                    for (int e = 0; e < 2; ++e)
                        bring[slot_r][e] = buf_load_f4(src, boff[tn >> 3] + (tn & 7) * 128 + e * 64, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // (address from an opaque copy of the lane id: hoisted out of the k-loop it gets spilled, and the reload --
            //  a vector-memory instruction -- drains the operand ring)
            int lane_o = lane;
            asm volatile("" : "+v"(lane_o));
            float *drow = dst + (4 * (lane_o >> 4)) * STRIDE + (wave + 4 * ui) * 16 + (lane_o & 15);
            const f32x4 ai0 = *reinterpret_cast<const f32x4 *>(s_ainv + astage_of(j) * kTilePix + 4 * (lane_o >> 4));
            const f32x4 ai1 = *reinterpret_cast<const f32x4 *>(s_ainv + astage_of(j) * kTilePix + 16 + 4 * (lane_o >> 4));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                drow[r * STRIDE] = (acc[0][r] * ai0[r]) * inv;
                drow[(16 + r) * STRIDE] = (acc[1][r] * ai1[r]) * inv;
            }
            // The fp16 guard, on the RESULTS since round 6 (eight values per lane and unit instead of a running maximum over all
            // 128 converted values: 4 VALU instructions per unit instead of 32).  A scaled source value v beyond fp16's range shows
            // up in every product it enters: hi = RTZ16(v) saturates at 65504, lo = RN16(v - hi) is exact below 65520 -- so
            // |v| < 131024 is still represented EXACTLY as hi + lo -- and infinite from there on; inf times anything (0 included:
            // NaN) makes the sums of the row's 32 D values non-finite.  NaN / inf inputs propagate the same way.
            // amax accumulates the SUM of the magnitudes (NaN and inf are sticky in a sum; a maximum would drop a NaN).
            amax += ((fabsf(acc[0][0]) + fabsf(acc[0][1])) + (fabsf(acc[0][2]) + fabsf(acc[0][3]))) +
                    ((fabsf(acc[1][0]) + fabsf(acc[1][1])) + (fabsf(acc[1][2]) + fabsf(acc[1][3])));
        }
        // overflow guard: some source value of this tile is beyond fp16's range -> the tile is redone in fp32
        if (__builtin_amdgcn_ballot_w64(!(amax < kF16ResultGuard)) != 0 && lane == 0) {
            // (KH == 2: the TILE goes to the list once, whichever half trips first; the other half's outputs are suppressed)
            if (atomicExch(&s_U[slot], -1) >= 0 && (KH == 1 || atomicExch(&s_dead[seq_of(j) & 3], 1) == 0))
                tp.ovf_list[atomicAdd(tp.ovf_count, 1)] = tile_of(j);
        }
    };
    // The reference rows of T_jc (1 KB per pixel, read once), on the VECTOR waves (the matrix waves are the critical
    // path of both phases): wave vw takes pixels PW vw .. + PW - 1, a lane four channels.  The loads are issued at the
    // start of phase B, ahead of SM -- the pixel ids come straight from the tile list through the constant address
    // space (scalar loads: as plain global loads the compiler cannot prove them uniform-and-invariant and they cost
    // dependent memory latencies) -- and are consumed behind SM: (a) + bias -> res_base when the caller wants the
    // additive term of the residual fusion, (b) scaled and split -> the fp16 A stage of G1(T_jc) (idle in phase B);
    // a value beyond fp16's range sends the tile to the exact-fp32 kernel.
    // (Round 4 tried the copy on the matrix waves again, behind G2, where they now wait 5 k cycles for the vector waves:
    //  1.07 vs 1.00 ms -- and in phase A on the vector waves, which wait 5-7 k cycles there, with a second A stage in place of
    //  the sample table (locations recomputed in SM): 1.03 vs 1.00 ms; profiles/r04_fwd_ab.txt.  The waits are not free time:
    //  the LDS pipe and the SIMDs are shared, and moving work between the phases moves the contention with it.)
    // Round 6: the copy of T_{i+1} runs in phase A(i) (loads ahead of S1, conversion behind S2), where the vector waves used to wait
    // 4-6 k cycles for G1, instead of in phase B(i) behind SM, where they are the critical path (profiles/r06_fwd_ab.txt).
    constexpr bool kCopyInA = (KH == 1);     // (KH == 2: one stage -- behind the second half's SM, once per tile)
    constexpr int kCopyPix = kTilePix / NV;
    float4 crow[kCopyPix];
    int cpx[kCopyPix];
    float4 bias4 = f4_zero();
    typedef __attribute__((address_space(4))) const int *const_int_ptr;
    const const_int_ptr perm_c = (const_int_ptr)(unsigned long long)tp.perm;
    const int cfirst = (wave - kWsMatrixWaves) * kCopyPix;    // first pixel of this (vector) wave
    auto copy_load = [&](int jc, bool valid) {
        const int tl = valid ? tile_of(jc) : 0;
        const __amdgpu_buffer_rsrc_t ref = make_rsrc(p.fref + (size_t)pair_map(p.ref_index, tl / tp.tiles_per_pair, p.M_ref) * HW * C, valid ? map_bytes : 0u);
#pragma unroll
        for (int ii = 0; ii < kCopyPix; ++ii) {
            cpx[ii] = valid ? perm_c[(size_t)tl * kTilePix + cfirst + ii] : -1;
            crow[ii] = buf_load_f4_nt(ref, cpx[ii] >= 0 ? cpx[ii] * kRowBytes + lane * 16 : kOob, 0);   // (padding pixel: zeros)
        }
        bias4 = buf_load_f4(make_rsrc(p.res_bias, p.res_base && p.res_bias ? (unsigned)kRowBytes : 0u), lane * 16, 0);
    };
    auto copy_finish = [&](int jc, bool valid) {
        if (!valid) return;
        const int cn = tile_of(jc) / tp.tiles_per_pair;
        // every reference row under the power of two of ITS OWN largest magnitude (a wave reduction, four rows at a
        // time): exact, so nothing overflows and a row that is tiny next to the rest of its map keeps all its bits -- a
        // per-map scale flushed such a row to zero and turned "some samples masked" (epipolar.py:298) into "all masked"
        float m[kCopyPix];
#pragma unroll
        for (int ii = 0; ii < kCopyPix; ++ii)
            m[ii] = fmaxf(fmaxf(fabsf(crow[ii].x), fabsf(crow[ii].y)), fmaxf(fabsf(crow[ii].z), fabsf(crow[ii].w)));
        wave_all_max4(m);
#pragma unroll
        for (int ii = 0; ii < kCopyPix; ++ii) {
            float s_ref, s_inv;
            pow2_scale_of(m[ii], s_ref, s_inv);
            const float v[4] = {crow[ii].x * s_ref, crow[ii].y * s_ref, crow[ii].z * s_ref, crow[ii].w * s_ref};
            unsigned h0, l0, h1, l1;
            split_f16_pair(v[0], v[1], h0, l0);
            split_f16_pair(v[2], v[3], h1, l1);
            typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
            const f16x4 hi = __builtin_bit_cast(f16x4, u32x2_t{h0, h1}), lo = __builtin_bit_cast(f16x4, u32x2_t{l0, l1});
            // (the lane's channels 4 lane .. + 3 = 32 ks + 16 e + 4 kg + w go to fp16 position 32 ks + 8 kg + 4 e + w: G1's k order
            // = half e of the row's chunk (ks, kg) = (lane >> 3, lane & 3), at the chunk's slot of et_lds_layout.h)
            const int apos = et_astage_off(cfirst + ii, lane >> 3, lane & 3) + ((lane >> 2) & 1) * 8;
            *reinterpret_cast<f16x4 *>(s_ahi + astage_of(jc) * kAStageBytes + apos) = hi;
            *reinterpret_cast<f16x4 *>(s_alo + astage_of(jc) * kAStageBytes + apos) = lo;
            if (lane == 0) s_ainv[astage_of(jc) * kTilePix + cfirst + ii] = s_inv;
        }
        if (p.res_base) {
#pragma unroll
            for (int ii = 0; ii < kCopyPix; ++ii) {
                if (cpx[ii] < 0) continue;
                const float4 o = make_float4(crow[ii].x + bias4.x, crow[ii].y + bias4.y, crow[ii].z + bias4.z, crow[ii].w + bias4.w);
                __builtin_nontemporal_store(f32x4{o.x, o.y, o.z, o.w}, reinterpret_cast<f32x4 *>(p.res_base + ((size_t)cn * HW + cpx[ii]) * C + lane * 4));
            }
        }
    };
    // G2(T_j): out = (B . F2_U) as split-fp16 products, this wave's 64 channels.  K-steps of 16 rows: as MFMA operand
    // a lane (lh, s, cq) = (lane >> 5, (lane >> 4) & 1, lane & 15) supplies, for accumulator t, channel
    // c0 + 4 cq + 2 s + t of rows 16 ks + 8 lh .. + 7.  Loading it that way would take eight 8-byte loads per k-step
    // (32 lanes x 8 B of one row each): the load path of a CU handles ~one instruction per 40 cycles whatever its
    // width (measured, scripts/micro/load_patterns.hip: 12.8 B/clk for this pattern, 54 B/clk for 4 rows x 256 B per
    // instruction), and G2 then waits for its operands.  So a lane LOADS 16 bytes -- channels c0 + 4 cq .. + 3 of row
    // 16 ks + 8 lh + 4 s + q, q = 0..3: four instructions of 4 rows x 256 B per k-step -- and trades half of them
    // with lane ^ 16 (v_permlane16_swap: one instruction per register pair): afterwards it holds channels
    // 2 s, 2 s + 1 of its quad for rows 8 lh .. 8 lh + 7 in order.  A = the B rows in LDS (scaled by 2^10 and split to
    // fp16 hi | lo per group of eight columns by SM).  Ring of kD2 k-steps, row indices read one k-step before their loads; the first ring
    // fill is issued one phase early (g2_prefetch).  (Row indices / B columns past the padded row count: whatever
    // LDS holds there, inside the block's allocation; offsets past the map read zeros; their MFMAs are never issued.)
    constexpr int kD2 = 4;       // ring depth in 16-row k-steps (round 4: 5 -> 4 together with kD1 8 -> 6: -1.5 %, fewer live registers)
    int mb_target = 0;          // FUSED: barrier count of the matrix waves (the same on all four: uniform control flow)
    float4 xring[kD2][4];
    int ridx[4];
    auto g2_rows = [&](const int *rows, int ks) {   // row indices of this lane's four loads of k-step ks
        const int4 a = *reinterpret_cast<const int4 *>(rows + ks * 16 + (lane >> 4) * 4);   // 8 lh + 4 s
        ridx[0] = a.x; ridx[1] = a.y; ridx[2] = a.z; ridx[3] = a.w;
    };
    auto g2_prefetch = [&](int j, bool valid) {
        const int slot = valid ? j % kWsSlots : 0;
        const int n = valid ? tile_of(j) / tp.tiles_per_pair : 0;
        const float *srcp = p.fsrc + (size_t)pair_map(p.src_index, n, p.M_src) * HW * C;
        const int voff = (wave * 64 + 4 * (lane & 15)) * 4;
        const int *rows = s_rows + slot * ROWS;
        const int nks = valid ? (s_U[slot] + 15) >> 4 : 0;      // (U = -1, an overflow tile: 0)
#pragma unroll
        for (int ks = 0; ks < kD2; ++ks) {
            g2_rows(rows, ks);
            unsigned nbytes = ks < nks ? map_bytes : 0u;
            asm volatile("" : "+s"(nbytes));
            const __amdgpu_buffer_rsrc_t srck = make_rsrc(srcp, nbytes);
#pragma unroll
            for (int q = 0; q < 4; ++q) xring[ks][q] = buf_load_f4(srck, ridx[q] * kRowBytes + voff, 0);
        }
        g2_rows(rows, kD2);
    };
    auto g2_main = [&](int j) {
        const int slot = j % kWsSlots;
        const int U = s_U[slot];
        if (U < 0) return;
        const int half = half_of(j);
        if (KH == 2 && __builtin_amdgcn_readfirstlane(s_dead[seq_of(j) & 3]) != 0) return;   // (the tile went to the list kernels)
        const int n = tile_of(j) / tp.tiles_per_pair;
        const float *srcp = p.fsrc + (size_t)pair_map(p.src_index, n, p.M_src) * HW * C;
        const float s_src = tp.scales[n * 4 + 2];
        const float inv = tp.scales[n * 4 + 3] * (1.f / 1024.f);
        const float *s_D = s_arr + (j & 1) * kArr;
        const int *rows = s_rows + slot * ROWS;
        const int nks = (U + 15) >> 4;
        const int c0 = wave * 64;
        const int voff = (c0 + 4 * (lane & 15)) * 4;
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
        // KH == 2, second half: the accumulators start as the first half's (this wave's own stash), rescaled to the common
        // maximum: alpha = exp(m0 - m) of the row's pixel.  Register r <-> pixel (r & 3) + 8 (r >> 2) + 4 lh.
        float *stash = s_stash + wave * (2 * 16 * kWave) + lane * 4;
        if (KH == 2 && half == 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 al4 = *reinterpret_cast<const f32x4 *>(s_alpha + 8 * q + 4 * lh);
                const f32x4 o0 = *reinterpret_cast<const f32x4 *>(stash + q * 4 * kWave);
                const f32x4 o1 = *reinterpret_cast<const f32x4 *>(stash + (4 + q) * 4 * kWave);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc0[4 * q + e] = o0[e] * al4[e];
                    acc1[4 * q + e] = o1[e] * al4[e];
                }
            }
        }
        const float *arow = s_D + li * STRIDE + lh * 8;
        auto kstep = [&](int ks, float4 (&xr)[4]) {
            const f16x8 ahi = *reinterpret_cast<const f16x8 *>(arow + ks * 16);        // (split by SM, stage 8)
            const f16x8 alo = *reinterpret_cast<const f16x8 *>(arow + ks * 16 + 4);
            // trade with lane ^ 16: for every load q, (channel 0 with channel 2) and (channel 1 with channel 3).  An even
            // 16-lane row ends with (own first, partner's first), an odd one with (partner's second, own second): in
            // both, ev[] / od[] hold rows 8 lh + 0 .. 7 of the lane's channel 2 s / 2 s + 1.
            f32x2 v[8];
            const f32x2 s2 = {s_src, s_src};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                auto r0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(xr[q].x), __float_as_uint(xr[q].z), false, false);
                auto r1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(xr[q].y), __float_as_uint(xr[q].w), false, false);
                v[q] = f32x2{__uint_as_float(r0[0]), __uint_as_float(r1[0])} * s2;          // in the registers of (x, y)
                v[4 + q] = f32x2{__uint_as_float(r0[1]), __uint_as_float(r1[1])} * s2;      // ... of (z, w)
            }
            f16x8 ehi, elo, ohi, olo;
            split_f16x8_pairs(v, ehi, elo, ohi, olo);   // (the rows were checked by G1)
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, ehi, acc0, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, elo, acc0, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, ehi, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, ohi, acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, olo, acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, ohi, acc1, 0, 0, 0);
            // (pinned: see G1) refill this ring entry with k-step ks + kD2 (its row indices were read one k-step ago),
            // then read the row indices of k-step ks + kD2 + 1
            __builtin_amdgcn_sched_barrier(0);
            {   // (past the last k-step: a resource of zero bytes -- zeros, no traffic; the size goes through an opaque
                //  scalar, or the compiler turns the uniform condition into branches around the loads)
                unsigned nbytes = ks + kD2 < nks ? map_bytes : 0u;
                asm volatile("" : "+s"(nbytes));
                const __amdgpu_buffer_rsrc_t srck = make_rsrc(srcp, nbytes);
#pragma unroll
                for (int q = 0; q < 4; ++q) xr[q] = buf_load_f4(srck, ridx[q] * kRowBytes + voff, 0);
            }
            g2_rows(rows, ks + kD2 + 1);
            __builtin_amdgcn_sched_barrier(0);
        };
        // straight-line over the (at most ROWS / 16) k-steps with forward exits only: in a loop the compiler's wait
        // insertion drains the vector-memory counter at the loop head (every fifth k-step waited a full latency)
#pragma unroll
        for (int ks = 0; ks < ROWS / 16; ++ks) {
            if (ks > 0 && ks >= nks) break;
            kstep(ks, xring[ks % kD2]);
        }
        // accumulator t, column n = 16 s + cq  <->  channel c0 + 4 cq + 2 s + t
        if (KH == 2 && half == 0) {
            // first half: the unnormalised partial sums wait in LDS for the second half (same wave, same lanes)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                *reinterpret_cast<f32x4 *>(stash + q * 4 * kWave) = f32x4{acc0[4 * q], acc0[4 * q + 1], acc0[4 * q + 2], acc0[4 * q + 3]};
                *reinterpret_cast<f32x4 *>(stash + (4 + q) * 4 * kWave) = f32x4{acc1[4 * q], acc1[4 * q + 1], acc1[4 * q + 2], acc1[4 * q + 3]};
            }
        } else if (!FUSED || p.out) {
            float *outp = p.out + (size_t)n * HW * C + c0 + 4 * (lane & 15) + 2 * ((lane >> 4) & 1);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int pix = s_pix[slot * kTilePix + m];
                const float k = KH == 2 ? inv * s_rinv[m] : inv;          // (KH == 2: 1 / the sum over all K samples)
                if (pix >= 0) __builtin_nontemporal_store(f32x2{acc0[r] * k, acc1[r] * k}, reinterpret_cast<f32x2 *>(outp + (size_t)pix * C));
            }
        }
        if constexpr (FUSED) {
            // ---- G3(T_j): x = feat_ref + bias + out . Wf^T (bn(z(out)) + out + feat with the eval-mode BN folded into z:
            // epipolar.py:250-253, resnet.py:388), the tile's 32 rows x this wave's 64 output channels ----
            // The out tile goes through LDS as fp16 hi | lo (the contraction runs over ALL 256 channels of out, i.e. over
            // the four waves' accumulators): into the B rows G2 has just consumed -- 32 rows x 512 B of hi, then of lo, the
            // 16-byte chunks of a row XOR-swizzled by the row (et_g3_stage_off: by m & 15 -- a lane group of the fragment reads
            // below holds sixteen different rows; m & 7, until this layout, put two of them on every slot: 8 LDS cycles per read
            // instead of 4) so that those reads are conflict-free without padding (the buffer is 32 x 1040 B: two padded stages
            // would not fit).  Scale: the pair's
            // s_src -- out is a convex combination of source rows that passed the fp16 guard, so |out s_src| < 2^15.
            // Two barriers among the matrix waves: every wave is done reading the B rows / every wave has written its part.
            char *stage = reinterpret_cast<char *>(s_arr + (j & 1) * kArr);
            // (everything lane-dependent below is derived from an opaque copy of the lane id, per tile: hoisted out of the tile
            //  loop these values are spilled -- the matrix waves sit at the register ceiling -- and every reload is a
            //  vector-memory instruction in the middle of the operand rings)
            int lane3 = lane;
            asm volatile("" : "+v"(lane3));
            const int li3 = lane3 & 31, lh3 = lane3 >> 5;
            // The ring of weight fragments (two k-steps: the matrix waves are at the register ceiling -- three spill and lose 6 %;
            // feat rows loaded behind the loop to make room for three or four: 1-2 % slower, profiles/r04_fwd_ab.txt) is filled BEFORE
            // the barrier and the staging of the out tile: one weight-fetch latency of sixteen off the chain (-0.9 %, r05_fwd_ab.txt)
            const __amdgpu_buffer_rsrc_t r_w = make_rsrc(tp.packed_w, (unsigned)kRgPackedWords * 4u);
            // Round 6: FOUR k-steps deep.  A weight fetch takes ~600 cycles from L2 and a k-step 6 MFMAs = 192: two deep, every
            // k-step waited ~200 cycles for its fragments -- 3 k of the ~7.6 k cycles G3 adds to a tile.  The registers come from
            // the feat rows: they are loaded LATE, at k-steps 12 and 13, into what the ring no longer refills (behind the loop
            // their latency was exposed whole: 1-2 % slower in round 4; before the loop they cost the ring its depth).
            // THREE deep since the A fragments are read a k-step ahead (8 more registers: with four the fused instances spill
            // 52-60 bytes per lane); round 6 measured three and four as equal, the feat rows now load at k-steps 13 and 14.
            constexpr int kRing3 = 3;
            u32x4 bq[kRing3][4];      // [k-step mod kRing3][2 nb + term]
            const int woff = (wave * 2) * 2 * 1024 + lane * 16;     // fragment (ks, nb = 2 wave, hi) of this lane, bytes
            auto wload = [&](int ks, u32x4 (&dst)[4]) {
#pragma unroll
                for (int t = 0; t < 4; ++t) dst[t] = __builtin_amdgcn_raw_buffer_load_b128(r_w, woff + ks * 8 * 2 * 1024 + t * 1024, 0, 0);
            };
#pragma unroll
            for (int ks = 0; ks < kRing3; ++ks) wload(ks, bq[ks]);
            __builtin_amdgcn_sched_barrier(0);
            mb_target += kWsMatrixWaves;
            matrix_barrier(s_U + 5, mb_target, lane, tp.err);
            {
                const int cb = c0 + 4 * (lane3 & 15) + 2 * ((lane3 >> 4) & 1);      // this lane's channel pair (cb, cb + 1)
                const float k = inv * s_src;                                      // acc * k = out * s_src
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = (r & 3) + 8 * (r >> 2) + 4 * lh3;
                    unsigned hh, ll;
                    split_f16_pair(acc0[r] * k, acc1[r] * k, hh, ll);
                    const int off = et_g3_stage_off(m, cb >> 3) + (cb & 7) * 2;
                    *reinterpret_cast<unsigned *>(stage + off) = hh;
                    *reinterpret_cast<unsigned *>(stage + 16384 + off) = ll;
                }
            }
            __builtin_amdgcn_sched_barrier(0);      // (G2's accumulators are dead from here: nothing of G3 is hoisted above)
            // the feat rows and the bias of this wave's outputs: accumulator nb, register r  <->  row m(r), channel c0 + 32 nb + li
            const __amdgpu_buffer_rsrc_t refb = make_rsrc(p.fref + (size_t)pair_map(p.ref_index, n, p.M_ref) * HW * C, map_bytes);
            float fr[2][16];
            auto xoff_of = [&](int r) {      // (re-read from LDS where it is needed: sixteen offsets would cost sixteen registers)
                const int m = (r & 3) + 8 * (r >> 2) + 4 * lh3;
                const int pix = s_pix[slot * kTilePix + m];
                return pix >= 0 ? pix * kRowBytes + (c0 + li3) * 4 : kOob;
            };
            auto feat_load = [&](int nb) {      // (late, inside the k-loop below: see kRing3)
#pragma unroll
                for (int r = 0; r < 16; ++r) fr[nb][r] = buf_load_f1_nt(refb, xoff_of(r) + nb * 128, 0);      // (padding pixel: zeros)
            };
            const float bias0 = tp.bias[c0 + li], bias1 = tp.bias[c0 + 32 + li];
            const float unscale = tp.scales[n * 4 + 3] * reinterpret_cast<const float *>(tp.packed_w)[kRgPackedWords];
            f32x16 g0, g1;
#pragma unroll
            for (int r = 0; r < 16; ++r) g0[r] = g1[r] = 0.f;
            mb_target += kWsMatrixWaves;
            matrix_barrier(s_U + 5, mb_target, lane, tp.err);
            // The A fragments of a k-step are read ONE k-step ahead, into a second pair of registers (as G1's LDS stage): the
            // vector waves are at the barrier while the matrix waves run G3, so nothing else on the SIMD covers the latency of
            // a read issued right in front of the MFMAs that consume it.
            f16x8 ga[2][2];      // [k-step & 1][hi, lo]
            auto g3_frag = [&](int ks, f16x8 (&d)[2]) {     // A[m = li][k = 16 ks + 8 lh .. + 7]: chunk 2 ks + lh of row li
                const char *sp = stage + et_g3_stage_off(li, 2 * ks + lh);
                d[0] = *reinterpret_cast<const f16x8 *>(sp);
                d[1] = *reinterpret_cast<const f16x8 *>(sp + 16384);
            };
            g3_frag(0, ga[0]);
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) {
                if (ks + 1 < 16) g3_frag(ks + 1, ga[(ks + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                const f16x8 ah = ga[ks & 1][0], al = ga[ks & 1][1];
                u32x4(&bb)[4] = bq[ks % kRing3];
                g0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, __builtin_bit_cast(f16x8, bb[0]), g0, 0, 0, 0);
                g0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, __builtin_bit_cast(f16x8, bb[1]), g0, 0, 0, 0);
                g0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, __builtin_bit_cast(f16x8, bb[0]), g0, 0, 0, 0);
                g1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, __builtin_bit_cast(f16x8, bb[2]), g1, 0, 0, 0);
                g1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, __builtin_bit_cast(f16x8, bb[3]), g1, 0, 0, 0);
                g1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, __builtin_bit_cast(f16x8, bb[2]), g1, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (ks + kRing3 < 16) wload(ks + kRing3, bq[ks % kRing3]);
                else if (ks == 16 - kRing3) feat_load(0);
                else if (ks == 17 - kRing3) feat_load(1);
                __builtin_amdgcn_sched_barrier(0);
            }
            const __amdgpu_buffer_rsrc_t xb = make_rsrc(tp.x + (size_t)n * HW * C, map_bytes);
#pragma unroll
            for (int r = 0; r < 16; ++r) {     // (padding pixel: offset past the buffer, the store is dropped)
                const int xo = xoff_of(r);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((fr[0][r] + bias0) + g0[r] * unscale), xb, xo, 0, 2);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((fr[1][r] + bias1) + g1[r] * unscale), xb, xo + 128, 0, 2);
            }
        }
    };

    // =====================================================================================================
    // vector waves
    // =====================================================================================================
#ifdef ET_WS_PROFILE
    unsigned pt[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};     // (32-bit: the low word of s_memtime is enough per launch)
    unsigned pl = (unsigned)__builtin_amdgcn_s_memtime();
// (-DET_WS_PROFILE=2: only the stamps at the block barriers and the ends of the two phases -- the full set costs
//  registers and distorts what it measures)
#define ET_WS_STAMP(k)                                                                              \
    do {                                                                                            \
        if (ET_WS_PROFILE != 2 || (k) == 0 || (k) == 1 || (k) == 3 || (k) == 4 || (k) == 5 || (k) == 6) {  \
            const unsigned now_ = (unsigned)__builtin_amdgcn_s_memtime();                           \
            pt[k] += now_ - pl;                                                                     \
            pl = now_;                                                                              \
        }                                                                                           \
    } while (0)
#else
#define ET_WS_STAMP(k)
#endif
    const int vw = wave - kWsMatrixWaves;   // 0 .. NV-1 (negative on matrix waves: unused there)
    const float step_k = p.steps[min(lane, K - 1)];
    const float step_k1 = KH == 2 ? p.steps[min(lane + kWave, K - 1)] : 0.f;      // sample 64 + lane (second half)
    const et::Pow2Recips pr = et::pow2_recips(d);
    // The lanes <-> samples code below is written in explicit stages over a batch of pixels and without branches
    // inside a batch: left to itself the compiler keeps the pixels of a batch in separate basic blocks (any
    // wave-uniform `if` splits them) and waits for every LDS read before issuing the next.

    // S1(T_j): segments of this wave's pixels; per sample the tap-space location (same arithmetic, same rounding
    // as the tail of et::sample_setup) -> table; the sample's 2 x 2 taps -> the column masks of the tile
    int pf_pix = -1;              // pixel id and segment of this lane's pixel (lane < PW) of the NEXT tile S1 will take,
    float4 pf_seg = f4_zero();    // loaded one step early (two dependent-free 2 k-cycle latencies off S1's chain)
    float4 pf_band = f4_zero();   // ... and the tile's base line (the same for every lane)
    float band_a = 0.f, band_b = 0.f;   // base line of the tile S1 took last (S2 runs on it)
    bool band_x = true;
    auto s1_prefetch = [&](int j, bool valid) {
        pf_pix = -1;
        pf_seg = f4_zero();
        pf_band = f4_zero();
        if (valid) {
            const int tl = tile_of(j);
            pf_band = tp.band[tl];
            if (lane < PW) {
                const size_t idx = (size_t)tl * kTilePix + vw * PW + lane;
                pf_pix = tp.perm[idx];
                pf_seg = tp.segs[idx];
            }
        }
    };
    // first row (minor coordinate) of column u's mask: bit i <-> row col_base(u) + i
    auto col_base = [&](int u) { return (int)floorf(__builtin_fmaf(band_b, (float)u, band_a)) - 1; };
    // The (x, y) table: sample `lane` of this wave's pixel ii.  S1 writes tab_next one step before SM reads it as tab_cur -- the
    // same wave, the same lanes, so it lives in registers (rotated at the end of a step); an LDS table of 2 x 16 KB until round 6.
    f32x2 tab_next[PW], tab_cur[PW];
#pragma unroll
    for (int ii = 0; ii < PW; ++ii) tab_next[ii] = tab_cur[ii] = f32x2{-2.f, -2.f};
    auto s1_impl = [&](int j, auto p2) {
        constexpr bool P2 = decltype(p2)::value;
        const int slot = j % kWsSlots;
        int mypix = -1;
        et::Segment sg;
        sg.sx = sg.sy = sg.vx = sg.vy = 0.f;
        if (lane < PW) {
            const int i = vw * PW + lane;
            mypix = pf_pix;
            const float4 sv = pf_seg;
            sg.sx = sv.x;
            sg.sy = sv.y;
            sg.vx = sv.z;
            sg.vy = sv.w;
            s_pix[slot * kTilePix + i] = mypix;
            *reinterpret_cast<float4 *>(s_seg + (slot * kTilePix + i) * 4) = sv;
        }
        band_a = lane_bcast(pf_band.x, 0);
        band_b = lane_bcast(pf_band.y, 0);
        band_x = lane_bcast(pf_band.z, 0) != 0.f;
        if constexpr (BT) {
            if (vw == 0 && lane == 0) *reinterpret_cast<float4 *>(s_band + slot * 4) = pf_band;
        }
        float x[PW], y[PW];
        int x0[PW], y0[PW];
        bool any[PW];
#pragma unroll
        for (int ii = 0; ii < PW; ++ii) {
            et::Segment q;
            q.sx = lane_bcast(sg.sx, ii);
            q.sy = lane_bcast(sg.sy, ii);
            q.vx = lane_bcast(sg.vx, ii);
            q.vy = lane_bcast(sg.vy, ii);
            float nx, ny;
            et::sample_location<P2>(d, q, (KH == 2 && half_of(j)) ? step_k1 : step_k, pr, nx, ny);
            x[ii] = et::unnormalize(nx, W, d.align_corners);
            y[ii] = et::unnormalize(ny, H, d.align_corners);
            x0[ii] = (int)fminf(fmaxf(floorf(x[ii]), -2.f), (float)W);
            y0[ii] = (int)fminf(fmaxf(floorf(y[ii]), -2.f), (float)H);
            // some tap inside the image <=> x0 in [-1, W-1] and y0 in [-1, H-1]
            any[ii] = __builtin_amdgcn_readlane(mypix, ii) >= 0 && lane + half_of(j) * kWave < K && x0[ii] >= -1 && x0[ii] < W &&
                      y0[ii] >= -1 && y0[ii] < H;
            tab_next[ii] = any[ii] ? f32x2{x[ii], y[ii]} : f32x2{-2.f, -2.f};
        }
        // the sample's cell (u0, v0) along (major, minor): rows v0, v0 + 1 of columns u0 and u0 + 1.  Columns -1 and
        // W (H) are the pad words of the array; rows outside the map are masked off by S2; a row outside a column's
        // window marks the tile as overflowing.
#pragma unroll
        for (int ii = 0; ii < PW; ++ii) {
            const int u0 = band_x ? x0[ii] : y0[ii], v0 = band_x ? y0[ii] : x0[ii];
            const int d0 = v0 - col_base(u0), d1 = v0 - col_base(u0 + 1);
            const unsigned m0 = (unsigned)d0 <= 14u ? 3u << d0 : kWsColOvf;
            const unsigned m1 = (unsigned)d1 <= 14u ? 3u << d1 : kWsColOvf;
            if (any[ii]) {
                atomicOr(&s_col[u0 + 2], m0);
                atomicOr(&s_col[u0 + 3], m1);
            }
        }
    };
    auto s1 = [&](int j) {
        if (pr.ok) s1_impl(j, std::true_type());
        else s1_impl(j, std::false_type());
    };
    // S2(T_j), ONE wave (the last to finish S1: every column mask is complete), lanes <-> columns of the major axis:
    // slot = rank of the (column, row) bit in column-major order.  Leaves the masks cleared for the next S1.
    // (one lane) the row count of the step's slot, the statistics, the overflow list.  KH == 2: a TILE goes to the list once --
    // when either half does not fit -- and is dead for both halves from then on (s_dead: SM and G2 of the other half return).
    auto s2_publish = [&](int j, int slot, bool fits, int U) {
        const int tl = tile_of(j);
        if constexpr (KH == 2) {
            int *dead = s_dead + (seq_of(j) & 3);
            const bool was_dead = half_of(j) != 0 && *dead != 0;
            s_U[slot] = (fits && !was_dead) ? U : -1;
            if (half_of(j) == 0) *dead = fits ? 0 : 1;
            else if (!fits && !was_dead) *dead = 1;
            if (tp.stats) tp.stats[tl] = (fits && !was_dead) ? (half_of(j) ? tp.stats[tl] + (U | (1 << 16)) : (U | (1 << 16))) : 0;
            if (!fits && !was_dead) tp.ovf_list[atomicAdd(tp.ovf_count, 1)] = tl;
        } else {
            s_U[slot] = fits ? U : -1;
            if (tp.stats) tp.stats[tl] = fits ? (U | (1 << 16)) : 0;
            if (!fits) tp.ovf_list[atomicAdd(tp.ovf_count, 1)] = tl;
        }
    };
    auto s2 = [&](int j) {
        const int slot = j % kWsSlots;
        int *rows = s_rows + slot * ROWS;
        unsigned short *st = s_slot + (j & 1) * slot_entries;
        const int umax = band_x ? W : H, vmax = band_x ? H : W;
        if constexpr (BT) {
            // two columns per lane (u = lane, lane + 64); the table gets ALL 16 entries of every column of the map (the pad
            // column for a row the tile does not touch or that lies outside the map), so nothing of an earlier tile is left in
            // it; the columns beside the map (u = -1, umax: taps outside the image) keep the pad entries of the kernel's start
            unsigned mb[2];
            int vb[2], c[2];
            bool ovf = false;
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                const int u = lane + h2 * kWave;
                const unsigned m = s_col[u + 2];
                vb[h2] = col_base(u);
                const int lo = max(0, -vb[h2]), hi = min(15, vmax - 1 - vb[h2]);
                const unsigned inmap = (u < umax && hi >= lo) ? ((2u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
                mb[h2] = m & inmap;
                c[h2] = __popc(mb[h2]);
                ovf = ovf || (u < umax && (m & kWsColOvf) != 0u);
            }
            // (a tap in the columns beside the map must stay inside its column's 16 entries as well)
            ovf = ovf || (lane == 0 && ((s_col[1] | s_col[min(umax, kColWords - 3) + 2]) & kWsColOvf) != 0u);
            __builtin_amdgcn_wave_barrier();
            s_col[lane] = 0u;
            s_col[kWave + lane] = 0u;
            if (lane < kColWords - 2 * kWave) s_col[2 * kWave + lane] = 0u;
            const bool window_ok = __builtin_amdgcn_ballot_w64(ovf) == 0;
            const int incl0 = wave_scan_incl(c[0]);
            const int tot0 = __builtin_amdgcn_readlane(incl0, kWave - 1);
            const int incl1 = wave_scan_incl(c[1]) + tot0;
            const int U = __builtin_amdgcn_readlane(incl1, kWave - 1);
            const bool fits = window_ok && U <= tp.rows_cap;
            if (fits) {
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    const int u = lane + h2 * kWave;
                    int rs = (h2 ? incl1 : incl0) - c[h2];
                    if (u < umax) {
                        unsigned *ent = reinterpret_cast<unsigned *>(st + (u + 2) * kWsBandStride);
#pragma unroll
                        for (int i = 0; i < 16; i += 2) {
                            unsigned e2 = 0;
#pragma unroll
                            for (int b2 = 0; b2 < 2; ++b2) {
                                unsigned e = (unsigned)kPad;
                                if ((mb[h2] >> (i + b2)) & 1u) {
                                    const int v = vb[h2] + i + b2;
                                    const int hh = band_x ? v : u, ww = band_x ? u : v;
                                    rows[rs] = hh * W + ww;
                                    e = (unsigned)rs++;
                                }
                                e2 |= e << (16 * b2);
                            }
                            ent[i >> 1] = e2;
                        }
                    }
                }
                const int upad = (U + 15) & ~15;
                if (lane < upad - U) rows[U + lane] = kTilePadRow;
            }
            if (lane == 0) s2_publish(j, slot, fits, U);
            return;
        }
        const unsigned m = s_col[lane + 2];
        __builtin_amdgcn_wave_barrier();    // (lane L clears the word lane L - 2 has just read: reads before clears, as in the band branch)
        s_col[lane] = 0u;
        if (lane < kWsColWords - kWave) s_col[kWave + lane] = 0u;
        const int vb = col_base(lane);
        // rows of this column inside the map: 0 <= vb + i < vmax
        const int lo = max(0, -vb), hi = min(15, vmax - 1 - vb);
        const unsigned inmap = (lane < umax && hi >= lo) ? ((2u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
        unsigned mb = m & inmap;
        const bool window_ok = __builtin_amdgcn_ballot_w64(lane < umax && (m & kWsColOvf) != 0u) == 0;
        const int c = __popc(mb);
        const int incl = wave_scan_incl(c);
        const int U = __builtin_amdgcn_readlane(incl, kWave - 1);
        const bool fits = window_ok && U <= tp.rows_cap;
        if (fits) {
            int rs = incl - c;
            while (mb) {
                const int v = vb + __ffs(mb) - 1;
                const int h = band_x ? v : lane, w = band_x ? lane : v;
                rows[rs] = h * W + w;
                st[(h + 2) * PWD + w + 2] = (unsigned short)rs;
                ++rs;
                mb &= mb - 1;
            }
            // G2 walks the rows in groups of 16: pad the list with row 0 of the source map (a valid address; the
            // matching B columns are zero)
            const int upad = (U + 15) & ~15;
            if (lane < upad - U) rows[U + lane] = kTilePadRow;
        }
        if (lane == 0) s2_publish(j, slot, fits, U);
    };
    // SM(T_j): resample D, masked soft-max, arg-max -> corr_pos, attention, B rows in place (lanes <-> samples), in ONE
    // piece in phase B(j).  G2(T_j) only runs in phase B(j + 1), so the B-row half could sit in phase A(j + 1), where the
    // vector waves idle for a third of the phase since the row set became column masks.  Measured in round 4
    // (profiles/r04_ws_tail_in_phase_a.txt): 1.00 -> 1.15 ms.  The B rows are LDS traffic (zero, read-modify-write, split in
    // place) and phase A is where G1 keeps the LDS pipe busy (ds_bpermute + A fragments): the half takes 6.7-10.3 k cycles
    // there instead of 4.5 k and G1 12-15 k instead of 8-11 k.  Even split in two but run back to back in phase B (its state
    // through 24 VGPRs) it cost 8 % (1.085 vs 1.004 ms, profiles/r04_fwd_ab.txt): one piece, one schedule.
    // KH == 2: what the first half's SM leaves for the second's (the same wave takes the same four pixels in both): the logit of
    // sample `lane`, the half's maximum and the sum of exp(logit - maximum) (wave-uniform, kept per lane)
    float lg_prev[PB], m_prev[PB], s_prev[PB];
#pragma unroll
    for (int t = 0; t < PB; ++t) lg_prev[t] = m_prev[t] = s_prev[t] = 0.f;
    auto sm_impl = [&](int j, auto smx) {
        constexpr bool SMX = decltype(smx)::value;
        const int slot = j % kWsSlots;
        const int U = s_U[slot];
        if (U < 0) return;
        const int half = half_of(j);
        if (KH == 2 && __builtin_amdgcn_readfirstlane(s_dead[seq_of(j) & 3]) != 0) return;   // (the tile went to the list kernels)
        const int n = tile_of(j) / tp.tiles_per_pair;
        float *s_D = s_arr + (j & 1) * kArr;
        const unsigned short *st = s_slot + (j & 1) * slot_entries;
        const int *pixs = s_pix + slot * kTilePix;
        // (band-table kernel: the base line of THIS tile -- S1 has moved on to the next one)
        const float4 bl = BT ? *reinterpret_cast<const float4 *>(s_band + slot * 4) : f4_zero();
        const bool bl_x = bl.z != 0.f;
        auto base_of = [&](int u) { return (int)floorf(__builtin_fmaf(bl.y, (float)u, bl.x)) - 1; };
        // outputs through raw buffers: a store whose offset is past the end is dropped, so "lane >= K", "not lane 0..3",
        // "padding pixel" and "output not requested" (empty buffer) need no branches
        const __amdgpu_buffer_rsrc_t attn_buf =
            make_rsrc(p.attn ? p.attn + (size_t)n * K * HW : nullptr, p.attn ? (unsigned)K * HW * 4u : 0u);
        const __amdgpu_buffer_rsrc_t corr_buf =
            make_rsrc(p.corr ? p.corr + (size_t)n * HW * 2 : nullptr, p.corr ? (unsigned)HW * 8u : 0u);
        const bool in = lane + half * kWave < K;
        static_assert(PW == PB, "one batch per wave and tile (the sample table is indexed statically)");
        {
            constexpr int i0 = 0;
            float a[PB], wt[PB][4];
            int sl[PB][4], best[PB], pix[PB], cidx[PB], cidx2[PB], cell[PB];
            f32x2 xy[PB];
            float *drow[PB], *dummy[PB];
            // ---- stage 1: table reads (and the pad column of this batch's D rows: 0) ----
            if (lane < PB) s_D[(vw * PW + i0 + lane) * STRIDE + kPad] = 0.f;
#pragma unroll
            for (int t = 0; t < PB; ++t) {
                const int i = vw * PW + i0 + t;
                pix[t] = pixs[i];
                xy[t] = tab_cur[i0 + t];
                drow[t] = s_D + i * STRIDE;
                dummy[t] = drow[t] + kPad + 1 + (lane & 1);     // unused columns behind the pad column (STRIDE = ROWS + 4)
            }
            // ---- stage 2: cells and weights ----
#pragma unroll
            for (int t = 0; t < PB; ++t) {
                pix[t] = __builtin_amdgcn_readfirstlane(pix[t]);
                const float xw = floorf(xy[t].x), yn = floorf(xy[t].y);
                const float w = xy[t].x - xw, e = 1.f - w, nn = xy[t].y - yn, so = 1.f - nn;
                const int x0 = (int)xw, y0 = (int)yn;
                cidx[t] = (y0 + 2) * PWD + x0 + 2;
                // (a sample without taps sits at (-2, -2): a cell of its own per lane, all four slots = pad)
                cell[t] = x0 == -2 ? -1 - lane : cidx[t];
                if constexpr (BT) {
                    // entries of the sample's two columns: (u0, v0), (u0, v0 + 1) at e0, e0 + 1; (u0 + 1, v0), (u0 + 1, v0 + 1) at
                    // e1, e1 + 1 (inside the columns' 16 entries for every sample S1 marked: the tile fits its band)
                    const int u0 = bl_x ? x0 : y0, v0 = bl_x ? y0 : x0;
                    const int e0 = (u0 + 2) * kWsBandStride + (v0 - base_of(u0)), e1 = (u0 + 3) * kWsBandStride + (v0 - base_of(u0 + 1));
                    cell[t] = x0 == -2 ? -1 - lane : (y0 + 2) * (W + 4) + x0 + 2;
                    cidx[t] = x0 == -2 ? 0 : e0;                       // (entry 0: a pad column's, = the pad slot)
                    cidx2[t] = x0 == -2 ? 0 : e1;
                }
                wt[t][0] = so * e;
                wt[t][1] = so * w;
                wt[t][2] = nn * e;
                wt[t][3] = nn * w;
            }
            // ---- stage 3: slots ----
#pragma unroll
            for (int t = 0; t < PB; ++t) {
                if constexpr (BT) {
                    // taps in nw, ne, sw, se order: along x the major axis (u = x): ne = (u0 + 1, v0), sw = (u0, v0 + 1); else swapped
                    const int a00 = st[cidx[t]], a01 = st[cidx[t] + 1], a10 = st[cidx2[t]], a11 = st[cidx2[t] + 1];
                    const bool none = cidx[t] == 0;                    // (its four entries would be those of ONE pad column)
                    sl[t][0] = a00;
                    sl[t][1] = none ? kPad : bl_x ? a10 : a01;
                    sl[t][2] = none ? kPad : bl_x ? a01 : a10;
                    sl[t][3] = none ? kPad : a11;
                } else {
                    sl[t][0] = st[cidx[t]];
                    sl[t][1] = st[cidx[t] + 1];
                    sl[t][2] = st[cidx[t] + PWD];
                    sl[t][3] = st[cidx[t] + PWD + 1];
                }
            }
            // ---- stage 4: D values, logits ----
            float dv[PB][4], lg[PB];
#pragma unroll
            for (int t = 0; t < PB; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) dv[t][r] = drow[t][sl[t][r]];   // (pad column: 0)
#pragma unroll
            for (int t = 0; t < PB; ++t) {
                float acc = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc = fmaf(wt[t][r], dv[t][r], acc);
                const float l = (acc == 0.f) ? -1e10f : acc;            // epipolar.py:298
                lg[t] = SMX ? l * d.softmax_scale : l / (float)K;      // epipolar.py:306 / 311
            }
            ET_WS_STAMP(8);
            // ---- stage 5: soft-max, arg-max ----
            float a_first[PB];      // KH == 2, second half: the attention of the FIRST half's sample `lane`
            if constexpr (KH == 2) {
                // online soft-max over the two halves (see the head of the kernel); a[] stays UNNORMALISED here -- the B rows are
                // built from exp(l - m) and G2 divides by the sum -- the attention proper goes out in stage 7
                float m[PB], ex[PB], sm4[PB];
#pragma unroll
                for (int t = 0; t < PB; ++t) m[t] = in ? lg[t] : neg_inf;
                wave_all_max4(m);
                if (half == 1) {
#pragma unroll
                    for (int t = 0; t < PB; ++t) m[t] = fmaxf(m[t], m_prev[t]);
                }
#pragma unroll
                for (int t = 0; t < PB; ++t) sm4[t] = ex[t] = in ? __expf(lg[t] - m[t]) : 0.f;
                wave_all_sum4(sm4);
                if (half == 0) {
#pragma unroll
                    for (int t = 0; t < PB; ++t) {
                        a[t] = ex[t];
                        lg_prev[t] = lg[t];
                        m_prev[t] = m[t];
                        s_prev[t] = sm4[t];
                        best[t] = 0;
                        a_first[t] = 0.f;
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < PB; ++t) {
                        const float alpha = __expf(m_prev[t] - m[t]);
                        const float rdn = __builtin_amdgcn_rcpf(s_prev[t] * alpha + sm4[t]);
                        a_first[t] = __expf(lg_prev[t] - m[t]) * rdn;          // (K > 64: every lane of the first half holds a sample)
                        a[t] = ex[t];
                        // first maximum over all K samples (torch.argmax on the attention VALUES): the largest logit has e == 1
                        const unsigned long long hit0 = __builtin_amdgcn_ballot_w64(a_first[t] == rdn);
                        const unsigned long long hit1 = __builtin_amdgcn_ballot_w64(in && ex[t] * rdn == rdn);
                        best[t] = hit0 ? (int)__builtin_ctzll(hit0) : hit1 ? kWave + (int)__builtin_ctzll(hit1) : 0;
                        if (lane == 0) {
                            s_alpha[vw * PW + i0 + t] = alpha;
                            s_rinv[vw * PW + i0 + t] = rdn;
                        }
                        s_prev[t] = rdn;                                       // (stage 7 normalises with it)
                    }
                }
            } else {
                float amax[PB], idx[PB];
                if constexpr (SMX) {
                    // hardware exp2 / reciprocal: ~1e-6 relative on the returned attention (tolerance 1e-5)
                    float m[PB], ex[PB], sm4[PB];
#pragma unroll
                    for (int t = 0; t < PB; ++t) m[t] = in ? lg[t] : neg_inf;
                    wave_all_max4(m);
#pragma unroll
                    for (int t = 0; t < PB; ++t) sm4[t] = ex[t] = in ? __expf(lg[t] - m[t]) : 0.f;
                    wave_all_sum4(sm4);
#pragma unroll
                    for (int t = 0; t < PB; ++t) {
                        const float rdn = __builtin_amdgcn_rcpf(sm4[t]);
                        a[t] = ex[t] * rdn;
                        amax[t] = rdn;  // the largest logit has e == 1
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < PB; ++t) {
                        a[t] = in ? lg[t] : 0.f;
                        amax[t] = in ? a[t] : neg_inf;
                    }
                    wave_all_max4(amax);
                }
                // first maximum over k (torch.argmax): the lowest lane that holds the maximum -- a ballot and a scalar
                // find-first-bit per pixel (a DPP minimum over the lane ids was 12 dependent vector instructions per batch)
#pragma unroll
                for (int t = 0; t < PB; ++t) {
                    const unsigned long long hit = __builtin_amdgcn_ballot_w64(in && a[t] == amax[t]);
                    best[t] = hit ? (int)__builtin_ctzll(hit) : 0;
                }
                (void)idx;
            }
            ET_WS_STAMP(9);
            // ---- stage 6: corr_pos of the batch's four pixels at once: lane t < 4 re-evaluates the location of pixel
            // t's best sample (same arithmetic as S1) and stores both coordinates ----
            if (p.corr && (KH == 1 || half == 1)) {
                const int t4 = lane & 3;
                const int bi = t4 == 0 ? best[0] : t4 == 1 ? best[1] : t4 == 2 ? best[2] : best[3];
                const int px = t4 == 0 ? pix[0] : t4 == 1 ? pix[1] : t4 == 2 ? pix[2] : pix[3];
                const float4 sv = *reinterpret_cast<const float4 *>(s_seg + (slot * kTilePix + vw * PW + i0 + t4) * 4);
                et::Segment q;
                q.sx = sv.x;
                q.sy = sv.y;
                q.vx = sv.z;
                q.vy = sv.w;
                float nx, ny;
                const float stb0 = __shfl(step_k, bi & (kWave - 1)), stb1 = KH == 2 ? __shfl(step_k1, bi & (kWave - 1)) : 0.f;
                const float stb = (KH == 2 && bi >= kWave) ? stb1 : stb0;
                if (pr.ok) et::sample_location<true>(d, q, stb, pr, nx, ny);
                else et::sample_location<false>(d, q, stb, pr, nx, ny);
                const f32x2 cv = f32x2{et::de_normalize(d, nx, W), et::de_normalize(d, ny, H)};
                typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(cv.x), __float_as_uint(cv.y)}, corr_buf,
                                                      (lane < PB && px >= 0) ? px * 8 : kDropped, 0, 0);
            }
            ET_WS_STAMP(10);
            // ---- stage 7: attention out; B rows: zero, then scatter a_k * w_kt onto the row slots (same wave: LDS ops
            // stay in order).  Taps outside the image land in the pad column, which is never read as B. ----
            RowRuns runs[PB];
            bool longer = false;
#pragma unroll
            for (int t = 0; t < PB; ++t) {
                if constexpr (KH == 2) {
                    // (the attention of both halves goes out behind the second half's soft-max: exp(l - m) / s with the common m, s)
                    if (half == 1) {
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(a_first[t]), attn_buf,
                                                              pix[t] >= 0 ? (lane * HW + pix[t]) * 4 : kDropped, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(a[t] * s_prev[t]), attn_buf,
                                                              (pix[t] >= 0 && in) ? ((kWave + lane) * HW + pix[t]) * 4 : kDropped, 0, 0);
                    }
                } else {
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(a[t]), attn_buf,
                                                          pix[t] >= 0 ? (lane * HW + pix[t]) * 4 : kDropped, 0, 0);
                }
                runs[t] = row_runs(cell[t]);
                longer = longer || runs[t].longer;
#pragma unroll
                for (int q = 0; q < (ROWS + kWave - 1) / kWave; ++q)
                    if (ROWS % kWave == 0 || q * kWave + lane < ROWS) drow[t][q * kWave + lane] = 0.f;
            }
            if (longer) {   // some pixel has a run of three or more samples in one cell (short segment): atomics
#pragma unroll
                for (int t = 0; t < PB; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) atomicAdd(&drow[t][sl[t][r]], (a[t] * 1024.f) * wt[t][r]);
            } else {
                // per tap stream r: equal slots only occur in runs of two neighbouring lanes -> one DPP add, the run's
                // last lane does a plain read-modify-write (the others: their dead table entry), four pixels at a time
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float *addr[PB], sum[PB], old[PB];
#pragma unroll
                    for (int t = 0; t < PB; ++t) {
                        const float v = (a[t] * 1024.f) * wt[t][r];   // B is kept scaled by 2^10 (G2 splits it to fp16)
                        const float pv = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, false));
                        sum[t] = runs[t].same ? v + pv : v;
                        addr[t] = runs[t].end ? drow[t] + sl[t][r] : dummy[t];
                        old[t] = *addr[t];
                    }
#pragma unroll
                    for (int t = 0; t < PB; ++t) *addr[t] = old[t] + sum[t];
                }
            }
            // ---- stage 8: the finished B rows -> fp16 hi | lo, in place per group of eight columns (32 bytes: eight hi
            // then eight lo), i.e. G2's A fragments become two plain 16-byte reads.  Done once here instead of by each of
            // the four matrix waves in every k-step (same wave as the scatter: LDS ops stay in order); lanes 0-31 take
            // the 32 groups of one pixel, lanes 32-63 those of the next. ----
#pragma unroll
            for (int t = 0; t < PB; t += 2) {
#pragma unroll
                for (int g0 = 0; g0 < ROWS / 8; g0 += 32) {          // (288-row arrays: 36 groups, the last four in a second pass)
                    const int grp = g0 + (lane & 31);
                    if (g0 + 32 <= ROWS / 8 || grp < ROWS / 8) {
                        float *gp = (lane < 32 ? drow[t] : drow[t + 1]) + grp * 8;
                        const float4 x0 = *reinterpret_cast<const float4 *>(gp), x1 = *reinterpret_cast<const float4 *>(gp + 4);
                        const float bv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
                        f16x8 bhi8, blo8;
                        float bdummy = 0.f;
                        split_f16x8<false>(bv, bhi8, blo8, bdummy);      // (B values are <= 2^10 by construction)
                        *reinterpret_cast<f16x8 *>(gp) = bhi8;
                        *reinterpret_cast<f16x8 *>(gp + 4) = blo8;
                    }
                }
            }
        }
    };
    auto sm = [&](int j) {
        if (KH == 2 || d.softmax_enabled) sm_impl(j, std::true_type());       // (KH == 2: the host takes this kernel with the soft-max on only)
        else sm_impl(j, std::false_type());
    };
    // =====================================================================================================
    // the pipeline
    // =====================================================================================================
    // Two loops, one per role, with the same number of block barriers: the roles' register sets (the matrix waves
    // carry their operand rings across the barriers) then do not add up in the allocation.
    if (is_matrix) {
        if (tp.setprio & 1) __builtin_amdgcn_s_setprio(1);
#pragma unroll 1
        for (int i = -1;; ++i) {
            if (i >= 1 && !has_tile(i - 1)) break;                 // (one step beyond the last tile: its G2)
#ifdef ET_WS_PROFILE
            if (!(tp.setprio & 128))
#endif
            if (has_tile(i)) g1_main(i);                           // phase A
            ET_WS_STAMP(6);
            g2_prefetch(i - 1, has_tile(i - 1));
            ET_WS_STAMP(0);
            lds_barrier();
            ET_WS_STAMP(1);
#ifdef ET_WS_PROFILE
            if (!(tp.setprio & 64))
#endif
            if (has_tile(i - 1)) g2_main(i - 1);                   // phase B
            ET_WS_STAMP(2);
            g1_prefetch(i + 1, has_tile(i + 1));
            ET_WS_STAMP(3);
            lds_barrier();
            ET_WS_STAMP(4);
        }
    } else {
        int vb_target = 0;
        s1_prefetch(0, true);
        const bool drawer = vw == 0 && lane == 0;
#pragma unroll 1
        for (int i = -1;; ++i) {
            if (i >= 1 && !has_tile(i - 1)) break;
            if (KH == 1 || (i & 1) == 0) draw_issue(drawer);       // the tile of step i + 3 (committed at the end of phase B)
            if (kCopyInA) copy_load(i + 1, has_tile(i + 1));
#ifdef ET_WS_PROFILE
            if (!(tp.setprio & 32))
#endif
            if (has_tile(i + 1)) s1(i + 1);
            s1_prefetch(i + 2, has_tile(i + 2));
            ET_WS_STAMP(1);
            vb_target += NV;
            const bool last = vector_arrive_last(s_U + 4, vb_target, lane);   // every column mask of T_{i+1} is in LDS
            ET_WS_STAMP(2);
            if (last && has_tile(i + 1)) s2(i + 1);
            ET_WS_STAMP(3);
            if (kCopyInA) copy_finish(i + 1, has_tile(i + 1));
            lds_barrier();
            ET_WS_STAMP(4);
#ifdef ET_WS_PROFILE
            const bool do_copy = !(tp.setprio & 16);
#else
            constexpr bool do_copy = true;
#endif
            // (KH == 2: the copy of a TILE, behind the SM of the last half of the tile before it)
            const bool copy_now = !kCopyInA && has_tile(i + 1) && half_of(i + 1) == 0 && do_copy;
            if (!kCopyInA) copy_load(i + 1, copy_now);          // phase B
#ifdef ET_WS_PROFILE
            if (!(tp.setprio & 8))
#endif
            if (has_tile(i)) sm(i);
            ET_WS_STAMP(0);
            if (!kCopyInA) copy_finish(i + 1, copy_now);
            if (KH == 1) draw_commit(i + 3, drawer);
            else if ((i & 1) == 0) draw_commit((i >> 1) + 2, drawer);
#pragma unroll
            for (int ii = 0; ii < PW; ++ii) tab_cur[ii] = tab_next[ii];
            ET_WS_STAMP(5);
            lds_barrier();
            ET_WS_STAMP(6);
        }
    }
#ifdef ET_WS_PROFILE
    if (tp.prof && lane == 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) tp.prof[((size_t)blockIdx.x * (kWsMatrixWaves + NV) + wave) * 12 + k] = pt[k];
    }
#endif
#undef ET_WS_STAMP
}
