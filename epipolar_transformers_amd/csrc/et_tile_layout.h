// The memory formats of the MFMA tile path, one definition each: the header words and the regions of the caller's workspace,
// and the dynamic LDS of the three tile kernel families (forward and backward one block per tile, persistent forward).  The
// host's size functions return the totals of these layouts and the kernels take their pointers from the same structs (the
// backward's one-block-per-tile kernel keeps a pointer chain, asserted term by term against its layout at compile time:
// kernels_backward_tile.inc says why), so a size and a carve cannot disagree.  Plain constexpr C++17 without a HIP header:
// tests/test_tile_layout_cpu.py compiles a host program against this file and checks order, alignment and the recorded
// sizes.  All offsets are in BYTES.
#pragma once
#include <cstddef>

namespace {     // (every user is a translation unit of its own: the tile units keep these names to themselves, as before)
#include "et_lds_layout.h"     // ET_ASTAGE_ROW_BYTES: the rows of the fp16 A stage

constexpr size_t tile_align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }

// ---- shapes ---------------------------------------------------------------------------------------------------------
constexpr int kTilePix = 32;                    // reference pixels per tile (MFMA M)
// Source rows a (sub)tile may touch = columns of the D/B array in LDS (template parameter ROWS of the kernel):
// 256 for maps up to 64 x 64 (51.5 KB LDS, 3 blocks per CU), 384 for larger maps whose lines are longer
// (68 KB, 2 blocks per CU; with 256 most tiles of a 96 x 96 map would overflow and split), 512 when one
// pixel alone can touch more than 384 rows (K > 96 on maps above 96 x 96; 2 blocks per CU).  The array's
// row stride is ROWS + 1: odd, so column reads are bank-conflict-free.
constexpr int kTileRowsSmall = 256, kTileRowsLarge = 384, kTileRowsHuge = 512;
// the warp-specialised persistent kernel above 64 x 64 (kernels_forward_tile_ws.inc, BT = true): 288-row arrays, maps up to
// 96 x 96 (every tile of a 96 x 96 map has at most 280 rows; 384-row arrays do not fit its LDS)
constexpr int kTileRowsWsLarge = 288, kWsMaxSideBand = 96, kWsMaxSideTwoPass = 128;
// Row-array widths of the backward's merged form (two arrays): 192 columns for maps up to 64 x 64 (three blocks per CU), 288
// for maps up to 96 x 96 (two, as the one-array kernel there); tiles with more rows are split into pixel groups.
constexpr int kTileRowsMerged = 192, kTileRowsMergedLarge = 288;
constexpr bool bwd_rows_merged(int rows) { return rows == kTileRowsMerged || rows == kTileRowsMergedLarge; }
constexpr int kTileWave = 64, kTileXcds = 8;    // (et_common.h's kWave and kXcds: et_tile_host.h asserts that they agree)

// ---- the workspace --------------------------------------------------------------------------------------------------
// Workspace of the tile forward (all int32, base aligned up to 256 bytes):
//   header (64 words): [0] overflow count, [1] sticky error word -- at the front, so that their offsets do not depend on
//   the shape of the call (a workspace is reused across shapes) |
//   perm[tiles * 32] | overflow list[tiles] | stats[tiles] | scales[4 * N] (float) |
//   segments[tiles * 32] (float4, 16-byte aligned; in tile order.  Until tile_order_kernel writes them the region of a pair
//   holds the pair's sort keys: 8 bytes per pixel, tile_keys_kernel) |
//   band[tiles] (float4: the tile's base line, warp-specialised kernel) | segments by pixel[N * HW] (float4)
// Header words beyond [0] / [1] are scratch of the kernels of ONE call, cleared by tile_keys_kernel (`header`) at its start:
//   forward:  [2 .. 9]  one tile counter per XCD (the blocks of an XCD draw their tiles from it)
//   backward: [2] four-group tiles met so far, [3] eight-or-more-group tiles met early (kernels_backward_tile.inc: the merged
//             kernel splits the first 128 / 32 of a call in place and defers the rest to its second launch), [4] over-capacity
//             tiles met so far (beyond the first 256 of a call they are deferred without a search)
//   deterministic backward (et_epipolar_backward_tiled_det): [0] deferred tiles that fit the second launch's kernel whole (listed from
//             the front of the overflow list), [2] those that do not (listed from its back, eight blocks each); [3], [4] unused --
//             which tile goes where is a function of the tile alone.  Behind the forward layout, from the next 256-byte boundary:
//             int64 accumulator[N * HW * 256] | quanta[4 * N] | partial maxima[4 * 32 * N]  (et_backward_tile.hip)
// The backward REUSES the forward's counter words: safe because every call starts with the ordering kernels on the same stream,
// which zero them -- a change to either user has to keep that (the static_assert below).  Which over-capacity tiles a
// backward call splits in place and which it defers depends on the order its blocks reach those counters and on blockIdx
// relative to gridDim: the SET of deferred tiles, and with it the order of the float-atomic additions into grad_src, differs
// from run to run (gradients reproducible to rounding, as documented; ops.backward_deferred_tiles() counts vary by a few tiles).
constexpr int kTileHdrWords = 64;
constexpr int kTileHdrCount = 0;            // overflow tiles (forward) / deferred tiles (backward)
static_assert(kTileHdrCount == 0, "the kernels' ovf_count / tile_count pointers stand in for the header's base: the other words are indexed from them");
constexpr int kTileHdrErr = 1;              // the sticky error word: never cleared by a call
constexpr int kTileHdrXcdCtr = 2;           // forward: kTileXcds tile counters, one per XCD
constexpr int kTileHdrBwdQuads = 2;         // backward: four-group tiles met so far
constexpr int kTileHdrBwdEarly = 3;         //           eight-or-more-group tiles met early
constexpr int kTileHdrBwdOverCap = 4;       //           over-capacity tiles met so far
constexpr int kTileHdrDetHard = 2;          // deterministic backward: deferred tiles beyond the second launch's capacity
constexpr int kTileHdrClearEnd = 10;        // tile_keys_kernel zeroes the words [0, kTileHdrClearEnd) except kTileHdrErr
static_assert(kTileHdrXcdCtr + kTileXcds <= kTileHdrClearEnd && kTileHdrBwdQuads < kTileHdrClearEnd &&
                  kTileHdrBwdEarly < kTileHdrClearEnd && kTileHdrBwdOverCap < kTileHdrClearEnd &&
                  kTileHdrDetHard < kTileHdrClearEnd && kTileHdrCount < kTileHdrClearEnd && kTileHdrClearEnd <= kTileHdrWords,
              "the ordering clears every counter word either direction uses");
static_assert(kTileHdrErr != kTileHdrCount && kTileHdrErr < kTileHdrXcdCtr, "no counter shares the sticky error word");

constexpr size_t kTileWorkspaceAlign = 256;     // of the base (the caller's pointer is rounded up) and of the deterministic tail
constexpr size_t kTileSegsAlign = 16;           // float4 regions
// Offsets from the aligned base.  `end` is where the layout ends AS SIZED: behind segs_pix plus whatever of the kTileSegsAlign
// bytes allowed for aligning `segs` this shape does not use, so that sizes do not depend on the padding a shape happens to need;
// `bytes` is what the caller provides: `end` and a full step for aligning the base.
struct TileWorkspaceLayout {
    size_t perm, ovf_list, stats, scales, segs, band, segs_pix, end, bytes;
};
constexpr TileWorkspaceLayout tile_workspace_layout(size_t tiles, size_t pairs, size_t hw)
{
    TileWorkspaceLayout l{};
    l.perm = kTileHdrWords * sizeof(int);
    l.ovf_list = l.perm + tiles * kTilePix * sizeof(int);
    l.stats = l.ovf_list + tiles * sizeof(int);
    l.scales = l.stats + tiles * sizeof(int);
    const size_t scales_end = l.scales + 4 * pairs * sizeof(float);
    l.segs = tile_align_up(scales_end, kTileSegsAlign);
    l.band = l.segs + tiles * kTilePix * 16;
    l.segs_pix = l.band + tiles * 16;
    l.end = l.segs_pix + pairs * hw * 16 + (scales_end + kTileSegsAlign - l.segs);
    l.bytes = l.end + kTileWorkspaceAlign;
    return l;
}
// The deterministic backward's tail behind a forward layout that ends at `fwd_end`: offsets from the same base; `extra_bytes`
// is what the tail adds to the forward's size (its regions and a full step for aligning it).
constexpr int kDetMaxBlocks = 32;       // blocks per pair of det_maxima_kernel (one partial result each)
struct DetWorkspaceLayout {
    size_t acc, quanta, partial, end, extra_bytes;
};
constexpr DetWorkspaceLayout det_workspace_layout(size_t fwd_end, size_t pairs, size_t hw)
{
    DetWorkspaceLayout l{};
    l.acc = tile_align_up(fwd_end, kTileWorkspaceAlign);
    l.quanta = l.acc + pairs * hw * 256 * sizeof(long long);
    l.partial = l.quanta + 4 * pairs * sizeof(float);
    l.end = l.partial + 4 * kDetMaxBlocks * pairs * sizeof(float);
    l.extra_bytes = kTileWorkspaceAlign + (l.end - l.acc);
    return l;
}

// ---- LDS: the one-block-per-tile kernels ----------------------------------------------------------------------------
// the forward's array: rows of ROWS + 4 floats (16-byte aligned: the split second GEMM reads 16-byte fragments), and at
// least the 2 x 32 x 528 bytes of fp16 stage of the split first GEMM
constexpr int fwd_tile_array_floats(int rows) { return kTilePix * (rows + 4) > 8448 ? kTilePix * (rows + 4) : 8448; }
// the backward's: one array of rows of ROWS + 1 floats, which also stages the 32 x kAStride A tile of the D-type GEMMs
// (kernels_tile_common.inc), or two arrays for the merged form
constexpr int kAStride = 260;  // floats per staged A row: 16-byte aligned rows, b128 fragment reads conflict-free
constexpr int tile_array_floats(int rows) { return kTilePix * (rows + 1 > kAStride ? rows + 1 : kAStride); }
constexpr int bwd_tile_array_floats(int rows)
{
    return bwd_rows_merged(rows)
               ? (2 * kTilePix * (rows + 1) > tile_array_floats(rows) ? 2 * kTilePix * (rows + 1) : tile_array_floats(rows))
               : tile_array_floats(rows);
}
constexpr int kTileNxyBytes = kTilePix * kTileWave * 8;     // the table of sample locations: [32][64] float2

// Forward, fwd_tile_body<KPL, ROWS>: `hw_words` = ceil(H W / 32), the words of the source-pixel bitmap.
struct FwdTileLds {
    int arr;        // [32][ROWS + 4] float  D, then B
    int rows;       // [ROWS] int            slot -> source pixel
    int pix;        // [32] int              tile pixel ids
    int U;          // int                   rows of the tile's row set                                          \ 48 words:
    int ainv;       // [32] float            1 / scale of the A rows                                             / "misc"
    int seg;        // [32][4] float         epipolar segments
    int bitmap;     // [hw_words] unsigned   source pixels the tile touches
    int prefix;     // [hw_words] int        exclusive popcount prefix
    int nxy;        // KPL == 1: [32][64] float2 normalised sample locations
    int end;
};
constexpr int kFwdMiscWords = 48, kFwdMiscAinvWord = 8;     // the misc block: U and 7 spare words, ainv, 8 spare words
static_assert(kFwdMiscAinvWord >= 1 && kFwdMiscAinvWord + kTilePix <= kFwdMiscWords, "U and ainv fit the misc block");
constexpr FwdTileLds fwd_tile_lds(int rows, int hw_words, int kpl)
{
    FwdTileLds l{};
    l.arr = 0;
    l.rows = l.arr + fwd_tile_array_floats(rows) * 4;
    l.pix = l.rows + rows * 4;
    l.U = l.pix + kTilePix * 4;
    l.ainv = l.U + kFwdMiscAinvWord * 4;
    l.seg = l.U + kFwdMiscWords * 4;
    l.bitmap = l.seg + kTilePix * 16;
    l.prefix = l.bitmap + hw_words * 4;
    l.nxy = l.prefix + hw_words * 4;
    l.end = l.nxy + (kpl == 1 ? kTileNxyBytes : 0);
    return l;
}
// Backward, bwd_tile_body<KPL, ROWS, DET>: the table of sample locations where the kernel keeps it (one sample per lane and
// not the merged form, whose second array takes its place).
struct BwdTileLds {
    int arr;        // [32][ROWS + 1] float  D, E, Bs, B in turn (merged form: two arrays)
    int rows;       // [ROWS] int            slot -> source pixel
    int pix;        // [32] int              tile pixel ids
    int U;          // int                   rows of the tile's row set                                          \.
    int group_rows; // int                   rows of a pixel group's row set (the search of a tile that is split) |
    int drawn;      // int                   what thread 0 drew from a header counter                             | 60 words:
    int red2;       // [2][4] float          block reduction: two maxima per wave                                 | "misc"
    int red1;       // [4] float             block reduction: one maximum per wave (and four spare words)         |
    int ainv;       // [32] float            1 / scale of the A rows                                             /
    int seg;        // [32][4] float         epipolar segments
    int bitmap;     // [hw_words] unsigned
    int prefix;     // [hw_words] int
    int nxy;        // [32][64] float2 normalised sample locations (see above)
    int end;
};
constexpr int kBwdMiscWords = 60;     // the misc block: U .. ainv and their spare words
constexpr int kBwdWaves = 4;          // waves of a block: one slot each in red1, two in red2
constexpr int kBwdRed2Words = 2 * kBwdWaves, kBwdRed1Words = kBwdWaves, kBwdRed1SpareWords = 4;
constexpr BwdTileLds bwd_tile_lds(int rows, int hw_words, int kpl)
{
    BwdTileLds l{};
    l.arr = 0;
    l.rows = l.arr + bwd_tile_array_floats(rows) * 4;
    l.pix = l.rows + rows * 4;
    l.U = l.pix + kTilePix * 4;
    l.group_rows = l.U + 4;
    l.drawn = l.group_rows + 4 + 4;      // (one spare word)
    l.red2 = l.drawn + 4;
    l.red1 = l.red2 + kBwdRed2Words * 4;
    l.ainv = l.red1 + (kBwdRed1Words + kBwdRed1SpareWords) * 4;
    l.seg = l.U + kBwdMiscWords * 4;     // (eight spare words behind ainv)
    l.bitmap = l.seg + kTilePix * 16;
    l.prefix = l.bitmap + hw_words * 4;
    l.nxy = l.prefix + hw_words * 4;
    l.end = l.nxy + ((kpl == 1 && !bwd_rows_merged(rows)) ? kTileNxyBytes : 0);
    return l;
}
static_assert(bwd_tile_lds(kTileRowsSmall, 0, 1).ainv + kTilePix * 4 <= bwd_tile_lds(kTileRowsSmall, 0, 1).seg, "U .. ainv fit the misc block");

// ---- LDS: the persistent forward kernel (kernels_forward_tile_ws.inc) -----------------------------------------------
constexpr int kWsMatrixWaves = 4;
constexpr int kWsSlots = 3;  // ring of set-up records (pixels, segments, row list, U)
// The padded pixel -> slot table (16-bit entries): rows of W + 4 entries rounded up to an ODD number of dwords, so that the
// 64 samples of a line that runs along the map's columns (one table row per lane) fall into different banks -- 68 entries
// are 34 dwords: lanes 16 apart collided, four to a bank.
constexpr int tile_ws_slot_width(int W) { return (((W + 4 + 1) >> 1) | 1) << 1; }
constexpr int tile_ws_slot_entries(int H, int W) { return (H + 4) * tile_ws_slot_width(W); }
// Bytes per pixel row of the fp16 A stage: unpadded, the row's 32 sixteen-byte chunks at the slots of et_lds_layout.h.  (Until
// this layout the rows were padded to 528 bytes "so that the b128 fragment reads are conflict-free" -- they are for contiguous
// 16-lane groups; gfx950 services a ds_read_b128 in the groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, in which one lane
// with kg = 1 landed on the slot of a lane with kg = 0: 8 LDS cycles per read instead of 4, tests/test_lds_layout_cpu.py.)
constexpr int kWsAStageRow = ET_ASTAGE_ROW_BYTES;
constexpr int kWsAStageBytes = 2 * kTilePix * kWsAStageRow;      // one stage: fp16 hi, then lo
constexpr int kWsStashBytes = kWsMatrixWaves * 2 * 16 * kTileWave * 4;   // two passes: the first half's G2 accumulators
static_assert(kWsAStageBytes >= kWsStashBytes, "the stash of the first half's accumulators fits the second A stage");
constexpr int kWsColWords = 72;     // column masks: 64 columns + 2 pad words on either side (+ 4 unused)
// Maps above 64 x 64 (BT = true, 288-row arrays: 96 x 96): a whole-map slot table would be 2 x 20 KB there and the block is at
// the LDS limit, so the table covers the tile's BAND only -- 16 entries per column of the major axis, entry (u + 2) * kWsBandStride + i
// <-> row col_base(u) + i (at a stride of kWsBandStride entries per column) -- and S2 runs two columns per lane.
constexpr int kWsColWordsBand = 136;          // 128 columns + 2 pad words on either side (+ 4 unused)
constexpr int kWsBandStride = 18;             // entries per column: 16 + 2 unused -- 9 dwords, so that the columns the 64 samples of a
                                              // line fall into start in different banks (16 entries = 8 dwords: four columns to a bank)
constexpr int kWsBandEntries = kWsColWordsBand * kWsBandStride;
// entries of ONE of the two slot tables (an even number: the tables are cleared in dwords)
constexpr int tile_ws_slot_table_entries(int H, int W, bool band_table)
{
    return band_table ? kWsBandEntries : (tile_ws_slot_entries(H, W) + 1) & ~1;
}
struct TileWsLds {
    int arr;        // [2][32][ROWS + 4] float  D/B ping, pong (16-byte aligned rows)
    int rows;       // [3][ROWS] int
    int pix;        // [3][32] int
    int seg;        // [3][32][4] float
    int U;          // [8] int    [3] U (or -1: overflow tile, skipped); [4] barrier counter of the vector waves
    int tq;         // [8] int    ring of this block's tile ids (-1: none left)
    int ainv;       // [2][32] float  1 / scale of the rows of the A stages
    int band;       // [3][4] float   base line of the slot's tile (SM of the band-table kernel)
    int dead;       // [4] int    two passes: tile (sequence number & 3) left to the list kernels
    int alpha;      // [32] float two passes: exp(m0 - m) per pixel of the tile (SM of half 1 -> G2)
    int rinv;       // [32] float             1 / (sum over all K samples)
    int col;        // [col_words] unsigned   column masks of the tile in S1 / S2
    int slot;       // [2][slot_entries] unsigned short: the pixel -> slot tables
    int astage;     // [2] A stages, at a multiple of 256 bytes: G1 steps through a row's chunks by XOR on the whole offset
                    // (et_astage_kstep_xor).  An OFFSET, never a rounded pointer: a pointer that went through an integer comes
                    // back as a generic one and every access through it becomes a FLAT load, which also ties up the
                    // vector-memory counter.
    int stash;      // two passes: the second stage's bytes hold the first half's accumulators
    int end;
    int bytes;      // what the launch asks for: a full 256-byte step for `astage`, whatever this shape's padding
};
constexpr TileWsLds tile_ws_lds_of(int rows, int slot_entries, bool band_table)
{
    TileWsLds l{};
    l.arr = 0;
    l.rows = l.arr + 2 * kTilePix * (rows + 4) * 4;
    l.pix = l.rows + kWsSlots * rows * 4;
    l.seg = l.pix + kWsSlots * kTilePix * 4;
    l.U = l.seg + kWsSlots * kTilePix * 16;
    l.tq = l.U + 8 * 4;
    l.ainv = l.tq + 8 * 4;
    l.band = l.ainv + 2 * kTilePix * 4;
    l.dead = l.band + kWsSlots * 16;
    l.alpha = l.dead + 4 * 4;
    l.rinv = l.alpha + kTilePix * 4;
    l.col = l.rinv + kTilePix * 4;
    l.slot = l.col + (band_table ? kWsColWordsBand : kWsColWords) * 4;
    const int slot_end = l.slot + 2 * slot_entries * 2;
    l.astage = (slot_end + 255) & ~255;
    l.stash = l.astage + kWsAStageBytes;
    l.end = l.astage + 2 * kWsAStageBytes;
    l.bytes = slot_end + 256 + 2 * kWsAStageBytes;
    return l;
}
constexpr TileWsLds tile_ws_lds(int rows, int H, int W, bool band_table)
{
    return tile_ws_lds_of(rows, tile_ws_slot_table_entries(H, W, band_table), band_table);
}
}  // namespace
