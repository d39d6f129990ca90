// The host side of a tile call, shared by the two tile translation units (et_forward_tile.hip, et_backward_tile.hip):
// eligibility, the workspace layout, begin_tile_call (checks, sizes, carved workspace), the ordering launches and the
// launch helper of the tile kernels.  In the anonymous namespace: each unit instantiates its own copies.
#pragma once
#include <algorithm>
#include "et_common.h"
#include "et_tile_layout.h"         // kTilePix, kTileRows*, the workspace's header words and regions, the kernels' LDS
namespace {
static_assert(kTileWave == kWave && kTileXcds == kXcds, "et_tile_layout.h restates them (it includes no HIP header)");
#include "kernels_tile_order.inc"   // tile_keys_kernel, tile_order_kernel

// The MFMA tile path applies to the 256-channel head when one reference pixel alone can never
// overflow the tile's row array: a pixel's K samples touch at most 4K source pixels, and a line
// through a W x H map at most 4 per column (or per row, whichever way it runs), i.e. 4 max(W, H).
int tile_rows_per_pixel(const EtLayerDesc *d)
{
    const int longest = d->W > d->H ? d->W : d->H;
    return (d->K < longest) ? 4 * d->K : 4 * longest;
}
// rows per tile the kernel is instantiated with: 256 up to 64 x 64 maps, 384 beyond (longer lines), 512 when a
// single pixel may need more than that
int tile_rows(const EtLayerDesc *d)
{
    if (tile_rows_per_pixel(d) > kTileRowsLarge) return kTileRowsHuge;
    return (d->W > 64 || d->H > 64) ? kTileRowsLarge : kTileRowsSmall;
}
int tile_rows_cap(const EtLayerDesc *d) { return (d->variant & ET_VARIANT_TILE_SPLIT) ? 64 : tile_rows(d); }

bool tile_eligible(const EtLayerDesc *d)
{
    if (d->C != 256 || d->K > 256) return false;
    const long long hw = (long long)d->H * d->W;
    if (hw > 16384) return false;  // bitonic sort of one pair's pixels lives in LDS
    return tile_rows_per_pixel(d) <= tile_rows_cap(d);
}

// the warp-specialised persistent kernels: lanes <-> samples (K <= 64), 256-row arrays.  Soft-max on only: their second
// GEMM holds the B rows (attention x bilinear weights, <= 1 with the soft-max) in fp16 pairs; with
// EPIPOLAR.SOFTMAX_ENABLED False the "attention" is sim / K -- unbounded, -1e10 / K on masked samples -- and the call
// takes the exact-fp32 one-block-per-tile kernel.
// Two instances: 256-row arrays and a whole-map slot table for maps up to 64 x 64; 288-row arrays and a slot table over the
// tile's band for maps up to 96 x 96 (every tile of a 96 x 96 map has at most 280 rows; ET_VARIANT_WS_BAND: also for smaller
// maps, where it must return what the first returns -- the test of the band-table code).
bool tile_ws_band(const EtLayerDesc *d)
{
    const int longest = d->W > d->H ? d->W : d->H;
    if ((d->variant & ET_VARIANT_TILE_CLASSIC) || !d->softmax_enabled || d->K > 64 || d->W < 2 || longest > kWsMaxSideBand)
        return false;
    return tile_rows(d) == kTileRowsLarge || ((d->variant & ET_VARIANT_WS_BAND) && tile_rows(d) == kTileRowsSmall);
}
// 64 < K <= 128 (round 6): the band-table instance in TWO passes of 64 samples per tile with an online soft-max
// (kernels_forward_tile_ws.inc, KH = 2), maps up to 128 x 128 (its column masks hold 128 columns).  Sample + attention only: the
// one-kernel layer keeps K <= 64.
bool tile_ws_two_pass(const EtLayerDesc *d)
{
    const int longest = d->W > d->H ? d->W : d->H;
    return !(d->variant & ET_VARIANT_TILE_CLASSIC) && d->softmax_enabled && d->K > 64 && d->K <= 128 && d->W >= 2 && longest <= kWsMaxSideTwoPass;
}
bool tile_ws_eligible(const EtLayerDesc *d)
{
    return (!(d->variant & ET_VARIANT_TILE_CLASSIC) && d->softmax_enabled && d->K <= 64 && d->W >= 2 &&
            tile_rows(d) == kTileRowsSmall) || tile_ws_band(d);
}
// The caller's workspace, carved: header words, regions and sizes are et_tile_layout.h's.
struct TileWorkspace {
    int *perm, *ovf_count, *err, *ovf_list, *stats;
    float *scales;
    float4 *segs, *band, *segs_pix;
    char *base;     // the aligned base: the offsets of a layout count from here
    size_t end;     // TileWorkspaceLayout::end of this call's shape
};
TileWorkspace carve_tile_workspace(void *workspace, size_t tiles, size_t pairs, size_t hw)
{
    const TileWorkspaceLayout l = tile_workspace_layout(tiles, pairs, hw);
    TileWorkspace w;
    w.base = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(workspace) + (kTileWorkspaceAlign - 1)) & ~(uintptr_t)(kTileWorkspaceAlign - 1));
    w.end = l.end;
    int *const header = reinterpret_cast<int *>(w.base);
    w.ovf_count = header + kTileHdrCount;
    w.err = header + kTileHdrErr;
    w.perm = reinterpret_cast<int *>(w.base + l.perm);
    w.ovf_list = reinterpret_cast<int *>(w.base + l.ovf_list);
    w.stats = reinterpret_cast<int *>(w.base + l.stats);
    w.scales = reinterpret_cast<float *>(w.base + l.scales);
    w.segs = reinterpret_cast<float4 *>(w.base + l.segs);
    w.band = reinterpret_cast<float4 *>(w.base + l.band);
    w.segs_pix = reinterpret_cast<float4 *>(w.base + l.segs_pix);
    return w;
}

// The pair table of an indexed call (ET_HAS_PAIR_INDEX): feat_ref / feat_src are pools of M_ref / M_src maps and pair n reads maps
// ref_index[n] / src_index[n] (device arrays of N int32; NULL: identity, the unindexed exports' call).
struct PairIndex {
    const int *ref_index = nullptr, *src_index = nullptr;
    int M_ref = 0, M_src = 0;
};
// The identity table of an unindexed call's N pairs, or the caller's after its checks (a pool of at least one map; a NULL index
// names map n, so its pool holds exactly N maps).
int make_pair_index(const EtLayerDesc *desc, const char *who, const int *ref_index, const int *src_index, int M_ref, int M_src,
                    PairIndex *ix)
{
    if (!desc) return fail("desc is NULL");
    if (M_ref <= 0 || M_src <= 0) return fail("%s: pools of M_ref=%d / M_src=%d maps", who, M_ref, M_src);
    if (!ref_index && M_ref != desc->N) return fail("%s: ref_index is NULL (identity) but M_ref=%d is not N=%d", who, M_ref, desc->N);
    if (!src_index && M_src != desc->N) return fail("%s: src_index is NULL (identity) but M_src=%d is not N=%d", who, M_src, desc->N);
    ix->ref_index = ref_index; ix->src_index = src_index;
    ix->M_ref = M_ref; ix->M_src = M_src;
    return 0;
}
template <class Params>
void set_pair_index(Params &p, const PairIndex &ix)
{
    p.ref_index = ix.ref_index; p.src_index = ix.src_index;
    p.M_ref = ix.M_ref; p.M_src = ix.M_src;
}

// The ordering of a tile call: tile_keys_kernel (segment and sort key of every reference pixel, whole device; clears the
// header words when `header`), then tile_order_kernel (one block per pair: sort -> perm, the segments in tile order and the
// tiles' base lines when `ws_tables`, the scale estimates when `scales`; `clear`: extra blocks that zero a buffer beside the
// sort -- the backward's grad_src).
int launch_tile_order(const EtLayerDesc *desc, const float *xs, const float *ys, const float *cam, const float *feat_ref,
                      const float *feat_src, const TileWorkspace &w, int tiles_per_pair, bool header, float *scales,
                      bool ws_tables, float4 *clear, size_t clear_vec4, hipStream_t st, const char *who,
                      const PairIndex &ix = PairIndex())
{
    const int HW = desc->H * desc->W;
    const int perm_stride = tiles_per_pair * kTilePix;
    int n2 = 64;
    while (n2 < HW) n2 <<= 1;
    const size_t lds_sort = tile_order_lds_bytes(n2);
    const int dev = current_device();
    ET_GRANT_LDS(tile_order_kernel, lds_sort, dev);
    // (the sort keys of a pair, 8 bytes per pixel, live in the region of its ordered segments until tile_order_kernel has
    //  consumed them: et_tile_layout.h)
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(w.segs);
    hipLaunchKernelGGL(tile_keys_kernel, dim3((unsigned)((HW + 255) / 256) * desc->N), dim3(256), 0, st, *desc, xs, ys, cam, perm_stride,
                       keys, w.segs_pix, header ? w.ovf_count : (int *)nullptr);
    // (the clearing blocks: >= 8 float4 stores per thread)
    const unsigned clear_blocks = clear ? (unsigned)std::min<size_t>(2048, (clear_vec4 + 8 * 1024 - 1) / (8 * 1024)) : 0u;
    hipLaunchKernelGGL(tile_order_kernel, dim3(desc->N + clear_blocks), dim3(1024), lds_sort, st, *desc, n2, perm_stride, keys,
                       w.segs_pix, w.perm, feat_ref, feat_src, scales, ws_tables ? w.segs : (float4 *)nullptr,
                       ws_tables ? w.band : (float4 *)nullptr, clear, clear_vec4, ix.ref_index, ix.src_index, ix.M_ref, ix.M_src);
    return check_launch(who);
}

// What every tile call starts from: the sizes of the call and its carved workspace.
struct TileCall {
    int HW, tiles_per_pair, total, hw_words, rows_cap;
    TileWorkspace w;
};
// The checks every tile export starts with, in this order -- the descriptor, `bad_args` (NULL, or what is wrong with the
// export's own arguments), eligibility (`instead`: the export to use for other shapes), the workspace's size (the forward's
// layout + `extra_bytes(pairs, pixels per map)` where given), the grid -- then the sizes and the carved workspace -> c.
int begin_tile_call(const EtLayerDesc *desc, const char *who, const char *bad_args, const char *instead,
                    size_t (*extra_bytes)(size_t, size_t), void *workspace, size_t workspace_bytes, TileCall *c)
{
    if (int e = validate(desc)) return e;
    if (bad_args) return fail("%s: %s", who, bad_args);
    if (!tile_eligible(desc))
        return fail("%s: needs C == 256, H*W <= 16384 and 4 min(K, max(W,H)) <= %d (got C=%d H=%d W=%d K=%d); use %s", who,
                    tile_rows_cap(desc), desc->C, desc->H, desc->W, desc->K, instead);
    c->HW = desc->H * desc->W;
    c->tiles_per_pair = (c->HW + kTilePix - 1) / kTilePix;
    const long long total = (long long)c->tiles_per_pair * desc->N;
    const size_t need = tile_workspace_layout((size_t)total, (size_t)desc->N, (size_t)c->HW).bytes +
                        (extra_bytes ? extra_bytes((size_t)desc->N, (size_t)c->HW) : 0);
    if (!workspace || workspace_bytes < need)
        return fail("%s: workspace of %zu bytes is smaller than the %zu required", who, workspace ? workspace_bytes : (size_t)0, need);
    // (one limit for both directions: kTilePix * total, the entries of perm, stays below 2^31 -- both index the same perm with
    //  int tile numbers; the backward used to check `total` alone, a bound no workspace of the forward's layout reaches)
    if (total > 0x7fffffffLL / kTilePix) return fail("grid too large");
    c->total = (int)total;
    c->hw_words = (c->HW + 31) / 32;
    c->rows_cap = tile_rows_cap(desc);
    c->w = carve_tile_workspace(workspace, (size_t)total, (size_t)desc->N, (size_t)c->HW);
    return 0;
}

// Grants `lds` bytes of dynamic LDS to a kernel instance (once per instance, device and process) and launches it.
template <auto Kernel, class Params>
int launch_tile_kernel(const char *name, unsigned grid, unsigned block, size_t lds, int dev, hipStream_t st, const Params &params)
{
    static int granted[64];
    if (int e = grant_lds(Kernel, lds, dev, granted, name)) return e;
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(block), lds, st, params);
    return 0;
}
}  // namespace
