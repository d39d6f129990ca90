// libepipolar_amd.so: the MFMA tile formulation of the forward (et_epipolar_forward_tiled, et_epipolar_forward_fused, and their
// *_ix forms: the same implementations with the pairs named by index into pools of maps, PairIndex in et_tile_host.h).
// Kernels: the ordering (kernels_tile_order.inc, through et_tile_host.h), the persistent warp-specialised kernel
// (kernels_forward_tile_ws.inc) and the one-block-per-tile kernel (kernels_forward_tile.inc over kernels_tile_common.inc).
#include "et_common.h"
#include <cstdlib>

#include "et_tile_host.h"               // the ordering kernels and the host side of a tile call

namespace {
#include "kernels_forward_tile.inc"     // epipolar_fwd_tile_kernel / _list_kernel (one block per tile)
#include "kernels_forward_tile_ws.inc"  // epipolar_fwd_tile_ws_kernel (warp-specialised, persistent): the default
}  // namespace

#ifdef ET_WS_PROFILE
static long long *g_ws_prof = nullptr;   // profiling builds only (python -m epipolar_transformers_amd.build --profile)
extern "C" int et_dev_ws_profile(long long *device_buffer)
{
    g_ws_prof = device_buffer;
    return 0;
}
#endif

namespace {
// The parameter block of the one-block-per-tile kernels (its FwdParams are the persistent kernel's too).
TileParams fwd_tile_params(const EtLayerDesc *desc, const TileCall &c, const float *xs, const float *ys, const float *steps,
                           const float *cam, const float *feat_ref, const float *feat_src, float *out, float *attn, float *corr_pos,
                           const PairIndex &ix)
{
    TileParams tp;
    FwdParams &p = tp.f;
    p.d = *desc;
    set_pair_index(p, ix);
    p.xs = xs; p.ys = ys; p.steps = steps; p.cam = cam;
    p.fref = feat_ref; p.fsrc = feat_src;
    p.out = out; p.attn = attn; p.corr = corr_pos;
    p.res_bias = nullptr; p.res_base = nullptr;
    p.blocks_per_pair = c.tiles_per_pair;
    p.total_blocks = c.total;
    tp.tiles_per_pair = c.tiles_per_pair;
    tp.hw_words = c.hw_words;
    tp.rows_cap = c.rows_cap;
    tp.perm = c.w.perm;
    tp.stats = c.w.stats;
    tp.tile_list = c.w.ovf_list;
    tp.tile_count = c.w.ovf_count;
    // (per-pair scale estimates of the source maps: for the split-fp16 GEMMs of the persistent kernel and
    //  of the one-block-per-tile kernel; ET_VARIANT_TILE_EXACT keeps the latter in exact fp32)
    // soft-max off: exact fp32 throughout, as the header promises (the first GEMM feeds the `== 0 -> -1e10` mask and the
    // "attention" sim / K is unbounded: no fp16 form of the B rows)
    tp.scales = ((desc->variant & ET_VARIANT_TILE_EXACT) || !desc->softmax_enabled) ? nullptr : c.w.scales;
    return tp;
}

// The persistent kernel's: everything but the fused export's own fields (packed_w, bias, x; there f.out on request only).
TileWsParams tile_ws_params(const FwdParams &f, const TileCall &c)
{
    TileWsParams wp;
    wp.f = f;
    wp.perm = c.w.perm;
    wp.tiles_per_pair = c.tiles_per_pair;
    wp.total_tiles = c.total;
    wp.rows_cap = c.rows_cap;
    wp.ovf_count = c.w.ovf_count;
    wp.ovf_list = c.w.ovf_list;
    wp.stats = c.w.stats;
    wp.scales = c.w.scales;
    wp.segs = c.w.segs;
    wp.band = c.w.band;
    wp.packed_w = nullptr;
    wp.bias = nullptr;
    wp.x = nullptr;
    wp.err = c.w.err;
    wp.tile_ctr = c.w.ovf_count + kTileHdrXcdCtr;
    wp.setprio = 0;
    wp.prof = nullptr;
    return wp;
}

// The persistent kernel, one block per compute unit.  Instances: 256-row arrays (maps up to 64 x 64); 288-row arrays and a
// slot table over the tile's band (above 64 x 64, up to 96 x 96); the latter in two passes of 64 samples per tile with an
// online soft-max (64 < K <= 128, maps up to 128 x 128: sample + attention only, no fused instance).
template <bool FUSED>
int launch_fwd_tile_ws(const EtLayerDesc *desc, TileWsParams wp, int dev, hipStream_t st)
{
    const int cus = device_cus(dev);
    const unsigned grid = (unsigned)(wp.total_tiles < cus ? wp.total_tiles : cus), block = (kWsMatrixWaves + 8) * kWave;
    const bool two_pass = !FUSED && tile_ws_two_pass(desc);
    if (!two_pass && !tile_ws_band(desc))
        return launch_tile_kernel<epipolar_fwd_tile_ws_kernel<kTileRowsSmall, 8, FUSED>>(
            "epipolar_fwd_tile_ws_kernel", grid, block, tile_ws_lds_bytes(kTileRowsSmall, desc->H, desc->W), dev, st, wp);
    if (wp.rows_cap > kTileRowsWsLarge) wp.rows_cap = kTileRowsWsLarge;
    const size_t lds = tile_ws_lds_bytes(kTileRowsWsLarge, desc->H, desc->W, true);
    if constexpr (!FUSED) {
        if (two_pass)
            return launch_tile_kernel<epipolar_fwd_tile_ws_kernel<kTileRowsWsLarge, 8, false, true, 2>>("epipolar_fwd_tile_ws_kernel", grid,
                                                                                                        block, lds, dev, st, wp);
    }
    return launch_tile_kernel<epipolar_fwd_tile_ws_kernel<kTileRowsWsLarge, 8, FUSED, true>>("epipolar_fwd_tile_ws_kernel", grid, block,
                                                                                             lds, dev, st, wp);
}

// One block per tile: (rows, samples per lane) -> the instance.
template <int KPL, int ROWS>
int launch_fwd_tile_as(const TileParams &tp, size_t lds, int dev, hipStream_t st)
{
    return launch_tile_kernel<epipolar_fwd_tile_kernel<KPL, ROWS>>("epipolar_fwd_tile_kernel", (unsigned)tp.f.total_blocks, 256, lds,
                                                                   dev, st, tp);
}
int launch_fwd_tile(const TileParams &tp, int rows, int kpl, int dev, hipStream_t st)
{
    const size_t lds = fwd_tile_lds_bytes(rows, tp.hw_words, kpl);
    if (rows == kTileRowsSmall)
        return kpl == 1   ? launch_fwd_tile_as<1, kTileRowsSmall>(tp, lds, dev, st)
               : kpl == 2 ? launch_fwd_tile_as<2, kTileRowsSmall>(tp, lds, dev, st)
                          : launch_fwd_tile_as<4, kTileRowsSmall>(tp, lds, dev, st);
    if (rows == kTileRowsLarge)
        return kpl == 1   ? launch_fwd_tile_as<1, kTileRowsLarge>(tp, lds, dev, st)
               : kpl == 2 ? launch_fwd_tile_as<2, kTileRowsLarge>(tp, lds, dev, st)
                          : launch_fwd_tile_as<4, kTileRowsLarge>(tp, lds, dev, st);
    return kpl == 2 ? launch_fwd_tile_as<2, kTileRowsHuge>(tp, lds, dev, st)      // (512 rows per pixel need K > 96)
                    : launch_fwd_tile_as<4, kTileRowsHuge>(tp, lds, dev, st);
}

// The tiles the persistent kernel left over, one block per tile: two blocks per compute unit walk the list.
template <int KPL, int ROWS>
int launch_fwd_tile_list_as(const TileParams &tp, size_t lds, int dev, hipStream_t st)
{
    const long long total = tp.f.total_blocks, cus = device_cus(dev);
    return launch_tile_kernel<epipolar_fwd_tile_list_kernel<KPL, ROWS>>("epipolar_fwd_tile_list_kernel",
                                                                        (unsigned)(total < 2 * cus ? total : 2 * cus), 256, lds, dev, st, tp);
}
int launch_fwd_tile_list(const TileParams &tp, int rows, int kpl, int dev, hipStream_t st)
{
    const size_t lds = fwd_tile_lds_bytes(rows, tp.hw_words, kpl);
    if (kpl == 2)                   // (the two-pass kernel's left-overs: whole tiles, all K samples, one block per tile)
        return rows == kTileRowsHuge    ? launch_fwd_tile_list_as<2, kTileRowsHuge>(tp, lds, dev, st)
               : rows == kTileRowsLarge ? launch_fwd_tile_list_as<2, kTileRowsLarge>(tp, lds, dev, st)
                                        : launch_fwd_tile_list_as<2, kTileRowsSmall>(tp, lds, dev, st);
    if (rows == kTileRowsLarge) return launch_fwd_tile_list_as<1, kTileRowsLarge>(tp, lds, dev, st);
    // (round 6, measured: the left-overs of a map up to 64 x 64 -- all beyond 256 rows -- through the 384-row instance, whole
    //  instead of in pixel groups, take as long: 136 against 131 us for the near-rectified rig's 640 tiles.  A left-over tile
    //  is ~65 us of latency in a block either way and the list is two trips of the resident blocks.)
    return launch_fwd_tile_list_as<1, kTileRowsSmall>(tp, lds, dev, st);
}
}  // namespace

namespace {
int forward_tiled_impl(const char *who, const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps, const float *cam,
                       const float *feat_ref, const float *feat_src, float *out, float *attn, float *corr_pos, const float *res_bias,
                       float *res_base, void *workspace, size_t workspace_bytes, void *stream, const PairIndex &ix);
int forward_fused_impl(const char *who, const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps, const float *cam,
                       const float *feat_ref, const float *feat_src, const void *packed_w, const float *bias, float *x, float *attn,
                       float *corr_pos, float *out_scratch, int32_t want_out, void *workspace, size_t workspace_bytes, void *stream,
                       const PairIndex &ix);
}  // namespace

extern "C" {

size_t et_epipolar_forward_workspace_bytes(const EtLayerDesc *desc)
{
    if (validate(desc) || !tile_eligible(desc)) return 0;
    const size_t tiles = (size_t)desc->N * (((size_t)desc->H * desc->W + kTilePix - 1) / kTilePix);
    return tile_workspace_layout(tiles, (size_t)desc->N, (size_t)desc->H * desc->W).bytes;
}

size_t et_epipolar_forward_workspace_error_offset(const EtLayerDesc *desc)
{
    if (validate(desc) || !tile_eligible(desc)) return 0;
    return kTileHdrErr * sizeof(int);   // in the header: the same place for every shape (a workspace is reused across shapes)
}

size_t et_epipolar_forward_workspace_stats_offset(const EtLayerDesc *desc)
{
    if (validate(desc) || !tile_eligible(desc)) return 0;
    const size_t tiles = (size_t)desc->N * (((size_t)desc->H * desc->W + kTilePix - 1) / kTilePix);
    return tile_workspace_layout(tiles, (size_t)desc->N, (size_t)desc->H * desc->W).stats;
}

int et_epipolar_forward_tiled(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                              const float *cam, const float *feat_ref, const float *feat_src, float *out,
                              float *attn, float *corr_pos, const float *res_bias, float *res_base,
                              void *workspace, size_t workspace_bytes, void *stream)
{
    return forward_tiled_impl("et_epipolar_forward_tiled", desc, xs, ys, steps, cam, feat_ref, feat_src, out, attn, corr_pos, res_bias,
                              res_base, workspace, workspace_bytes, stream, PairIndex());
}

int et_epipolar_forward_tiled_ix(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                 const float *cam, const float *feat_ref, const float *feat_src, float *out,
                                 float *attn, float *corr_pos, const float *res_bias, float *res_base,
                                 void *workspace, size_t workspace_bytes, void *stream, const int32_t *ref_index,
                                 const int32_t *src_index, int32_t M_ref, int32_t M_src)
{
    PairIndex ix;
    if (int e = make_pair_index(desc, "et_epipolar_forward_tiled_ix", ref_index, src_index, M_ref, M_src, &ix)) return e;
    return forward_tiled_impl("et_epipolar_forward_tiled_ix", desc, xs, ys, steps, cam, feat_ref, feat_src, out, attn, corr_pos,
                              res_bias, res_base, workspace, workspace_bytes, stream, ix);
}

int et_epipolar_forward_fused(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                              const float *cam, const float *feat_ref, const float *feat_src, const void *packed_w,
                              const float *bias, float *x, float *attn, float *corr_pos, float *out_scratch,
                              int32_t want_out, void *workspace, size_t workspace_bytes, void *stream)
{
    return forward_fused_impl("et_epipolar_forward_fused", desc, xs, ys, steps, cam, feat_ref, feat_src, packed_w, bias, x, attn,
                              corr_pos, out_scratch, want_out, workspace, workspace_bytes, stream, PairIndex());
}

int et_epipolar_forward_fused_ix(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                 const float *cam, const float *feat_ref, const float *feat_src, const void *packed_w,
                                 const float *bias, float *x, float *attn, float *corr_pos, float *out_scratch,
                                 int32_t want_out, void *workspace, size_t workspace_bytes, void *stream,
                                 const int32_t *ref_index, const int32_t *src_index, int32_t M_ref, int32_t M_src)
{
    PairIndex ix;
    if (int e = make_pair_index(desc, "et_epipolar_forward_fused_ix", ref_index, src_index, M_ref, M_src, &ix)) return e;
    return forward_fused_impl("et_epipolar_forward_fused_ix", desc, xs, ys, steps, cam, feat_ref, feat_src, packed_w, bias, x, attn,
                              corr_pos, out_scratch, want_out, workspace, workspace_bytes, stream, ix);
}

}  // extern "C"

namespace {
// et_epipolar_forward_tiled and its indexed form (a default PairIndex: the identity, pair n owns map n)
int forward_tiled_impl(const char *who, const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps, const float *cam,
                       const float *feat_ref, const float *feat_src, float *out, float *attn, float *corr_pos, const float *res_bias,
                       float *res_base, void *workspace, size_t workspace_bytes, void *stream, const PairIndex &ix)
{
    const char *bad_args = (!xs || !ys || !steps || !cam || !feat_ref || !feat_src || !out) ? "NULL pointer"
                           : (res_bias && !res_base)                                        ? "res_bias given without res_base"
                                                                                            : nullptr;
    TileCall c;
    if (int e = begin_tile_call(desc, who, bad_args, "et_epipolar_forward", nullptr, workspace, workspace_bytes, &c))
        return e;
    hipStream_t st = (hipStream_t)stream;
    TileParams tp = fwd_tile_params(desc, c, xs, ys, steps, cam, feat_ref, feat_src, out, attn, corr_pos, ix);
    tp.f.res_bias = res_bias;
    tp.f.res_base = res_base;
    // 1. order every pair's reference pixels by their epipolar line (also clears the overflow counter)
    if (int e = launch_tile_order(desc, xs, ys, cam, feat_ref, feat_src, c.w, c.tiles_per_pair, true, c.w.scales, true, nullptr, 0, st,
                                  "et_epipolar_forward_tiled(order)", ix))
        return e;
    const int dev = current_device();
    const int kpl = (desc->K + 63) / 64;
    const int rows = tile_rows(desc);
    if (tile_ws_eligible(desc) || tile_ws_two_pass(desc)) {
        // 2a. the persistent, warp-specialised kernel (kernels_forward_tile_ws.inc): the default ...
        TileWsParams wp = tile_ws_params(tp.f, c);
        wp.setprio = (desc->variant & ET_VARIANT_WS_SETPRIO) ? 1 : 0;
#ifdef ET_WS_PROFILE
        wp.prof = g_ws_prof;
        if (const char *e = getenv("ET_WS_EXPERIMENT")) wp.setprio |= atoi(e);
#endif
        if (int e = launch_fwd_tile_ws<false>(desc, wp, dev, st)) return e;
        if (int e = check_launch("et_epipolar_forward_tiled(ws)")) return e;
        // ... 2b. and the tiles it left over one block per tile
        if (int e = launch_fwd_tile_list(tp, rows, kpl, dev, st)) return e;
        return check_launch("et_epipolar_forward_tiled(list)");
    }
    // 2. one block per tile
    if (int e = launch_fwd_tile(tp, rows, kpl, dev, st)) return e;
    return check_launch("et_epipolar_forward_tiled");
}


// The layer's eval-mode forward as ONE data kernel: sampling + attention (as et_epipolar_forward_tiled) with
// x = feat_ref + bias + out . Wf^T -- bn(z(out)) + out + feat with the BN folded into z (epipolar.py:250-253, resnet.py:388;
// what et_residual_gemm computes from `out` in a second pass) -- as a third GEMM of the persistent kernel.
int forward_fused_impl(const char *who, const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps, const float *cam,
                       const float *feat_ref, const float *feat_src, const void *packed_w, const float *bias, float *x, float *attn,
                       float *corr_pos, float *out_scratch, int32_t want_out, void *workspace, size_t workspace_bytes, void *stream,
                       const PairIndex &ix)
{
    if (int e = validate(desc)) return e;
    if (!xs || !ys || !steps || !cam || !feat_ref || !feat_src || !packed_w || !bias || !x || !out_scratch)
        return fail("et_epipolar_forward_fused: NULL pointer");
    if (reinterpret_cast<uintptr_t>(packed_w) & 15) return fail("et_epipolar_forward_fused: packed weight must be 16-byte aligned");
    if (!tile_eligible(desc) || !tile_ws_eligible(desc))
        return fail("et_epipolar_forward_fused: needs the warp-specialised tile kernel (C == 256, maps up to 96 x 96, K <= 64, "
                    "soft-max on; got C=%d H=%d W=%d K=%d variant=%d): use et_epipolar_forward_tiled + et_residual_gemm",
                    desc->C, desc->H, desc->W, desc->K, desc->variant);
    // (its own, narrower eligibility and message above: the descriptor and the shape pass begin_tile_call's checks)
    TileCall c;
    if (int e = begin_tile_call(desc, who, nullptr, "et_epipolar_forward_tiled", nullptr, workspace, workspace_bytes, &c))
        return e;
    hipStream_t st = (hipStream_t)stream;
    const TileParams tp = fwd_tile_params(desc, c, xs, ys, steps, cam, feat_ref, feat_src, out_scratch, attn, corr_pos, ix);
    if (int e = launch_tile_order(desc, xs, ys, cam, feat_ref, feat_src, c.w, c.tiles_per_pair, true, c.w.scales, true, nullptr, 0, st,
                                  "et_epipolar_forward_fused(order)", ix))
        return e;
    const int dev = current_device();
    TileWsParams wp = tile_ws_params(tp.f, c);
    wp.f.out = want_out ? out_scratch : nullptr;      // (the persistent kernel writes `out` on request only)
    wp.packed_w = reinterpret_cast<const unsigned *>(packed_w);
    wp.bias = bias;
    wp.x = x;
#ifdef ET_WS_PROFILE
    wp.prof = g_ws_prof;
#endif
    if (int e = launch_fwd_tile_ws<true>(desc, wp, dev, st)) return e;
    if (int e = check_launch("et_epipolar_forward_fused(ws)")) return e;
    // the tiles it left over: `out` rows one block per tile (K <= 64: one sample per lane), then their x rows
    if (int e = launch_fwd_tile_list(tp, tile_rows(desc), 1, dev, st)) return e;
    if (int e = check_launch("et_epipolar_forward_fused(list)")) return e;
    // their x rows: the residual GEMM kernel over the list, two tiles per block and trip (round 6: the plain-fp32 kernel this replaces
    // took 76 us for the near-rectified rig's 640 left-over tiles -- 256 KB of weight fragments per eight pixel rows; now 24 us)
    return et_internal_residual_rows_list(c.w.perm, c.w.ovf_list, c.w.ovf_count, c.tiles_per_pair, c.HW, c.total, out_scratch, feat_ref,
                                          reinterpret_cast<const unsigned *>(packed_w), bias, x, st, ix.ref_index, ix.M_ref);
}
}  // namespace
