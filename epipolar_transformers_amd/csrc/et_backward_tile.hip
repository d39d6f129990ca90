// libepipolar_amd.so: the MFMA tile formulation of the backward (et_epipolar_backward_tiled).
#include <algorithm>
#include "et_common.h"

namespace {
#include "kernels_forward_tile.inc"   // tile_order_kernel and the tile helpers shared with the forward
#include "kernels_backward_tile.inc"  // epipolar_bwd_tile_kernel
#include "kernels_backward_det.inc"   // the deterministic form: maxima, quantum, int64 -> fp32
}  // namespace
#include "et_tile_host.h"

namespace {
// Workspace of the deterministic form: the forward-layout workspace (same header, same sticky error word), then, from the next
// 256-byte boundary: acc int64[N * HW * 256] | quanta float[4 * N] | partial maxima float[4 * kDetMaxBlocks * N].
struct DetWorkspace {
    long long *acc;
    float *quanta, *partial;
};
size_t det_extra_bytes(size_t pairs, size_t hw)
{
    return 256 + pairs * hw * 256 * sizeof(long long) + pairs * 4 * sizeof(float) + pairs * kDetMaxBlocks * 4 * sizeof(float);
}
DetWorkspace carve_det_workspace(const TileWorkspace &w, size_t tiles, size_t pairs, size_t hw)
{
    DetWorkspace dw;
    const uintptr_t end = reinterpret_cast<uintptr_t>(w.ovf_count) + tile_workspace_words(tiles, pairs, hw) * sizeof(int);
    dw.acc = reinterpret_cast<long long *>((end + 255) & ~(uintptr_t)255);
    dw.quanta = reinterpret_cast<float *>(dw.acc + pairs * hw * 256);
    dw.partial = dw.quanta + 4 * pairs;
    return dw;
}
int backward_tiled_impl(bool det, const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                        const float *cam, const float *feat_ref, const float *feat_src, const float *attn,
                        const float *grad_out, float *grad_ref, float *grad_src, void *workspace,
                        size_t workspace_bytes, void *stream);
}  // namespace

extern "C" {

size_t et_epipolar_backward_tiled_det_workspace_bytes(const EtLayerDesc *desc)
{
    const size_t fwd = et_epipolar_backward_tiled_workspace_bytes(desc);
    if (fwd == 0) return 0;
    return fwd + det_extra_bytes((size_t)desc->N, (size_t)desc->H * desc->W);
}

int et_epipolar_backward_tiled_det(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                   const float *cam, const float *feat_ref, const float *feat_src, const float *attn,
                                   const float *grad_out, float *grad_ref, float *grad_src, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    return backward_tiled_impl(true, desc, xs, ys, steps, cam, feat_ref, feat_src, attn, grad_out, grad_ref, grad_src, workspace,
                               workspace_bytes, stream);
}

int et_debug_host_det_quantum(const EtLayerDesc *desc, float m_ref, float m_src, float m_g, float *q, float *bound)
{
    if (!desc || !q || !bound) return fail("et_debug_host_det_quantum: NULL pointer");
    if (!desc->softmax_enabled) return fail("et_debug_host_det_quantum: no bound with the soft-max off (sim / K is unbounded)");
    if (!(m_ref >= 0.f) || !(m_src >= 0.f) || !(m_g >= 0.f)) return fail("et_debug_host_det_quantum: maxima must be >= 0");
    const DetQuantum r = det_quantum(desc->softmax_scale, m_ref, m_src, m_g);
    *q = r.q;
    *bound = r.bound;
    return 0;
}

size_t et_epipolar_backward_tiled_workspace_bytes(const EtLayerDesc *desc)
{
    if (validate(desc) || !tile_eligible(desc)) return 0;
    return et_epipolar_forward_workspace_bytes(desc);
}

int et_epipolar_backward_tiled(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                               const float *cam, const float *feat_ref, const float *feat_src,
                               const float *grad_out, float *grad_ref, float *grad_src, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    return backward_tiled_impl(false, desc, xs, ys, steps, cam, feat_ref, feat_src, nullptr, grad_out, grad_ref, grad_src,
                               workspace, workspace_bytes, stream);
}

int et_epipolar_backward_tiled_attn(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                    const float *cam, const float *feat_ref, const float *feat_src, const float *attn,
                                    const float *grad_out, float *grad_ref, float *grad_src, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    return backward_tiled_impl(false, desc, xs, ys, steps, cam, feat_ref, feat_src, attn, grad_out, grad_ref, grad_src, workspace,
                               workspace_bytes, stream);
}

}  // extern "C"

namespace {
int backward_tiled_impl(bool det, const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                        const float *cam, const float *feat_ref, const float *feat_src, const float *attn,
                        const float *grad_out, float *grad_ref, float *grad_src, void *workspace,
                        size_t workspace_bytes, void *stream)
{
    if (int e = validate(desc)) return e;
    if (!xs || !ys || !steps || !cam || !feat_ref || !feat_src || !grad_out || !grad_ref || !grad_src)
        return fail("et_epipolar_backward_tiled: NULL pointer");
    const size_t need = det ? et_epipolar_backward_tiled_det_workspace_bytes(desc) : et_epipolar_backward_tiled_workspace_bytes(desc);
    if (need == 0)
        return fail("et_epipolar_backward_tiled: needs C == 256, H*W <= 16384 and 4 min(K, max(W,H)) <= %d "
                    "(got C=%d H=%d W=%d K=%d); use et_epipolar_backward", tile_rows_cap(desc), desc->C, desc->H,
                    desc->W, desc->K);
    if (!workspace || workspace_bytes < need)
        return fail("et_epipolar_backward_tiled: workspace of %zu bytes is smaller than the %zu required",
                    workspace ? workspace_bytes : (size_t)0, need);
    if (det && !desc->softmax_enabled)
        return fail("et_epipolar_backward_tiled_det: needs the soft-max (EPIPOLAR.SOFTMAX_ENABLED False makes the attention sim / K, "
                    "-1e10 / K under the mask: no bound to take the fixed-point quantum from); et_epipolar_backward with a workspace "
                    "is the bit-reproducible form there");
    hipStream_t st = (hipStream_t)stream;
    const int HW = desc->H * desc->W;
    BwdTileParams tp;
    std::memset(&tp, 0, sizeof(tp));
    BwdParams &p = tp.b;
    p.d = *desc;
    p.xs = xs; p.ys = ys; p.steps = steps; p.cam = cam;
    p.fref = feat_ref; p.fsrc = feat_src; p.gout = grad_out;
    p.gref = grad_ref; p.gsrc = grad_src;
    tp.tiles_per_pair = (HW + kTilePix - 1) / kTilePix;
    p.blocks_per_pair = tp.tiles_per_pair;
    const long long total = (long long)tp.tiles_per_pair * desc->N;
    if (total > 0x7fffffffLL) return fail("grid too large");
    p.total_blocks = (int)total;
    tp.hw_words = (HW + 31) / 32;
    tp.rows_cap = tile_rows_cap(desc);
    tp.attn = attn;
    // (with the per-pair scale estimates of the source maps: the merged kernels run their row-type GEMMs as split-fp16
    //  products; the workspace has the forward's layout.  grad_src is cleared by extra blocks of the ordering kernel: the
    //  tile kernel adds into it)
    const TileWorkspace w = carve_tile_workspace(workspace, (size_t)total, (size_t)desc->N, (size_t)HW);
    tp.perm = w.perm;
    tp.scales = w.scales;
    // deterministic form: the clearing blocks zero the int64 accumulator instead (twice the bytes); grad_src is written whole by
    // det_finish_kernel
    const DetWorkspace dw = carve_det_workspace(w, (size_t)total, (size_t)desc->N, (size_t)HW);
    const size_t clear_vec4 = (size_t)desc->N * HW * (desc->C / 4) * (det ? 2 : 1);     // (C == 256)
    // (header = true: the ordering clears the workspace's overflow counter, which the merged launch below counts into)
    if (int e = launch_tile_order(desc, xs, ys, cam, feat_ref, feat_src, w, tp.tiles_per_pair, true, w.scales, false,
                                  det ? reinterpret_cast<float4 *>(dw.acc) : reinterpret_cast<float4 *>(grad_src), clear_vec4, st,
                                  "et_epipolar_backward_tiled(order)"))
        return e;
    const unsigned vec4_per_pair = (unsigned)HW * (desc->C / 4);
    if (det) {
        // the pair's exact maxima -> its quantum (kernels_backward_det.inc)
        hipLaunchKernelGGL(det_maxima_kernel, dim3(kDetMaxBlocks, desc->N), dim3(256), 0, st, reinterpret_cast<const float4 *>(feat_ref),
                           reinterpret_cast<const float4 *>(feat_src), reinterpret_cast<const float4 *>(grad_out), vec4_per_pair,
                           dw.partial);
        hipLaunchKernelGGL(det_quantum_kernel, dim3((desc->N + 63) / 64), dim3(64), 0, st, desc->N, kDetMaxBlocks, desc->softmax_scale,
                           dw.partial, dw.quanta);
        if (int e = check_launch("et_epipolar_backward_tiled_det(quantum)")) return e;
        tp.det_acc = dw.acc;
        tp.det_q = dw.quanta;
        tp.det_err = w.err;
    }
    const int dev = current_device();
    const int kpl = (desc->K + 63) / 64;
    // 64 x 64 maps, K <= 64: the merged form (two 192-column arrays, one round of atomics per tile) unless the caller
    // asks for the one-array kernel (ET_VARIANT_TILE_CLASSIC)
    const bool merged = (tile_rows(desc) == kTileRowsSmall || tile_rows(desc) == kTileRowsLarge) && kpl == 1 &&
                        !(desc->variant & ET_VARIANT_TILE_CLASSIC);
    const int rows = !merged ? tile_rows(desc) : tile_rows(desc) == kTileRowsSmall ? kTileRowsMerged : kTileRowsMergedLarge;
    if (merged && tp.rows_cap > rows) tp.rows_cap = rows;
    auto lds_of = [&](int r, bool m) {
        return (size_t)(bwd_tile_array_floats(r) + r + kTilePix + 60 + kTilePix * 4) * 4 + (size_t)tp.hw_words * 8 +
               ((kpl == 1 && !m) ? (size_t)kTilePix * kWave * 8 : 0);
    };
    size_t lds = lds_of(rows, merged);
    // merged launches defer the tiles beyond their columns to a second launch of the one-array kernel (unless the caller tests the
    // splitting: ET_VARIANT_TILE_SPLIT)
    const bool defer = merged && !(desc->variant & (ET_VARIANT_TILE_SPLIT | ET_VARIANT_BWD_SPLIT_IN_PLACE));
    if (defer) {
        tp.ovf_count = w.ovf_count;
        tp.ovf_list = w.ovf_list;
    }
    // capacity of the second launch's kernel: a deferred tile beyond it is shared by kDetHardParts blocks there (deterministic form)
    tp.list_cap = (tile_rows(desc) == kTileRowsSmall && ET_BWD_LIST_MERGED) ? kTileRowsMergedLarge : tile_rows_cap(desc);
#define ET_BTILE_(KK, RR, DD)                                                                                        \
    do {                                                                                                             \
        ET_GRANT_LDS((epipolar_bwd_tile_kernel<KK, RR, DD>), lds, dev);                                              \
        hipLaunchKernelGGL((epipolar_bwd_tile_kernel<KK, RR, DD>), dim3((unsigned)total), dim3(256), lds, st, tp);   \
    } while (0)
#define ET_BTILE(KK, RR)                     \
    do {                                     \
        if (det) ET_BTILE_(KK, RR, true);    \
        else ET_BTILE_(KK, RR, false);       \
    } while (0)
#define ET_BLIST_(RR, DD)                                                                                            \
    do {                                                                                                             \
        ET_GRANT_LDS((epipolar_bwd_tile_list_kernel<1, RR, DD>), lds, dev);                                          \
        hipLaunchKernelGGL((epipolar_bwd_tile_list_kernel<1, RR, DD>), dim3(lgrid), dim3(256), lds, st, tp);         \
    } while (0)
#define ET_BLIST(RR)                     \
    do {                                 \
        if (det) ET_BLIST_(RR, true);    \
        else ET_BLIST_(RR, false);       \
    } while (0)
    if (rows == kTileRowsMerged || rows == kTileRowsMergedLarge) {
        if (rows == kTileRowsMerged) ET_BTILE(1, kTileRowsMerged);
        else ET_BTILE(1, kTileRowsMergedLarge);
        if (defer) {
            if (int e = check_launch("et_epipolar_backward_tiled(merged)")) return e;
            tp.tile_list = w.ovf_list;
            tp.tile_count = w.ovf_count;
            tp.ovf_list = nullptr;
            tp.ovf_count = nullptr;
            tp.rows_cap = tile_rows_cap(desc);
            lds = lds_of(tile_rows(desc), false);
            // (two blocks per compute unit -- what is resident at once -- walk the list)
            const int cus = device_cus(dev);
            const unsigned lgrid = (unsigned)(total < 2LL * cus ? total : 2LL * cus);
            if (tile_rows(desc) == kTileRowsSmall && ET_BWD_LIST_MERGED) {
                // round 6: the deferred tiles of a 64 x 64 map (193 .. ~280 rows) by the MERGED kernel of 288 columns -- one
                // derivation of the samples' slots for both arrays, no half passes (a tile beyond 288 rows is split there)
                tp.rows_cap = kTileRowsMergedLarge;
                lds = lds_of(kTileRowsMergedLarge, true);
                ET_BLIST(kTileRowsMergedLarge);
            } else if (tile_rows(desc) == kTileRowsSmall) {
                ET_BLIST(kTileRowsSmall);
            } else {
                ET_BLIST(kTileRowsLarge);
            }
        }
    } else if (rows == kTileRowsSmall) {
        if (kpl == 1) ET_BTILE(1, kTileRowsSmall);
        else if (kpl == 2) ET_BTILE(2, kTileRowsSmall);
        else ET_BTILE(4, kTileRowsSmall);
    } else if (rows == kTileRowsLarge) {
        if (kpl == 1) ET_BTILE(1, kTileRowsLarge);
        else if (kpl == 2) ET_BTILE(2, kTileRowsLarge);
        else ET_BTILE(4, kTileRowsLarge);
    } else {
        if (kpl == 2) ET_BTILE(2, kTileRowsHuge);   // (512 rows per pixel need K > 96)
        else ET_BTILE(4, kTileRowsHuge);
    }
#undef ET_BTILE
#undef ET_BTILE_
#undef ET_BLIST
#undef ET_BLIST_
    if (det) {
        if (int e = check_launch("et_epipolar_backward_tiled_det(tiles)")) return e;
        // int64 -> fp32: eight blocks of 256 threads per 64 pixel rows
        const unsigned fblocks = std::min<unsigned>(256u, (vec4_per_pair + 2047u) / 2048u);
        hipLaunchKernelGGL(det_finish_kernel, dim3(fblocks, desc->N), dim3(256), 0, st, dw.acc, dw.quanta,
                           reinterpret_cast<float4 *>(grad_src), vec4_per_pair);
    }
    return check_launch("et_epipolar_backward_tiled");
}
}  // namespace
