// libepipolar_amd.so: the MFMA tile formulation of the backward (et_epipolar_backward_tiled, _attn, _det and their _ga forms;
// et_epipolar_backward_tiled_ix: the float form with the pairs named by index -- grad_src is then the source pool's gradient).
// Kernels: the ordering (kernels_tile_order.inc, through et_tile_host.h) and the tile kernel (kernels_backward_tile.inc over
// kernels_tile_common.inc, the helpers shared with the forward).
#include <algorithm>
#include "et_common.h"
#include "et_tile_host.h"             // the ordering kernels and the host side of a tile call

namespace {
#include "kernels_backward_tile.inc"  // epipolar_bwd_tile_kernel / _list_kernel
#include "kernels_backward_det.inc"   // the deterministic form: maxima, quantum, int64 -> fp32
}  // namespace

namespace {
// Workspace of the deterministic form: the forward-layout workspace (same header, same sticky error word), then the tail of
// et_tile_layout.h's det_workspace_layout: acc | quanta | partial maxima.
struct DetWorkspace {
    long long *acc;
    float *quanta, *partial;
};
size_t det_extra_bytes(size_t pairs, size_t hw) { return det_workspace_layout(0, pairs, hw).extra_bytes; }
DetWorkspace carve_det_workspace(const TileWorkspace &w, size_t pairs, size_t hw)
{
    const DetWorkspaceLayout l = det_workspace_layout(w.end, pairs, hw);
    DetWorkspace dw;
    dw.acc = reinterpret_cast<long long *>(w.base + l.acc);
    dw.quanta = reinterpret_cast<float *>(w.base + l.quanta);
    dw.partial = reinterpret_cast<float *>(w.base + l.partial);
    return dw;
}
int backward_tiled_impl(bool det, const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                        const float *cam, const float *feat_ref, const float *feat_src, const float *attn,
                        const float *grad_out, const float *grad_attn, float *grad_ref, float *grad_src, void *workspace,
                        size_t workspace_bytes, void *stream, const PairIndex &ix = PairIndex());
}  // namespace

extern "C" {

size_t et_epipolar_backward_tiled_det_workspace_bytes(const EtLayerDesc *desc)
{
    const size_t fwd = et_epipolar_backward_tiled_workspace_bytes(desc);
    if (fwd == 0) return 0;
    return fwd + det_extra_bytes((size_t)desc->N, (size_t)desc->H * desc->W);
}

int et_epipolar_backward_tiled_det_ga(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                      const float *cam, const float *feat_ref, const float *feat_src, const float *attn,
                                      const float *grad_out, const float *grad_attn, float *grad_ref, float *grad_src,
                                      void *workspace, size_t workspace_bytes, void *stream)
{
    return backward_tiled_impl(true, desc, xs, ys, steps, cam, feat_ref, feat_src, attn, grad_out, grad_attn, grad_ref, grad_src,
                               workspace, workspace_bytes, stream);
}

int et_epipolar_backward_tiled_det(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                   const float *cam, const float *feat_ref, const float *feat_src, const float *attn,
                                   const float *grad_out, float *grad_ref, float *grad_src, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    return et_epipolar_backward_tiled_det_ga(desc, xs, ys, steps, cam, feat_ref, feat_src, attn, grad_out, nullptr, grad_ref, grad_src,
                                             workspace, workspace_bytes, stream);
}

int et_debug_host_det_quantum_ga(const EtLayerDesc *desc, float m_ref, float m_src, float m_g, float m_ga, float *q, float *bound)
{
    if (!desc || !q || !bound) return fail("et_debug_host_det_quantum: NULL pointer");
    if (!desc->softmax_enabled) return fail("et_debug_host_det_quantum: no bound with the soft-max off (sim / K is unbounded)");
    if (!(m_ref >= 0.f) || !(m_src >= 0.f) || !(m_g >= 0.f) || !(m_ga >= 0.f))
        return fail("et_debug_host_det_quantum: maxima must be >= 0");
    const DetQuantum r = det_quantum(desc->softmax_scale, m_ref, m_src, m_g, m_ga);
    *q = r.q;
    *bound = r.bound;
    return 0;
}

int et_debug_host_det_quantum(const EtLayerDesc *desc, float m_ref, float m_src, float m_g, float *q, float *bound)
{
    return et_debug_host_det_quantum_ga(desc, m_ref, m_src, m_g, 0.f, q, bound);
}

size_t et_epipolar_backward_tiled_workspace_bytes(const EtLayerDesc *desc)
{
    if (validate(desc) || !tile_eligible(desc)) return 0;
    return et_epipolar_forward_workspace_bytes(desc);
}

int et_epipolar_backward_tiled_ga(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                  const float *cam, const float *feat_ref, const float *feat_src, const float *attn,
                                  const float *grad_out, const float *grad_attn, float *grad_ref, float *grad_src,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    return backward_tiled_impl(false, desc, xs, ys, steps, cam, feat_ref, feat_src, attn, grad_out, grad_attn, grad_ref, grad_src,
                               workspace, workspace_bytes, stream);
}

int et_epipolar_backward_tiled_ix(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                  const float *cam, const float *feat_ref, const float *feat_src, const float *attn,
                                  const float *grad_out, const float *grad_attn, float *grad_ref, float *grad_src,
                                  void *workspace, size_t workspace_bytes, void *stream, const int32_t *ref_index,
                                  const int32_t *src_index, int32_t M_ref, int32_t M_src)
{
    PairIndex ix;
    if (int e = make_pair_index(desc, "et_epipolar_backward_tiled_ix", ref_index, src_index, M_ref, M_src, &ix)) return e;
    return backward_tiled_impl(false, desc, xs, ys, steps, cam, feat_ref, feat_src, attn, grad_out, grad_attn, grad_ref, grad_src,
                               workspace, workspace_bytes, stream, ix);
}

int et_epipolar_backward_tiled(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                               const float *cam, const float *feat_ref, const float *feat_src,
                               const float *grad_out, float *grad_ref, float *grad_src, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    return et_epipolar_backward_tiled_ga(desc, xs, ys, steps, cam, feat_ref, feat_src, nullptr, grad_out, nullptr, grad_ref, grad_src,
                                         workspace, workspace_bytes, stream);
}

int et_epipolar_backward_tiled_attn(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                    const float *cam, const float *feat_ref, const float *feat_src, const float *attn,
                                    const float *grad_out, float *grad_ref, float *grad_src, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    return et_epipolar_backward_tiled_ga(desc, xs, ys, steps, cam, feat_ref, feat_src, attn, grad_out, nullptr, grad_ref, grad_src,
                                         workspace, workspace_bytes, stream);
}

}  // extern "C"

namespace {
// One block per tile: (rows, samples per lane, deterministic form) -> the instance.
template <int KPL, int ROWS>
int launch_bwd_tile_as(const BwdTileParams &tp, bool det, size_t lds, int dev, hipStream_t st)
{
    const unsigned grid = (unsigned)tp.b.total_blocks;
    return det ? launch_tile_kernel<epipolar_bwd_tile_kernel<KPL, ROWS, true>>("epipolar_bwd_tile_kernel", grid, 256, lds, dev, st, tp)
               : launch_tile_kernel<epipolar_bwd_tile_kernel<KPL, ROWS, false>>("epipolar_bwd_tile_kernel", grid, 256, lds, dev, st, tp);
}
int launch_bwd_tile(const BwdTileParams &tp, int rows, int kpl, bool det, int dev, hipStream_t st)
{
    const size_t lds = bwd_tile_lds_bytes(rows, tp.hw_words, kpl);
    if (rows == kTileRowsMerged) return launch_bwd_tile_as<1, kTileRowsMerged>(tp, det, lds, dev, st);
    if (rows == kTileRowsMergedLarge) return launch_bwd_tile_as<1, kTileRowsMergedLarge>(tp, det, lds, dev, st);
    if (rows == kTileRowsSmall)
        return kpl == 1   ? launch_bwd_tile_as<1, kTileRowsSmall>(tp, det, lds, dev, st)
               : kpl == 2 ? launch_bwd_tile_as<2, kTileRowsSmall>(tp, det, lds, dev, st)
                          : launch_bwd_tile_as<4, kTileRowsSmall>(tp, det, lds, dev, st);
    if (rows == kTileRowsLarge)
        return kpl == 1   ? launch_bwd_tile_as<1, kTileRowsLarge>(tp, det, lds, dev, st)
               : kpl == 2 ? launch_bwd_tile_as<2, kTileRowsLarge>(tp, det, lds, dev, st)
                          : launch_bwd_tile_as<4, kTileRowsLarge>(tp, det, lds, dev, st);
    return kpl == 2 ? launch_bwd_tile_as<2, kTileRowsHuge>(tp, det, lds, dev, st)      // (512 rows per pixel need K > 96)
                    : launch_bwd_tile_as<4, kTileRowsHuge>(tp, det, lds, dev, st);
}

// The second launch of a merged call (K <= 64) over its list of deferred tiles: two blocks per compute unit -- what is
// resident at once -- walk the list.
template <int ROWS>
int launch_bwd_tile_list_as(const BwdTileParams &tp, bool det, int dev, hipStream_t st)
{
    const long long total = tp.b.total_blocks, cus = device_cus(dev);
    const unsigned grid = (unsigned)(total < 2 * cus ? total : 2 * cus);
    const size_t lds = bwd_tile_lds_bytes(ROWS, tp.hw_words, 1);
    return det ? launch_tile_kernel<epipolar_bwd_tile_list_kernel<1, ROWS, true>>("epipolar_bwd_tile_list_kernel", grid, 256, lds, dev, st, tp)
               : launch_tile_kernel<epipolar_bwd_tile_list_kernel<1, ROWS, false>>("epipolar_bwd_tile_list_kernel", grid, 256, lds, dev, st, tp);
}

int backward_tiled_impl(bool det, const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                        const float *cam, const float *feat_ref, const float *feat_src, const float *attn,
                        const float *grad_out, const float *grad_attn, float *grad_ref, float *grad_src, void *workspace,
                        size_t workspace_bytes, void *stream, const PairIndex &ix)
{
    const char *bad_args = (!xs || !ys || !steps || !cam || !feat_ref || !feat_src || !grad_out || !grad_ref || !grad_src) ? "NULL pointer" : nullptr;
    TileCall c;
    if (int e = begin_tile_call(desc, "et_epipolar_backward_tiled", bad_args, "et_epipolar_backward",
                                det ? det_extra_bytes : nullptr, workspace, workspace_bytes, &c))
        return e;
    if (det && !desc->softmax_enabled)
        return fail("et_epipolar_backward_tiled_det: needs the soft-max (EPIPOLAR.SOFTMAX_ENABLED False makes the attention sim / K, "
                    "-1e10 / K under the mask: no bound to take the fixed-point quantum from); et_epipolar_backward with a workspace "
                    "is the bit-reproducible form there");
    hipStream_t st = (hipStream_t)stream;
    const int HW = c.HW;
    const TileWorkspace &w = c.w;
    BwdTileParams tp;
    std::memset(&tp, 0, sizeof(tp));
    BwdParams &p = tp.b;
    p.d = *desc;
    set_pair_index(p, ix);
    p.xs = xs; p.ys = ys; p.steps = steps; p.cam = cam;
    p.fref = feat_ref; p.fsrc = feat_src; p.gout = grad_out; p.gattn = grad_attn;
    p.gref = grad_ref; p.gsrc = grad_src;
    p.blocks_per_pair = c.tiles_per_pair;
    p.total_blocks = c.total;
    tp.tiles_per_pair = c.tiles_per_pair;
    tp.hw_words = c.hw_words;
    tp.rows_cap = c.rows_cap;
    tp.attn = attn;
    // (with the per-pair scale estimates of the source maps: the merged kernels run their row-type GEMMs as split-fp16
    //  products; the workspace has the forward's layout.  grad_src is cleared by extra blocks of the ordering kernel: the
    //  tile kernel adds into it)
    tp.perm = w.perm;
    tp.scales = w.scales;
    // deterministic form: the clearing blocks zero the int64 accumulator instead (twice the bytes); grad_src is written whole by
    // det_finish_kernel
    const DetWorkspace dw = carve_det_workspace(w, (size_t)desc->N, (size_t)HW);
    // (an indexed call's grad_src is the source POOL's gradient: M_src maps, every one cleared -- a map no pair names stays 0)
    const size_t clear_maps = ix.src_index ? (size_t)ix.M_src : (size_t)desc->N;
    const size_t clear_vec4 = clear_maps * HW * (desc->C / 4) * (det ? 2 : 1);     // (C == 256)
    // (header = true: the ordering clears the workspace's overflow counter, which the merged launch below counts into)
    if (int e = launch_tile_order(desc, xs, ys, cam, feat_ref, feat_src, w, c.tiles_per_pair, true, w.scales, false,
                                  det ? reinterpret_cast<float4 *>(dw.acc) : reinterpret_cast<float4 *>(grad_src), clear_vec4, st,
                                  "et_epipolar_backward_tiled(order)", ix))
        return e;
    const unsigned vec4_per_pair = (unsigned)HW * (desc->C / 4);
    if (det) {
        // the pair's exact maxima -> its quantum (kernels_backward_det.inc)
        hipLaunchKernelGGL(det_maxima_kernel, dim3(kDetMaxBlocks, desc->N), dim3(256), 0, st, reinterpret_cast<const float4 *>(feat_ref),
                           reinterpret_cast<const float4 *>(feat_src), reinterpret_cast<const float4 *>(grad_out), vec4_per_pair,
                           grad_attn, (unsigned)desc->K * (unsigned)HW, dw.partial);
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
    // merged launches defer the tiles beyond their columns to a second launch of the one-array kernel (unless the caller tests the
    // splitting: ET_VARIANT_TILE_SPLIT)
    const bool defer = merged && !(desc->variant & (ET_VARIANT_TILE_SPLIT | ET_VARIANT_BWD_SPLIT_IN_PLACE));
    if (defer) {
        tp.ovf_count = w.ovf_count;
        tp.ovf_list = w.ovf_list;
    }
    // capacity of the second launch's kernel: a deferred tile beyond it is shared by kDetHardParts blocks there (deterministic form)
    tp.list_cap = tile_rows(desc) == kTileRowsSmall ? kTileRowsMergedLarge : tile_rows_cap(desc);
    if (int e = launch_bwd_tile(tp, rows, kpl, det, dev, st)) return e;
    if (defer) {
        if (int e = check_launch("et_epipolar_backward_tiled(merged)")) return e;
        tp.tile_list = w.ovf_list;
        tp.tile_count = w.ovf_count;
        tp.ovf_list = nullptr;
        tp.ovf_count = nullptr;
        tp.rows_cap = tile_rows_cap(desc);
        int e;
        if (tile_rows(desc) == kTileRowsSmall) {
            // round 6: the deferred tiles of a 64 x 64 map (193 .. ~280 rows) by the MERGED kernel of 288 columns -- one
            // derivation of the samples' slots for both arrays, no half passes (a tile beyond 288 rows is split there);
            // measured against the one-array kernel of 256 rows in profiles/r06_bwd_ab.txt
            tp.rows_cap = kTileRowsMergedLarge;
            e = launch_bwd_tile_list_as<kTileRowsMergedLarge>(tp, det, dev, st);
        } else {
            e = launch_bwd_tile_list_as<kTileRowsLarge>(tp, det, dev, st);
        }
        if (e) return e;
    }
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
