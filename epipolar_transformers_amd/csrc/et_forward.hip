// libepipolar_amd.so: the fused forward for any shape (et_epipolar_forward).
#include "et_common.h"

namespace {
#include "kernels_sample_table.inc"
#include "kernels_pixel_phases.inc"
#include "kernels_forward.inc"   // SampleTable, epipolar_fwd_kernel, epipolar_fwd_multi_kernel

template <int CPL, int KPL>
void launch_fwd_k(const FwdParams &p, dim3 grid, size_t lds, hipStream_t st)
{
    // K % 4 == 0 but % 8 != 0 also takes the ragged build (fewer instances)
    if (p.d.K % 8) hipLaunchKernelGGL((epipolar_fwd_kernel<CPL, KPL, true>), grid, dim3(256), lds, st, p);
    else hipLaunchKernelGGL((epipolar_fwd_kernel<CPL, KPL, false>), grid, dim3(256), lds, st, p);
}

template <int CPL>
void launch_fwd(const FwdParams &p, int kpl, dim3 grid, size_t lds, hipStream_t st)
{
    if (kpl == 1) launch_fwd_k<CPL, 1>(p, grid, lds, st);
    else if (kpl == 2) launch_fwd_k<CPL, 2>(p, grid, lds, st);
    else launch_fwd_k<CPL, 4>(p, grid, lds, st);
}
}  // namespace

extern "C" {

int et_epipolar_forward(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                        const float *cam, const float *feat_ref, const float *feat_src, float *out,
                        float *attn, float *corr_pos, const float *res_bias, float *res_base, void *stream)
{
    if (int e = validate(desc)) return e;
    if (!xs || !ys || !steps || !cam || !feat_ref || !feat_src || !out)
        return fail("et_epipolar_forward: NULL pointer");
    if (res_bias && !res_base) return fail("et_epipolar_forward: res_bias given without res_base");
    FwdParams p;
    p.d = *desc;
    p.xs = xs; p.ys = ys; p.steps = steps; p.cam = cam;
    p.fref = feat_ref; p.fsrc = feat_src;
    p.out = out; p.attn = attn; p.corr = corr_pos;
    p.res_bias = res_bias; p.res_base = res_base;
    const int HW = desc->H * desc->W;
    p.blocks_per_pair = (HW + kPixPerBlock - 1) / kPixPerBlock;
    const long long total = (long long)p.blocks_per_pair * desc->N;
    if (total > 0x7fffffffLL) return fail("grid too large");
    p.total_blocks = (int)total;
    const dim3 grid((unsigned)total);
    const int cpl = (desc->C + 255) / 256, kpl = (desc->K + 63) / 64;
    const size_t lds = (attn ? (size_t)desc->K * kPixPerBlock * sizeof(float) : 0) +
                       (size_t)kWavesPerBlock * kpl * kWave * 4 * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    // The tuned kernels (measured on MI355X, profiles/), whatever `variant` holds: for the 256-channel head with K <= 64
    // four pixels per wave in lockstep; otherwise one pixel per wave, batches of 4 samples, <= 96 VGPRs (5 waves/SIMD),
    // waves of a block interleaved over neighbouring pixels
    if (desc->C == 256 && kpl == 1) {   // K > 64: its LDS records cut occupancy (measured 1.8x slower)
        // per-wave LDS: 4 pixels * (64 records of 32 bytes + a 16-byte segment)
        const size_t lds_m = (attn ? (size_t)desc->K * kPixPerBlock * sizeof(float) : 0) +
                             (size_t)kWavesPerBlock * (4 * kWave * 32 + 4 * 16);
        hipLaunchKernelGGL((epipolar_fwd_multi_kernel), grid, dim3(256), lds_m, st, p);
        return check_launch("et_epipolar_forward(multi)");
    }
    if (cpl == 1) launch_fwd<1>(p, kpl, grid, lds, st);
    else launch_fwd<2>(p, kpl, grid, lds, st);
    return check_launch("et_epipolar_forward");
}

}  // extern "C"
