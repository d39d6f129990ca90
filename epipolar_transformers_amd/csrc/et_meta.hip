// libepipolar_amd.so: the Meta fusion layer's per-pair GEMMs (C = 256) -- et_meta_pack, et_meta_gemm, et_meta_wgrad.
#include "et_common.h"

namespace {
#include "et_wave_reduce.h"
#include "kernels_residual_gemm.inc"      // the GEMM family these kernels belong to: fragment layout, stage, scale, wgrad stage
#include "kernels_meta.inc"

// a pair's rows over ceil(HW / 2048) blocks: a function of HW alone, so that a pair's grad_w does not depend on the batch around it
int meta_wgrad_blocks_per_pair(long long HW) { return (int)((HW + kMetaWgRowsPerBlock - 1) / kMetaWgRowsPerBlock); }
}  // namespace

extern "C" {

int et_meta_pack(int32_t N, int32_t C, const float *weight, const float *share, int32_t transpose, void *packed, void *stream)
{
    if (C != 256) return fail("et_meta_pack: C = %d (the kernel is written for the 256-channel head)", C);
    if (N <= 0) return fail("et_meta_pack: bad sizes");
    if (!weight || !packed) return fail("et_meta_pack: NULL pointer");
    if (reinterpret_cast<uintptr_t>(packed) & 15) return fail("et_meta_pack: packed buffer must be 16-byte aligned");
    const long long blocks = (long long)N * kRgPackBlocks;
    if (blocks > 0x7fffffffLL) return fail("et_meta_pack: too many pairs");
    hipLaunchKernelGGL(meta_pack_kernel, dim3((unsigned)blocks), dim3(1024), 0, (hipStream_t)stream, weight, share, (int)(transpose != 0),
                       reinterpret_cast<unsigned *>(packed));
    return check_launch("et_meta_pack");
}

int et_meta_gemm(int32_t N, int32_t HW, int32_t C, const float *src, const float *feat, const void *packed, const float *bias,
                 float *x, void *stream)
{
    if (C != 256) return fail("et_meta_gemm: C = %d (the kernel is written for the 256-channel head)", C);
    if (N <= 0 || HW <= 0) return fail("et_meta_gemm: bad sizes");
    if (!src || !packed || !x) return fail("et_meta_gemm: NULL pointer");
    if (reinterpret_cast<uintptr_t>(packed) & 15) return fail("et_meta_gemm: packed buffer must be 16-byte aligned");
    const int tiles_per_pair = (int)(((long long)HW + kRgRows - 1) / kRgRows);
    const long long blocks = (long long)N * tiles_per_pair;
    if (blocks > 0x7fffffffLL) return fail("et_meta_gemm: too many tiles (%lld)", blocks);
    hipStream_t st = (hipStream_t)stream;
    const int dev = current_device();
    if (feat) {
        ET_GRANT_LDS(meta_gemm_kernel<true>, kRgLdsBytes, dev);
        hipLaunchKernelGGL(meta_gemm_kernel<true>, dim3((unsigned)blocks), dim3(256), kRgLdsBytes, st, src, feat,
                           reinterpret_cast<const unsigned *>(packed), bias, x, (int)HW, tiles_per_pair);
    } else {
        ET_GRANT_LDS(meta_gemm_kernel<false>, kRgLdsBytes, dev);
        hipLaunchKernelGGL(meta_gemm_kernel<false>, dim3((unsigned)blocks), dim3(256), kRgLdsBytes, st, src, feat,
                           reinterpret_cast<const unsigned *>(packed), bias, x, (int)HW, tiles_per_pair);
    }
    return check_launch("et_meta_gemm");
}

size_t et_meta_wgrad_workspace_bytes(int32_t N, int32_t HW)
{
    if (N <= 0 || HW <= 0) return 0;
    return (size_t)N * (size_t)meta_wgrad_blocks_per_pair(HW) * (65536 + 256) * sizeof(float);   // (one partial result per block)
}

int et_meta_wgrad(int32_t N, int32_t HW, int32_t C, const float *g, const float *src, float *grad_w, float *grad_b, void *workspace,
                  size_t workspace_bytes, void *stream)
{
    if (C != 256) return fail("et_meta_wgrad: C = %d (the kernel is written for the 256-channel head)", C);
    if (N <= 0 || HW <= 0) return fail("et_meta_wgrad: bad sizes");
    if (!g || !src || !grad_w || !workspace) return fail("et_meta_wgrad: NULL pointer");
    if (workspace_bytes < et_meta_wgrad_workspace_bytes(N, HW))
        return fail("et_meta_wgrad: workspace of %zu bytes is smaller than the %zu required", workspace_bytes,
                    et_meta_wgrad_workspace_bytes(N, HW));
    const int per_pair = meta_wgrad_blocks_per_pair(HW);
    const long long blocks = (long long)N * per_pair, finish = (long long)N * 256 + 1;
    if (blocks > 0x7fffffffLL || finish > 0x7fffffffLL) return fail("et_meta_wgrad: too many pairs (%lld blocks)", blocks);
    // a block's rows: the pair's share rounded up to whole 16-row steps (at most 2048: its byte offsets stay far below 2^31)
    const int rows_per_block = (int)((((long long)HW + per_pair - 1) / per_pair + kWgRows - 1) / kWgRows * kWgRows);
    hipStream_t st = (hipStream_t)stream;
    const int dev = current_device();
    float *pw = reinterpret_cast<float *>(workspace), *pb = pw + (size_t)blocks * 65536;
    ET_GRANT_LDS(meta_wgrad_kernel, kWgbLdsBytes, dev);
    hipLaunchKernelGGL(meta_wgrad_kernel, dim3((unsigned)blocks), dim3(512), kWgbLdsBytes, st, g, src, (int)HW, per_pair, rows_per_block,
                       pw, pb);
    if (int e = check_launch("et_meta_wgrad")) return e;
    hipLaunchKernelGGL(meta_wgrad_finish_kernel, dim3((unsigned)(grad_b ? finish : finish - 1)), dim3(256), 0, st, pw, pb, (int)N, per_pair,
                       grad_w, grad_b);
    return check_launch("et_meta_wgrad(finish)");
}

}  // extern "C"
