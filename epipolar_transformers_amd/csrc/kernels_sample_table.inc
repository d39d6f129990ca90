// Per-pixel sample table shared by the per-pixel forward (kernels_forward.inc) and backward (kernels_backward.inc)
// kernels.  Included inside the translation unit's anonymous namespace.
// ----------------------------------------------------------------------------
// per-pixel sample table, lanes <-> samples
// ----------------------------------------------------------------------------
// Everything a sample needs inside the channel loop is precomputed here, 64
// samples at a time, so that the loop itself spends one v_readlane + a handful
// of scalar bit tests per sample on bookkeeping:
//   off[r]  byte offset of the source row routed to tap register r (-1: none)
//   w[r]    its bilinear weight (0 for out-of-image taps and for k >= K)
//   need    bit r set when register r does not already hold that row, i.e.
//           the previous sample's tap r was a different row -- or when the tap
//           is absent and the previous one was not: the register is then
//           CLEARED (tap_row_* below), because its weight 0 times a stale row
//           that holds a NaN or an Inf would be NaN, where the reference's zero
//           padding contributes nothing
template <int KPL>
struct SampleTable {
    int off[KPL][4];
    float w[KPL][4];
    int need[KPL];
    float nx[KPL], ny[KPL];
};

template <int KPL>
__device__ __forceinline__ void build_sample_table(const EtLayerDesc &d, const et::Segment &seg,
                                                   const float *__restrict__ steps, int lane, int row_bytes,
                                                   SampleTable<KPL> &t)
{
#pragma unroll
    for (int s = 0; s < KPL; ++s) {
        const int k = s * kWave + lane;
        const bool in = k < d.K;
        const et::SampleSetup su = et::sample_setup(d, seg, in ? steps[k] : 0.f);
        t.nx[s] = su.nx;
        t.ny[s] = su.ny;
        int need = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int off = (in && su.tap[r] >= 0) ? su.tap[r] * row_bytes : -1;
            t.off[s][r] = off;
            t.w[s][r] = in ? su.weight[r] : 0.f;
            int prev = __shfl_up(off, 1);
            if (lane == 0) prev = -1;
            if (s > 0) {
                const int carry = __shfl(t.off[s > 0 ? s - 1 : 0][r], kWave - 1);
                if (lane == 0) prev = carry;
            }
            if (off != prev) need |= 1 << r;
        }
        t.need[s] = need;
    }
}


// Register r of a needed tap: the source row at byte offset `off` (wave-uniform), or zeros for an absent tap (off < 0).
__device__ __forceinline__ float4 tap_row_f4(__amdgpu_buffer_rsrc_t src, int voff, int off)
{
    return off >= 0 ? buf_load_f4(src, voff, off) : f4_zero();
}
__device__ __forceinline__ float tap_row_f1(__amdgpu_buffer_rsrc_t src, int voff, int off)
{
    return off >= 0 ? buf_load_f1(src, voff, off) : 0.f;
}
