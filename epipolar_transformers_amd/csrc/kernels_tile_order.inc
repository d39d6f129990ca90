// Included inside the anonymous namespace of a tile translation unit (et_tile_host.h does it): the ORDERING of a tile call (the shapes
// of the MFMA tile path: et_tile_layout.h) -- the sort key of every reference pixel's epipolar line, then one bitonic sort per
// pair in LDS -> perm (kernels_forward_tile.inc explains the tile formulation itself).
//   tile_keys_kernel    per pixel, whole device: segment and sort key
//   tile_order_kernel   one block per pair: sort -> perm, segments in tile order, base lines, scale estimates
#pragma once

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- ordering ------------------------------------------------------------------------------
// The sort's keys in LDS: one spare slot after every 16 (a thread's 8 keys of a small-stride round are then 17 slots from its
// neighbour's, not 16: the 8-byte reads of a wave fall into different banks).
__device__ __host__ constexpr int order_key_slot(int i) { return i + (i >> 4); }
constexpr size_t tile_order_lds_bytes(int n2) { return (size_t)order_key_slot(n2) * sizeof(unsigned long long); }
// S stages of the bitonic network (strides jj_top, jj_top / 2, ... jj_top >> (S - 1)) of the merge step k in one trip.
// The keys are DOUBLES (an integer below 2^47 each: order_key below), kept as their bit patterns: a compare-exchange is then
// v_min_f64 + v_max_f64 -- two instructions -- where 64-bit integer keys cost a compare and four selects; the kernel is bound by
// exactly this arithmetic (one block per pair: 24 k compare-exchanges per stage on one compute unit).  A descending block sorts
// the negated keys ascending (the sign bit flipped on the way in and out).
__device__ __forceinline__ unsigned long long order_key(unsigned k32, int j)      // (line angle | line offset, pixel < 2^14)
{
    return (unsigned long long)__double_as_longlong((double)(((unsigned long long)k32 << 14) | (unsigned)j));
}
constexpr unsigned long long kOrderPadKey = 0x42E0000000000000ull;               // 2^47 as a double: behind every pixel
__device__ __forceinline__ int order_key_pixel(unsigned long long bits)
{
    return (int)((unsigned long long)__longlong_as_double((long long)bits) & 0x3FFFull);
}
template <int S>
__device__ __forceinline__ void order_sort_round(unsigned long long *s_key, int n2, int k, int jj_top)
{
    constexpr int R = 1 << S;
    const int jlow = jj_top >> (S - 1);
    for (int t = threadIdx.x; t < (n2 >> S); t += blockDim.x) {
        const int base = ((t & ~(jlow - 1)) << S) | (t & (jlow - 1));    // S zero bits at the positions of the strides
        const unsigned long long flip = (base & k) == 0 ? 0ull : 0x8000000000000000ull;   // (r * jlow < k: the same for all R keys)
        double v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = __longlong_as_double((long long)(s_key[order_key_slot(base + r * jlow)] ^ flip));
#pragma unroll
        for (int st = S - 1; st >= 0; --st)
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (!(r & (1 << st))) {
                    const double a = v[r], b = v[r | (1 << st)];
                    double lo, hi;
                    asm("v_min_f64 %0, %1, %2" : "=v"(lo) : "v"(a), "v"(b));
                    asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(a), "v"(b));
                    v[r] = lo;
                    v[r | (1 << st)] = hi;
                }
#pragma unroll
        for (int r = 0; r < R; ++r) s_key[order_key_slot(base + r * jlow)] = (unsigned long long)__double_as_longlong(v[r]) ^ flip;
    }
    __syncthreads();
}

// The ordering runs as TWO kernels: the per-pixel part (segment, sort key) over the whole device, then one block per pair
// for the part that needs a pair's keys together.  As one kernel (rounds 1-4) a pair's 4096 segments, atan2f / sincosf keys
// and, after the sort, the segments again were all computed by ONE compute unit: ~6000 VALU instructions per wave x 16 waves,
// 50 us of a 0.93 ms forward (profiles/r04_*kernel_stats.csv), 180-210 us at 96 x 96 / 128 x 128.
//   keys[n * 2 * perm_stride + j], j < HW : the sort key of pixel j (the region of pair n's ordered segments: consumed by
//                                           block n of tile_order_kernel before it writes them)
//   segs_pix[n * HW + j]                  : its epipolar segment
__global__ __launch_bounds__(256) void tile_keys_kernel(const EtLayerDesc d, const float *__restrict__ xs,
                                                        const float *__restrict__ ys, const float *__restrict__ cam_all,
                                                        int perm_stride, unsigned long long *__restrict__ keys,
                                                        float4 *__restrict__ segs_pix, int *__restrict__ zero_word)
{
    const int HW = d.H * d.W;
    const int blocks_per_pair = (HW + (int)blockDim.x - 1) / (int)blockDim.x;
    const int n = blockIdx.x / blocks_per_pair, j = (blockIdx.x - n * blocks_per_pair) * blockDim.x + threadIdx.x;
    // the workspace header's counter words of both directions (et_tile_layout.h); the STICKY error word is never cleared here
    if (zero_word && blockIdx.x == 0 && threadIdx.x < kTileHdrClearEnd && threadIdx.x != kTileHdrErr) zero_word[threadIdx.x] = 0;
    if (j >= HW) return;
    const float *cam = cam_all + (size_t)n * ET_CAM_STRIDE;
    const float cx = 0.5f * (d.xmin + d.xmax), cy = 0.5f * (d.ymin + d.ymax);
    const float rmax = 0.5f * sqrtf((d.xmax - d.xmin) * (d.xmax - d.xmin) + (d.ymax - d.ymin) * (d.ymax - d.ymin)) + 1.f;
    const float kPi = 3.14159265358979f;
    // Every epipolar line of the pair passes through the epipole e2, so a line is determined by its direction, and the
    // directions towards the image form a fan around the direction from e2 to the image centre.  Angles are compared
    // modulo pi: measured from a fixed axis the fan can straddle 0 = pi, and the sorted sequence then jumps from one
    // end of the fan to the other in the MIDDLE of the list -- one tile per pair got lines from both ends (twice the rows;
    // its taps fit no common band: round 4's column masks sent it to the overflow list).  Measured from the fan's own
    // axis the jump sits at the ends of the list, where it belongs.
    float th0 = atan2f(cy - cam[25], cx - cam[24]);
    if (!(fabsf(th0) <= 4.f)) th0 = 0.f;                 // (epipole at infinity / not finite: any origin will do)
    const int h = j / d.W, w = j - h * d.W;
    const et::Segment seg = et::epipolar_segment(d, cam, xs[w], ys[h]);
    unsigned k32 = 0xFFFFFFFFu;  // pixels without a segment go last
    if (seg.vx != 0.f || seg.vy != 0.f) {
        float th = atan2f(seg.vy, seg.vx);
        if (th < 0.f) th += kPi;
        if (th >= kPi) th -= kPi;
        float sn, cs;
        sincosf(th, &sn, &cs);
        const float rho = (seg.sy - cy) * cs - (seg.sx - cx) * sn;  // signed offset from the image centre
        float tk = th - th0 + 0.5f * kPi;                       // the fan's axis at pi / 2
        tk -= kPi * floorf(tk * (1.f / kPi));
        const int tb = min(16383, max(0, (int)(tk * (16384.f / kPi))));
        const int rq = min(65535, max(0, (int)((rho / rmax * 0.5f + 0.5f) * 65535.f)));
        k32 = ((unsigned)tb << 16) | (unsigned)rq;
    }
    keys[(size_t)n * 2 * perm_stride + j] = order_key(k32, j);
    segs_pix[(size_t)n * HW + j] = make_float4(seg.sx, seg.sy, seg.vx, seg.vy);
}

__global__ __launch_bounds__(1024) void tile_order_kernel(const EtLayerDesc d, int n2, int perm_stride,
                                                          const unsigned long long *__restrict__ keys,
                                                          const float4 *__restrict__ segs_pix, int *__restrict__ perm,
                                                          const float *__restrict__ fref = nullptr,
                                                          const float *__restrict__ fsrc = nullptr,
                                                          float *__restrict__ scales = nullptr,
                                                          float4 *__restrict__ segs = nullptr,
                                                          float4 *__restrict__ band = nullptr,
                                                          float4 *__restrict__ clear = nullptr, size_t clear_vec4 = 0,
                                                          const int *__restrict__ ref_index = nullptr,
                                                          const int *__restrict__ src_index = nullptr, int M_ref = 0, int M_src = 0)
{
    extern __shared__ unsigned long long s_key[];
    // Blocks beyond the pairs (the backward's launch): clear `clear` (grad_src, which the tile kernel adds into) BESIDE the
    // sort -- the sort keeps N compute units busy with LDS latency, the clearing is HBM stores: one after the other they
    // cost their sum (hipMemsetAsync + this kernel), together the longer of the two.
    if (blockIdx.x >= (unsigned)d.N) {
        const size_t nblk = gridDim.x - d.N, first = (size_t)(blockIdx.x - d.N) * blockDim.x + threadIdx.x;
        for (size_t i = first; i < clear_vec4; i += nblk * blockDim.x) clear[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int n = blockIdx.x;
    const int HW = d.H * d.W;
    // Power-of-two scales for the split-fp16 GEMMs of the warp-specialised forward (C == 256): an ESTIMATE of each
    // map's largest magnitude from 64 whole pixel rows spread over the map, placed at 2^10 -- fp16 then has a factor
    // 32 to 64 of headroom above it, and the kernel checks every value it converts (a tile that would overflow is
    // redone in exact fp32).  scales[n] = { s_ref, 1 / s_ref, s_src, 1 / s_src }.  (The loads go out first: their
    // latency passes behind the sort.)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float m[2] = {0.f, 0.f};
    if (scales) {
        const int pstep = max(1, HW / 64);
        for (int which = 0; which < 2; ++which) {
            // (pair n's maps inside the pools: pair_map, et_common.h)
            const int nm = which ? pair_map(src_index, n, M_src) : pair_map(ref_index, n, M_ref);
            const float4 *map = reinterpret_cast<const float4 *>((which ? fsrc : fref) + (size_t)nm * HW * d.C);
            for (int k = wave; k < 64; k += 16) {
                const int pix = min(k * pstep, HW - 1);
                const float4 v = map[(size_t)pix * (d.C >> 2) + (lane % (d.C >> 2))];
                // (a NaN or an Inf says nothing about the scale of the rest of the map: it counts as 0 here, and the tile that
                //  holds it is redone in exact fp32 by the guards of the kernels that convert it)
                auto mag = [](float x) { const float a = fabsf(x); return a <= kLargestFinite ? a : 0.f; };
                m[which] = fmaxf(m[which], fmaxf(fmaxf(mag(v.x), mag(v.y)), fmaxf(mag(v.z), mag(v.w))));
            }
        }
    }
    for (int j = threadIdx.x; j < n2; j += blockDim.x)
        s_key[order_key_slot(j)] = (j < HW) ? keys[(size_t)n * 2 * perm_stride + j] : kOrderPadKey;
    __syncthreads();
    // Bitonic sort, up to three stages (strides jj, jj / 2, jj / 4) per trip through LDS: a thread takes the 8 keys that
    // differ in those three index bits, runs the stages in registers and puts them back -- 30 trips (and block barriers)
    // instead of 78 for a 64 x 64 map, a third of the LDS traffic (one block per pair: the kernel is bound by the LDS
    // pipe and the barrier latency of a single CU).  Same comparisons, same result as one stage per pass.
    for (int k = 2; k <= n2; k <<= 1) {
        int jj = k >> 1;
        while (jj > 0) {
            if (jj >= 4) {
                order_sort_round<3>(s_key, n2, k, jj);
                jj >>= 3;
            } else if (jj == 2) {
                order_sort_round<2>(s_key, n2, k, jj);
                jj = 0;
            } else {
                order_sort_round<1>(s_key, n2, k, jj);
                jj = 0;
            }
        }
    }
    const float4 *pair_segs = segs_pix + (size_t)n * HW;
    for (int j = threadIdx.x; j < perm_stride; j += blockDim.x) {
        const int pix = (j < HW) ? order_key_pixel(s_key[order_key_slot(j)]) : -1;
        perm[(size_t)n * perm_stride + j] = pix;
        // the segments again, in tile order: the warp-specialised forward reads them instead of recomputing
        if (segs) segs[(size_t)n * perm_stride + j] = pix >= 0 ? pair_segs[pix] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // The tile's base line (warp-specialised forward), in tap space, as minor = a + b * major along the axis the tile's
    // lines mostly run: the kernel keeps the tile's row set as one 16-bit mask per column u of the major axis, bit i <->
    // minor coordinate floor(a + b u) - 1 + i, so the base line has to lie BELOW every line of the tile in every column.
    // The lines of a pair form a pencil through the epipole and the tile's pixels are sorted by angle, so at any column the
    // tile's lines lie between its first and its last (valid) pixel's; the base line is the chord of the lower envelope
    // min(first, last) between the two ends of the map -- the envelope is concave, the chord never above it.  (Rounds 2-4 took
    // the first pixel's line itself: right for an epipole far outside the map -- the ring rig: the lines of a tile do not
    // cross inside the map and the first is the lowest everywhere -- but with the epipole INSIDE or at the edge of the map the
    // lines cross there, the later ones lie below the first on one side, and three tiles in four went to the overflow list;
    // tests/test_gpu_rigs.py.)  Pixels without a segment sort last: a tile whose first pixel has none touches nothing.
    if (band) {
        auto line_of = [&](const float4 &v, bool force, bool xm_in, float &a, float &b, bool &xm) -> bool {
            et::Segment sg;
            sg.sx = v.x; sg.sy = v.y; sg.vx = v.z; sg.vy = v.w;
            float nx0, ny0, nx1, ny1;
            et::sample_location<false>(d, sg, 0.f, et::Pow2Recips(), nx0, ny0);
            et::sample_location<false>(d, sg, 1.f, et::Pow2Recips(), nx1, ny1);
            const float x0 = et::unnormalize(nx0, d.W, d.align_corners), y0 = et::unnormalize(ny0, d.H, d.align_corners);
            const float dx = et::unnormalize(nx1, d.W, d.align_corners) - x0;
            const float dy = et::unnormalize(ny1, d.H, d.align_corners) - y0;
            xm = force ? xm_in : fabsf(dx) >= fabsf(dy);
            a = b = 0.f;
            if (xm) {
                if (dx != 0.f) b = dy / dx;
                else if (force) return false;
                a = y0 - b * x0;
            } else {
                if (dy == 0.f) return false;
                b = dx / dy;
                a = x0 - b * y0;
            }
            return fabsf(a) < 1e6f && fabsf(b) <= 4.f;
        };
        for (int t = threadIdx.x; t < perm_stride / kTilePix; t += blockDim.x) {
            const int j = t * kTilePix;
            const int pix = (j < HW) ? order_key_pixel(s_key[order_key_slot(j)]) : -1;
            float a = 0.f, b = 0.f, xmaj = 1.f;
            if (pix >= 0) {
                const float4 v = pair_segs[pix];
                bool xm = true;
                if ((v.z != 0.f || v.w != 0.f) && line_of(v, false, true, a, b, xm)) {
                    xmaj = xm ? 1.f : 0.f;
                    // the tile's last pixel with a segment
                    float4 vl = v;
                    for (int jj = min(j + kTilePix, HW) - 1; jj > j; --jj) {
                        const float4 c = pair_segs[order_key_pixel(s_key[order_key_slot(jj)])];
                        if (c.z != 0.f || c.w != 0.f) {
                            vl = c;
                            break;
                        }
                    }
                    float a2, b2;
                    bool xm2;
                    if (line_of(vl, true, xm, a2, b2, xm2)) {
                        // columns -1 .. umax (the taps of a sample reach one column beyond the map on either side)
                        const float ulo = -1.f, uhi = (float)(xm ? d.W : d.H);
                        const float m0 = fminf(a + b * ulo, a2 + b2 * ulo), m1 = fminf(a + b * uhi, a2 + b2 * uhi);
                        b = (m1 - m0) / (uhi - ulo);
                        a = m0 - b * ulo;
                    }
                    if (!(fabsf(a) < 1e6f)) a = 0.f, b = 0.f;   // (never with a finite segment; keeps the int conversions defined)
                } else {
                    a = 0.f, b = 0.f;
                }
            }
            band[(size_t)n * (perm_stride / kTilePix) + t] = make_float4(a, b, xmaj, 0.f);
        }
    }
    if (scales) {
        __syncthreads();
        float *s_red = reinterpret_cast<float *>(s_key);
        for (int which = 0; which < 2; ++which) {
            for (int o = 32; o >= 1; o >>= 1) m[which] = fmaxf(m[which], __shfl_xor(m[which], o));
            if (lane == 0) s_red[which * 16 + wave] = m[which];
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            float mx = 0.f;
            for (int w = 0; w < 16; ++w) mx = fmaxf(mx, s_red[threadIdx.x * 16 + w]);
            int e = 0;
            float sc = 1.f;
            if (mx > 0.f && mx < 3e38f) {
                frexpf(mx, &e);                               // mx = f * 2^e, f in [0.5, 1)
                e = min(60, max(-60, 11 - e));                // mx * 2^(11 - e) in [2^10, 2^11)
                sc = ldexpf(1.f, e);
            }
            scales[n * 4 + threadIdx.x * 2] = sc;
            scales[n * 4 + threadIdx.x * 2 + 1] = 1.f / sc;
        }
    }
}
