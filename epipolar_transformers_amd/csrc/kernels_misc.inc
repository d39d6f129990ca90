// Part of epipolar_kernels.hip (one translation unit, one anonymous namespace): sample_locs, residual epilogue and layout kernels.
// Included from epipolar_kernels.hip after the shared device helpers; not a stand-alone header.
// ----------------------------------------------------------------------------
// sample_locs (debug / VIS.EPIPOLAR_LINE / parity gate on the geometry)
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_locs_kernel(const EtLayerDesc d, const float *xs, const float *ys,
                                                           const float *steps, const float *cam, float *locs)
{
    const int HW = d.H * d.W;
    const size_t total = (size_t)d.N * HW;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int n = (int)(i / HW);
        const int pix = (int)(i - (size_t)n * HW);
        const int h = pix / d.W, w = pix - h * d.W;
        const et::Segment seg = et::epipolar_segment(d, cam + (size_t)n * ET_CAM_STRIDE, xs[w], ys[h]);
        for (int k = 0; k < d.K; ++k) {
            const et::SampleSetup su = et::sample_setup(d, seg, steps[k]);
            float2 *o = reinterpret_cast<float2 *>(locs) + ((size_t)k * d.N + n) * HW + pix;
            *o = make_float2(su.nx, su.ny);
        }
    }
}

// ----------------------------------------------------------------------------
// residual epilogue: x = feat + out + (y*scale + shift)    (HBM-bound stream)
// ----------------------------------------------------------------------------
template <bool HAS_Y>
__global__ __launch_bounds__(256) void residual_epilogue_kernel(size_t nvec_total, int nvec_c, const float4 *feat,
                                                                 const float4 *out, const float4 *y,
                                                                 const float4 *scale, const float4 *shift,
                                                                 float4 *finalout, float4 *x)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec_total;
         i += (size_t)gridDim.x * blockDim.x) {
        const float4 o = out[i];
        float4 fo = o;
        if constexpr (HAS_Y) {
            const int c = (int)(i % (size_t)nvec_c);
            const float4 yy = y[i], sc = scale[c], sh = shift[c];
            // bn(z(out)) + out  (epipolar.py:250-253): affine first, then the residual add
            fo.x = fmaf(yy.x, sc.x, sh.x) + o.x;
            fo.y = fmaf(yy.y, sc.y, sh.y) + o.y;
            fo.z = fmaf(yy.z, sc.z, sh.z) + o.z;
            fo.w = fmaf(yy.w, sc.w, sh.w) + o.w;
        }
        if (finalout) finalout[i] = fo;
        if (x) {
            const float4 f = feat[i];
            x[i] = make_float4(fo.x + f.x, fo.y + f.y, fo.z + f.z, fo.w + f.w);  // resnet.py:388
        }
    }
}

// ----------------------------------------------------------------------------
// NCHW <-> NHWC (per image: [C][HW] <-> [HW][C] transpose through LDS)
// ----------------------------------------------------------------------------
constexpr int kTile = 64;
// src is [rows][cols] row-major, dst is [cols][rows]; batch stride rows*cols
__global__ __launch_bounds__(256) void transpose_kernel(int rows, int cols, const float *src, float *dst)
{
    __shared__ float tile[kTile][kTile + 1];
    const size_t img = (size_t)blockIdx.z * rows * cols;
    const int c0 = blockIdx.x * kTile, r0 = blockIdx.y * kTile;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < kTile; i += 4) {
        const int r = r0 + i, c = c0 + tx;
        if (r < rows && c < cols) tile[i][tx] = src[img + (size_t)r * cols + c];
    }
    __syncthreads();
    for (int i = ty; i < kTile; i += 4) {
        const int c = c0 + i, r = r0 + tx;
        if (r < rows && c < cols) dst[img + (size_t)c * rows + r] = tile[tx][i];
    }
}


// ----------------------------------------------------------------------------
// soft-argmax peak finder: find_tensor_peak_batch (modeling/backbones/basic_batch.py:17-63), which the reference
// runs once per sample in a Python loop (resnet.py:424-430, ~15 tiny ATen launches each).  One block per
// (sample, joint) heat map:
//   1. score, index = max over H*W (first maximum, as torch.max);  index_w = index % W,  index_h = index / W
//      (TRUE division under torch >= 1.5, integer division in the torch the authors used: `legacy_floor`)
//   2. a (2 r + 1)^2 window around it, resampled bilinearly exactly as F.affine_grid + F.grid_sample
//      (align_corners = False, zero padding) do for the box [index -+ radius] normalised with -1 + 2 x / (L - 1)
//   3. values <= threshold dropped, centre of mass with the ramp arange(-radius, radius, radius / r) + index,
//      then pix2coord (x * downsample + downsample / 2 - 0.5).
// The arithmetic of one map is et_peaks.h's (shared with the host hook); here: the block's reduction layout.
// ----------------------------------------------------------------------------
// arg-max of one map by the block (NaN above every value, then the value, then the lowest index: et_peaks.h); every thread returns
// the raw index (et_peaks::kNoCandidate for a map without a candidate) and the score
__device__ __forceinline__ int peaks_block_argmax(const float *__restrict__ hm, int HW, float *s_val, int *s_idx, float &score)
{
    constexpr int kThreads = et_peaks::kThreads;
    const int tid = threadIdx.x;
    float best = -__builtin_huge_valf();
    int bidx = et_peaks::kNoCandidate;
    for (int i = tid; i < HW; i += kThreads) {
        const float v = hm[i];
        if (et_peaks::takes_over(v, best)) {
            best = v;
            bidx = i;
        }
    }
    s_val[tid] = best;
    s_idx[tid] = bidx;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const float v = s_val[tid + s];
            const int i = s_idx[tid + s];
            if (et_peaks::outranks(v, i, s_val[tid], s_idx[tid])) {
                s_val[tid] = v;
                s_idx[tid] = i;
            }
        }
        __syncthreads();
    }
    score = s_val[0];
    return s_idx[0];
}

// the three sums of the resampled window by the block: per-wave totals in s_acc[k][wave], valid after the barrier at the end;
// the block's totals are (s_acc[k][0] + s_acc[k][1]) + (s_acc[k][2] + s_acc[k][3])
__device__ __forceinline__ void peaks_block_sums(const float *__restrict__ hm, int H, int W, const et_peaks::Window &win, float (*s_acc)[4])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float sum = 0.f, sx = 0.f, sy = 0.f;
    for (int e = tid; e < win.side * win.side; e += et_peaks::kThreads) {
        float rx, ry;
        const float v = et_peaks::window_sample(hm, H, W, win, e, rx, ry);
        sum += v;
        sx += v * rx;
        sy += v * ry;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        sum += __shfl_xor(sum, o);
        sx += __shfl_xor(sx, o);
        sy += __shfl_xor(sy, o);
    }
    if (lane == 0) {
        s_acc[0][wave] = sum;
        s_acc[1][wave] = sx;
        s_acc[2][wave] = sy;
    }
    __syncthreads();
}

__global__ __launch_bounds__(et_peaks::kThreads) void heatmap_peaks_kernel(const float *__restrict__ heat, int H, int W, float radius,
                                                                            float downsample, float threshold, int legacy_floor,
                                                                            float *__restrict__ locs, float *__restrict__ scores)
{
    constexpr int kThreads = et_peaks::kThreads;
    __shared__ float s_val[kThreads];
    __shared__ int s_idx[kThreads];
    __shared__ float s_acc[3][4];
    const float *hm = heat + (size_t)blockIdx.x * H * W;
    // ---- 1. arg-max ----
    float score;
    const int index = peaks_block_argmax(hm, H * W, s_val, s_idx, score);
    // ---- 2. / 3. the resampled window ----
    const et_peaks::Window win = et_peaks::make_window(et_peaks::resolve_index(index), H, W, radius, threshold, legacy_floor);
    peaks_block_sums(hm, H, W, win, s_acc);
    if (threadIdx.x == 0) {
        float x, y;
        et_peaks::finish((s_acc[0][0] + s_acc[0][1]) + (s_acc[0][2] + s_acc[0][3]), (s_acc[1][0] + s_acc[1][1]) + (s_acc[1][2] + s_acc[1][3]),
                         (s_acc[2][0] + s_acc[2][1]) + (s_acc[2][2] + s_acc[2][3]), win, downsample, x, y);
        locs[(size_t)blockIdx.x * 2] = x;
        locs[(size_t)blockIdx.x * 2 + 1] = y;
        scores[blockIdx.x] = score;
    }
}

// ----------------------------------------------------------------------------
// The peak finder's backward: d(locs), d(scores) -> d(heat map), one block per map, the forward's index, window and sums
// recomputed by the forward's own block routines.  Gather form (et_peaks.h, cell_grad): every cell of the map is written by exactly
// one thread -- 0 outside the window's clipped footprint, inside it the sum over the elements that tap the cell in ascending
// element order, plus d(score) on the arg-max cell -- so there are no atomics and the bits do not depend on the batch.
// grad_locs / grad_scores may be NULL (not both): without d(locs) the window is not visited at all.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(et_peaks::kThreads) void heatmap_peaks_bwd_kernel(const float *__restrict__ heat, int H, int W, float radius,
                                                                                float downsample, float threshold, int legacy_floor,
                                                                                const float *__restrict__ grad_locs,
                                                                                const float *__restrict__ grad_scores,
                                                                                float *__restrict__ grad_heat)
{
    constexpr int kThreads = et_peaks::kThreads;
    __shared__ float s_val[kThreads];
    __shared__ int s_idx[kThreads];
    __shared__ float s_acc[3][4];
    const int tid = threadIdx.x;
    const float *hm = heat + (size_t)blockIdx.x * H * W;
    float *grad = grad_heat + (size_t)blockIdx.x * H * W;
    const int HW = H * W;
    float score;
    const int index = et_peaks::resolve_index(peaks_block_argmax(hm, HW, s_val, s_idx, score));
    const bool has_score = grad_scores != nullptr;
    const float g_score = has_score ? grad_scores[blockIdx.x] : 0.f;
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1;                           // the footprint; empty without d(locs)
    if (grad_locs) {
        const et_peaks::Window win = et_peaks::make_window(index, H, W, radius, threshold, legacy_floor);
        peaks_block_sums(hm, H, W, win, s_acc);
        const et_peaks::GradCoef coef = et_peaks::make_coef(
            (s_acc[0][0] + s_acc[0][1]) + (s_acc[0][2] + s_acc[0][3]), (s_acc[1][0] + s_acc[1][1]) + (s_acc[1][2] + s_acc[1][3]),
            (s_acc[2][0] + s_acc[2][1]) + (s_acc[2][2] + s_acc[2][3]), grad_locs[(size_t)blockIdx.x * 2], grad_locs[(size_t)blockIdx.x * 2 + 1],
            downsample);
        et_peaks::footprint(win.t00, win.t02, win.side, W, x0, x1);
        et_peaks::footprint(win.t11, win.t12, win.side, H, y0, y1);
        // the footprint's cells, one per thread and trip: x0 <= x <= x1 <= W - 1, y0 <= y <= y1 <= H - 1
        const int fw = x1 - x0 + 1, fh = y1 - y0 + 1;
        if (fw > 0 && fh > 0)
            for (int c = tid; c < fw * fh; c += kThreads) {
                const int y = y0 + c / fw, x = x0 + c % fw;
                const int i = y * W + x;
                const float g = et_peaks::cell_grad(hm, H, W, win, coef, y, x);
                grad[i] = (has_score && i == index) ? g + g_score : g;
            }
    }
    // every other cell (an empty footprint, x1 < x0 or y1 < y0, holds none)
    for (int i = tid; i < HW; i += kThreads) {
        const int y = i / W, x = i - y * W;
        if (x >= x0 && x <= x1 && y >= y0 && y <= y1) continue;
        grad[i] = (has_score && i == index) ? 0.f + g_score : 0.f;
    }
}

// Diagnostic (bench.py's `extra.atomic_probe`): the float-atomic pattern of the tiled backward's d(feat_src) accumulation
// (kernels_backward_tile.inc: one buffer_atomic_fadd_f32 per lane, a wave-instruction = two 128-byte runs in two pixel rows of a
// (rows, 256) fp32 array), on pseudo-random rows, nothing else in the kernel: the L2 atomic request rate of THIS box.
__global__ __launch_bounds__(256) void atomic_probe_kernel(float *__restrict__ dst, unsigned rows, int iters)
{
    const int lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    const __amdgpu_buffer_rsrc_t buf = make_rsrc(dst, rows * 1024u);
    unsigned state = wave * 2654435761u + 12345u;
    for (int i = 0; i < iters; ++i) {
        state = state * 1664525u + 1013904223u;
        const unsigned row = ((state >> 8) + (unsigned)lh * 4u) % rows;
        const int off = (int)(row * 1024u + (unsigned)((i & 7) * 32 + li) * 4u);
        __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(1.0f, buf, off, 0, 0);
    }
}
