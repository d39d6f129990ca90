/*
 * epipolar_amd.h -- C ABI of the MI355X-native Epipolar Transformer hot path.
 *
 * Drop-in boundary: these entry points are what a
 * binding of the reference's `Epipolar` operator
 * (modeling/layers/epipolar.py:11-269, called from
 * modeling/backbones/resnet.py:377-388) calls instead of the per-sample Python
 * loop.  Plain pointers and sizes only; no torch types.  Every pointer is a
 * DEVICE pointer unless its comment says "host".  The library allocates
 * nothing, never synchronises the device and enqueues all work on `stream`
 * (a hipStream_t passed as void*; NULL = the default stream), so it is
 * re-entrant under nn.DataParallel-style threading (SURVEY.md 8b "Threading").
 *
 * Return value: 0 on success, non-zero on error; et_last_error() then returns
 * a thread-local description.  No error is ever turned into NaNs silently.
 *
 * Feature maps are channels-last: (N, H, W, C) float32, C contiguous, C % 4 == 0.
 * (The reference hands NCHW tensors; et_nchw_to_nhwc / et_nhwc_to_nchw convert,
 * and a torch tensor in torch.channels_last memory format already IS this
 * layout.)
 */
#ifndef EPIPOLAR_AMD_H_
#define EPIPOLAR_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ET_ABI_VERSION 14
/* The *_ga entry points (gradient through the returned attention) were added without touching an existing signature, so the
 * version stays; a caller tests for them with this macro. */
#define ET_HAS_ATTN_GRAD 1
/* The *_ix entry points (pairs named by index into a stack of maps, below et_epipolar_forward_fused) were added the same way. */
#define ET_HAS_PAIR_INDEX 1
/* The et_meta_* entry points (the Meta fusion layer's per-pair GEMMs, below et_z_wgrad) were added the same way. */
#define ET_HAS_META_FUSION 1

/* Static description of one layer call: the cfg keys the reference reads in
 * Epipolar.__init__ (epipolar.py:12-54) and at call time (epipolar.py:303-311,
 * 409-414; vision/multiview.py:25-57,154-163). */
typedef struct EtLayerDesc {
    int32_t N;                 /* (reference view, source view) pairs in the batch          */
    int32_t C;                 /* cfg.KEYPOINT.NFEATS (channels), multiple of 4             */
    int32_t H, W;              /* cfg.KEYPOINT.HEATMAP_SIZE                                 */
    int32_t K;                 /* cfg.EPIPOLAR.SAMPLESIZE, 2 <= K <= 256                    */
    float xmin, ymin;          /* epipolar.py:46-47 (first pixel centre, image coords)      */
    float xmax, ymax;          /* epipolar.py:48-49 (last pixel centre)                     */
    float eps;                 /* epipolar.py:20  (0.001)                                   */
    float downsample;          /* cfg.BACKBONE.DOWNSAMPLE            (multiview.py:159-163) */
    float image_resize;        /* cfg.DATASETS.IMAGE_RESIZE          (epipolar.py:411)      */
    float predict_resize;      /* cfg.DATASETS.PREDICT_RESIZE        (epipolar.py:411)      */
    int32_t correct_normalize; /* cfg.EPIPOLAR.USE_CORRECT_NORMALIZE (multiview.py:29,45)   */
    int32_t align_corners;     /* F.grid_sample semantics (epipolar.py:199): 0 = torch>=1.3 default */
    float softmax_scale;       /* cfg.EPIPOLAR.SOFTMAXSCALE          (epipolar.py:306)      */
    int32_t softmax_enabled;   /* cfg.EPIPOLAR.SOFTMAX_ENABLED       (epipolar.py:303-311)  */
    int32_t src_grad_mask;     /* backward only, cfg.EPIPOLAR.OTHER_GRAD (epipolar.py:141-153):
                                  bit0 = gradient reaches feat_src through the similarity ('other1'),
                                  bit1 = through the sampled values ('other2'); reference default 3 */
    int32_t variant;           /* kernel variant bits, 0 = library default (testing/tuning) */
} EtLayerDesc;

/* Floats per pair in the `cam` array consumed below:
 *   [0..11]  P1inv  4x3 row-major : pinverse(P_ref)            epipolar.py:336
 *   [12..23] P2     3x4 row-major : P_src                      epipolar.py:340
 *   [24..26] e2     epipole P2 @ centre(P_ref), divided by z   epipolar.py:344-348
 * This O(N) algebra stays on the host in float32 torch. */
#define ET_CAM_STRIDE 27

/* Variant bits (EtLayerDesc.variant).  0 is the library default; the bits below select another kernel of a family
 * (testing, tuning, reproducibility).  The per-pixel kernels (et_epipolar_forward / _backward) have one tuned
 * instance per shape class -- four pixels per wave for C == 256 and K <= 64, else one pixel per wave with
 * reductions per 4 samples -- and take it whatever else the word holds. */
/* (bits 1, 2, 4, 8, 16, 32, 256, 512, 1024, 2048 were the per-pixel kernels' round-1 tuning switches -- reduction form, tap cache, pixel order, batch size, register budgets, pixels per wave: measured in round 1 (profiles/r01_variant_sweep_last.json), the winners are the kernels above; the bits stay accepted and now select nothing) */
/* (bits 64 and 128 were roofline ablations that computed wrong results by construction: reserved, and rejected) */
#define ET_VARIANT_BWD_ATOMIC 4096 /* backward: float-atomic scatter even when a workspace is given      */
#define ET_VARIANT_BWD_UNSORTED 8192 /* backward gather: sum in arrival order (faster, not bit-reproducible) */
#define ET_VARIANT_NO_TILE 16384  /* host wrappers: do not route C == 256 calls to et_epipolar_forward_tiled */
#define ET_VARIANT_TILE_SPLIT 32768 /* et_epipolar_forward_tiled, testing: 64-row tiles, so that tiles overflow and split */
#define ET_VARIANT_TILE_CLASSIC 65536 /* et_epipolar_forward_tiled: the one-block-per-tile kernel (split-fp16 GEMMs, exact-fp32 redo of overflowing tiles) instead of the warp-specialised persistent one */
/* (bit 131072 was ET_VARIANT_WS_V2, a second-generation persistent kernel on pre-split source planes: measured slower in rounds 3-4 (profiles/r03_ws2_vs_v1_timing.txt), retired in round 5; the bit is reserved and now selects nothing) */
#define ET_VARIANT_WS_SETPRIO 262144 /* warp-specialised kernel (first generation), tuning: s_setprio 1 on the matrix waves */
#define ET_VARIANT_WS_BAND 1048576 /* et_epipolar_forward_tiled / _fused, testing: the persistent kernel's instance for maps above 64 x 64 (288-row arrays, slot table over the tile's band) also for smaller maps */
#define ET_VARIANT_TILE_EXACT 524288 /* et_epipolar_forward_tiled, one-block-per-tile kernel: both GEMMs in exact fp32 (v_mfma_f32_32x32x2_f32) instead of split-fp16 products */
#define ET_VARIANT_BWD_SPLIT_IN_PLACE 2097152 /* et_epipolar_backward_tiled: split EVERY tile beyond the merged kernel's columns in place (rounds 2-4) instead of deferring the hard ones (those whose group chain would outlast the launch) to a second launch of the one-array kernel: equal to 3.5 % faster on the ring rig, 1.5-2 x slower on geometries with many such tiles */
#define ET_VARIANT_BWD_DETERMINISTIC 4194304 /* host wrappers / the Python binding: prefer the deterministic tile backward (et_epipolar_backward_tiled_det) where the tile path applies; the kernels never look at it */

int et_abi_version(void);
const char *et_last_error(void);

/* grid2sample_locs (epipolar.py:323-418).
 *   xs[W], ys[H] : pixel-centre grid in image coordinates       epipolar.py:35-38
 *   steps[K]     : torch.range(0, 1, 1/(K-1))                   epipolar.py:54
 *   cam[N*27]    : see ET_CAM_STRIDE
 *   sample_locs  : (K, N, H, W, 2) normalised coordinates, as the reference returns them */
int et_sample_locs(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                   const float *cam, float *sample_locs, void *stream);

/* Non-finite values -- a NaN, +Inf or -Inf in feat_ref / feat_src / the maps of the general entry points, in grad_out or in a
 * prior -- go through the attention operator as they go through the reference on the CPU (pinned to outputs of the reference
 * itself: tests/golden/nonfinite/, tests/test_gpu_nonfinite.py).  The rule, for every entry point that says "non-finite: the
 * rule" below:
 *   never lost    where the reference's result is non-finite, so is ours.  The per-pixel kernels and the general kernels also
 *                 return the same kind (NaN, +Inf, -Inf), forward and -- the per-pixel backward forms -- gradients; the tile
 *                 kernels guarantee the finiteness only (a split-fp16 product turns Inf into NaN);
 *   confined      where the reference's result is finite, ours is finite and as accurate as on finite inputs: a value spreads to
 *                 the pixels whose bilinear taps include it (an in-image tap of weight 0 counts, as in F.grid_sample; a tap
 *                 outside the image contributes nothing, whatever a register still holds) and no further.  The
 *                 tile kernels multiply a whole tile with its whole row set, so a tile that meets a non-finite logit is
 *                 processed pixel by pixel (the splitting path of an overflowing row set): slower, same result;
 *   arg-max       corr_pos is torch.argmax's sample: a NaN ranks above every value and the first one wins -- a pixel whose
 *                 weights are all NaN returns sample 0 --, then the value, then the lowest index.  Never an index outside
 *                 the samples;
 *   pair          a pair with finite inputs returns the same bits whatever another pair of the batch holds; no bit of the
 *                 sticky error word is set.
 * The tiled backward forms (et_epipolar_backward_tiled*, et_epipolar_backward_tiled_det*) keep "never lost" (finiteness) and
 * "pair", not "confined to the pixel": their GEMMs contract over a tile's 32 pixels and its whole row set, and their operands are
 * scaled by the tile's largest magnitude.  A non-finite value of feat_ref / feat_src / grad_out may therefore make non-finite, or
 * (an Inf, through the scale) inaccurate, grad_ref of every pixel of the tiles that hold or tap it and grad_src of every source
 * row those tiles tap -- entries of its OWN PAIR only.  Use the gather form for a step whose gradients may be non-finite and must
 * stay confined.
 *
 * Fused hot loop of Epipolar.forward in the headline mode (MERGE late,
 * ATTENTION avg, SIMILARITY dot): epipolar.py:178-247 + epipolar_similarity
 * (272-321) + de_normalize (multiview.py:39-57), never materialising
 * sample_locs or the K x C x H x W sampled tensor.
 *   feat_ref, feat_src : (N,H,W,C)
 *   out                : (N,H,W,C)  sum_k attn_k * sampled_k           (epipolar.py:243)
 *   attn      nullable : (N,K,H,W)  the reference's `depth` return     (epipolar.py:263)
 *   corr_pos  nullable : (N,H,W,2)  de-normalised arg-max sample       (epipolar.py:237-242)
 *   res_base  nullable : (N,H,W,C)  feat_ref + res_bias[c] (res_bias nullable = 0): the additive
 *                        term of the residual fusion, written while the reference row is in
 *                        registers.  With eval-mode BN folded into z, `ret + feat` (resnet.py:388,
 *                        epipolar.py:250-253) is then ONE GEMM:  x = res_base + (I + W') out.
 * Non-finite: the rule (above), kinds included. */
int et_epipolar_forward(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                        const float *cam, const float *feat_ref, const float *feat_src, float *out,
                        float *attn, float *corr_pos, const float *res_bias, float *res_base,
                        void *stream);

/* The same operator in its MFMA tile formulation (C == 256 head): reference pixels are ordered by
 * their epipolar line, 32 neighbouring lines form a tile, and the channel-long work of the tile runs
 * as two GEMMs on the matrix cores against the union of the source rows the tile touches (each source
 * row is fetched per tile, not per pixel).  For K <= 64 on maps up to 96 x 96 with the soft-max on
 * (BASELINE configs[0..3]) the call is one persistent block per compute unit whose waves are
 * specialised: matrix waves run the two GEMMs of consecutive tiles back to back as split-fp16 MFMAs
 * with fp32 accumulation (~22 significant bits per product; the fp32 operands are scaled by powers of
 * two, split into fp16 hi + lo at the point of use and every converted value is range-checked), vector
 * waves do the geometry / row-set / soft-max work of the neighbouring tiles meanwhile (two instances:
 * 256-row arrays up to 64 x 64 maps; 288-row arrays and a slot table over the tile's band above).
 * Other shapes (maps above 96 x 96, K > 64) run one block per tile with the same split-fp16 GEMMs.  A tile with a value beyond
 * fp16's range is redone in exact fp32, and so is every call with the soft-max off
 * (EPIPOLAR.SOFTMAX_ENABLED False: the "attention" sim / K is unbounded) and every call with
 * ET_VARIANT_TILE_EXACT.  Same arguments and results as et_epipolar_forward (rounding differs at the
 * 1e-6 level: the sums are re-associated), plus
 *   workspace : device scratch of at least et_epipolar_forward_workspace_bytes(desc) bytes.  The base
 *               need NOT be 256-byte aligned (16 bytes is what the tests exercise and what a caller may
 *               rely on): the library rounds the base up to the next 256-byte boundary
 *               itself (the header and every offset below are counted from THERE -- a caller that reads
 *               the words does the same) and et_epipolar_forward_workspace_bytes includes the 256 bytes
 *               this can cost; nothing is written outside [base, base + workspace_bytes).
 *               ZERO-INITIALISED ONCE by the caller when it is allocated, of which the kernels rely on
 *               ONE word only: word 1 of the header (the sticky error word) must not hold stale bits.
 *               Header words 0 and 2..9 (the counters of one call) are cleared by every call before it
 *               uses them, everything behind the header is written by a call before it reads it, and
 *               header words 10..63 are touched by nothing (reserved: keep them zero).  One workspace
 *               may therefore serve calls of any shape, variant and direction (et_epipolar_forward_tiled,
 *               _fused, et_epipolar_backward_tiled(_attn)) in any order, as long as they are ordered on
 *               one stream and it is large enough for each; concurrent streams need one each
 *               (tests/test_gpu_workspace_contracts.py pins all of this).  It starts with a
 *               64-word header -- word 0 the overflow-tile count, word 1 a STICKY int32 error word
 *               (et_epipolar_forward_workspace_error_offset(desc) = 4 bytes in, whatever the shape, so
 *               that a workspace reused across shapes keeps ONE error word: the kernels only ever OR
 *               bits into it; bit 0 / bit 1: a wave of a persistent kernel gave up waiting at an
 *               internal barrier -- the results of that call are invalid.  Such a barrier exists in
 *               front of the third GEMM of et_epipolar_forward_fused (bit 1; bit 0 belonged to a kernel
 *               retired in round 5); the default kernel's waves never wait on each other
 *               outside the hardware barrier.  The library never synchronises, so the caller reads the word when
 *               it synchronises anyway: ops.check_tile_errors in the Python binding) -- followed by
 *               the per-pair pixel order, the overflow-tile list, per-pair scales, the epipolar
 *               segments in tile order, one base line per tile and the segments by pixel, and
 *                 - one int32 of statistics per tile ( U | groups << 16 : size of the tile's
 *                   source-row set, number of groups it was split into) starting
 *                   et_epipolar_forward_workspace_stats_offset(desc) bytes in, in tile order
 *                   (pair-major), readable by the caller after the call.
 * et_epipolar_forward_workspace_bytes returns 0 when the tile path does not apply to `desc`
 * (then et_epipolar_forward_tiled fails and et_epipolar_forward is the path to call).
 * Non-finite: the rule (head of this section), finiteness only.  The persistent kernel's fp16 guard lists a tile whose first GEMM
 * is not finite, the one-block-per-tile kernel redoes it in exact fp32 and, on a non-finite logit, pixel by pixel; the per-pair
 * scale estimate skips NaN / Inf, so the rest of that pair's map keeps its precision. */
size_t et_epipolar_forward_workspace_bytes(const EtLayerDesc *desc);
size_t et_epipolar_forward_workspace_stats_offset(const EtLayerDesc *desc);
size_t et_epipolar_forward_workspace_error_offset(const EtLayerDesc *desc);
int et_epipolar_forward_tiled(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                              const float *cam, const float *feat_ref, const float *feat_src, float *out,
                              float *attn, float *corr_pos, const float *res_bias, float *res_base,
                              void *workspace, size_t workspace_bytes, void *stream);

/* The operator's parameterised / pooled / prior branches as one kernel.
 * The reference applies its optional 1x1 convolutions to the maps BEFORE sampling (epipolar.py:138-153), so these
 * branches are the headline operator over three tensors instead of two:
 *   q        : (N,H,W,c_sim)  feat1 or theta(feat1)                          (epipolar.py:144-145)
 *   map_sim  : (N,H,W,c_sim)  feat2 or phi(feat2): sampled for the similarity (epipolar.py:138-143, :199)
 *   map_val  : (N,H,W,c_val)  feat2 or g(feat2):   sampled for the output     (epipolar.py:147-153, :210)
 *   prior    nullable : (N,K',H,W)  EPIPOLAR.PRIOR: the (camera, other camera) prior of every pair, added to the masked
 *                        similarity (epipolar.py:300-301) or, with ET_GENERAL_PRIOR_MUL, multiplied onto the soft-max
 *                        output (epipolar.py:308-309)
 *   flags    : ET_GENERAL_POOLING -- EPIPOLAR.POOLING (epipolar.py:200-202, 211-213): per-channel maximum of samples
 *              k and k + K/2 of both sampled maps; K' = K / 2 similarities per pixel (K even).  Otherwise K' = K.
 *   out      : (N,H,W,c_val)  sum_k' attn_k' * (pooled) sample_k' of map_val   (epipolar.py:243)
 *   attn     nullable : (N,K',H,W);  corr_pos nullable : (N,H,W,2), the location of sample arg-max_k' attn of the
 *              unpooled list (epipolar.py:237-242).
 * ATTENTION avg | max, SIMILARITY dot | cos | prior; FIND_CORR rgb is q = ref1, map_sim = ref2 (3 channels); soft-max on or off
 * as `desc` says; desc->C is ignored
 * (c_sim <= 512, c_val <= 4096, any positive value).  Nothing of size K x C x H x W is materialised.
 * Non-finite: the rule (head of this section), kinds included: POOLING takes torch.max's maximum (a NaN wins over every value,
 * of two NaNs the first), the arg-max of ATTENTION max and of corr_pos is torch.argmax's. */
#define ET_GENERAL_POOLING 1
#define ET_GENERAL_PRIOR_MUL 2
#define ET_GENERAL_COSINE 4          /* SIMILARITY cos: F.cosine_similarity(q, sample) (epipolar.py:290-293), then mask / prior / soft-max as for dot */
#define ET_GENERAL_ATTENTION_MAX 8   /* ATTENTION max (epipolar.py:282-286, 222-235): attn = the raw cosine similarity, out = the arg-max sample of map_val; no prior */
#define ET_GENERAL_SIM_PRIOR 16      /* SIMILARITY prior (epipolar.py:288-289) and an externally supplied `depth` (:217-218): attn = the given (N,K',H,W) weights as they are (no similarity, mask or soft-max; q / map_sim are not read); excludes PRIOR_MUL / COSINE; with ATTENTION_MAX the output is the arg-max sample of those weights */
int et_epipolar_forward_general(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                const float *cam, const float *q, const float *map_sim, const float *map_val,
                                const float *prior, int c_sim, int c_val, int flags, float *out, float *attn,
                                float *corr_pos, void *stream);

/* Backward of et_epipolar_forward_general w.r.t. its three tensors and the prior, for every branch (same `flags` as
 * the forward; ABI 12 -- ABI 11 covered the dot-product branches without a prior only):  grad_out (N,H,W,c_val)  ->
 * grad_q (N,H,W,c_sim), written;  grad_map_sim (N,H,W,c_sim) and grad_map_val (N,H,W,c_val), each nullable (OTHER_GRAD
 * without 'other1' / 'other2', epipolar.py:138-150) and ACCUMULATED with float atomics -- the caller zeroes them first;
 * sums over pixels arrive in any order, so the result is reproducible to rounding only;  grad_prior nullable:
 * (N,K',H,W), written -- the gradient of every pair's prior rows (the caller sums the pairs of one camera pair into the
 * (camera, other camera) table, epipolar.py:73-80).  The similarities and the soft-max are recomputed from the inputs;
 * the gradient of POOLING's per-channel maximum goes to the sample that won (the first on a tie, as torch.max); cosine
 * similarity is differentiated as torch does (through the unclamped norms); ATTENTION max passes grad_out to the first
 * arg-max sample of map_val only (grad_q = 0, nothing into map_sim); SIMILARITY prior: grad_prior_k' = grad_out . V_k'.
 * `corr_pos` carries no gradient (an arg-max location).
 *
 * et_epipolar_backward_general_ga: the same with grad_attn = d loss / d attn, nullable, (N,K',H,W) -- the returned attention is an
 * ordinary differentiable output in the reference (epipolar.py:245, 263).  With e_k' = grad_out . V_k' and ga_k' = grad_attn:
 *   ATTENTION avg, every similarity and prior: e_k' + ga_k' takes the place of e_k' everywhere -- the soft-max receives it (times
 *     prior_k' under PRIOR_MUL, where grad_prior_k' = softmax_k' (e_k' + ga_k')); soft-max off: d sim_k' = (e_k' + ga_k') / K'; zero
 *     under the `sim == 0` mask either way; SIMILARITY prior: grad_prior_k' = e_k' + ga_k';
 *   ATTENTION max: the attention is the raw cosine, so d sim_k' = ga_k' (no mask) goes through the cosine derivative into grad_q
 *     and grad_map_sim (both zero without grad_attn); with SIM_PRIOR beside it grad_prior_k' = ga_k'.  The value gradient is unchanged.
 * grad_out stays required (a loss on the attention alone passes zeros); grad_attn NULL = et_epipolar_backward_general, bit for bit.
 * Non-finite: the rule (head of this section); the map gradients arrive through float atomics, pairs with finite inputs agree to
 * rounding.  Where nothing flows through the similarity (every mode but the cosine) q does not enter grad_q: a NaN in q stays out. */
int et_epipolar_backward_general(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                 const float *cam, const float *q, const float *map_sim, const float *map_val,
                                 const float *prior, const float *grad_out, int c_sim, int c_val, int flags, float *grad_q,
                                 float *grad_map_sim, float *grad_map_val, float *grad_prior, void *stream);
int et_epipolar_backward_general_ga(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                    const float *cam, const float *q, const float *map_sim, const float *map_val,
                                    const float *prior, const float *grad_out, const float *grad_attn, int c_sim, int c_val,
                                    int flags, float *grad_q, float *grad_map_sim, float *grad_map_val, float *grad_prior,
                                    void *stream);

/* Backward of et_epipolar_forward w.r.t. both feature maps (sample locations
 * carry no gradient, epipolar.py:178-183).  Everything is recomputed from the
 * inputs; nothing saved by the forward is needed.
 *   grad_out  : (N,H,W,C)
 *   grad_ref  : (N,H,W,C) written
 *   grad_src  : (N,H,W,C) written
 *   workspace : device scratch of at least et_epipolar_backward_workspace_bytes(desc)
 *               bytes, or NULL.  With a workspace d(feat_src) is computed in gather
 *               form (per-(pixel,row) coefficients -> counting sort by source row ->
 *               one wave per source pixel sums alpha*g_p + beta*f_p in ascending p):
 *               no float atomics, bit-reproducible.  With NULL (or variant bit
 *               ET_VARIANT_BWD_ATOMIC) grad_src is zero-filled and accumulated with
 *               float atomics (bilinear-transpose scatter, run-to-run rounding noise).
 * Non-finite: the rule (head of this section), both forms, kinds included. */
size_t et_epipolar_backward_workspace_bytes(const EtLayerDesc *desc);
int et_epipolar_backward(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                         const float *cam, const float *feat_ref, const float *feat_src,
                         const float *grad_out, float *grad_ref, float *grad_src, void *workspace,
                         size_t workspace_bytes, void *stream);

/* Gradient through the returned attention (ET_HAS_ATTN_GRAD): every backward of the headline operator in a second form that
 * also takes grad_attn = d loss / d attn, nullable, (N,K,H,W) float32 -- `attn` is an ordinary differentiable output in the
 * reference (epipolar.py:245, 263).  With a = attn, e_k = grad_out . S_k and ga = grad_attn, the gradient reaching a_k through
 * out = sum_k a_k S_k and through the attention itself is e_k + ga_k:
 *     soft-max on :  d sim_k = softmax_scale a_k ((e_k + ga_k) - sum_j a_j (e_j + ga_j)),   0 under the `sim == 0` mask
 *     soft-max off:  d sim_k = (e_k + ga_k) / K   (a = sim / K),                             0 under the mask
 * and everything behind d sim_k (grad_ref, the similarity part of grad_src) is as without it; the value part of grad_src,
 * a_k grad_out into the samples, does not involve ga.  grad_out stays required: a loss on the attention alone passes zeros.
 * With grad_attn NULL each is the entry point without _ga, bit for bit (those call these).  Workspaces: as for the forms
 * without _ga, same sizes and layouts. */
int et_epipolar_backward_ga(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                            const float *cam, const float *feat_ref, const float *feat_src,
                            const float *grad_out, const float *grad_attn, float *grad_ref, float *grad_src, void *workspace,
                            size_t workspace_bytes, void *stream);

/* The backward in the same MFMA tile formulation (C == 256, K <= 256): per 32-pixel tile the similarity and
 * g.S_k come from two GEMMs against the tile's source rows, d(feat_ref) from a third, and d(feat_src) from
 * two pixel-contracting GEMMs whose U x C results are added into grad_src with float atomics (grad_src is
 * zero-filled first).  ~50x fewer atomics than the scatter form and ~3x faster than the gather form, but the
 * cross-tile summation order is not fixed: reproducible to rounding only.  Same arguments as
 * et_epipolar_backward; workspace of et_epipolar_backward_tiled_workspace_bytes(desc) bytes (0: the tile path
 * does not apply to `desc`, call et_epipolar_backward). */
size_t et_epipolar_backward_tiled_workspace_bytes(const EtLayerDesc *desc);
int et_epipolar_backward_tiled(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                               const float *cam, const float *feat_ref, const float *feat_src,
                               const float *grad_out, float *grad_ref, float *grad_src, void *workspace,
                               size_t workspace_bytes, void *stream);

/* The same with the attention the forward returned ((N,K,H,W), what autograd saves in the reference): the soft-max
 * is not recomputed, i.e. one of the five GEMMs, its resampling and the soft-max forward are skipped.  attn may be
 * NULL (= et_epipolar_backward_tiled). */
int et_epipolar_backward_tiled_attn(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                    const float *cam, const float *feat_ref, const float *feat_src,
                                    const float *attn, const float *grad_out, float *grad_ref, float *grad_src,
                                    void *workspace, size_t workspace_bytes, void *stream);
/* ... and with grad_attn (see et_epipolar_backward_ga); attn and grad_attn each nullable.  One limit with BOTH given and the
 * soft-max on: the kernel knows the all-masked pixel (zero reference row) from its attention alone, every a_k = 1 / K, and gives
 * it d sim = 0.  An UNMASKED pixel whose logits all agree to the last bit (a constant source region, vanishing features) has
 * the same attention, and its true d sim_k = softmax_scale / K (ga_k - mean_j ga_j) is dropped as well; without grad_attn that
 * term is zero anyway.  With attn NULL the kernel recomputes the logits, sees the mask itself and keeps the term. */
int et_epipolar_backward_tiled_ga(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                  const float *cam, const float *feat_ref, const float *feat_src, const float *attn,
                                  const float *grad_out, const float *grad_attn, float *grad_ref, float *grad_src,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* The tiled backward, BIT-REPRODUCIBLE (ABI 14): the same tiles and GEMMs, but the U x C results are not added into grad_src with
 * float atomics.  Each is scaled by 1 / q -- q one power of two per pair, derived from a BOUND on a contribution,
 *     32 (2 |softmax_scale| 256 M_g M_src M_ref + M_g) (1 + 1/64),   M_* = max |.| of the pair's grad_out / feat_src / feat_ref,
 *     q = 2^(floor(log2 bound) + 1 + 14 - 62), at least 2^-100
 * -- rounded to int64 and added with 64-bit integer atomics into an accumulator in the workspace: integer sums do not depend on
 * the order.  A last pass writes grad_src = (float)acc * q (one rounding per element).  How a tile is grouped is a pure function
 * of the tile (every tile beyond the merged kernel's columns goes to the second launch; no counters, no block indices), so the
 * gradients of a pair are the same bits run after run, on any stream, alone or anywhere in a batch.  grad_ref is per pixel.
 *   attn      : nullable, as et_epipolar_backward_tiled_attn
 *   workspace : et_epipolar_backward_tiled_det_workspace_bytes(desc) bytes (0 exactly where the tiled form's is 0): the
 *               forward-layout workspace -- same 64-word header, same rules (zero-initialised once; any base alignment; may be
 *               shared with the other tile calls on one stream) -- followed by the int64 accumulator (N H W 256 x 8 bytes), the
 *               pairs' quanta and maxima, all written before they are read.  Sticky error word, bit 2 (value 4): a FINITE
 *               contribution of 2^48 quanta or more was met and NOT added -- impossible under the bound; the results of that
 *               call are invalid.
 * Non-finite: the tiled rule (head of this section).  The maxima skip NaN / Inf, so the pair's finite values keep their quantum; a
 * contribution that is NaN or infinite marks its accumulator element, which comes out NaN -- no error bit, same bits run after run.
 * Fails (et_last_error) with the soft-max off (the "attention" sim / K has no bound: et_epipolar_backward with a workspace is the
 * bit-reproducible form there), on a workspace that is too small, and where the tile path does not apply.
 * et_debug_host_det_quantum: HOST test hook, no GPU -- q and the bound for given maxima (desc: softmax_scale).
 * et_epipolar_backward_tiled_det_ga: with grad_attn (see et_epipolar_backward_ga).  |e_k + ga_k| <= 256 M_g M_src + M_ga, M_ga =
 * max |grad_attn| of the pair (taken in the pass that takes the other maxima; it lives in the maxima region: the workspace size
 * does not change), so the bound is
 *     32 (2 |softmax_scale| (256 M_g M_src + M_ga) M_ref + M_g) (1 + 1/64)
 * -- the bits above for M_ga = 0, and a proper quantum for a loss on the attention alone (M_g = 0, M_ga > 0).
 * et_debug_host_det_quantum_ga: the host hook with m_ga. */
size_t et_epipolar_backward_tiled_det_workspace_bytes(const EtLayerDesc *desc);
int et_epipolar_backward_tiled_det(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                   const float *cam, const float *feat_ref, const float *feat_src,
                                   const float *attn, const float *grad_out, float *grad_ref, float *grad_src,
                                   void *workspace, size_t workspace_bytes, void *stream);
int et_debug_host_det_quantum(const EtLayerDesc *desc, float m_ref, float m_src, float m_g, float *q, float *bound);
int et_epipolar_backward_tiled_det_ga(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                      const float *cam, const float *feat_ref, const float *feat_src, const float *attn,
                                      const float *grad_out, const float *grad_attn, float *grad_ref, float *grad_src,
                                      void *workspace, size_t workspace_bytes, void *stream);
int et_debug_host_det_quantum_ga(const EtLayerDesc *desc, float m_ref, float m_src, float m_g, float m_ga, float *q, float *bound);

/* Residual fusion epilogue: x = feat + out + (y * scale[c] + shift[c])
 *   (epipolar.py:250-253 with ZRESIDUAL, then resnet.py:388 `ret + feat`),
 * y = z(out) is the 1x1-conv (GEMM) result, scale/shift = batch-norm affine
 * folded with its (running or batch) statistics.  y/scale/shift may be NULL
 * for the un-parameterised layer (x = feat + out).  finalout nullable:
 * receives out + y*scale + shift (what Epipolar.forward returns).  All (N,H,W,C).
 * Non-finite: element by element, as IEEE arithmetic has it. */
int et_residual_epilogue(int64_t num_pixels, int32_t C, const float *feat, const float *out,
                         const float *y, const float *scale, const float *shift, float *finalout,
                         float *x, void *stream);

/* The same fusion in eval mode as ONE GEMM for the 256-channel head (replaces the reference's conv1x1 + BN +
 * two adds, epipolar.py:250-253, resnet.py:388):
 *     x[m, :] = [feat[m, :] +] bias + out[m, :] . Wf^T,   Wf = diag(s) W [+ I],  bias = s b + beta - mean s,
 * s = gamma / sqrt(var + eps)  (the caller folds; Wf is (256 out, 256 in) row-major fp32).  The products run as
 * split-fp16 MFMAs with fp32 accumulation (fp32-level error; every row of `out` is scaled by its own power of
 * two).  et_residual_gemm_pack lays Wf out for the kernel into `packed` (et_residual_gemm_packed_bytes() bytes,
 * 16-byte aligned; repack when the weights change).  feat nullable (then x = bias + out . Wf^T, what
 * Epipolar.forward returns).  out / feat / x: (num_pixels, 256) fp32, x may not alias out or feat.
 * Non-finite: a row of `out` that holds a NaN / Inf gives a non-finite row of x; every other row -- those of its 32-row block
 * included -- is computed as on finite inputs. */
size_t et_residual_gemm_packed_bytes(void);
int et_residual_gemm_pack(const float *wf, void *packed, void *stream);
int et_residual_gemm(int64_t num_pixels, int32_t C, const float *out, const float *feat, const void *packed,
                     const float *bias, float *x, void *stream);

/* First pass of the layer's TRAINING-mode epilogue (ABI 12): the z branch with BATCH statistics -- bn(z(out)) with
 * training = True (epipolar.py:250-251, modeling/layers/BN.py:59-82) -- for the 256-channel head:
 *   y    : (num_pixels, 256) written: out . Wz^T + z_bias, the batch norm's input (what autograd keeps for the backward)
 *   mean : (256) written: per-channel mean of y over all num_pixels rows
 *   var  : (256) written: per-channel BIASED variance of y (what the batch norm normalises with; the running estimate
 *          takes var * n / (n - 1))
 * `packed_wz` = et_residual_gemm_pack of the raw z weight (256 out x 256 in).  Per 64-row block the kernel keeps a mean and
 * a centred sum of squares per channel (workspace: et_z_batch_stats_workspace_bytes(num_pixels) bytes, no initialisation
 * needed), merged pairwise in double precision -- no sum-of-squares cancellation, no float atomics, bit-reproducible.
 * The second pass is et_residual_gemm with the statistics folded into the weight:
 *   Wf = diag(gamma / sqrt(var + eps)) Wz [+ I],  bias = (z_bias - mean) gamma / sqrt(var + eps) + beta. */
size_t et_z_batch_stats_workspace_bytes(int64_t num_pixels);
int et_z_batch_stats(int64_t num_pixels, int32_t C, const float *out, const void *packed_wz, const float *z_bias, float *y,
                     float *mean, float *var, void *workspace, size_t workspace_bytes, void *stream);

/* Backward of that epilogue, x = bn(z(out)) [+ out] (+ feat) with batch statistics, w.r.t. `out` and the batch norm's affine
 * parameters (ABI 12), from g = d loss / d x and what et_z_batch_stats left (y, mean, invstd = 1 / sqrt(var + eps)):
 *   grad_gamma, grad_beta : (256) written (per-block sums merged in double, no atomics)
 *   grad_y   : (num_pixels, 256) written: the batch norm's input gradient
 *              gamma invstd (g - mean_rows(g) - yhat mean_rows(g yhat)),  yhat = (y - mean) invstd;
 *              d Wz = grad_y^T out and d bz = sum_rows grad_y are left to the caller (library GEMM / reduction)
 *   grad_out : (num_pixels, 256) written: grad_y . Wz, + g when `zresidual` (EPIPOLAR.ZRESIDUAL, epipolar.py:253)
 * `packed_wzt` = et_residual_gemm_pack of the TRANSPOSED z weight.  d feat = g needs no kernel.
 * workspace: et_z_backward_workspace_bytes(num_pixels) bytes, no initialisation needed. */
size_t et_z_backward_workspace_bytes(int64_t num_pixels);
int et_z_backward(int64_t num_pixels, int32_t C, const float *g, const float *y, const float *mean, const float *invstd,
                  const float *gamma, const void *packed_wzt, int32_t zresidual, float *grad_out, float *grad_y, float *grad_gamma,
                  float *grad_beta, void *workspace, size_t workspace_bytes, void *stream);

/* The weight gradient that closes et_z_backward (ABI 12): grad_w (256 out x 256 in) = grad_y^T . out and grad_b (256) =
 * sum_rows grad_y over the num_pixels rows -- a GEMM contracted over the rows on the matrix cores (each fp32 value as three bf16
 * terms, six cross terms per product, fp32 accumulation: no scale, no range limit; rounds 5-6: exact fp32 MFMAs),
 * one block per compute unit, per-block partial results in `workspace` (et_z_wgrad_workspace_bytes bytes, no initialisation
 * needed) summed in a fixed order: no float atomics, bit-reproducible. */
size_t et_z_wgrad_workspace_bytes(int64_t num_pixels);
int et_z_wgrad(int64_t num_pixels, int32_t C, const float *grad_y, const float *out, float *grad_w, float *grad_b, void *workspace,
               size_t workspace_bytes, void *stream);

/* The Meta fusion layer (ET_HAS_META_FUSION; modeling/layers/meta.py:27-50 and the hourglass caller's `ret + feat`,
 * ProHG.py:219-220,239) for the 256-channel head: every (reference, source) pair n applies a 256 x 256 weight of ITS OWN to its
 * source map,
 *     x[n, m, :] = [feat[n, m, :] +] [bias +] src[n, m, :] . W_n^T,      W_n = weight[n] + share,
 * the reference's loop of N conv2d calls + shared 1x1 convolution + two adds as ONE pass over the maps.  Rows are channels-last:
 * src / feat / x / g are (N, HW, 256) fp32 contiguous, weight / grad_w (N, 256 out, 256 in), share (256, 256).
 *   et_meta_pack  : `weight[n] + share` (share nullable: weight[n] alone), or its TRANSPOSE when `transpose` != 0, split and laid
 *                   out as et_residual_gemm_pack lays Wf out -- pair n at byte n * et_residual_gemm_packed_bytes() of `packed`
 *                   (16-byte aligned), under a power-of-two scale from the largest magnitude of THAT pair's sum.
 *   et_meta_gemm  : the product above on the split-fp16 MFMA scheme of et_residual_gemm (fp32-level error, every row of `src`
 *                   under its own scale), B read from pair n's pack.  Tiles of 64 rows PER PAIR: ceil(HW / 64) tiles each, none
 *                   spans two pairs, the rows of a pair's last tile at or beyond HW are neither loaded nor stored.  feat, bias
 *                   nullable.  With the transposed packs and neither: d src[n] = g[n] . W_n.  x may not alias src or feat.
 *   et_meta_wgrad : grad_w[n] = g[n]^T . src[n] per pair and grad_b (256, nullable) = the sum of g over ALL N HW rows: the
 *                   three-term bf16 MFMA form of et_z_wgrad, a pair's rows split over ceil(HW / 2048) blocks (a number that depends
 *                   on HW alone), partial results in `workspace` (et_meta_wgrad_workspace_bytes(N, HW) bytes, no initialisation
 *                   needed) summed in a fixed order.  d share = sum_n grad_w[n] is left to the caller.
 * No kernel uses atomics: the same inputs give the same bits, and pair n's rows of x / d src / grad_w are the same bits whether
 * the pair is computed alone or inside any batch.  Non-finite: as et_residual_gemm (a non-finite row of src gives a non-finite
 * row of x, every other row is computed as on finite inputs); a non-finite weight is packed as et_residual_gemm_pack packs one and
 * reaches the rows of its own pair only. */
int et_meta_pack(int32_t N, int32_t C, const float *weight, const float *share, int32_t transpose, void *packed, void *stream);
int et_meta_gemm(int32_t N, int32_t HW, int32_t C, const float *src, const float *feat, const void *packed, const float *bias,
                 float *x, void *stream);
size_t et_meta_wgrad_workspace_bytes(int32_t N, int32_t HW);
int et_meta_wgrad(int32_t N, int32_t HW, int32_t C, const float *g, const float *src, float *grad_w, float *grad_b, void *workspace,
                  size_t workspace_bytes, void *stream);

/* The whole eval-mode layer as ONE data kernel (ABI 11): the sampling + attention of et_epipolar_forward_tiled with
 *     x = feat_ref + bias + out . Wf^T
 * -- `bn(z(out)) + out` (epipolar.py:250-253) and the backbone's `ret + feat` (resnet.py:388) with the eval-mode BN
 * folded into z, i.e. what et_residual_gemm computes from `out` in a second pass -- as a third GEMM of the persistent
 * kernel, on the tile's 32 `out` rows while they are still on chip: `out` is neither written nor re-read (1.07 GB less
 * traffic and one launch less per forward at Config 2).  Applies where the warp-specialised kernel does (C == 256, maps
 * up to 96 x 96, K <= 64, soft-max on, no ET_VARIANT_TILE_CLASSIC); otherwise the call fails and
 * et_epipolar_forward_tiled + et_residual_gemm is the path.
 *   packed_w    : Wf laid out by et_residual_gemm_pack;   bias : (256)
 *   x           : (N,H,W,256)                              attn / corr_pos : as et_epipolar_forward, nullable
 *   out_scratch : (N,H,W,256), required: the rows of tiles the persistent kernel hands to its overflow list (a row set
 *                 beyond its arrays, a source value beyond fp16's range) are produced there by the one-block-per-tile
 *                 kernel and their x rows by a small follow-up kernel; with want_out != 0 every row of `out` is written.
 *   workspace   : as et_epipolar_forward_tiled (same size, same sticky error word).
 * Non-finite: the rule (head of this section), finiteness only; the tile that meets the value goes to the overflow follow-up. */
int et_epipolar_forward_fused(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                              const float *cam, const float *feat_ref, const float *feat_src, const void *packed_w,
                              const float *bias, float *x, float *attn, float *corr_pos, float *out_scratch,
                              int32_t want_out, void *workspace, size_t workspace_bytes, void *stream);

/* Pairs named by index into a stack of maps (ET_HAS_PAIR_INDEX).  A backbone runs once per view and returns ONE stack of maps;
 * the entry points above address their maps as base + n * H*W*C, so a caller had to gather a private copy of both maps of every
 * pair first.  The *_ix forms of the tile family take two POOLS instead,
 *   feat_ref : (M_ref,H,W,256)    feat_src : (M_src,H,W,256)        (they may be the same memory)
 *   ref_index, src_index : (N) int32 DEVICE arrays, each nullable
 * and pair n reads feat_ref[ref_index[n]] and feat_src[src_index[n]].  Every other array -- cam, out, x, attn, corr_pos, res_base,
 * out_scratch, grad_out, grad_attn, grad_ref, the workspace -- stays per pair, N of each, and every other argument is its unindexed
 * sibling's.  A NULL index is the identity (its pool then holds exactly N maps, M == N, else an error); with both NULL a call is
 * its sibling's, bit for bit: the siblings ARE these functions with NULL indices.
 *   et_epipolar_forward_tiled_ix  : et_epipolar_forward_tiled
 *   et_epipolar_forward_fused_ix  : et_epipolar_forward_fused (the feat_ref row of x = feat_ref + bias + out . Wf^T through ref_index)
 *   et_epipolar_backward_tiled_ix : et_epipolar_backward_tiled_ga (float atomics; attn and grad_attn nullable).
 *       grad_src : (M_src,H,W,256), the gradient of the source POOL: all M_src maps are cleared, pair n's rows are added into map
 *                  src_index[n] (several pairs may name one map; a map no pair names comes back 0).
 *       grad_ref : (N,H,W,256), per pair as before: the caller adds pair n's map into pool map ref_index[n].
 * The index values must lie in [0, M): the caller checks them (the Python binding does, on the host).  The kernels clamp what they
 * read into that range, so a bad index gives a wrong answer but never an access outside the pools.
 * Not indexed: the deterministic tile backward (its quantum and int64 accumulator are per pair), the per-pixel forward, the gather
 * and atomic per-pixel backward, the general kernels, and every shape the tile path does not take (C != 256): gather the pairs'
 * maps and call the unindexed entry points there. */
int et_epipolar_forward_tiled_ix(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                 const float *cam, const float *feat_ref, const float *feat_src, float *out,
                                 float *attn, float *corr_pos, const float *res_bias, float *res_base,
                                 void *workspace, size_t workspace_bytes, void *stream, const int32_t *ref_index,
                                 const int32_t *src_index, int32_t M_ref, int32_t M_src);
int et_epipolar_forward_fused_ix(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                 const float *cam, const float *feat_ref, const float *feat_src, const void *packed_w,
                                 const float *bias, float *x, float *attn, float *corr_pos, float *out_scratch,
                                 int32_t want_out, void *workspace, size_t workspace_bytes, void *stream,
                                 const int32_t *ref_index, const int32_t *src_index, int32_t M_ref, int32_t M_src);
int et_epipolar_backward_tiled_ix(const EtLayerDesc *desc, const float *xs, const float *ys, const float *steps,
                                  const float *cam, const float *feat_ref, const float *feat_src, const float *attn,
                                  const float *grad_out, const float *grad_attn, float *grad_ref, float *grad_src,
                                  void *workspace, size_t workspace_bytes, void *stream, const int32_t *ref_index,
                                  const int32_t *src_index, int32_t M_ref, int32_t M_src);

/* Peak finder of the pose head: find_tensor_peak_batch (modeling/backbones/basic_batch.py:17-63), which
 * PoseResNet.forward calls once per sample in a Python loop (resnet.py:424-430).  One launch for all maps.
 *   heatmaps : (num_maps, H, W) float32, num_maps = N * joints (the NCHW output of final_layer as it lies in memory)
 *   radius   : cfg.KEYPOINT.SIGMA ;  downsample : cfg.BACKBONE.DOWNSAMPLE ;  threshold : 1e-6 in the reference
 *   legacy_floor_division : index / W as integer division (torch < 1.5, what the authors trained with) instead of
 *                           the true division the torch of this image performs
 *   locs     : (num_maps, 2) image coordinates (x, y) ;  scores : (num_maps) the maximum of each map
 * H, W >= 2 and 0.5 <= radius <= 4096 (int(radius + 0.5) >= 1), else an error.
 * Non-finite maps, as torch.max / F.grid_sample / F.threshold treat them: a NaN ranks above every value and the first one wins,
 * so a map that holds a NaN has score NaN and -- the NaN lies in its own window and a sample is dropped only when it is
 * <= threshold -- NaN coordinates; a +inf cell gives score +inf and NaN coordinates (inf / inf).  A map of -inf alone has no
 * candidate: index 0, score -inf, and the location of cell 0 or NaN (its window holds -inf * weight, and a weight may be zero);
 * never a value outside the image.
 * et_debug_host_heatmap_peaks: HOST test hook, no GPU -- the kernel's per-map routine (csrc/et_peaks.h) in a serial loop, its
 * sums taken in the kernel's order; host pointers. */
int et_heatmap_peaks(int64_t num_maps, int32_t H, int32_t W, const float *heatmaps, float radius, float downsample,
                     float threshold, int32_t legacy_floor_division, float *locs, float *scores, void *stream);
int et_debug_host_heatmap_peaks(int64_t num_maps, int32_t H, int32_t W, const float *heatmaps, float radius, float downsample,
                                float threshold, int32_t legacy_floor_division, float *locs, float *scores);

/* The peak finder's backward: the gradient find_tensor_peak_batch's autograd (F.grid_sample, F.threshold, the two weighted sums,
 * torch.max) leaves in the heat maps.  One launch for all maps, no atomics, every sum in a fixed order: the same bits from run to
 * run and whatever else the batch holds.  The leading arguments are et_heatmap_peaks's, on the same maps.
 *   grad_locs   : (num_maps, 2) gradient of locs, or NULL ;  grad_scores : (num_maps) gradient of scores, or NULL (not both NULL)
 *   grad_heat   : (num_maps, H, W), EVERY element written
 * The index, the window and its three sums S, Sx, Sy are recomputed by the forward's own routines (csrc/et_peaks.h).  With
 * tot = S + eps, window element e -- thresholded value v_e, ramps rx_e, ry_e -- receives
 *   c_e = downsample (g_x (rx_e - Sx / tot) + g_y (ry_e - Sy / tot)) / tot   if the sample was kept (not <= threshold: a NaN is
 * kept), else 0 -- evaluated as downsample (g_x (rx_e tot - Sx) + g_y (ry_e tot - Sy)) / tot / tot, which is exactly 0 where one
 * sample alone survives the threshold and the location therefore does not depend on the map; each of its four bilinear taps inside the map receives c_e times the tap's weight; the arg-max cell (the first
 * maximum) receives grad_scores on top; every other cell is 0.  index_w, index_h and the box are constants, as in the reference
 * (.data).  With grad_locs NULL the window is not visited: a map with a NaN still returns the one finite grad_scores entry.
 * et_debug_host_heatmap_peaks_bwd: HOST test hook, no GPU, the same per-cell routine and summation order; host pointers. */
int et_heatmap_peaks_bwd(int64_t num_maps, int32_t H, int32_t W, const float *heatmaps, float radius, float downsample,
                         float threshold, int32_t legacy_floor_division, const float *grad_locs, const float *grad_scores,
                         float *grad_heat, void *stream);
int et_debug_host_heatmap_peaks_bwd(int64_t num_maps, int32_t H, int32_t W, const float *heatmaps, float radius, float downsample,
                                    float threshold, int32_t legacy_floor_division, const float *grad_locs,
                                    const float *grad_scores, float *grad_heat);

/* KEYPOINT.TRIANGULATION epipolar / epipolar_dlt: triangulate_epipolar (vision/triangulation.py:234-348), the lifting that
 * consumes the layer's corr_pos.  Every (frame, joint) is independent; inputs float32, all arithmetic float64.  One launch.
 *   pts       : (F, V, J, 2) image coordinates, already multiplied by resize = IMAGE_RESIZE * PREDICT_RESIZE
 *   conf      : (F, V, J) ;  krt : (F, V, 3, 4) ;  other_krt : (F, V, 3, 4) the projection of each view's source view
 *   corr_pos  : (F, V, H, W, 2) feature-map pixels, [..., 0] = x: the layer's output for the frame-major batch
 *   downsample: cfg.BACKBONE.DOWNSAMPLE ;  conf_thres / ransac_thres : cfg.KEYPOINT.CONF_THRES / RANSAC_THRES
 *   dlt       : 0 = epipolar, else epipolar_dlt
 *   out       : (F, J, 3) float64 world points ;  info : (F, J) int32 or NULL
 * A view is selected when conf > float32(conf_thres), compared in float32.  None selected: the first arg-max of conf alone
 * (branch 2); one selected: branch 1; both triangulate that view's detection against its corr_pos entry in the source view
 * (DLT of the two views' rows).  Two or more (branch 0): with dlt, the DLT over the selected views; otherwise every pair a < b
 * of selected views is a hypothesis (its two-view DLT point p), its inliers are the selected views whose ray through their
 * detection passes p closer than ransac_thres, and the FIRST hypothesis with the largest inlier count wins: more than two
 * inliers -> the DLT over them, one or two -> p, none -> (0, 0, 0).
 * Two deviations from the reference: the hypotheses are always enumerated (the reference samples 100 random pairs when
 * J >= 10: the same set for V <= 8, in an order that only decides ties), and a corr_pos index outside the map is clamped into
 * it and flagged (the reference wraps a negative index and raises on a large one).
 *   info bits 0-7  : selected views           bits 8-15 : the views the returned point was computed from (none: 0)
 *        bits 16-17: branch                   bit 18    : no hypothesis had an inlier       bit 19 : the lookup was clamped
 * V <= 8.  No atomics: bit-reproducible. */
int et_triangulate_epipolar(int32_t F, int32_t V, int32_t J, int32_t H, int32_t W, const float *pts, const float *conf,
                            const float *krt, const float *other_krt, const float *corr_pos, float downsample, float resize,
                            double conf_thres, double ransac_thres, int32_t dlt, double *out, int32_t *info, void *stream);

/* Test hook (HOST pointers, runs on the CPU, no GPU needed): the per-joint routine of et_triangulate_epipolar
 * (csrc/et_triangulate.h, shared with the kernel) in a serial loop over frames, joints and hypotheses.  Not a CPU fallback of
 * the path. */
int et_debug_host_triangulate_epipolar(int32_t F, int32_t V, int32_t J, int32_t H, int32_t W, const float *pts, const float *conf,
                                       const float *krt, const float *other_krt, const float *corr_pos, float downsample,
                                       float resize, double conf_thres, double ransac_thres, int32_t dlt, double *out,
                                       int32_t *info);

/* KEYPOINT.TRIANGULATION pymvg / naive / refine (vision/triangulation.py:425-441, 99-154, 162-232): the liftings that need only
 * detections, scores and projections.  Every (frame, joint) is independent; inputs float32, all arithmetic float64.  One launch.
 *   pts : (F, V, J, 2) image coordinates ;  conf : (F, V, J) ;  krt : (F, V, 3, 4)
 *   method : 0 = pymvg, 1 = naive, 2 = refine ;  conf_thres / ransac_thres : cfg.KEYPOINT.CONF_THRES / RANSAC_THRES
 *   out : (F, J, 3) float64 world points ;  info : (F, J) int32 or NULL
 * pymvg: t = conf_thres; the views with conf > float32(t), compared in float32, are selected; while at most one is and t >= -1,
 * t -= 0.05 in float64 (repeated subtraction: the rounding of the sequence is part of the rule); then the DLT over the selected
 * views.  Fewer than two views at the end (V = 1, NaN scores, scores <= -1): (0, 0, 0) and bit 18 -- the reference fails there.
 * ransac_thres is not read.
 * naive: the views with conf > float32(conf_thres); at most one: (0, 0, 0) and bit 18.  Otherwise every pair a < b of selected
 * views in lexicographic order is a hypothesis (its two-view DLT point p), its inliers are the selected views whose ray through
 * their detection passes p closer than ransac_thres, and the FIRST hypothesis with the largest count wins: its p, or (0, 0, 0)
 * and bit 18 when no hypothesis has an inlier.
 * refine: the same search; a winner with more than one inlier returns the DLT over its inliers, with exactly one its p.
 * One deviation from the reference: naive and refine there draw 100 random ordered pairs per joint; here every pair is
 * enumerated.  For V <= 8 the draws "all ordered pairs in lexicographic order, cyclically" are one sequence the reference can
 * produce, it visits every pair, and its result is the result of the enumeration.
 *   info bits 0-7  : views selected           bits 8-15 : the views the returned point was computed from (none: 0)
 *        bit 18    : zeros written            bits 24-30: threshold steps taken (pymvg)
 * V <= 8, conf_thres finite and <= 2 (at most 61 steps).  No atomics: bit-reproducible. */
int et_triangulate_views(int32_t F, int32_t V, int32_t J, const float *pts, const float *conf, const float *krt, int32_t method,
                         double conf_thres, double ransac_thres, double *out, int32_t *info, void *stream);

/* Test hook (HOST pointers, runs on the CPU, no GPU needed): the per-joint routine of et_triangulate_views
 * (csrc/et_triangulate.h, shared with the kernels) in a serial loop.  Not a CPU fallback of the path. */
int et_debug_host_triangulate_views(int32_t F, int32_t V, int32_t J, const float *pts, const float *conf, const float *krt,
                                    int32_t method, double conf_thres, double ransac_thres, double *out, int32_t *info);

/* The liftings' backward: the gradient of et_triangulate_views (pymvg, naive, refine) and of et_triangulate_epipolar (epipolar,
 * epipolar_dlt) in the detections.  One launch, one lane per (frame, joint), float64 arithmetic rounded once to float32 on the
 * store; no atomics, no workspace: the same bits from run to run and whatever else the batch holds.
 *   pts, krt, other_krt, corr_pos, downsample, resize : the forward's
 *   info      : (F, J) int32, the word the forward wrote for these inputs
 *   grad_out  : (F, J, 3) float64 gradient of the world points
 *   grad_pts  : (F, V, J, 2) float32, EVERY element written
 * other_krt and corr_pos both NULL: the backward of et_triangulate_views; H, W, downsample and resize are then not read, and a word
 * with branch bits gives zeros for its joint.  Both non-NULL: the backward of et_triangulate_epipolar.  One of them NULL is an error.
 * Nothing is searched and nothing was saved: the word names the DLT that produced the point, and that DLT is replayed.
 *   (info >> 8 & 0xff) == 0 (zeros written, no inlier, fewer than two views), or one view without branch bits: all 2 V values 0
 *   (info >> 16 & 3) != 0  : the rows of the one view of bits 8-15 and the two rows of other_krt at the correspondence the forward
 *                            read from corr_pos (the same pixel arithmetic, the same clamp).  The correspondence is a constant --
 *                            it is piecewise constant in the detection -- so only that view's detection receives a gradient
 *   otherwise              : the DLT over the views of bits 8-15 -- pymvg's selection, naive's winning pair, refine's inliers,
 *                            epipolar's pair or inliers, epipolar_dlt's selection
 * With the rows A (two per view: x P[2] - P[0], y P[2] - P[1]) fixed at that decision, v the unit right singular vector of the
 * smallest singular value s4, X = v[:3] / v[3] and gX = grad_out:
 *   gv = (gX / v3, -(gX . v[:3]) / v3^2) ;  w = - sum_{k<4} v_k (v_k . gv) / (s_k^2 - s4^2) ;  gA = (A w) v^T + (A v) w^T
 * and the detection (x, y) of a used view receives gA[row_x] . P[2], gA[row_y] . P[2]; a view that was not used receives exactly 0.
 * The selection is discrete: nothing goes to the scores, and nothing to the projections or corr_pos.  A vanishing gap
 * s3^2 - s4^2 is NOT guarded: the result is then inf or NaN, as float64 autograd through an SVD gives there.
 * The argument checks are the forwards' (sizes, V <= 8, NULL pointers, map size, downsample / resize) and come before any launch.
 * et_debug_host_triangulate_bwd: HOST test hook, no GPU -- the kernel's per-joint routine (csrc/et_triangulate.h) in a serial loop;
 * host pointers. */
int et_triangulate_bwd(int32_t F, int32_t V, int32_t J, int32_t H, int32_t W, const float *pts, const float *krt,
                       const float *other_krt, const float *corr_pos, float downsample, float resize, const int32_t *info,
                       const double *grad_out, float *grad_pts, void *stream);
int et_debug_host_triangulate_bwd(int32_t F, int32_t V, int32_t J, int32_t H, int32_t W, const float *pts, const float *krt,
                                  const float *other_krt, const float *corr_pos, float downsample, float resize,
                                  const int32_t *info, const double *grad_out, float *grad_pts);

/* KEYPOINT.TRIANGULATION rpsm: the recursive pictorial structure model (modeling/pictorial_cuda.py:222-254) for F frames at once,
 * float32 as the reference.  A first stage scores first_nbins^3 candidate positions per joint (a grid of grid_size around
 * center[f]) against every view's heat map and runs max-product over the limbs of the skeleton; recur_depth levels follow, each
 * with a grid of recur_nbins^3 bins around every joint's current position, of size grid_size / first_nbins / recur_nbins^k.
 *   heatmaps : (F, V, J, H, W) ;  cams : (F, V, 3, 4) projections to IMAGE pixels ;  trans : (F, V, 2, 3) crop transforms
 *   center   : (F, 3) ;  limb_length : (F, J - 1), limb e ends at the e-th non-root joint in ascending order
 *   first_limb_length : as limb_length, for the first stage; NULL = limb_length
 *   parent   : J int32 on the HOST, the root has -1 ;  image_w / image_h : cfg.DATASETS.IMAGE_SIZE
 *   out      : (F, J, 3) ;  path : (F, 1 + recur_depth, J) int32 or NULL, the chosen bin of every level
 * A bin: b = (ix * n + iy) * n + iz at linspace(-size/2, size/2, n)[i] + centre per axis.  Its unary: the sum over the views, in
 * ascending order, of one bilinear sample (zero padding; align_corners as given) of heatmaps[f, v, j] at the projection
 * p = cam . (X, 1), xy = p[:2] / p[2], through trans, times (W, H) / (image_w, image_h), normalised as xy / (H - 1, W - 1) * 2 - 1
 * (x by H - 1: the reference's).  Parent bin a and child bin c of a limb of length L are compatible when
 * | ||x_a - x_c + 1e-6|| + 1e-9 - L | < tolerance: this band stands in for the reference's PICT_STRUCT.PAIRWISE_FILE, and a file that
 * is not such a band cannot be expressed.  E_j = unary_j times, for each child in ascending joint index, max_c(compat(a, c) *
 * E_child[c]); every arg-max is the FIRST index among equal values; the root takes the arg-max of its energy and the children
 * follow the remembered indices.
 * Limits: V in [1, 8], J in [1, 32] with parent a tree that has one root, first_nbins in [2, 16], recur_nbins in [2, 3],
 * recur_depth in [0, 16].  The workspace (et_rpsm_workspace_bytes; 0 for sizes outside the limits) may have any alignment and
 * needs no initialisation.  No atomics: bit-reproducible. */
size_t et_rpsm_workspace_bytes(int32_t F, int32_t J, int32_t first_nbins, int32_t recur_nbins);
int et_rpsm(int32_t F, int32_t V, int32_t J, int32_t H, int32_t W, const float *heatmaps, const float *cams, const float *trans,
            const float *center, const float *limb_length, const float *first_limb_length, const int32_t *parent, float image_w,
            float image_h, double grid_size, int32_t first_nbins, int32_t recur_nbins, int32_t recur_depth, float tolerance,
            int32_t align_corners, float *out, int32_t *path, void *workspace, size_t workspace_bytes, void *stream);

/* Test hook (HOST pointers, runs on the CPU, no GPU needed): the per-frame routine of et_rpsm (csrc/et_rpsm.h, its pieces shared
 * with the kernels) in a serial loop over frames, joints and bins.  Not a CPU fallback of the path. */
int et_debug_host_rpsm(int32_t F, int32_t V, int32_t J, int32_t H, int32_t W, const float *heatmaps, const float *cams,
                       const float *trans, const float *center, const float *limb_length, const float *first_limb_length,
                       const int32_t *parent, float image_w, float image_h, double grid_size, int32_t first_nbins,
                       int32_t recur_nbins, int32_t recur_depth, float tolerance, int32_t align_corners, float *out, int32_t *path);

/* The evaluation metrics of Modelbuilder.forward's test-time branch (modeling/model.py:339-351, 372-404), on the device: the
 * reference copies both heat-map stacks to the host and walks N * J items in Python.  Every value below is a count of exact
 * decisions or a float64 expression of the reference's operands in the reference's order, each operation rounded once (no FMA
 * contraction), so the results equal the reference's to the bit; the sums run in a fixed order without atomics, so they are
 * bit-reproducible.  Inputs are finite by contract: the result for a map or a point that holds a NaN is unspecified.
 *
 * et_eval_jdr: JDR (modeling/metrics/metrics2d.py:294-324, hm_type 'gaussian') with get_max_preds (basic_batch.py:67-95),
 * calc_dists (:269-281) and dist_acc (:284-291).
 *   pred, target : (N, J, H, W) float32, predicted and target heat maps ;  thr : the reference's 0.5
 *   dists : (J, N) float64, the reference's own layout ;  acc : (J + 1) float64
 *   pred_xy, target_xy : (N, J, 2) float32 or NULL -- what get_max_preds returns
 * Per map the FIRST maximum (value, then lowest flat index, as np.argmax; -0.0 and +0.0 tie): x = idx % W, y = idx / W, both
 * set to 0 unless the maximum is > 0.  dists[j][n] = -1 unless the target's x > 1 and y > 1; otherwise the float64 norm of
 * (pred - target) / normalize with normalize = (H / 10, W / 10) applied to (x, y) IN THAT ORDER -- the reference divides x by
 * the height term, and so does this.  acc[1 + j] = (dists[j] < thr among dists[j] != -1) / their number, or -1 when no sample
 * counts; acc[0] = the sum of the non-negative acc[1 + j] in joint order / their number -- NaN when no joint counts (the
 * reference divides zero by zero there and raises).  2 <= H, 2 <= W, H * W <= 16384. */
int et_eval_jdr(int32_t N, int32_t J, int32_t H, int32_t W, const float *pred, const float *target, double thr, double *dists,
                double *acc, float *pred_xy, float *target_xy, void *stream);

/* et_eval_pck: calculate_err (metrics2d.py:199-235), whose PCKs are calc_pck's (:238-265).
 *   locs : (N, J, 2) float32 detections ;  gt : (N, J, 2) float64 ;  vis : (N, J) float32 or NULL (all visible); an item counts
 *   when vis != 0
 *   thresholds : T float64 (cfg.TEST.THRESHOLDS) ;  curve : M float64 (np.linspace(0, MAX_TH, num=int(MAX_TH)))
 *   pck : T float64 ;  err_joints : (N, M) float64 ;  total_joints : (N) float64
 * The error of a counted item is |double(locs.x) - gt.x| -- x ONLY: the reference's `detected_points[:1, j]` selects the first
 * row of its (2, J) array, and this reproduces it.  pck[t] = count(err < thresholds[t]) * 100.0 / count over the whole batch (NaN
 * when nothing counts); err_joints[n][m] = count over sample n of err < curve[m]; total_joints[n] = counted items of sample n.
 * T == 0 and M == 0 are valid and write nothing of their array (which may then be NULL). */
int et_eval_pck(int32_t N, int32_t J, const float *locs, const double *gt, const float *vis, int32_t T, const double *thresholds,
                int32_t M, const double *curve, double *pck, double *err_joints, double *total_joints, void *stream);

/* et_eval_epe: EPEmean (modeling/metrics/metrics3d.py:5-46) in float64.
 *   pred, gt : (F, J, 3) float64 ;  vis : (F, J) float32 or NULL ;  unit, max_dist : the batch's unit, cfg.TEST.EPEMEAN_MAX_DIST
 *   mean : 1 float64 ;  per_joint : (F, J) float64 (the reference returns row 0 of it)
 * err = sqrt((dx^2 + dy^2) + dz^2) * unit, replaced by max_dist where it exceeds it; mean = the mean over all F * J items --
 * visibility does not enter it, as in the reference -- summed in a fixed order (256 strided partial sums, then a pairwise tree);
 * per_joint = err with the items of vis == 0 set to 0. */
int et_eval_epe(int32_t F, int32_t J, const double *pred, const double *gt, const float *vis, double unit, double max_dist,
                double *mean, double *per_joint, void *stream);

/* Test hooks (HOST pointers, run on the CPU, no GPU needed): the per-item routines of the three calls above (csrc/et_metrics.h,
 * shared with the kernels) in serial loops, the mean in the kernel's summation order.  Not a CPU fallback of the path. */
int et_debug_host_eval_jdr(int32_t N, int32_t J, int32_t H, int32_t W, const float *pred, const float *target, double thr,
                           double *dists, double *acc, float *pred_xy, float *target_xy);
int et_debug_host_eval_pck(int32_t N, int32_t J, const float *locs, const double *gt, const float *vis, int32_t T,
                           const double *thresholds, int32_t M, const double *curve, double *pck, double *err_joints,
                           double *total_joints);
int et_debug_host_eval_epe(int32_t F, int32_t J, const double *pred, const double *gt, const float *vis, double unit, double max_dist,
                           double *mean, double *per_joint);

/* The training loss of Modelbuilder.forward (modeling/model.py:59-71, 249-258) and the heat-map targets of its data loader, on the
 * device.  Maps hold at most 16384 elements (H, W >= 1, H * W <= 16384); N, J >= 1.  No call synchronises, none uses atomics:
 * every output is bit-reproducible, and the host hooks below give the bits of the kernels wherever no exp or pow is involved
 * (their exp and pow are the C library's, the kernels' the device library's: both well inside what one rounding to float32
 * hides, except next to a rounding midpoint).
 *
 * et_heatmap_targets: Heatmapcreator.get (data/transforms/keypoints2d.py:3-36), called without valid_vec as the data set does.
 *   points : (N, J, 2) float64, (u, v) in image pixels ;  out : (N, J, H, W) float32
 * s = sigma * 2**0.5 in float64.  The grid value of row i is float32(float32(float32(i) * float32(downsample) +
 * float32(downsample / 2.0 - 0.5)) / float32(s)) -- one IEEE float32 division -- and the same for column k.  r = v / s - grid_i:
 * v, the SECOND coordinate, pairs with the row; c = u / s - grid_k; q = r * r + c * c, all float64; out = float32(exp(-min(q,
 * 4.60517019))).  There is no visibility mask and the background is float32(exp(-4.60517019)) = 0.01, not zero. */
int et_heatmap_targets(int32_t N, int32_t J, int32_t H, int32_t W, const double *points, double sigma, double downsample, float *out,
                       void *stream);

/* et_heatmap_loss: the criterion `kind` of predicted against target heat maps, a float32 scalar.
 *   pred    : (N, J, H, W) float32
 *   target  : (N, J, H, W) float32, or NULL with points : (N, J, 2) float64 and sigma / downsample -- then every lane makes the
 *             target value of its own pixels as et_heatmap_targets does and no dense target exists.  Exactly one of the two.
 *   weight  : (N, J) float32 or NULL (ones); must be NULL for ET_LOSS_MSE
 *   partials: N * J float64 of scratch, the caller's (any contents before, unspecified after)
 *   loss    : 1 float32 ;  den : 1 float64, the denominator -- et_heatmap_loss_bwd reads it
 * The float32 term of an element, each operation rounded once, as the reference computes it:
 *   ET_LOSS_JOINT      (JointsMSELoss)            d = pred * w - gt * w ;  term = d * d ;  den = N * H * W * (per_joint ? 1 : J)
 *   ET_LOSS_SMOOTHMSE  (KeypointsMSESmoothLoss)   d = gt - pred ;  t = (d * d) * w ;  term = t, or float32(t ** 0.1) * float32(400 **
 *                                                 0.9) where t > 400 ;  den = H * W * max(1, sum of the weights)
 *   ET_LOSS_MSE        (MaskedMSELoss, no mask)   d = pred - gt ;  term = d * d ;  den = N * J * H * W
 * loss = float32(sum / den), the sum in float64 in a fixed order: lane t of a map's 256 owns the 4-float quads
 * first + t, first + t + 256, ... of the flat tensor (first = the quad the map starts in) and adds the elements of them that lie
 * in the map in ascending order; the 256 partial sums go through a pairwise tree (p[t] += p[t + half], half = 128 .. 1); the
 * per-map sums are added per joint over n ascending, then over the joints ascending.
 * et_heatmap_loss_bwd: grad_pred (N, J, H, W) = d loss / d pred * grad_out[0]; grad_out and den are DEVICE pointers.  An
 * element is float32(2 * d * w * c) for joint, float32(2 * d * c) for mse and float32(-2 * d * w * c), times 0.1 * t ** -0.9 *
 * 400 ** 0.9 where t > 400, for smoothmse -- float64 from the float32 d, c = grad_out / den.  The weight carries no gradient. */
#define ET_LOSS_JOINT 0
#define ET_LOSS_SMOOTHMSE 1
#define ET_LOSS_MSE 2
int et_heatmap_loss(int32_t kind, int32_t N, int32_t J, int32_t H, int32_t W, const float *pred, const float *target,
                    const double *points, double sigma, double downsample, const float *weight, int32_t per_joint, double *partials,
                    float *loss, double *den, void *stream);
int et_heatmap_loss_bwd(int32_t kind, int32_t N, int32_t J, int32_t H, int32_t W, const float *pred, const float *target,
                        const double *points, double sigma, double downsample, const float *weight, const double *den,
                        const float *grad_out, float *grad_pred, void *stream);

/* Test hooks (HOST pointers, run on the CPU, no GPU needed): the per-lane routines of the three calls above (csrc/et_loss.h,
 * shared with the kernels) in serial loops, in the kernels' summation order.  Not a CPU fallback of the path. */
int et_debug_host_heatmap_targets(int32_t N, int32_t J, int32_t H, int32_t W, const double *points, double sigma, double downsample,
                                  float *out);
int et_debug_host_heatmap_loss(int32_t kind, int32_t N, int32_t J, int32_t H, int32_t W, const float *pred, const float *target,
                               const double *points, double sigma, double downsample, const float *weight, int32_t per_joint,
                               double *partials, float *loss, double *den);
int et_debug_host_heatmap_loss_bwd(int32_t kind, int32_t N, int32_t J, int32_t H, int32_t W, const float *pred, const float *target,
                                   const double *points, double sigma, double downsample, const float *weight, const double *den,
                                   const float *grad_out, float *grad_pred);

/* Layout converters between the reference's NCHW and the kernels' NHWC. */
int et_nchw_to_nhwc(int32_t N, int32_t C, int32_t H, int32_t W, const float *src, float *dst, void *stream);
int et_nhwc_to_nchw(int32_t N, int32_t C, int32_t H, int32_t W, const float *src, float *dst, void *stream);

/* Test hook (HOST pointers, runs on the CPU, no GPU needed): evaluates the
 * per-sample set-up code that is shared with the device kernels for ONE pair
 * (cam points at its 27 floats), pixel (h, w): taps[k*4 + r] = linear index
 * y*W+x of the source pixel routed to tap register r (-1: outside the image),
 * weights[k*4 + r] = its bilinear weight, locs[k*2 .. k*2+1] = normalised
 * sample location.  It computes no features and is not a CPU fallback of the
 * path. */
int et_debug_host_sample_setup(const EtLayerDesc *desc, const float *xs, const float *ys,
                               const float *steps, const float *cam, int32_t h, int32_t w,
                               int32_t *taps, float *weights, float *locs);

/* Diagnostic (no reference counterpart; bench.py reports it beside the backward's time): `blocks` x 4 waves each issue
 * `iters` float-atomic wave-instructions onto pseudo-random pixel rows of dst (rows, 256) fp32 -- the access pattern of the
 * tiled backward's d(feat_src) accumulation (two 128-byte runs in two rows per instruction) with nothing around it.  dst is
 * modified (1.0 is added); rows < 2^22. */
int et_debug_atomic_probe(float *dst, int64_t rows, int32_t blocks, int32_t iters, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EPIPOLAR_AMD_H_ */
