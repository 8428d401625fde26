/*
 * dmvs.h -- C ABI of libdmvs_hip.so: the MI355X (gfx950) kernels behind DMVSNet's
 * cost-volume hot path.  This is the drop-in boundary below the Python host module
 * (dmvsnet_amd.MVSNet, same forward() signature as /root/reference/networks/mvsnet.py:188).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the comment says "host";
 *   - every kernel is enqueued on `stream` (a hipStream_t passed as void*; 0 = null stream);
 *   - nothing allocates, nothing synchronises, nothing throws; the caller owns all buffers;
 *   - return value: 0 on success, a positive hipError_t from the launch, or a negative
 *     DMVS_E* argument error.  dmvs_error_string() decodes both;
 *   - batch size is 1 (the reference's eval loader, model.py:330-336, always uses B=1);
 *     volumes are planar fp32: activations [C][D][H][W], hypotheses [D][H][W];
 *     2D feature maps handed to the warp are pixel-major ("HWC"): element (y,x,c) at
 *     ((y*W + x)*pix_stride + c).
 *
 * Each entry point cites the reference code it replaces (file:line under /root/reference).
 */
#ifndef DMVS_H
#define DMVS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dmvs_stream_t; /* hipStream_t */

#define DMVS_VERSION 140 /* 0.1.4: + N6 dmvs_dual_depth_loss / _workspace (additive, same version); + N5 dmvs_cloud_cell_keys / _cell_runs / _thin_round / _nn / _in_mask / _above_plane / _in_box (additive, same version); 0.1.4 (r06): + dmvs_prob_regress / dmvs_depth_select (`prob` -> K4); 0.1.3 (r06): + K3z dmvs_conv3d_zmarch / _weight_floats / dmvs_pack_conv_weights_zmarch, + the bf16-split probe dmvs_conv3d_split_probe / _weight_floats / dmvs_pack_conv_weights_split; 0.1.2 (r05): + K3r dmvs_conv3d_coarse / _weight_floats / dmvs_pack_conv_weights_coarse; 0.1.1: DMVS_OUT_Q4 moved to bit 3 (value 8); bit 2 (value 4, r02's DMVS_OUT_HWC2: two
                            PIXEL-MAJOR halves) is retired and rejected with DMVS_EUNSUPPORTED -- a caller built against
                            version 100 can no longer get the quad-planar layout silently; dmvs_tune("k1_variant") is
                            gone (the launch variant is an argument of dmvs_warp_corr_q4) */

#define DMVS_EINVAL (-1)      /* bad dimension / null pointer */
#define DMVS_EUNSUPPORTED (-2) /* channel count or mode not compiled in */

#define DMVS_MAX_SRC_VIEWS 16

/* conv flags */
#define DMVS_RELU 1
#define DMVS_SKIP_UP2 2    /* skip is [Cout][D][Ho/2][Wo/2]: nearest x2 upsample fused into the residual add
                              (FeatureNet top-down path, module.py:328,333); K3 conv modes only */
#define DMVS_FLAG_RETIRED_4 4 /* was DMVS_OUT_HWC2 in version 100; every conv entry point returns DMVS_EUNSUPPORTED for it */
#define DMVS_OUT_Q4 8      /* out is TWO quad-planar tensors back to back, [Do][Cout/8][Ho][Wo][4] each (channels
                              [0, Cout/2) then [Cout/2, Cout); with kdepth = 1 the depth slices are the views, so every
                              view's half is one contiguous [C/4][H][W][4] map): FeatureNet's stageK / stageK_c halves
                              (module.py:326-336) written directly in the layout dmvs_warp_corr_q4 samples; K3 conv
                              modes, no residual, Cout % 8 == 0 */
#define DMVS_BN_TRAIN 32   /* dmvs_bn_relu_forward / _backward only: batch statistics (train mode); without it the running ones (eval) */
#define DMVS_IN_VIEWS 16   /* dmvs_conv3d_mfma, Cin = 4, kdepth 1, DMVS_CONV_S1 only (FeatureNet's first layer, module.py:283): `in`
                              is the eval loader's image stack [D = V][3][H][W] (general_eval.py:89,186) read in place -- channel c
                              of view v at ((v * 3 + c) * H * W) -- instead of a planar [4][V][H][W] copy with a zero channel.  The
                              4th channel of the MFMA k-group carries ZERO weights and reads the next view's first channel (finite
                              pixel values: the product is exactly 0) or, for the last view, past the end of the buffer
                              descriptor (returns 0) */
/* conv modes */
#define DMVS_CONV_S1 0     /* Conv3d k3 s1 p1                         module.py:142 */
#define DMVS_CONV_S2 1     /* Conv3d k3 s2 p1                         module.py:142 */
#define DMVS_DECONV_S2 2   /* ConvTranspose3d k3 s2 p1 output_pad 1   module.py:187 */
#define DMVS_CONV2D_K5S2 3 /* Conv2d k5 s2 p2 per depth slice (kdepth = 1)    module.py:289,295 */
#define DMVS_CONV2D_K1 4   /* Conv2d 1x1 per depth slice (kdepth = 1)         module.py:301,305,306 */

int dmvs_version(void);
/* Tuning knobs (A/B measurements, autotuning); not needed for correct results.  Known names:
 *   "k3_single_buf_min_blocks"  3D conv layers with at least this many workgroups run with one LDS stage (default
 *                               0: all of them; smaller grids keep two stages)
 *   "k3_min_blocks"             the big K3 tiles are used when they yield at least this many workgroups (768)
 *   "k3_split_blocks"           two-block (Cout = 64) layers whose small tiles yield fewer workgroups than this split
 *                               their M blocks over the waves (1024)
 *   "k3_deconv_prefetch"        1 (default): transposed convs with a residual prefetch it under their MFMAs; 0: residual loads
 *                               in the epilogue (A/B)
 *   "wino_stages"               LDS stages of the 3D Winograd layers: 0 = per-layer default, 1 = one, 2 = two where they fit
 *   "wino_persistent"           0: one tile per workgroup instead of the persistent tile walk (A/B; default 1)
 *   "wino_conv0_grid"           persistent workgroups of the conv0 Winograd kernel (multiple of 8; default 512)
 *   "k3r_grid"                  persistent workgroups of a K3r launch (dmvs_conv3d_coarse): 32 .. 1024 in multiples of 32 (8 XCDs x up
 *                               to 4 cout groups); default 256 = one per CU
 *   "k3r_counted_wait"          1 (default): K3r waits for a ring stage with a counted vmcnt; 0: vmcnt(0) (bit-identical, A/B + gate)
 *   "c8_rows"                   rows per wave of the K3s row sweep (0 = chosen from the wave count)
 *   "k3z_grid"                  persistent workgroups of a K3z launch (dmvs_conv3d_zmarch; multiple of 8, 0 = as many as are resident)
 *   "k3z_zs"                    cap of a z segment's length in K3z (0 = none; results do not depend on it)
 *   "zpad_skip"                 1 (default): 3x3x3 layers on volumes of depth <= 4 leave out the depth taps that only meet zero
 *                               padding (dmvs_zpad_live_mask; value-equal for finite inputs); 0: every tap is multiplied (A/B + gate)
 * Returns 0, DMVS_EINVAL (bad value) or DMVS_EUNSUPPORTED (unknown name).  Process-wide, not thread-safe. */
int dmvs_tune(const char* name, int value);
const char* dmvs_error_string(int code);
/* The live (plane, depth tap) pairs of a tile of TZ planes starting at plane oz0 of a 3x3x3 layer on a depth-D volume: bit
 * 3 * p + kz is set when plane oz0 + p takes a plane that is not zero padding through tap kz.  form 0: stride 1 (output planes),
 * 1: stride 2 (output planes of D -> (D + 1) / 2), 2: transposed stride 2 in gather form (input planes; tap 0 reads plane
 * z + 1).  The kernels behind "zpad_skip" derive what they skip from this function.  -1: bad argument (TZ in 1..10). */
long dmvs_zpad_live_mask(int form, int D, int oz0, int TZ);

/* [C_total][H][W] planar slice c0..c0+C  ->  [H][W][C] pixel-major.
 * Layout glue between FeatureNet's NCHW output (module.py:326-336, the stageK / stageK_c channel
 * split) and the warp kernel; no arithmetic. */
int dmvs_nchw_to_hwc(const float* src_chw, int c0, int C, int H, int W, float* dst_hwc, dmvs_stream_t stream);
/* the same with an explicit channel stride (floats): src points at one view's plane of a [C][V][H][W] stack. */
int dmvs_planar_to_hwc(const float* src, long chan_stride, int c0, int C, int H, int W, float* dst_hwc,
                       dmvs_stream_t stream);

/* Image ingest of the scan-level eval path: one decoded image -> the [3][H][W] fp32 planes FeatureNet reads, bit-identical
 * to the eval loader's host work it replaces (eval_io.MVSDataset: PIL decode / 255, eval_io.ResizePolicy.apply ->
 * eval_io.resize_linear; the reference's general_eval.py:97-110 + cv2.resize).  Layout glue: not a logged kernel.
 *   src         [h][w][3] uint8 (src_u8 = 1; converted through lut256, the host's np.float32(u) / 255.0) or fp32
 *   tx_idx/wt   [2][W]: source columns (i0, i1) and weights (1 - f, f) of eval_io.resize_taps(W, w); ty_* the same [2][H]
 *               for rows.  Ignored (may be NULL) when (h, w) == (H, W): the identity, as in resize_linear.
 *   dst         [3][H][W] planes (out_hwc = 0; e.g. one slot of a [V][3][H][W] FeatureNet input stack) or [H][W][3]
 *               fp32 (out_hwc = 1: the first pass of a chained resize).
 * Per output value: r_k = a_k*(1-fx) + b_k*fx for the source rows y0, y1, then r_0*(1-fy) + r_1*fy, unfused fp32. */
int dmvs_image_ingest(const void* src, int src_u8, int h, int w, const float* lut256, const int* tx_idx,
                      const float* tx_wt, const int* ty_idx, const float* ty_wt, int H, int W, float* dst, int out_hwc,
                      dmvs_stream_t stream);

/* Relative projections for all source views of one stage.
 * proj_pairs [V][2][4][4] (view 0 = reference): [v][0] extrinsic, [v][1][:3][:3] intrinsics.
 * out [V-1][12]: rot (row-major 3x3) then trans (3) of  (K_s E_s) (K_r E_r)^-1.
 * Replaces mvsnet.py:133-136 (composition) + module.py:223-225 (inverse, matmul, slicing). */
int dmvs_relative_proj(const float* proj_pairs, int V, float* out12, dmvs_stream_t stream);

/* First-stage hypothesis planes, module.py:560-579 (linear) / 598-634 (inverse).
 * depth_values [n] (only [0] and [n-1] are read).  out [D][H][W]; out_interval [1]. */
int dmvs_hypotheses_first(const float* depth_values, int n, int D, int H, int W, int inverse,
                          float* out_dhw, float* out_interval, dmvs_stream_t stream);

/* Later-stage hypothesis planes around last_depth [h][w] (previous stage's resolution),
 * then x2 bilinear upsample (align_corners=False) to [D][2h][2w] in the same kernel.
 * Replaces module.py:582-594 / 636-648 (+ 476-507, 525-554) and mvsnet.py:196,226-227,232-233.
 * ratio = depth_interval_ratio[stage]; depth_interval = (dv[n-1]-dv[0])/n is computed on device. */
int dmvs_hypotheses_next(const float* last_depth, int h, int w, const float* depth_values, int n,
                         float ratio, int D, int inverse, float* out_dhw, float* out_interval,
                         dmvs_stream_t stream);

/* Affine form of the LINEAR-depth hypotheses: every plane of a stage is
 *   plane d = base[y][x] + d * interval      (module.py:476-507, 560-579: lo + d * (hi - lo) / (D - 1))
 * so only `base` -- plane 0 of the functions above, [H][W] (the later stages: [2h][2w], upsampled) -- is produced and
 * dmvs_warp_corr_affine / dmvs_depth_regress_affine form the planes in registers: the [D][H][W] volume is neither
 * written nor read (3 x 30 / 61 / 61 MB per main pass at config 2).  Inverse-depth sampling is not affine in d and
 * keeps the volume.  out_interval as above; it is also the plane spacing. */
int dmvs_hypothesis_base_first(const float* depth_values, int n, int D, int H, int W, float* base_hw,
                               float* out_interval, dmvs_stream_t stream);
int dmvs_hypothesis_base_next(const float* last_depth, int h, int w, const float* depth_values, int n, float ratio,
                              int D, float* base_hw, float* out_interval, dmvs_stream_t stream);

/* The later-stage planes with an explicit resize factor: up = 2 is dmvs_hypotheses_next / dmvs_hypothesis_base_next,
 * up = 1 the SAME-RESOLUTION transition of pyramids deeper than the reference's three stages (a declared extension:
 * BASELINE configs[4]; the reference's resize to an equal size is the identity).  base_only: the affine form (plane 0). */
int dmvs_hypotheses_next_up(const float* last_depth, int h, int w, int up, const float* depth_values, int n, float ratio,
                            int D, int inverse, int base_only, float* out, float* out_interval, dmvs_stream_t stream);

/* K1: fused inverse-homography warp + bilinear gather + 2-group correlation + view sum.
 * Replaces CostAgg.forward (mvsnet.py:111-153) and homo_warping (module.py:212-251); the
 * [C][D][H][W] warped volume is never materialised.
 *   ref_hwc           reference feature, pixel-major, C channels, pix_stride floats per pixel
 *   src_hwc (host)    array of nsrc device pointers, same layout
 *   proj12            [nsrc][12] from dmvs_relative_proj (rows of the LOCAL source views)
 *   depth_dhw         [D][H][W] hypothesis planes
 *   sim_2dhw          [2][D][H][W]; group k = (2/C) sum_g warped[2g+k]*ref[2g+k], summed over views
 *   accumulate        0: overwrite, 1: add to what is there (view shards processed in pieces)
 * C in {8,16,32}; 1 <= nsrc <= DMVS_MAX_SRC_VIEWS. */
int dmvs_warp_corr(const float* ref_hwc, const float* const* src_hwc, int nsrc, int pix_stride,
                   const float* proj12, const float* depth_dhw, float* sim_2dhw,
                   int C, int D, int H, int W, int accumulate, dmvs_stream_t stream);

/* K1 on affine hypotheses: depth_dhw is replaced by base_hw [H][W] and step [1] (a device scalar: the interval). */
int dmvs_warp_corr_affine(const float* ref_hwc, const float* const* src_hwc, int nsrc, int pix_stride,
                          const float* proj12, const float* base_hw, const float* step, float* sim_2dhw,
                          int C, int D, int H, int W, int accumulate, dmvs_stream_t stream);

/* K1, product kernel: the same operator on QUAD-PLANAR features, [C/4][H][W][4] (channel quad q of pixel (y,x) at
 * ((q*H + y)*W + x)*4 floats) -- the layout FeatureNet's output layers write with DMVS_OUT_Q4.  A lane owns a pixel,
 * a workgroup a 32 x 8 tile x 8 (4) hypothesis planes; per source view the tile's window is bounded from the 8
 * corners of its (x, y, depth) box, staged in LDS with LDS-direct loads in 2^m channel slabs (m chosen so that the
 * window fits) and sampled with ds_read_b128; see csrc/warp_corr.hip.  Replaces the same reference code as
 * dmvs_warp_corr (mvsnet.py:111-153, module.py:212-251).
 *   depth_dhw [D][H][W], or NULL: plane d = base_hw[y][x] + d * step[0] (affine hypotheses, as dmvs_warp_corr_affine)
 *   variant   launch configuration (results agree to fp32 rounding): 0 default; low 3 bits 1 / 2 / 3 = 4 / 3 / 2
 *             workgroups per CU (40 / 53 / 80 KB windows); +8 = 4 planes per workgroup also when D > 4.  An explicit
 *             argument: no process-wide state.
 * Everything else as dmvs_warp_corr. */
int dmvs_warp_corr_q4(const float* ref_q4, const float* const* src_q4, int nsrc, const float* proj12,
                      const float* depth_dhw, const float* base_hw, const float* step, float* sim_2dhw,
                      int C, int D, int H, int W, int accumulate, int variant, dmvs_stream_t stream);

/* The same kernel on fp16 features (a declared extension: BASELINE configs[4] "fp16 features"; the reference raises
 * a dtype error there): quad-planar [C/4][H][W][4] of IEEE half, 8 bytes per pixel quad.  Products and
 * sums are fp32 (v_dot2_f32_f16); hypotheses, projections and the similarity volume stay fp32.  Halves the window
 * bytes in HBM and LDS.  Needs an even W.  Parity target: the fp32 path on the same (fp16-rounded) features. */
int dmvs_warp_corr_q4_f16(const void* ref_q4h, const void* const* src_q4h, int nsrc, const float* proj12,
                          const float* depth_dhw, const float* base_hw, const float* step, float* sim_2dhw,
                          int C, int D, int H, int W, int accumulate, int variant, dmvs_stream_t stream);

/* K1b: backward of the fused warp + correlation with respect to the FEATURE MAPS.  Differentiates CostAgg.forward
 * (mvsnet.py:111-153) over homo_warping (module.py:212-251); the sampling grid is built under torch.no_grad()
 * (module.py:222-243), so the cameras and the hypotheses receive no gradient -- there is none to compute.  With
 * G = gsim_2dhw and W_v = source view v sampled bilinearly (zeros padding, align_corners=True):
 *   gref_chw[c][y][x]         = (2/C) sum_v sum_d G[c & 1][d][y][x] * W_v[c][d][y][x]       (plain stores, reproducible)
 *   gsrc_chw[v][c][tap]      += w_tap * (2/C) * G[c & 1][d][y][x] * ref[c][y][x]            (fp32 global atomics)
 *   ref_q4, src_q4 (host)     quad-planar [C/4][H][W][4] features, as dmvs_warp_corr_q4
 *   proj12, depth_dhw         as dmvs_warp_corr (taps in the reference's op order, the generic kernel's routine)
 *   gsim_2dhw                 [2][D][H][W] upstream gradient
 *   gref_chw                  [C][H][W] planar, or NULL: the reference-gradient kernel is skipped
 *   gsrc_chw (host)           array of nsrc device pointers to [C][H][W] planar gradients that the CALLER has zeroed, or
 *                             NULL; a NULL entry skips that view; all NULL skips the source-gradient kernel
 * The source gradients depend on the arrival order of the atomics: equal run to run only to fp32 rounding
 * (dmvs_warp_corr_backward_det below is the order-free form).
 * C in {8,16,32}; 1 <= nsrc <= DMVS_MAX_SRC_VIEWS; any D. */
int dmvs_warp_corr_backward(const float* ref_q4, const float* const* src_q4, int nsrc, const float* proj12,
                            const float* depth_dhw, const float* gsim_2dhw, float* gref_chw, float* const* gsrc_chw,
                            int C, int D, int H, int W, dmvs_stream_t stream);

/* K1b, deterministic mode (additive, same version): dmvs_warp_corr_backward with the source gradients accumulated in FIXED
 * POINT (the entry above's scatter kernel on the FixedSink of csrc/warp_corr_bwd_det.h; docs/kernels/K1b_warp_corr_backward.md,
 * "Deterministic mode").  Every addend t = w_tap * ((gsim * 2/C) * ref) -- the fp32 addend of the entry above, formed by the
 * same code -- is added as the 64-bit integer rint(t * 2^k) with an integer atomic, and a finalize kernel WRITES every
 * element of every wanted gsrc as (float)((double)sum * 2^-k): the result is a pure function of the inputs, whatever the
 * arrival order, the launch decomposition or the set of wanted views.
 *   k          one per launch: min(62 - ceil(log2(D H W)), 50) - (eg + er + 2 + log2(2 / C)) with eg, er = floor(log2(max|.|))
 *              of gsim_2dhw and of ref_q4, taken by a pre-pass on the device (no host read-back: the entry can be captured
 *              in a graph).  A maximum of zero: every gsrc element is 0.  A maximum that is not finite (or addends that may
 *              overflow fp32, eg + er + 2 + log2(2 / C) > 127): every element of every wanted gsrc is NaN.
 *   gsrc_chw   as above but NOT zeroed by the caller: fully overwritten (and used as scratch before that)
 *   gref_chw   as above: the same kernel, the same bits
 *   workspace  dmvs_warp_corr_backward_det_workspace(C, H, W, nact) BYTES, 8-byte aligned, nact = the non-NULL gsrc entries:
 *              the int64 sums [nact][C][H][W], cleared on the stream by the entry.  NULL, misaligned or workspace_bytes too
 *              small with nact > 0: DMVS_EINVAL
 *   variant    launch configuration, the same bits for every value: 0 default; 1 = planes walked in reverse, 4 planes per
 *              chunk instead of 8, workgroups mapped in reverse (for tests of the order freedom).  Else DMVS_EINVAL.
 * Limits as dmvs_warp_corr_backward. */
long dmvs_warp_corr_backward_det_workspace(int C, int H, int W, int nact);
int dmvs_warp_corr_backward_det(const float* ref_q4, const float* const* src_q4, int nsrc, const float* proj12,
                                const float* depth_dhw, const float* gsim_2dhw, float* gref_chw, float* const* gsrc_chw,
                                int C, int D, int H, int W, void* workspace, size_t workspace_bytes, int variant,
                                dmvs_stream_t stream);

/* K1b with a PRE-SUMMED source scatter (additive, same version; csrc/warp_corr_bwd_presum.h; docs/kernels/K1b_warp_corr_backward.md,
 * "Pre-summed scatter"): the backward autograd records for CostAgg.forward (mvsnet.py:111-153) over homo_warping
 * (module.py:212-251), as the two entries above, in either of their modes.  A workgroup (64 x 4 pixels, one plane chunk) takes
 * the bounding box of its in-image taps, sums its addends in an LDS window of that box and issues one global add per window
 * element that is not zero; a box above the capacity falls back to the plain scatter's global adds per tap, an empty box adds
 * nothing.  The addends are those of the entries above, formed by the same code.
 *   det          0: fp32 atomics into the caller's ZEROED gsrc_chw (workspace ignored), equal to dmvs_warp_corr_backward to fp32
 *                rounding (another order of the same sum); 1: the workspace, pre-pass, clear and finalize of
 *                dmvs_warp_corr_backward_det, and its bits (integer sums do not depend on grouping)
 *   variant      0..3, else DMVS_EINVAL.  Bit 0 as dmvs_warp_corr_backward_det's 1 (4-plane chunks, planes and workgroups in
 *                reverse); bit 1: a test capacity of 256 texels.  The same values (det = 1: bits) for every variant.
 *   path_counts  NULL, or three device words the caller has zeroed: workgroups that took the window, the fallback, had no tap
 *   gref_chw     as above: the same kernel, the same bits
 * dmvs_warp_corr_backward_presum_cap: the window capacity in texels of (C, det, variant); 0 for arguments the entry refuses.
 * Limits and refusals otherwise as the entries above. */
long dmvs_warp_corr_backward_presum_cap(int C, int det, int variant);
int dmvs_warp_corr_backward_presum(const float* ref_q4, const float* const* src_q4, int nsrc, const float* proj12,
                                   const float* depth_dhw, const float* gsim_2dhw, float* gref_chw, float* const* gsrc_chw,
                                   int C, int D, int H, int W, int det, void* workspace, size_t workspace_bytes, int variant,
                                   unsigned* path_counts, dmvs_stream_t stream);

/* [C_total][H][W] planar slice c0..c0+C with a channel stride of chan_stride floats -> quad-planar [C/4][H][W][4]:
 * layout glue between torch feature maps (module.py:326-336: the stageK / stageK_c `split` halves are views that keep
 * the parent's channel stride; a batch sample is a pointer offset) and dmvs_warp_corr_q4 / dmvs_warp_corr_backward.
 * No arithmetic.  C in {8,16,32}; dst_q4 16-byte aligned. */
int dmvs_nchw_to_q4(const float* src, long chan_stride, int c0, int C, int H, int W, float* dst_q4, dmvs_stream_t stream);

/* K2: direct LDS-tiled 3D convolution / transposed convolution, fp32 VALU, fused epilogue
 *        y = conv(x) * scale[co] + shift[co];  relu;  y += skip
 * which is Conv3d/Deconv3d + BatchNorm(eval) + ReLU (module.py:151-157, 196-202) followed by the
 * U-Net residual add (module.py:394-396).  scale/shift may be NULL (the `prob` conv, module.py:379).
 *   in  [Cin][D][H][W];  out [Cout][Do][Ho][Wo] with (Do,Ho,Wo) = (D,H,W) for S1,
 *   ((D+1)/2,(H+1)/2,(W+1)/2) for S2 (kdepth=3) and (2D,2H,2W) for DECONV_S2.
 *   kdepth = 3: full 3x3x3 kernel.  kdepth = 1: 1x3x3 kernel applied per depth slice, depth
 *   stride 1 -- the 2D bottleneck of CostRegNet_part_refine (module.py:411-414) run on [C][1][H][W].
 *   w_packed: dmvs_pack_conv_weights layout [kd][kh][kw][Cin][Cout] (Cout fastest), for DECONV the
 *   same with the ConvTranspose weight [Cin][Cout][k][k][k] re-indexed (no flip; gather form). */
int dmvs_conv3d_direct(const float* in, float* out, const float* w_packed, const float* scale,
                       const float* shift, const float* skip, int Cin, int Cout, int D, int H, int W,
                       int mode, int kdepth, int flags, dmvs_stream_t stream);

/* K3: the same operator as an implicit-GEMM on the fp32 matrix cores (v_mfma_f32_32x32x2_f32 /
 * 16x16x4_f32; exact fp32 products, k-ordered fmaf chain).  Same arguments and layouts as
 * dmvs_conv3d_direct except w_packed, which is the MFMA A-fragment order produced by
 * dmvs_pack_conv_weights_mfma (host).  Supported (Cin, Cout, mode, kdepth) combinations are the layers of
 * CostRegNet_part(_refine) (module.py:358-436) and, with kdepth = 1 on a [C][V][H][W] stack of views, the
 * layers of FeatureNet (module.py:283-311); anything else returns DMVS_EUNSUPPORTED.  With kdepth = 1 the depth
 * axis is a batch axis (no depth taps, no depth stride). */
int dmvs_conv3d_mfma(const float* in, float* out, const float* w_packed, const float* scale,
                     const float* shift, const float* skip, int Cin, int Cout, int D, int H, int W,
                     int mode, int kdepth, int flags, dmvs_stream_t stream);

/* Introspection (tests, tooling): which workgroup tile dmvs_conv3d_mfma would launch for this layer and input size.
 * Returns TZ * 256 + TY (tile rows along depth / height; every tile is 32 voxels wide), bit 16 set when the 16-byte
 * tile loader is eligible (W % 4 == 0; it additionally needs a 16-byte aligned input), bit 17 for the M-block-split
 * variant of a two-block (Cout = 64) layer on a small volume, or DMVS_EUNSUPPORTED.  The
 * big tiles (TY >= 8 for 3D stride-1, >= 4 for 3D stride-2, 16 / 8 for per-slice layers) are the ones the full-size
 * configs run; the parity tests use this to prove they exercise them. */
int dmvs_conv3d_mfma_plan(int Cin, int Cout, int D, int H, int W, int mode, int kdepth);

/* K3w: the stride-1 3x3(x3) layers of K3 in Winograd F(2x2, 3x3) form on the same fp32 matrix cores
 * (csrc/conv3d_wino.hip): 2.25x fewer multiplies than the direct form, fp32 inputs / products / sums, result equal to
 * dmvs_conv3d_mfma's at re-association level.  Same operator and layouts as dmvs_conv3d_mfma(mode DMVS_CONV_S1) without
 * residual:  out = relu(conv(in) * scale + shift)  (module.py:120-157; layers module.py:364, 367, 370, 406, 409, 412
 * and FeatureNet's module.py:291-292, 296-297, 309-310).  flags: DMVS_RELU, DMVS_OUT_Q4.
 *   w_packed: dmvs_pack_conv_weights_wino (host) -- G g G^T of every (cout, cin, kz) filter, formed in double, in the
 *   kernel's consumption order; dmvs_conv3d_wino_weight_floats gives its length, 0 for a layer shape not compiled.
 * Needs W % 4 == 0 and 16-byte aligned in / out, otherwise DMVS_EUNSUPPORTED (the caller then runs dmvs_conv3d_mfma). */
int dmvs_conv3d_wino(const float* in, float* out, const float* w_packed, const float* scale, const float* shift,
                     int Cin, int Cout, int D, int H, int W, int kdepth, int flags, dmvs_stream_t stream);
/* Introspection / dispatch policy: the number of workgroups dmvs_conv3d_wino would launch for this layer and input size
 * (the host uses it to leave volumes of a few dozen workgroups to dmvs_conv3d_mfma), or DMVS_EUNSUPPORTED. */
int dmvs_conv3d_wino_plan(int Cin, int Cout, int D, int H, int W, int kdepth);
long dmvs_conv3d_wino_weight_floats(int Cin, int Cout, int kdepth);
int dmvs_pack_conv_weights_wino(const float* w /* [Cout][Cin][kd][3][3] */, float* out, int Cin, int Cout, int kdepth);

/* K3r: the coarse-level stride-1 3x3(x3) layers -- conv4 (32 -> 32) and conv6 (64 -> 64) of CostRegNet_part / _part_refine
 * (module.py:367, 370, 409, 412; Conv3d / Conv2d + BatchNorm(eval) + ReLU, module.py:120-157) and their 2D forms (kdepth 1:
 * the refine nets' bottleneck, and the middle 3x3 slice of a 3D layer on a depth-1 volume) -- in Winograd F(2x2, 3x3) form
 * with REGISTER-STATIONARY filters (csrc/conv3d_coarse.hip): 256 persistent 512-thread workgroups, each wave keeps its
 * share of G g G^T in VGPRs for the whole launch and walks 8 x 8-output groups of the volume; input tiles through a ring of
 * LDS stages.  Same operator, layouts and fp32 arithmetic as dmvs_conv3d_wino without DMVS_OUT_Q4 / residual:
 *   out = relu(conv(in) * scale + shift), in [Cin][D][H][W], out [Cout][D][H][W].  flags: DMVS_RELU.
 *   w_packed: dmvs_pack_conv_weights_coarse (host); dmvs_conv3d_coarse_weight_floats = its length, 0 for a shape not compiled
 *   ((32,32) and (64,64), kdepth 3 or 1).  Any W (W % 4 != 0 or an unaligned base: dword tile loads).
 * DMVS_EUNSUPPORTED: shape not compiled or a tensor of >= 2^29 elements (the caller then runs dmvs_conv3d_wino / _mfma). */
int dmvs_conv3d_coarse(const float* in, float* out, const float* w_packed, const float* scale, const float* shift,
                       int Cin, int Cout, int D, int H, int W, int kdepth, int flags, dmvs_stream_t stream);
long dmvs_conv3d_coarse_weight_floats(int Cin, int Cout, int kdepth);
int dmvs_pack_conv_weights_coarse(const float* w /* [Cout][Cin][kd][3][3] */, float* out, int Cin, int Cout, int kdepth);

/* K3z: conv2 of the regularisation nets (module.py:364, 406: Conv3d 16 -> 16, 3x3x3, stride 1) in Winograd F(2x2, 3x3) form with
 * register-stationary filters, marching along z (csrc/conv3d_zmarch.hip): a 256-thread workgroup = the 4 transform rows, each
 * wave keeps its share of G g G^T for all 3 depth taps in VGPRs; one pipeline stage = one input plane of an 8 x 8-output column,
 * transformed once and used as depth tap 0 / 1 / 2 of three output planes; 2 persistent workgroups per CU.
 *   out = relu(conv(in) * scale + shift), in [16][D][H][W], out [16][D][H][W].  flags: DMVS_RELU.
 *   w_packed: dmvs_pack_conv_weights_zmarch (host); dmvs_conv3d_zmarch_weight_floats = its length, 0 for a shape not compiled
 *   (only (16, 16, kdepth 3)).  Needs W % 4 == 0 and 16-byte aligned tensors.
 * DMVS_EUNSUPPORTED: shape / alignment not covered or >= 2^29 elements (the caller then runs dmvs_conv3d_wino / _mfma). */
int dmvs_conv3d_zmarch(const float* in, float* out, const float* w_packed, const float* scale, const float* shift,
                       int Cin, int Cout, int D, int H, int W, int kdepth, int flags, dmvs_stream_t stream);
long dmvs_conv3d_zmarch_weight_floats(int Cin, int Cout, int kdepth);
int dmvs_pack_conv_weights_zmarch(const float* w /* [Cout][Cin][3][3][3] */, float* out, int Cin, int Cout, int kdepth);

/* K3b -- a PROBE outside the product path (csrc/conv3d_split.hip): conv1 of the regularisation nets
 * (module.py:363, 405: Conv3d 8 -> 16, 3x3x3, stride 2, BN + ReLU) with the fp32 operands split into bf16 terms
 * (x = h + m + l exactly) and multiplied on v_mfma_f32_16x16x32_bf16 with fp32 accumulation: terms = 6 keeps hh + hm + mh + hl +
 * mm + lh (emulated fp32: error of the order of fp32 rounding), terms = 3 keeps hh + hm + mh (2^-16).
 *   in [8][D][H][W] -> out [16][(D+1)/2][(H+1)/2][(W+1)/2] = relu(conv(in) * scale + shift); flags: DMVS_RELU.
 *   w_split: dmvs_pack_conv_weights_split of the weight [16][8][3][3][3] (dmvs_conv3d_split_weight_floats 32-bit words of raw
 *   bf16 pairs; 0 for any other (Cin, Cout)).  Never selected by the product's dispatch. */
int dmvs_conv3d_split_probe(const float* in, float* out, const float* w_split, const float* scale, const float* shift,
                            int D, int H, int W, int terms, int flags, dmvs_stream_t stream);
long dmvs_conv3d_split_weight_floats(int Cin, int Cout);
int dmvs_pack_conv_weights_split(const float* w, float* out, int Cin, int Cout);

/* K3s: FeatureNet's two full-resolution layers (module.py:283-286: conv0 = Conv2d(3 -> 8) + Conv2d(8 -> 8), 3x3, stride 1,
 * pad 1, BN + ReLU) as a register-only row sweep on v_mfma_f32_4x4x1_16b_f32 (csrc/conv2d_c8.hip): with 8 output channels
 * the 16-row MFMA of dmvs_conv3d_mfma runs half empty; here one issue is 4 output channels x 64 pixels, a wave walks a
 * 62-pixel column strip down the image with the stencil's three rows in registers -- no LDS, no barrier.
 *   out[8][V][H][W] = relu(conv3x3(in) * scale + shift);  in: [Cin][V][H][W] planar, or with DMVS_IN_VIEWS (Cin = 3 only)
 *   the loader's image stack [V][3][H][W] read in place.  Cin in {3, 8}; flags: DMVS_RELU, DMVS_IN_VIEWS.
 *   w_packed: dmvs_pack_conv_weights_c8 of the nn.Conv2d weight [8][Cin][3][3] (dmvs_conv2d_c8_weight_floats floats; 0 for
 *   a Cin not compiled).  DMVS_EUNSUPPORTED beyond 2^28 output elements (the caller then runs dmvs_conv3d_mfma). */
int dmvs_conv2d_c8(const float* in, float* out, const float* w_packed, const float* scale, const float* shift,
                   int Cin, int V, int H, int W, int flags, dmvs_stream_t stream);
/* ... and both layers in ONE sweep (module.py:283-286 as a whole): out[8][V][H][W] = conv0.1(conv0.0(imgs)), the 8-channel
 * intermediate kept in registers (never stored: 2 x 303 MB per depth map at config 2).  imgs: the loader's [V][3][H][W] stack;
 * w0 / w1: dmvs_pack_conv_weights_c8 of the two weights (Cin = 3, 8); scale / shift: folded BN of each layer (required); both
 * layers end in ReLU.  Same result as two dmvs_conv2d_c8 calls, bit for bit. */
int dmvs_featurenet_conv0(const float* imgs, float* out, const float* w0_packed, const float* scale0, const float* shift0,
                          const float* w1_packed, const float* scale1, const float* shift1, int V, int H, int W,
                          dmvs_stream_t stream);
long dmvs_conv2d_c8_weight_floats(int Cin);
int dmvs_pack_conv_weights_c8(const float* w /* [8][Cin][3][3] */, float* out, int Cin);

/* FeatureNet's level-3 top-down merge (module.py:333-336) as ONE Winograd convolution (csrc/conv3d_wino.hip,
 * fpn_wino_kernel):  out = conv3x3(intra),  intra[k] = b_lat[k] + sum_j w_lat[k][j] * lat[j] + td[k] upsampled x2 (nearest),
 * zero padded -- inner2 (1x1 lateral conv + bias), the x2 upsample + add and out3 in one kernel; the 32-channel
 * full-resolution `intra` tensor is never formed.  The 1x1 lateral conv and its bias are folded into composite 3x3 filters
 * on the host (the bias as a filter on a constant-one image, so that it does not leak into the zero padding), and the
 * x2-upsampled top-down tensor needs only 9 of the 16 transform positions.  kdepth = 1 layout: lat [8][D][H][W],
 * td [32][D][H/2][W/2], out [16][D][H][W] (or its DMVS_OUT_Q4 halves).  Compiled for (Cl, Cin, Cout) = (8, 32, 16);
 * H even, W % 8 == 0, 16-byte aligned tensors, otherwise DMVS_EUNSUPPORTED (the caller then runs inner2 and out3 as two
 * layers; r01-r03's VALU-built fused variants dmvs_conv3d_mfma_fpn / dmvs_conv3d_wino_fpn were removed in r04).
 *   w_packed: dmvs_pack_conv_weights_wino_fpn(w3 [16][32][3][3], w_lat [32][8], b_lat [32]) -- length
 *   dmvs_conv3d_wino_fpn_weight_floats(); ones_hw: H*W floats of 1.0 on the device. */
int dmvs_conv3d_wino_fpn2(const float* lat, const float* td, const float* ones_hw, float* out, const float* w_packed,
                          const float* scale, const float* shift, int D, int H, int W, int flags, dmvs_stream_t stream);
long dmvs_conv3d_wino_fpn_weight_floats(void);
int dmvs_pack_conv_weights_wino_fpn(const float* w3, const float* w_lat, const float* b_lat, float* out);

/* number of floats dmvs_conv3d_mfma expects in w_packed for a layer (host helper). */
long dmvs_conv3d_mfma_weight_floats(int Cin, int Cout, int mode, int kdepth);
/* host-side packing: w is the PyTorch weight ([Cout][Cin][kd][3][3], or [Cin][Cout][kd][3][3]
 * for DECONV), kd = kdepth.  Both pointers are HOST pointers. */
int dmvs_pack_conv_weights_mfma(const float* w, float* w_packed, int Cin, int Cout, int mode, int kdepth);

/* K4: dual-depth regression.  Replaces DepthNet.forward (mvsnet.py:15-66) when mode = 0 and
 * DepthNet.refine (mvsnet.py:67-100) when mode = 1; softmax over D of alpha*logits, expectation,
 * min/max of the (small, huge) pairs, checkerboard selection, confidence.
 *   logits_4dhw [4][D][H][W]; depth_dhw [D][H][W]; interval [1] (device scalar)
 *   dsp_4hw     [4][H][W]   depth_sub_plus
 *   sel         mode 0: [4][H][W] refine hypotheses (depth_values_c); mode 1: [H][W] final depth
 *   conf_hw     [H][W] photometric confidence
 *   prob_4dhw   optional [4][D][H][W] softmax volume (training / parity only), may be NULL */
int dmvs_depth_regress(const float* logits_4dhw, const float* depth_dhw, const float* interval,
                       float alpha, int mode, int D, int H, int W, float* dsp_4hw, float* sel,
                       float* conf_hw, float* prob_4dhw, dmvs_stream_t stream);

/* `prob` -> K4 in one kernel for the passes whose volume one workgroup can hold (r06; module.py:379, 397 + mvsnet.py:19-20,
 * 68-69): the branch's `prob` head (Conv3d 8 -> 2, as dmvs_conv3d_direct runs it) followed by the softmax over D of alpha * logits
 * and the depth expectation of its two channels -- the [2][D][H][W] logits are never written.  The same operations in the same order
 * as dmvs_conv3d_direct + dmvs_depth_regress: bit-identical expectations.
 *   in [Cin][D][H][W]; w_packed as for dmvs_conv3d_direct (Cout = 2); hyp_dhw [D][H][W], or NULL: plane d = base_hw + d * step[0]
 *   dsp_2hw [2][H][W]: the branch's slice of depth_sub_plus (small: channels 0-1, huge: 2-3)
 * D must be 4 or 8, W % 4 == 0, `in` 16-byte aligned, Cin even and <= 16; otherwise DMVS_EUNSUPPORTED (callers fall back to the two
 * kernels). */
int dmvs_prob_regress(const float* in, const float* w_packed, int Cin, int D, int H, int W, const float* hyp_dhw,
                      const float* base_hw, const float* step, float alpha, float* dsp_2hw, dmvs_stream_t stream);
/* ... and K4's remainder on the four expectations (mvsnet.py:22-61 mode 0, 72-97 mode 1): min / max of the (small, huge) pairs,
 * checkerboard selection, confidence.  dsp_4hw [4][H][W] in; sel / conf_hw as dmvs_depth_regress. */
int dmvs_depth_select(const float* dsp_4hw, const float* interval, int mode, int H, int W, float* sel, float* conf_hw,
                      dmvs_stream_t stream);

/* K4 on affine hypotheses: depth_dhw is replaced by base_hw [H][W]; plane d = base + d * interval[0]. */
int dmvs_depth_regress_affine(const float* logits_4dhw, const float* base_hw, const float* interval,
                              float alpha, int mode, int D, int H, int W, float* dsp_4hw, float* sel,
                              float* conf_hw, float* prob_4dhw, dmvs_stream_t stream);

/* K4b: backward of dmvs_depth_regress (csrc/depth_regress_bwd.h; host side dmvsnet_amd/head.py).  The softmax is recomputed from the
 * logits in the forward's operation order (nothing but logits, hypotheses and dsp is kept from the forward), and min / max route to
 * the channel the forward selected, read off the forward's dsp_4hw.
 *   logits_4dhw, hyp_dhw, alpha, mode, D, H, W   as the forward call (hypotheses as a volume; the affine form has no backward)
 *   dsp_4hw      [4][H][W] the forward's expectations E
 *   g_dsp_4hw    [4][H][W] upstream gradient on depth_sub_plus, or NULL
 *   g_sel        upstream gradient on the selection -- mode 0: [4][H][W] (depth_values_c), mode 1: [H][W] (depth) -- or NULL;
 *                at least one of g_dsp_4hw, g_sel is required.  G[c] = g_dsp[c] + what g_sel sends to channel c through the eight
 *                (mode 0, mvsnet.py:33-56) or four (mode 1, mvsnet.py:80-91) checkerboard cases and (min, max) of the pair.
 *   g_logits_4dhw [4][D][H][W] out: alpha * p[c][d] * (hyp[d] - E[c]) * G[c], p = softmax_d(alpha * logits[c])
 *   g_hyp_dhw    [D][H][W] out or NULL: ((p[0][d] G[0] + p[1][d] G[1]) + p[2][d] G[2]) + p[3][d] G[3]
 * The confidence is computed under no_grad in the reference and has no gradient.  Plain stores, one writer per element: bitwise
 * reproducible.  1 <= D <= 64, above: DMVS_EUNSUPPORTED; any H, W. */
int dmvs_depth_regress_backward(const float* logits_4dhw, const float* hyp_dhw, float alpha, int mode, int D, int H, int W,
                                const float* dsp_4hw, const float* g_dsp_4hw, const float* g_sel, float* g_logits_4dhw,
                                float* g_hyp_dhw, dmvs_stream_t stream);

/* N4: geometric-consistency check of one (reference, source) depth-map pair -- the inner step of the fusion
 * filter.  Replaces reproject_with_depth_pytorch + check_geometric_consistency (filter/pcd.py:151-242).
 *   depth_ref, depth_src [H][W]; proj33: 33 floats folded on the host from the two cameras:
 *     [0..11]  A1, b1: K_src*xyz_src = A1*(x,y,1)*d_ref + b1          (A1 = K_s R_rel K_r^-1, b1 = K_s t_rel)
 *     [12..23] A2, t2: xyz_reprojected = A2*(xs,ys,1)*d_sampled + t2  (A2 = R_rel^-1.. K_s^-1, in the ref camera)
 *     [24..32] K_ref
 *   pixel kept iff |reprojection - pixel| < dist_thresh and |d_reproj - d_ref| / d_ref < rel_thresh.
 *   mask [H][W] u8 and depth_reproj [H][W] (0 where rejected) are written; vote_sum [H][W] i32 and depth_sum
 *   [H][W] are ACCUMULATED (the per-pixel sums filter_depth builds over the source views, pcd.py:283-300).
 *   Any of the four outputs may be NULL. */
int dmvs_geo_consistency(const float* depth_ref, const float* depth_src, const float* proj33, int H, int W,
                         float dist_thresh, float rel_thresh, unsigned char* mask, float* depth_reproj,
                         int* vote_sum, float* depth_sum, dmvs_stream_t stream);

/* N4, dynamic-threshold variant (filter/dypcd_tanks.py:164-184, the Tanks&Temples filter): the same reprojection,
 * judged by nine gates  dist < i * dist_base  and  |d_reproj - d_ref| / d_ref < i * rel_base,  i = 2..10.
 *   level_votes [9][H][W] i32, ACCUMULATED: gate i adds to level_votes[i-2] (geo_mask_sums, dypcd_tanks.py:236-252)
 *   mask / depth_reproj / vote_sum / depth_sum: as in dmvs_geo_consistency, for the last gate (i = 10)
 * Zero reference depths are not patched here (the reference divides by them: every gate is false).  Outputs may be NULL. */
int dmvs_geo_consistency_ladder(const float* depth_ref, const float* depth_src, const float* proj33, int H, int W,
                                float dist_base, float rel_base, int* level_votes, unsigned char* mask,
                                float* depth_reproj, int* vote_sum, float* depth_sum, dmvs_stream_t stream);

/* N4, scan-level fusion (fusion.ScanFusion): one launch per reference view against all of its sources.
 *   DMVS_FUSE_MAX_SRC sources at most (10 for the dynamic variant: its geo mask reads the nine gates up to i = nsrc).
 *   dmvs_fuse_workgroups(H, W): number of workgroups of both launches = the length of `counts` (offsets: + 1).
 *   dmvs_fuse_view: depth_ref, conf3 / conf2 / conf1 [H][W] (pass conf3 for a missing stage map); depth_src: a HOST
 *     array of nsrc device pointers; proj33: a HOST array of nsrc x 33 floats (fusion.fold_projection per pair, in pair
 *     order).  Per pixel, with the per-pair arithmetic of dmvs_geo_consistency(_ladder) (gates dist / rel; the ladder's
 *     bases when dynamic) accumulated in registers:
 *       photo = conf3 > t3 && conf2 > t2 && conf1 > t1
 *       geo   = votes >= thres_view (static) | votes >= nsrc + 1 || any_{i=2..nsrc} level[i-2] >= i (dynamic)
 *       masks [3][H][W] u8: photo, geo, photo && geo as 0 / 255
 *       depth_avg [H][W] = (float)avg, depth_avg64 [H][W] = avg at final pixels only, where
 *       avg = (double)(sum + d_base) / (double)(votes + 1), d_base = 1e-4f for a zero depth (static), else the depth
 *     counts [workgroups] i32: final pixels per workgroup.
 *   dmvs_fuse_emit: offsets [workgroups + 1] i32 (exclusive scan of counts; offsets[workgroups] = total) and the world
 *     points xyz [total][3] fp32 of the final pixels in row-major order: Einv . [Kinv . (x d, y d, d); 1] in fp64 with
 *     kinv9 / einv16 HOST arrays (row-major), rounded to fp32.  xyz must hold H * W points (the total is not known on
 *     the host when the launch is enqueued). */
#define DMVS_FUSE_MAX_SRC 16
long dmvs_fuse_workgroups(int H, int W);
int dmvs_fuse_view(const float* depth_ref, const float* conf3, const float* conf2, const float* conf1, int H, int W,
                   int nsrc, const float* const* depth_src, const float* proj33, float t1, float t2, float t3,
                   int dynamic, int thres_view, float dist, float rel, unsigned char* masks, float* depth_avg,
                   double* depth_avg64, int* counts, dmvs_stream_t stream);
int dmvs_fuse_emit(const unsigned char* masks, const double* depth_avg64, const int* counts, int H, int W,
                   const double* kinv9, const double* einv16, int* offsets, float* xyz, dmvs_stream_t stream);

/* N5: DTU point-cloud evaluation (csrc/cloud_eval.h, host side dmvsnet_amd/cloud_eval.py) -- accuracy / completeness of a fused
 * cloud against the scanned reference cloud; replaces the arithmetic of scripts/evaluation_dtu/*.m.  Clouds are [n][3] fp32;
 * every difference and distance is fp64 (dx*dx + dy*dy + dz*dz in that order, unfused, compared squared, one sqrt at the end).
 * origin3 / dims3 / bb0 / lo3 / hi3 / plane4 / mask_dims3 are HOST arrays.
 *
 * dmvs_cloud_cell_keys: keys [n] i64 = (iz * ny + iy) * nx + ix of the cell floor((p - origin) / cell) per axis (x fastest), or
 *   INT64_MAX outside the grid.  DMVS_EINVAL when an axis has more than 2^21 cells.  The caller sorts the cloud by key; its
 *   occupied cells are the sorted unique keys ukeys [M] with ustart [M + 1] i32 the first point of each.
 * dmvs_cloud_cell_runs: runs [M][9][2] i32 = the point ranges [begin, end) of the nine x-runs of every occupied cell's 27-cell
 *   neighbourhood (the candidates of rangesearch, reducePts_haa.m:21; one binary search per run and cell).
 * dmvs_cloud_thin_round: one sweep of the thinning loop reducePts_haa.m:23-29 written as a fixed-point iteration with the same
 *   result.  state [n] u8: 0 undecided / 1 kept / 2 removed; prio [n] i32 = position in the visit order (RandOrd,
 *   reducePts_haa.m:9); cell_of [n] i32 = occupied cell of each (key-sorted) point; todo [n_todo] i32 the points to visit, or
 *   NULL: all of 0 .. n_todo - 1.  An undecided point is removed when an earlier neighbour (distance <= dst) is kept, kept when
 *   every earlier neighbour is removed.  remaining [1] i32 is INCREASED by the number of points left undecided.  The grid's
 *   cell must be >= dst * (1 + 1e-6).
 * dmvs_cloud_nn: one pass of the bounded nearest neighbour that MaxDistCP.m:31-33 computes block by block, on one grid level:
 *   to_xyz key-sorted with ukeys / ustart; queries q_xyz[q_idx[k]], k < nq (q_idx NULL: k), which must lie inside the grid.
 *   Rings of cells outwards, at most `rings`; best2 [N_from] f64 (in / out, +inf at the start) and nn [N_from] i32 (in / out,
 *   optional) carry the best squared distance / its point to the next, coarser level; resolved [nq] u8 = 1 when no unexamined
 *   point can be nearer or the searched radius reached max_dist, and then dist [N_from] f64 = min(sqrt(best2), max_dist).
 *   examined: NULL or one u64 counter of distances evaluated.
 * dmvs_cloud_in_mask: DataInMask, PointCompareMain.m:33-42: v = floor((p - bb0) / res + 1 + 0.5) (MATLAB's round on every value
 *   that can land in range), 1 <= v <= mask_dims and mask[vx - 1][vy - 1][vz - 1] != 0 (u8 volume, z fastest).
 * dmvs_cloud_above_plane: StlAbovePlane, PointCompareMain.m:54: p0 x + p1 y + p2 z + p3 > 0.
 * dmvs_cloud_in_box: the from-points MaxDistCP.m:10-18 searches at all: lo <= p < hi on every axis. */
int dmvs_cloud_cell_keys(const float* xyz, int n, const double* origin3, double cell, const int* dims3, long long* keys,
                         dmvs_stream_t stream);
int dmvs_cloud_cell_runs(const long long* ukeys, const int* ustart, int M, const int* dims3, int* runs, dmvs_stream_t stream);
int dmvs_cloud_thin_round(const float* xyz, const int* prio, const int* cell_of, const int* runs, unsigned char* state,
                          const int* todo, int n_todo, double dst, int* remaining, dmvs_stream_t stream);
int dmvs_cloud_nn(const float* to_xyz, const long long* ukeys, const int* ustart, int M, const double* origin3, double cell,
                  const int* dims3, const float* q_xyz, const int* q_idx, int nq, int rings, double max_dist, double* best2,
                  int* nn, double* dist, unsigned char* resolved, unsigned long long* examined, dmvs_stream_t stream);
int dmvs_cloud_in_mask(const float* xyz, int n, const double* bb0, double res, const unsigned char* mask, const int* mask_dims3,
                       unsigned char* out, dmvs_stream_t stream);
int dmvs_cloud_above_plane(const float* xyz, int n, const double* plane4, unsigned char* out, dmvs_stream_t stream);
int dmvs_cloud_in_box(const float* xyz, int n, const double* lo3, const double* hi3, unsigned char* out, dmvs_stream_t stream);

/* N6: validation mode (csrc/validate.h, host side dmvsnet_amd/validate.py) -- one stage of the dual-depth regression loss and / or
 * the depth metrics against ground truth, in two launches (the fused pass and a one-workgroup finishing kernel).  Replaces the
 * arithmetic of loss.py:5-80 (mvs_loss, mode "regression"), loss.py:106-159 (Monte_Carlo_sampling_loss mode "center",
 * regression_loss) and tools.py:159-201 (AbsDepthError_metrics, Thres_metrics).  Unlike the entries above it takes a batch.
 *   dsp_main, dsp_refine [B][4][h][w] (depth_sub_plus, depth_sub_plus_refine), both or neither (NULL: metrics only);
 *   gt, mask [B][h][w], a pixel is valid iff mask > 0.5; depth [B][h][w] or NULL (NULL: loss only); weight: the stage's dlossw;
 *   thres3: HOST array of the three error thresholds (needed with depth).
 *   Per-element terms are fp32 in the reference's operation order, sl1(d) = |d| < 1 ? 0.5 d d : |d| - 0.5, term = sl1 * weight;
 *   invalid pixels and 2x2 cells (any corner invalid) are selected out, never multiplied by zero; sums are fp64, added in a fixed
 *   order, each mean rounded to fp32 once; cells do not straddle images; the cell centre is (((nw + ne) + sw) + se) * 0.25.
 *   total_loss [1]: += ((2 m0 + 2 m1) + m2 + m3 + (((m4 + m5) + m6) + m7)) of the main outputs, then of the refine outputs, fp32,
 *     with terms16 [2][8] = m0..m7: mean over 2n of channels {0,1}, of {2,3}; var small, var huge over n; the four centre terms over
 *     n_cells (surfaces where(cm, min, max), where(~cm, min, max) of channels {0,1}, then of {2,3}; cm = row % 2 == col % 2).
 *     An empty mask gives NaN.  counts2 [2] i64: n, n_cells.  At least one of the three is required with dsp_*.
 *   image_sums [B][5] f64: sum |depth - gt|, n_valid, n with |depth - gt| > thres3[0..2] per image; metrics4 [4]: the batch means
 *     of (abs error, the three rates), an empty image counting 0.  At least one of the two is required with depth.
 *   workspace: dmvs_dual_depth_loss_workspace(B, h, w) doubles (one row per workgroup), overwritten.
 * DMVS_EINVAL on h < 2, w < 2, B < 1 or a missing pointer. */
long dmvs_dual_depth_loss_workspace(int B, int h, int w);
int dmvs_dual_depth_loss(const float* dsp_main, const float* dsp_refine, const float* gt, const float* mask, const float* depth,
                         int B, int h, int w, float weight, const float* thres3, double* workspace, float* total_loss,
                         float* terms16, long long* counts2, double* image_sums, float* metrics4, dmvs_stream_t stream);

/* N6b: backward of the loss of dmvs_dual_depth_loss: g_dsp_* = g_total[0] * d total_loss / d dsp_*, every term as the forward defines
 * it (the doubled smooth-L1 depth terms; the two "variance" terms, through both arguments: var_gt depends on the estimate; the four
 * cell-centre terms with exact quarter weights over the cells whose four corners are valid).  A gather: a pixel collects its own
 * terms and a quarter of each of the up to four cells it is a corner of, each divided by the forward's count.
 *   dsp_main, dsp_refine, gt, mask, B, h, w, weight   as the forward call
 *   counts2 [2] i64 (device): n, n_cells as the forward wrote them;  g_total [1] (device): upstream gradient on the total
 *   g_dsp_main, g_dsp_refine [B][4][h][w] out, one of them may be NULL (skipped); fully overwritten.
 * Masked pixels get exactly 0 (selected, never multiplied): NaN under the mask does not leak; with an empty mask (forward: NaN) the
 * gradient is all zeros.  No atomics: bitwise reproducible. */
int dmvs_dual_depth_loss_backward(const float* dsp_main, const float* dsp_refine, const float* gt, const float* mask, int B, int h,
                                  int w, float weight, const long long* counts2, const float* g_total, float* g_dsp_main,
                                  float* g_dsp_refine, dmvs_stream_t stream);

/* K3g: weight gradient of the stride-1 3x3(x3) pad-1 square convolutions on the fp32 matrix cores (csrc/conv3d_wgrad.h,
 * docs/kernels/K3g_conv_wgrad.md) -- what autograd computes for the weight of the reference's Conv3d / Conv2d blocks
 * (networks/module.py:28-70, 142) on conv2 / conv4 / conv6, the 2D conv6 and FeatureNet's conv1.1 / 1.2 / 2.1 / 2.2.
 * (Their data gradient is dmvs_conv3d_mfma itself on the weight transposed in (co, ci) and flipped in every tap.)
 *   x, gy      [C][D][H][W]: the layer's input and the gradient on its output
 *   gw         [C][C][kdepth][3][3] out (nn.Conv3d / nn.Conv2d layout):
 *              gw[co][ci][kz][ky][kx] (+)= sum_{z,y,x} gy[co][z][y][x] * x[ci][z+kz-1][y+ky-1][x+kx-1], zero outside the volume
 *   workspace  dmvs_conv3d_wgrad_workspace(...) floats; partial sums, fully overwritten where read
 *   accumulate 0: gw is overwritten; 1: the sum is added to gw (a batch runs as its samples one after the other)
 * C in {16, 32, 64}, kdepth 3 or 1 (1: no z taps, D independent slices), else DMVS_EUNSUPPORTED; null pointers, empty sizes or more than
 * 2^22 tiles: DMVS_EINVAL.  Two launches (partials, then their sum in a fixed order); no atomics: bitwise reproducible. */
int dmvs_conv3d_wgrad(const float* x, const float* gy, float* gw, float* workspace, int C, int D, int H, int W, int kdepth,
                      int accumulate, dmvs_stream_t stream);
/* Workspace of dmvs_conv3d_wgrad in floats: one partial [9 * kdepth][C][C] per voxel share, 256 / (C / 32)^2 shares at most -- it does
 * not depend on the volume.  0 for a shape the kernel is not compiled for. */
long dmvs_conv3d_wgrad_workspace(int C, int D, int H, int W, int kdepth);
/* Host only: the launch dmvs_conv3d_wgrad will make, as tiles * 512 + workgroups.  tiles = D * ceil(H / 4) * ceil(W / 32) voxel tiles
 * of 1 x 4 x 32; workgroups = the size of the first launch's grid (a multiple of 8, at most 256); workgroups past
 * min(tiles, 256 / blocks) * blocks, blocks = (C / 32)^2 or 1, exit at once and own no partial.  Negative DMVS_E* as dmvs_conv3d_wgrad. */
int dmvs_conv3d_wgrad_plan(int C, int D, int H, int W, int kdepth);

/* K3h: weight gradient of the stride-2 and the transposed 3x3(x3) convolutions (kernel 3, stride 2, padding 1; transposed:
 * output_padding 1) on the fp32 matrix cores (csrc/conv3d_wgrad_s2.h, docs/kernels/K3h_conv_wgrad_s2.md) -- what autograd computes
 * for the weight of conv1 / 3 / 5 and conv7 / 9 / 11 of the regularisation U-Nets and the 2D conv5 / conv7 of the refine net.
 * (Their data gradient is dmvs_conv3d_mfma in the OTHER stride-2 mode on the same weight tensor.)
 *   coarse     [Ca][Dc][Hc][Wc]: the gradient on a stride-2 conv's output, or the input of a transposed conv
 *   fine       [Ca / 2][Df][2 Hc][2 Wc], Df = 2 Dc (kdepth 3) or Dc (kdepth 1): the conv's input, or the gradient on the transposed
 *              conv's output
 *   gw         [Ca][Ca / 2][kdepth][3][3] out -- nn.Conv3d's [out][in] and nn.ConvTranspose3d's [in][out] alike:
 *              gw[a][b][kz][ky][kx] (+)= sum_{z,y,x} coarse[a][z][y][x] * fine[b][2z+kz-1][2y+ky-1][2x+kx-1], zero outside `fine`
 *              (kdepth 1: plane z, no kz)
 *   workspace  dmvs_conv3d_wgrad_s2_workspace(...) floats; partial sums, fully overwritten where read
 *   accumulate 0: gw is overwritten; 1: the sum is added to gw (a batch runs as its samples one after the other)
 * (Ca, kdepth) in {(16, 3), (32, 3), (64, 3), (64, 1)}, else DMVS_EUNSUPPORTED; null pointers, empty sizes, an extent above 2^20 or more
 * than 2^22 tiles: DMVS_EINVAL.  Two launches (partials, then their sum in a fixed order); no atomics: bitwise reproducible. */
int dmvs_conv3d_wgrad_s2(const float* coarse, const float* fine, float* gw, float* workspace, int Ca, int Dc, int Hc, int Wc, int kdepth,
                         int accumulate, dmvs_stream_t stream);
/* Workspace of dmvs_conv3d_wgrad_s2 in floats: one partial [9 * kdepth][Ca][Ca / 2] per voxel share, 256 (Ca = 64: 128) shares at most
 * -- it does not depend on the volume.  0 for a shape the kernel is not compiled for. */
long dmvs_conv3d_wgrad_s2_workspace(int Ca, int Dc, int Hc, int Wc, int kdepth);
/* Host only: the launch dmvs_conv3d_wgrad_s2 will make, as tiles * 512 + workgroups.  tiles = Dc * ceil(Hc / TY) * ceil(Wc / 32) coarse
 * voxel tiles of 1 x TY x 32, TY = 4 (2 for Ca = 64, kdepth 3); workgroups = the size of the first launch's grid (a multiple of 8, at
 * most 256); workgroups past min(tiles, 256 / blocks) * blocks, blocks = 2 for Ca = 64, else 1, exit at once and own no partial.
 * Negative DMVS_E* as dmvs_conv3d_wgrad_s2. */
int dmvs_conv3d_wgrad_s2_plan(int Ca, int Dc, int Hc, int Wc, int kdepth);

/* K3k / K3d: weight and data gradient of FeatureNet's 5x5 stride-2 pad-2 2D convolutions conv1.0 (8 -> 16) and conv2.0 (16 -> 32)
 * (networks/module.py:289, :295) on the fp32 matrix cores (csrc/conv2d_k5s2_bwd.h, docs/kernels/K3k_conv_wgrad_k5s2.md) -- what
 * autograd computes behind DMVS_CONV2D_K5S2.  A sample is D independent planes (K3's kdepth-1 layout); Cb = Ca / 2,
 * Hc = (Hf + 1) / 2, Wc = (Wf + 1) / 2: even and odd fine extents.
 *   gy         [Ca][D][Hc][Wc]: the gradient on the layer's output;  x [Cb][D][Hf][Wf]: its input;  w [Ca][Cb][5][5]: nn.Conv2d's weight
 *   gw         [Ca][Cb][5][5] out: gw[a][b][ky][kx] (+)= sum_{z,y,x} gy[a][z][y][x] * x[b][z][2y+ky-2][2x+kx-2], zero outside `x`
 *   gx         [Cb][D][Hf][Wf] out, every element written once:
 *              gx[b][z][Y][X] = sum_{a,ky,kx : Y+2-ky = 2y, X+2-kx = 2x, 0 <= y < Hc, 0 <= x < Wc} gy[a][z][y][x] * w[a][b][ky][kx]
 *   workspace  dmvs_conv2d_k5s2_wgrad_workspace(...) floats; partial sums, fully overwritten where read
 *   accumulate 0: gw is overwritten; 1: the sum is added to gw (a batch runs as its samples one after the other)
 * Ca in {16, 32}, else DMVS_EUNSUPPORTED; null pointers, extents < 1 (or above 2^21) or 2^22 tiles and more: DMVS_EINVAL.  The weight
 * gradient is two launches (partials, then their sum in a fixed order), the data gradient one gather launch that reads `w` as it
 * lies; no atomics: both are bitwise reproducible. */
int dmvs_conv2d_k5s2_wgrad(const float* gy, const float* x, float* gw, float* workspace, int Ca, int D, int Hf, int Wf, int accumulate,
                           dmvs_stream_t stream);
int dmvs_conv2d_k5s2_dgrad(const float* gy, const float* w, float* gx, int Ca, int D, int Hf, int Wf, dmvs_stream_t stream);
/* Workspace of dmvs_conv2d_k5s2_wgrad in floats: one partial [25][Ca][Ca / 2] per share, 256 shares at most -- it does not depend on
 * the image.  0 for a shape the kernel is not compiled for or an extent < 1. */
long dmvs_conv2d_k5s2_wgrad_workspace(int Ca, int D, int Hf, int Wf);
/* Host only: the launch dmvs_conv2d_k5s2_wgrad will make, as tiles * 512 + workgroups.  tiles = D * ceil(Hc / 4) * ceil(Wc / 32) coarse
 * tiles of 1 x 4 x 32; workgroups = the size of the first launch's grid (a multiple of 8, at most 256); workgroups past
 * min(tiles, 256) exit at once and own no partial.  Negative DMVS_E* as dmvs_conv2d_k5s2_wgrad. */
int dmvs_conv2d_k5s2_wgrad_plan(int Ca, int D, int Hf, int Wf);

/* K3f: weight and bias gradient of FeatureNet's rectangular stride-1 2D convolutions on the fp32 matrix cores
 * (csrc/conv2d_wgrad_fpn.h, docs/kernels/K3f_conv_wgrad_fpn.md) -- what autograd computes for the weight of conv0.0 (3 -> 8, 3x3;
 * networks/module.py:284), conv0.1 (8 -> 8, 3x3; :285), out1 (32 -> 64, 1x1; :301), inner1 (16 -> 32, 1x1, bias; :305), inner2
 * (8 -> 32, 1x1, bias; :306) and out3 (32 -> 16, 3x3; :309), and for the bias of the two that have one.  A sample is D independent
 * planes (K3's kdepth-1 layout); ksize 3 means padding 1, ksize 1 padding 0; stride 1.
 * (Their forward is dmvs_conv3d_mfma in DMVS_CONV_S1 / DMVS_CONV2D_K1; their data gradient is the same entry on the layer Cout -> Cin
 * with the weight transposed in (co, ci) and flipped in every tap.)
 *   x          [Cin][D][H][W]: the layer's input;  gy [Cout][D][H][W]: the gradient on its output
 *   gw         [Cout][Cin][ksize][ksize] out (nn.Conv2d layout):
 *              gw[co][ci][ky][kx] (+)= sum_{d,y,x} gy[co][d][y][x] * x[ci][d][y+ky-ksize/2][x+kx-ksize/2], zero outside the plane
 *   gbias      [Cout] out or NULL: gbias[co] (+)= sum_{d,y,x} gy[co][d][y][x], from the same launch (one more GEMM column whose x value
 *              is the constant 1).  Only inner1 and inner2 take one; non-NULL for another layer: DMVS_EINVAL
 *   workspace  dmvs_conv2d_wgrad_fpn_workspace(...) floats; partial sums, fully overwritten where read
 *   accumulate 0: gw and gbias are overwritten; 1: the sums are added to them (a batch runs as its samples one after the other)
 * (Cin, Cout, ksize) in {(3,8,3), (8,8,3), (32,16,3), (32,64,1), (16,32,1), (8,32,1)}, else DMVS_EUNSUPPORTED; null pointers, extents
 * < 1 or 2^22 tiles and more: DMVS_EINVAL.  Any H, W >= 1.  Two launches (partials, then their sum in a fixed order); no atomics:
 * bitwise reproducible. */
int dmvs_conv2d_wgrad_fpn(const float* x, const float* gy, float* gw, float* gbias, float* workspace, int Cin, int Cout, int D, int H,
                          int W, int ksize, int accumulate, dmvs_stream_t stream);
/* Workspace of dmvs_conv2d_wgrad_fpn in floats: one partial [Cout][Cin * ksize * ksize (+ 1 for the bias column)] per share, 256 shares
 * at most -- it does not depend on D, H, W.  0 for a shape the kernel is not compiled for or an extent < 1. */
long dmvs_conv2d_wgrad_fpn_workspace(int Cin, int Cout, int ksize, int D, int H, int W);
/* Host only: the launch dmvs_conv2d_wgrad_fpn will make, as tiles * 512 + workgroups.  tiles = D * ceil(H / 4) * ceil(W / 32) tiles of
 * 1 x 4 x 32; workgroups = the size of the first launch's grid (a multiple of 8, at most 256); workgroups past min(tiles, 256) exit at
 * once and own no partial.  Negative DMVS_E* as dmvs_conv2d_wgrad_fpn. */
int dmvs_conv2d_wgrad_fpn_plan(int Cin, int Cout, int ksize, int D, int H, int W);

/* K2g: weight gradient of the 2-channel ends of the regularisation U-Nets, conv0 (2 -> 8) and `prob` (8 -> 2), 3x3x3, stride 1, pad 1
 * (csrc/conv3d_wgrad_c2.h, docs/kernels/K2g_conv_wgrad_c2.md) -- what autograd computes for the weight of the reference's conv0 block
 * and `prob` (networks/module.py:361, 379, 403, 421).  fp32 VALU, lane = voxel.
 * (Their forward and data gradient are dmvs_conv3d_direct: each one's data gradient has the other one's shape.)
 *   x          [Cin][D][H][W]: the layer's input;  gy [Cout][D][H][W]: the gradient on its output
 *   gw         [Cout][Cin][3][3][3] out (nn.Conv3d layout):
 *              gw[co][ci][kz][ky][kx] (+)= sum_{z,y,x} gy[co][z][y][x] * x[ci][z+kz-1][y+ky-1][x+kx-1], zero outside the volume
 *   workspace  dmvs_conv3d_wgrad_c2_workspace(...) floats; partial sums, fully overwritten where read
 *   accumulate 0: gw is overwritten; 1: the sum is added to gw (a batch runs as its samples one after the other)
 * (Cin, Cout) in {(2, 8), (8, 2)}, else DMVS_EUNSUPPORTED; null pointers, empty sizes or more than 2^22 tiles: DMVS_EINVAL.  Two launches
 * (partials, then their sum in a fixed order); no atomics: bitwise reproducible. */
int dmvs_conv3d_wgrad_c2(const float* x, const float* gy, float* gw, float* workspace, int Cin, int Cout, int D, int H, int W,
                         int accumulate, dmvs_stream_t stream);
/* Workspace of dmvs_conv3d_wgrad_c2 in floats: one partial [27][8][2] per voxel share, 256 shares at most -- it does not depend on the
 * volume.  0 for a shape the kernel is not compiled for. */
long dmvs_conv3d_wgrad_c2_workspace(int Cin, int Cout, int D, int H, int W);
/* Host only: the launch dmvs_conv3d_wgrad_c2 will make, as tiles * 512 + workgroups.  tiles = D * ceil(H / 4) * ceil(W / 64) voxel tiles
 * of 1 x 4 x 64; workgroups = the size of the first launch's grid (a multiple of 8, at most 256); workgroups past min(tiles, 256) exit
 * at once and own no partial.  Negative DMVS_E* as dmvs_conv3d_wgrad_c2. */
int dmvs_conv3d_wgrad_c2_plan(int Cin, int Cout, int D, int H, int W);

/* K5: BatchNorm + ReLU of the reference's Conv3d / Deconv3d / Conv2d / Deconv2d blocks (networks/module.py: `self.bn(...)`, then
 * `F.relu(x, inplace=True)`), forward and backward, train and eval mode (csrc/batchnorm.h, docs/kernels/K5_batchnorm_relu.md).
 *   x, y, gy, gx   [B][C][V] fp32, V = D * H * W (2D layers: H * W); the batch is handled inside the kernels
 *   gamma, beta, mean, invstd, running_mean, running_var, g_gamma, g_beta   [C]
 *   flags          DMVS_RELU: y = max(pre, 0) and the gradient is masked by [pre > 0]; DMVS_BN_TRAIN: batch statistics
 *   workspace      dmvs_bn_workspace(...) floats: per-share partial sums, fully overwritten where read
 * Forward, train: pre = fmaf(x - mean, invstd * gamma, beta) with mean and the BIASED variance of the B * V elements of a channel
 * (invstd = 1 / sqrt(var + eps)); mean / invstd are stored for the backward; running_mean = (1 - momentum) * running_mean + momentum *
 * mean, running_var likewise with the UNBIASED variance var * n / (n - 1).  Two launches (partial statistics; fold + apply).
 * Forward, eval: mean = running_mean, invstd = 1 / sqrt(running_var + eps) (both also stored to mean / invstd); the running buffers are
 * only read.  One launch.
 * Backward: g = gy * [pre > 0] with pre RECOMPUTED from x by the forward's own function (y is not an argument);
 * g_beta = sum g, g_gamma = sum g * xhat, xhat = (x - mean) * invstd; gx = gamma * invstd * (g - g_beta / n - xhat * g_gamma / n) in train
 * mode, gamma * invstd * g in eval mode.  gx may be NULL: g_gamma / g_beta alone.  Two launches.
 * The variance is formed from sums around a per-channel pivot (never E[x^2] - E[x]^2 of the raw values); partials are added in a fixed
 * order in fp64.  No atomics: bitwise reproducible.
 * DMVS_EINVAL: C not in {8, 16, 32, 64}, a null pointer (other than gx), B < 1, V < 1, B * V < 2 in train mode, B * V above 2^31 - 2^13,
 * unknown flag bits, momentum outside [0, 1], eps < 0. */
int dmvs_bn_relu_forward(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var, float* y,
                         float* mean, float* invstd, float* workspace, int B, int C, int V, float momentum, float eps, int flags,
                         dmvs_stream_t stream);
int dmvs_bn_relu_backward(const float* x, const float* gy, const float* gamma, const float* beta, const float* mean, const float* invstd,
                          float* gx, float* g_gamma, float* g_beta, float* workspace, int B, int C, int V, int flags,
                          dmvs_stream_t stream);
/* Workspace of the two in floats: [C][Smax][2] partials and [C] pivots, Smax = 2048 / C -- it does not depend on the volume.  0 for
 * arguments the kernels refuse. */
long dmvs_bn_workspace(int C, int B, int V);
/* Host only: the number of shares S = min(ceil(B * V / 1024), 2048 / C) every K5 launch cuts a channel into (grid: C * S workgroups of
 * 256 lanes; a chunk is 256 lanes x 4 floats).  DMVS_EINVAL as above. */
int dmvs_bn_plan(int C, int B, int V);
/* Host only: the range [*lo, *hi) of the flattened index b * V + v that share s of a channel owns -- the very function the kernels call.
 * Whole chunks [s * chunks / S, (s + 1) * chunks / S), the last one cut at B * V.  DMVS_EINVAL as above, and for s outside [0, S). */
int dmvs_bn_share_range(int C, int B, int V, int s, long* lo, long* hi);

/* K5, synchronised statistics: BatchNorm + ReLU in train mode over the batches of R ranks, the semantics of torch.nn.SyncBatchNorm
 * (which the reference's train.sh switches on with --sync_bn).  The two collectives are the caller's: each entry works on device buffers
 * and knows no process group.  Rank r holds x_r [B_r][C][V_r], n_r = B_r * V_r >= 1 values per channel; N = sum n_r >= 2.
 * Tensors, flags (DMVS_RELU only: there is no eval form) and workspace as above; moments / sums / gathered are fp64 device buffers.
 *
 * dmvs_bn_sync_moments: moments[C][3] = (n_r, mean_r, M2_r), M2_r = sum (x - mean_r)^2, from partial sums around the rank's own pivot p:
 * mean_r = p + f0 / n_r, M2_r = f1 - f0^2 / n_r with f0 = sum (x - p), f1 = sum (x - p)^2 folded in share order in fp64.  Moments travel
 * between ranks, never raw sums: pivots differ from rank to rank.  Two launches (partial statistics; fold, C workgroups).
 * dmvs_bn_sync_forward: gathered[R][C][3] is every rank's moments in rank order (all_gather_into_tensor of the above).  In the order
 * r = 0 .. R-1 in fp64: N = sum n_r, mean = sum n_r mean_r / N, M2 = sum (M2_r + n_r (mean_r - mean)^2), var = M2 / N;
 * y = relu(fmaf(x - mean, invstd * gamma, beta)), invstd = 1 / sqrt(var + eps); mean / invstd are stored; the running buffers are
 * blended with mean and M2 / (N - 1).  Every rank reads the same buffer in the same order: mean, invstd and the running buffers are the
 * same bits on all ranks.  *n_total (host) receives N.  The n_r are read back and checked on the host before the launch: the entry
 * synchronises the stream once.  One launch.
 * dmvs_bn_sync_backward_sums: g = gy * [pre > 0] on the global mean / invstd; sums[C][2] = this rank's (sum g, sum g * xhat) in fp64,
 * g_beta / g_gamma the same two in fp32 (the LOCAL sums, as the stock module leaves them for DDP to average).  Two launches.
 * dmvs_bn_sync_backward_apply: gathered[R][C][2] is every rank's sums in rank order; added in the order r = 0 .. R-1 in fp64;
 * gx = gamma * invstd * (g - sum_g / N - xhat * sum_gxhat / N).  One launch.  A caller that wants no gx calls the sums entry alone.
 * No atomics: bitwise reproducible.
 * DMVS_EINVAL: a null pointer, C not in {8, 16, 32, 64}, B < 1, V < 1, B * V above 2^31 - 2^13, unknown flag bits, R outside [1, 16],
 * momentum outside [0, 1], eps < 0, N < 2 (or below this rank's own B * V), a gathered n_r that is not a positive integer or differs
 * between the channels of a rank. */
int dmvs_bn_sync_moments(const float* x, double* moments, float* workspace, int B, int C, int V, dmvs_stream_t stream);
int dmvs_bn_sync_forward(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                         const double* gathered, float* y, float* mean, float* invstd, long* n_total, int B, int C, int V, int R,
                         float momentum, float eps, int flags, dmvs_stream_t stream);
int dmvs_bn_sync_backward_sums(const float* x, const float* gy, const float* gamma, const float* beta, const float* mean,
                               const float* invstd, double* sums, float* g_gamma, float* g_beta, float* workspace, int B, int C, int V,
                               int flags, dmvs_stream_t stream);
int dmvs_bn_sync_backward_apply(const float* x, const float* gy, const float* gamma, const float* beta, const float* mean,
                                const float* invstd, const double* gathered, float* gx, int B, int C, int V, int R, long N, int flags,
                                dmvs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DMVS_H */
