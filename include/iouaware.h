/*
 * iouaware.h -- C-ABI of the MI355X-native (gfx950) IoU-aware RetinaNet
 * post-conv hot path.  Shared library: libiouaware_hip.so (built by
 * iou-aware-single-stage-object-detector_amd/csrc/build.py with hipcc).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / ATen types.
 *   - every pointer is a DEVICE pointer unless the name ends in _host or the
 *     comment says "host"; `stream` is a hipStream_t passed as void*.
 *   - nothing is allocated: callers pass a workspace sized by the matching
 *     *_workspace_bytes() query.  Calls are asynchronous on `stream`.
 *   - return value: 0 = ok, negative = IA_E_* argument error, positive =
 *     hipError_t of a failed launch.
 *   - feature maps are (B, ch, H, W) tensors, dtype IA_F32 or IA_BF16, channel
 *     a*C+c (cls), a*4+k (reg), a (iou) -- the reference head's output
 *     (reference mmdet/models/anchor_heads/iou_aware_retina_head.py:171-219) -- stored
 *     contiguously either NCHW or channels-last (memory (B, H, W, ch), what MIOpen's
 *     NHWC convolutions write: exactly the reference's permute(0,2,3,1) view, :502-507);
 *     ia_head_geom.layout says which.  The training kernels take NCHW only.
 *
 * Each entry point names the reference interface it replaces (paths relative
 * to the reference repository root).
 */
#ifndef IOUAWARE_H
#define IOUAWARE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IA_MAX_LEVELS 8
#define IA_MAX_ANCHORS 16
#define IA_MAX_NMS_PRE 4096
#define IA_MAX_CANDIDATES 8192     /* sum over levels of min(nms_pre, N_l) */
#define IA_MAX_PER_IMG 1024

#define IA_F32 0
#define IA_BF16 1
#define IA_F16 2      /* the dtype-generic operator entries only (ia_sigmoid_focal_loss_*_dt) */
#define IA_F64 3      /* ia_sigmoid_focal_loss_*_dt, ia_nms_f64 */

#define IA_LAYOUT_NCHW 0
#define IA_LAYOUT_NHWC 1     /* needs C * sizeof(dtype) to be a multiple of 16, <= 512 bytes */

#define IA_CLS_SIGMOID 0
#define IA_CLS_SOFTMAX 1
#define IA_CLS_SIGMOID_NOIOU 2   /* plain RetinaNet (retina_head.py): no IoU map, score = sigmoid(cls) */
#define IA_CLS_SOFTMAX_NOIOU 3   /* plain RetinaNet, use_sigmoid_cls=False: score = softmax(cls) */

#define IA_LOSS_SLOTS 64     /* partial sums written by the *_fwd loss kernels */

#define IA_E_ARG (-1)        /* invalid argument / unsupported size */
#define IA_E_WORKSPACE (-2)  /* workspace too small */
/* a size above what the kernels are built for; the reference ops have no such limits
 * (mmdet/ops/nms/src/nms_cpu.cpp:4-59 takes any n) -- the caller can tell them apart: */
#define IA_E_LIMIT_BOXES (-3)    /* more than IA_MAX_CANDIDATES boxes / candidates in one call */
#define IA_E_LIMIT_NMS_PRE (-4)  /* nms_pre above IA_MAX_NMS_PRE */
#define IA_E_LIMIT_PER_IMG (-5)  /* max_per_img above IA_MAX_PER_IMG */

/* Static geometry of one head for one padded input size. */
typedef struct ia_head_geom {
    int32_t num_levels;                 /* L <= IA_MAX_LEVELS */
    int32_t num_anchors;                /* A <= IA_MAX_ANCHORS */
    int32_t num_classes;                /* C, foreground classes (80): columns of scores_t / labels */
    int32_t nms_pre;                    /* <= 0: no per-level top-k */
    int32_t H[IA_MAX_LEVELS];
    int32_t W[IA_MAX_LEVELS];
    int32_t stride[IA_MAX_LEVELS];
    float base_anchors[IA_MAX_LEVELS][IA_MAX_ANCHORS][4];  /* AnchorGenerator.base_anchors */
    float means[4], stds[4];            /* target_means / target_stds */
    int32_t layout;                     /* IA_LAYOUT_*: memory order of the head outputs */
    /* classification activation (iou_aware_retina_head.py:504-507,538-541).
     * IA_CLS_SIGMOID: cls has A*C channels, score_c = sqrt(sigmoid(x_c)) * sqrt(sigmoid(iou)).
     * IA_CLS_SOFTMAX (use_sigmoid_cls=False): cls has A*(C+1) channels, channel 0 of an anchor is
     * the background; score_c = sqrt(softmax(x)_{c+1}) * sqrt(sigmoid(iou)) for c = 0..C-1 and the
     * row maximum runs over the foreground columns only (scores[:, 1:].max).  Everything behind the
     * gather (NMS, labels) is the same.  Covers the inference entries (row-max, top-k, gather,
     * ia_get_bboxes*, ia_decode_stage); the loss entries are sigmoid-only.
     * IA_CLS_SIGMOID_NOIOU / IA_CLS_SOFTMAX_NOIOU: the plain RetinaHead (retina_head.py, scores as in
     * anchor_head.py:364-450): no IoU branch, score_c = sigmoid(x_c), resp. softmax(x)_{c+1} with the
     * row maximum over the foreground columns; the ranking is by these values (equal scores from
     * different logits tie, lower index first).  Every p->iou[l] must be NULL with these kinds and
     * non-NULL with the IoU-aware ones (IA_E_ARG otherwise).
     * The fused head-loss entries (ia_head_loss_*: a sigmoid focal loss) take IA_CLS_SIGMOID and
     * IA_CLS_SIGMOID_NOIOU; both softmax kinds are IA_E_ARG there (workspace size 0).  With
     * IA_CLS_SIGMOID_NOIOU the node is FocalLoss + SmoothL1Loss alone (anchor_head.py:234-299):
     * p->iou[l] and grads->iou[l] must be NULL for every level (a non-NULL one is IA_E_ARG),
     * strides->iou / grad_strides->iou and cfg->attach_iou_target are ignored, no IoU map is read and
     * no IoU gradient written.  The result keeps its 3L + 4 layout: the losses_iou[L] entries and
     * their total are written as 0.0f.  cfg->grad_rows_start_at_reg then describes a gradient row
     * [reg 4A | padding]: the backward writes the zero gradient of the stride - 4A (<= 64) channels
     * behind the reg slice.                                                                       */
    int32_t cls_activation;
} ia_head_geom;

/* Per-level device pointers of the three head outputs, each (B, ch, H, W).  The plain FCOS entries
 * (ia_point_ctr_*) carry the centerness map (B, 1, H, W) in the iou slot; the plain RetinaNet kinds
 * (IA_CLS_*_NOIOU) leave it NULL. */
typedef struct ia_level_ptrs {
    const void *cls[IA_MAX_LEVELS];
    const void *reg[IA_MAX_LEVELS];
    const void *iou[IA_MAX_LEVELS];
} ia_level_ptrs;

/* Derived sizes (host helper): N = anchors per image, R = candidates per image,
 * Rs = R rounded up to 64 (row stride of class-major score / keep arrays).   */
int ia_geom_sizes(const ia_head_geom *g, int32_t *N, int32_t *R, int32_t *Rs);

const char *ia_version(void);

/* ------------------------------------------------------------------ inference
 * Stage entry points.  Together they replace IoUawareRetinaHead.get_bboxes /
 * get_bboxes_single (iou_aware_retina_head.py:390-564) and multiclass_nms
 * (mmdet/core/post_processing/bbox_nms.py:6-67).                             */

/* iou_aware_retina_head.py:502-531,539: per anchor max over classes of
 * sqrt(sigmoid(cls)) * sqrt(sigmoid(iou)) (IA_CLS_SIGMOID_NOIOU: of sigmoid(cls)).
 * rowmax: (B, N) fp32; inside an image each level is an (A, H*W) block (anchor-major), i.e.
 * element a*HW + p holds the reference's anchor index p*A + a (IA_LAYOUT_NCHW), or the reference's own order
 * p*A + a (IA_LAYOUT_NHWC).  ia_select_topk reads whichever g->layout implies.   */
int ia_decode_fuse_rowmax(const ia_head_geom *g, const ia_level_ptrs *p, int batch, int dtype,
                          float *rowmax, void *stream);

/* iou_aware_retina_head.py:536-544 (topk per level, descending; ties broken by
 * ascending anchor index).  cand_idx: (B, R) int32 level-local anchor index.  */
size_t ia_select_topk_workspace_bytes(const ia_head_geom *g, int batch);
int ia_select_topk(const ia_head_geom *g, const float *rowmax, int batch, int32_t *cand_idx,
                   void *workspace, size_t workspace_bytes, void *stream);

/* The same two stages the way ia_get_bboxes chains them: the row-max kernel also leaves, inside
 * the top-k workspace (ia_select_topk_workspace_bytes), the maxima of groups of 64 / 16 / 4
 * consecutive scores of the large levels and the cleared candidate counters, which is where
 * ia_select_topk_grouped starts (ia_select_topk derives them from `rowmax` with an extra pass).
 * Both calls take the SAME workspace, back to back on one stream.                              */
int ia_decode_fuse_rowmax_grouped(const ia_head_geom *g, const ia_level_ptrs *p, int batch,
                                  int dtype, float *rowmax, void *select_workspace,
                                  size_t workspace_bytes, void *stream);
int ia_select_topk_grouped(const ia_head_geom *g, const float *rowmax, int batch,
                           int32_t *cand_idx, void *select_workspace, size_t workspace_bytes,
                           void *stream);

/* iou_aware_retina_head.py:545-558 + mmdet/core/bbox/transforms.py:44-78
 * (delta2bbox) + anchor_generator.py:53-70 (anchors regenerated, never read).
 * img_hw: (B,2) fp32 (img_shape h,w); scale_factor: (B,4) fp32.
 * boxes: (B,R,4) fp32; scores_t: (B,C,Rs) fp32 class-major fused scores;
 * best_score: (B,R) fp32 max over classes per candidate (optional, may be NULL).
 * Like the row-max and top-k entries: any R (IA_MAX_CANDIDATES is the capacity of the batched NMS
 * behind ia_get_bboxes / ia_multiclass_nms, not of this stage).                      */
int ia_gather_decode(const ia_head_geom *g, const ia_level_ptrs *p, int batch, int dtype,
                     const int32_t *cand_idx, const float *img_hw, const float *scale_factor,
                     int rescale, float *boxes, float *scores_t, float *best_score, void *stream);

/* bbox_nms.py:33-56 + mmdet/ops/nms/src/nms_cpu.cpp:4-59 (greedy, ">=",
 * ascending kept indices), all (image, class) problems in one launch, then the
 * per-image top max_per_img.  Outputs: dets (B,max_per_img,5) fp32, labels and
 * rows (B,max_per_img) int32 (row = candidate row id), num (B) int32,
 * keep_count (B,C) int32, keep_rows (B,C,Rs) int32 ascending.  best_score (B,R)
 * optional: rows with best_score <= score_thr are skipped when the per-image
 * suppression bit matrix (the workspace) is built.                             */
size_t ia_multiclass_nms_workspace_bytes(int batch, int R, int C);
int ia_multiclass_nms(const float *boxes, const float *scores_t, const float *best_score,
                      int batch, int R, int C, float score_thr, float iou_thr, int max_per_img,
                      void *workspace, size_t workspace_bytes, float *dets, int32_t *labels,
                      int32_t *rows, int32_t *num, int32_t *keep_count, int32_t *keep_rows,
                      void *stream);

/* multiclass_nms with test_cfg.nms.type = 'soft_nms' (bbox_nms.py:29-56 ->
 * mmdet/ops/nms/nms_wrapper.py:52-78 -> src/soft_nms_cpu.pyx:22-127): per class the
 * boxes with score > score_thr go through soft-NMS in candidate order; survivors keep
 * their DECAYED score; then the per-image top max_per_img.  method: IA_SOFT_LINEAR /
 * IA_SOFT_GAUSSIAN (anything else: hard suppression, as in the .pyx).  Outputs as
 * ia_multiclass_nms, except keep_rows lists each class's survivors in selection order
 * and dets[...,4] are decayed scores.  workspace additionally holds the (B,C,Rs)
 * decayed scores.                                                              */
#define IA_SOFT_LINEAR 1
#define IA_SOFT_GAUSSIAN 2
size_t ia_multiclass_soft_nms_workspace_bytes(int batch, int R, int C);
int ia_multiclass_soft_nms(const float *boxes, const float *scores_t, int batch, int R, int C,
                           float score_thr, float iou_thr, int method, float sigma,
                           float min_score, int max_per_img, void *workspace,
                           size_t workspace_bytes, float *dets, int32_t *labels, int32_t *rows,
                           int32_t *num, int32_t *keep_count, int32_t *keep_rows, void *stream);

/* Whole path in one call (what the Python head calls).
 * WORKSPACE CONTRACT of ia_get_bboxes / ia_get_bboxes_lazy / ia_decode_stage: the workspace holds a
 * few words of state (arrival counters of the fused row-max + top-k-filter launch).  Zero-fill it
 * ONCE before its first use; every call leaves it ready for the next one.  Do not let anything else
 * write to it between calls (if something did, zero it again; the entry points do so themselves
 * when they fail between the fused launch and the kernel that resets the state).
 * Bounded waits: a filter workgroup of the fused launch that gives up waiting for the row-max
 * wavefronts (GPU shared with another process, CU masking, a debugger) records the call in the
 * status words, and the next kernel of the same call selects from the complete row maxima instead
 * of the candidate lists -- the detections are the same, the call is slower.
 * ia_get_bboxes_status_offset() = byte offset of two uint32 words: [0] the id of the last call
 * that took this fallback (0: never), [1] the number of such calls.  ia_debug_fused_spin_limit()
 * sets the bound of the waits (tests: 0 forces the fallback; negative: the default, 2^21 polls). */
size_t ia_get_bboxes_workspace_bytes(const ia_head_geom *g, int batch);
size_t ia_get_bboxes_status_offset(const ia_head_geom *g, int batch);
int ia_debug_fused_spin_limit(int64_t limit);
/* Profiling hook (bench.py): two caller-owned hipEvent_t (as void *) that every later
 * ia_get_bboxes / ia_get_bboxes_lazy / ia_decode_stage call records on ITS stream -- `begin` in
 * front of the decode stage's first launch (row-max), `end` behind its last one (gather / decode) --
 * so the stage can be timed inside real steps.  Both NULL (the default) switch it off; one NULL:
 * IA_E_ARG.  The pair belongs to ONE stream: the first stage call after installation binds the
 * hook to its stream and calls on other streams do not record (no cross-stream event records from
 * concurrent callers).  The caller keeps the events alive while they are set and clears the hook
 * (NULL, NULL) before releasing them. */
int ia_profile_stage_events(void *begin, void *end);
int ia_get_bboxes(const ia_head_geom *g, const ia_level_ptrs *p, int batch, int dtype,
                  const float *img_hw, const float *scale_factor, int rescale, float score_thr,
                  float iou_thr, int max_per_img, void *workspace, size_t workspace_bytes,
                  float *dets, int32_t *labels, int32_t *rows, int32_t *num, void *stream);

/* The same result (dets / labels / rows / num) with the NMS evaluated lazily: the (class, box)
 * pairs of an image are walked in the final order (score desc, class asc, row asc) and a pair
 * is kept iff no already kept pair of its class suppresses it; max_per_img survivors end the
 * walk -- greedy per-class NMS decides a box from higher-ranked boxes only, so these are exactly
 * the detections multiclass_nms returns (bbox_nms.py:33-56), without resolving 80 complete class
 * problems.  candidates: pairs walked per image at most (0 = default: 1024, then 4096 for the
 * images that need more); an image that runs
 * out of them with fewer than max_per_img survivors takes the complete path.  The per-class
 * keep lists in the workspace are NOT produced by this entry point.                        */
int ia_get_bboxes_lazy(const ia_head_geom *g, const ia_level_ptrs *p, int batch, int dtype,
                       const float *img_hw, const float *scale_factor, int rescale,
                       float score_thr, float iou_thr, int max_per_img, int candidates,
                       void *workspace, size_t workspace_bytes, float *dets, int32_t *labels,
                       int32_t *rows, int32_t *num, void *stream);

/* The NMS stage of ia_get_bboxes_lazy on its own (inputs as ia_multiclass_nms).             */
size_t ia_multiclass_nms_lazy_workspace_bytes(int batch, int R, int C);
int ia_multiclass_nms_lazy(const float *boxes, const float *scores_t, const float *best_score,
                           int batch, int R, int C, float score_thr, float iou_thr,
                           int max_per_img, int candidates, void *workspace,
                           size_t workspace_bytes, float *dets, int32_t *labels, int32_t *rows,
                           int32_t *num, void *stream);

/* The decode stage of ia_get_bboxes on its own -- row-max (+ group maxima), top-k, gather / decode
 * (iou_aware_retina_head.py:499-558; SURVEY 8(d)'s unit) -- in the ia_get_bboxes workspace, where
 * ia_get_bboxes_workspace_layout finds cand_idx, boxes, scores_t and best_score afterwards.   */
int ia_decode_stage(const ia_head_geom *g, const ia_level_ptrs *p, int batch, int dtype,
                    const float *img_hw, const float *scale_factor, int rescale, void *workspace,
                    size_t workspace_bytes, void *stream);

/* Workspace carve-up of ia_get_bboxes (host helper for stage-level tests):
 * byte offsets of rowmax, cand_idx, boxes, scores_t, keep_count, keep_rows,
 * best_score, NMS stage workspace (bit matrix, sorted rows, counts).          */
int ia_get_bboxes_workspace_layout(const ia_head_geom *g, int batch, size_t offsets[8]);

/* mmdet.ops.nms.nms (mmdet/ops/nms/nms_wrapper.py:8-49 -> nms_cpu.nms /
 * nms_cuda.nms): dets (n,5) fp32 on device, ANY n like the reference op (up to
 * IA_MAX_CANDIDATES boxes: one n x n suppression bit matrix; more: the same greedy NMS in
 * chunks of IA_MAX_CANDIDATES sorted boxes, csrc/bignms.hip).
 * keep (n) int32 ascending input indices, count (1) int32.                      */
size_t ia_nms_workspace_bytes(int n);
int ia_nms(const float *dets, int n, float iou_thr, int32_t *keep, int32_t *count, void *workspace,
           size_t workspace_bytes, void *stream);

/* The same operator on DOUBLE boxes: nms_cpu_kernel<double> (nms_cpu.cpp:63 dispatches float and
 * double; areas, intersections and the quotient in fp64, the float threshold promoted to double --
 * the fp32 entry is not a substitute: float(1/3) as threshold suppresses an IoU of exactly 1/3 in
 * fp32 and does not in fp64).  n <= 16384 (IA_E_LIMIT_BOXES above; csrc/nms64.hip).            */
size_t ia_nms_f64_workspace_bytes(int n);
int ia_nms_f64(const double *dets, int n, float iou_thr, int32_t *keep, int32_t *count,
               void *workspace, size_t workspace_bytes, void *stream);

/* mmdet.ops.nms.soft_nms (nms_wrapper.py:52-78 -> soft_nms_cpu.pyx:22-127): dets (n,5)
 * fp32 on device, n <= IA_MAX_CANDIDATES.  out_dets (n,5): surviving boxes in selection
 * order with decayed scores; out_inds (n) int32 their input indices; count (1) int32.
 * The reference runs this op on the host only (numpy); there is no reference CUDA path. */
int ia_soft_nms(const float *dets, int n, float iou_thr, int method, float sigma, float min_score,
                float *out_dets, int32_t *out_inds, int32_t *count, void *stream);

/* Image pre-processing in front of the backbone: ImageTransform.__call__
 * (mmdet/datasets/transforms.py:31-50): cv2 bilinear resize of the uint8 BGR image to
 * (dst_h, dst_w) (the caller computes the size like mmcv.imrescale / imresize), BGR->RGB,
 * (x - mean) / std, horizontal flip, zero padding to (pad_h, pad_w), HWC->CHW; one launch
 * per <= 16 images.  imgs: HOST array of descriptors whose src pointers are DEVICE uint8
 * (src_h, src_w, 3) images.  out: (B,3,pad_h,pad_w) fp32, or (B,pad_h,pad_w,3) when
 * channels_last (the memory layout of a channels-last (B,3,H,W) tensor).              */
typedef struct {
    const uint8_t *src;
    int32_t src_h, src_w, dst_h, dst_w, flip;
} ia_image_desc;
int ia_image_transform(const ia_image_desc *imgs, int batch, const float *mean, const float *std,
                       int to_rgb, int pad_h, int pad_w, int channels_last, float *out,
                       void *stream);

/* Winograd F(4x4,3x3) transforms around a library batched GEMM, for the 3x3 / stride-1 / pad-1
 * convolutions of the head towers and outputs (iou_aware_retina_head.py:171-219; replaces
 * ConvModule.forward, mmdet/models/utils/conv_module.py:149-163, and the three output
 * nn.Conv2d) and of the FPN outputs (mmdet/models/necks/fpn.py:124-127) at inference.
 * All pyramid levels of a batch form ONE tile list (tiles of 4x4 outputs, level-major, then
 * image, then row-major), so a shared-weight layer is one batched GEMM:
 *   V (groups*36, T, C/groups)  = input transform of channels-last activations (B,H_l,W_l,C)
 *   M[k] = V[k] . U[k]          (caller: rocBLAS / hipBLASLt; U = G g G^T, (36, Cin, Cout))
 *   output transform of M (groups*36, T, C/groups) + bias (+ ReLU) -> channel ranges
 *   ("segments") of channels-last destination tensors.                                   */
typedef struct {
    int32_t num_levels, batch;
    int32_t H[IA_MAX_LEVELS], W[IA_MAX_LEVELS];
} ia_wino_geom;
typedef struct {
    int32_t c0, n;                  /* output channels [c0, c0+n) of the GEMM result ...   */
    int32_t dst_channels, dst_offset;   /* ... go to channels [dst_offset, +n) of dst     */
    float *dst[IA_MAX_LEVELS];      /* per level (B, H_l, W_l, dst_channels)               */
} ia_wino_seg;
int ia_wino_tiles(const ia_wino_geom *g, int32_t *tiles);
/* pre_shift != NULL: the input is read as relu?(x * pre_scale[c] + pre_shift[c]) (pre_scale
 * NULL = 1): the folded BatchNorm + ReLU of the producing 1x1 convolution, applied on load.  */
int ia_wino_input_transform(const ia_wino_geom *g, const float *const *x, int channels, int groups,
                            const float *pre_scale, const float *pre_shift, int pre_relu, float *V,
                            void *stream);
int ia_wino_output_transform(const ia_wino_geom *g, const float *M, int channels, int groups,
                             const float *bias, int relu, int nseg, const ia_wino_seg *segs,
                             void *stream);
/* Output transform of a layer and input transform of the next 3x3 convolution of the SAME
 * geometry in one launch: V = B^T relu?(A^T M A + bias) B per tile, the activation in between
 * (zero outside the feature maps) stays on chip.  M (groups_m*36, T, C/groups_m) -> V
 * (groups_v*36, T, C/groups_v): the bits that ia_wino_output_transform(groups_m) into a
 * (B, H_l, W_l, channels) tensor per level followed by ia_wino_input_transform(groups_v) of those
 * tensors gives.  C/groups_m % 32 == 0, C/groups_v % 32 == 0; M, V, bias 16-byte aligned; V must
 * not overlap M.                                                                              */
int ia_wino_mid_transform(const ia_wino_geom *g, const float *M, int channels, int groups_m,
                          const float *bias, int relu, float *V, int groups_v, void *stream);
/* Input transform and the 36 products behind it in one launch: M[k] (T, channels) = V[k] . U[k]
 * with V never written to memory -- the bits that ia_wino_input_transform(groups = 1) followed
 * by ia_batched_gemm_stream(36, T, channels, channels) gives.  channels == 64 (Cin == Cout).
 * u_packed: U (36, Cin, Cout) in MFMA fragment order, (36, Cout/16, Cin/16, 64, 4):
 *   u_packed[k][nb][j][16 q + p][c] = U[k][16 j + 4 q + c][16 nb + p]
 * (iouaware/winograd.py pack_u_fragments).  pre_scale / pre_shift / pre_relu as for
 * ia_wino_input_transform; x, u_packed, M, pre_* 16-byte aligned.                            */
int ia_wino_in_gemm(const ia_wino_geom *g, const float *const *x, int channels, const float *pre_scale,
                    const float *pre_shift, int pre_relu, const float *u_packed, float *M, void *stream);
/* The whole 3x3 / stride-1 / pad-1 convolution of 64 -> 64 channels in one launch: input
 * transform, the 36 products and the output transform (+bias, +ReLU), V and M never written to
 * memory -- the bits that ia_wino_in_gemm followed by ia_wino_output_transform(groups = 1, one
 * segment of all 64 channels into y) gives.  x, u_packed, pre_* as for ia_wino_in_gemm; bias (64)
 * or NULL; y[l] (B, H_l, W_l, 64) channels-last per level, must not overlap x.  channels == 64;
 * x, y, u_packed, bias, pre_* 16-byte aligned.                                               */
int ia_wino_conv3x3_c64(const ia_wino_geom *g, const float *const *x, int channels, const float *pre_scale,
                        const float *pre_shift, int pre_relu, const float *u_packed, const float *bias,
                        int relu, float *const *y, void *stream);

/* Training: gradient of the output transform, dM = A dY A^T per tile (dY (B,H,W,channels)
 * channels-last per level, zero outside the map), written as 36 matrices (36, tiles, channels)
 * like V -- the right-hand operand of the Winograd-domain weight gradient
 * dU[k] = V[k]^T dM[k]  (then dW = G^T dU G on the host side).                          */
int ia_wino_grad_output_transform(const ia_wino_geom *g, const float *const *dy, int channels,
                                  float *dM, void *stream);

/* Training: the per-iteration weight transforms of the Winograd convolution nodes
 * (iouaware/winograd_train.py) and the fused ReLU-backward / bias-gradient pass of the
 * convolution nodes (iouaware/train_fuse.py); they stand where the reference's training step
 * runs torch's convolution / BatchNorm / ReLU backward (mmdet/models/backbones/resnet.py:215-255,
 * mmdet/models/anchor_heads/iou_aware_retina_head.py:171-219 under autograd).
 *   ia_wino_weight_transform: U (36, n_in, n_out), U[6a+b][i][o] = (G w(o,i) G^T)[a][b]; w is
 *     addressed by element strides (any memory format; swap stride_in / stride_out and set
 *     flip=1 for the input-gradient convolution = correlation with w^T rotated by 180 degrees).
 *     G: the 6x3 kernel-transform matrix of F(4x4,3x3), row-major doubles (host memory).
 *   ia_wino_weight_grad: dW (n_out, n_in, 3, 3), addressed by element strides like w above
 *     = G^T dU(.,i,o) G, the adjoint.
 *   ia_bn_fold_fwd / _bwd: eval-mode BatchNorm (`norm_eval=True`, resnet.py:520-527) folded into the
 *     convolution in front of it, differentiably: w_out[o][:] = w[o][:] * s, b_out = beta - mean * s,
 *     s = gamma * inv_std (inv_std = 1/sqrt(running_var + eps), a constant); backward gives dw,
 *     dgamma, dbeta from the gradients w.r.t. w_out / b_out.  Weights are (cout, K) rows, dense in
 *     memory (contiguous or channels-last alike; all four weight-shaped arrays share one layout).
 *   ia_relu_bwd_bias_grad: dy, y, g (rows, n) row-major fp32 (n % 4 == 0, 16-byte aligned):
 *     g = dy where y > 0 else 0 (y == NULL: no mask, nothing written), db[n] = column sums of
 *     the masked gradient (db == NULL: not computed).  The sums go through per-strip partial
 *     rows in the workspace and are added in a fixed order (same bits every run).            */
#define IA_COLSUM_MAX_STRIPS 512
size_t ia_relu_bwd_bias_grad_workspace_bytes(int64_t rows, int n);
int ia_wino_weight_transform(const float *w, int n_in, int n_out, int64_t stride_in,
                             int64_t stride_out, int64_t stride_ky, int64_t stride_kx, int flip,
                             const double *G, float *U, void *stream);
int ia_wino_weight_grad(const float *dU, int n_in, int n_out, const double *G, float *dW,
                        int64_t stride_in, int64_t stride_out, int64_t stride_ky, int64_t stride_kx,
                        void *stream);
int ia_bn_fold_fwd(const float *w, const float *gamma, const float *beta, const float *mean,
                   const float *inv_std, int cout, int K, float *w_out, float *b_out, void *stream);
int ia_bn_fold_bwd(const float *dw_folded, const float *db_folded, const float *w, const float *gamma,
                   const float *mean, const float *inv_std, int cout, int K, float *dw,
                   float *dgamma, float *dbeta, void *stream);
int ia_relu_bwd_bias_grad(const float *dy, const float *y, int64_t rows, int n, float *g, float *db,
                          void *workspace, size_t workspace_bytes, void *stream);

/* 1x1 convolution on a channels-last activation as one library GEMM (hipBLASLt) with the folded
 * BatchNorm bias, the residual and the ReLU in its epilogue (Bottleneck.forward,
 * mmdet/models/backbones/resnet.py:215-255, at inference):
 *   D (rows, n) = act(A (rows, k) . W (k, n) + bias[n] + residual (rows, n)),  rows = B*H*W
 * all row-major fp32; bias / residual optional; residual != D.  The library handle is created on
 * first use; the first call of a shape times the heuristic's candidates on `stream`.         */
int ia_linear_bias_act(const float *A, const float *W, const float *bias, const float *residual,
                       float *D, int64_t rows, int k, int n, int relu, void *workspace,
                       size_t workspace_bytes, void *stream);
/* The same with bf16 operands (A, W, residual, D bf16; bias fp32; fp32 accumulation) for the
 * bf16 configuration (BASELINE config 3).                                                    */
int ia_linear_bias_act_bf16(const void *A, const void *W, const float *bias, const void *residual,
                            void *D, int64_t rows, int k, int n, int relu, void *workspace,
                            size_t workspace_bytes, void *stream);
/* The batched GEMM between the Winograd transforms, D[b] (rows, n) = A[b] (rows, k) . W[b] (k, n),
 * b < batch, contiguous row-major stacks; same library, same per-shape candidate timing.      */
int ia_batched_gemm(const float *A, const float *W, float *D, int batch, int64_t rows, int k, int n,
                    void *workspace, size_t workspace_bytes, void *stream);
/* The same product for the HBM-bound shapes -- (k, n) in {(64, 64), (128, 128), (256, 48)}: the
 * Winograd-domain GEMMs of the 64- / 128-channel bottleneck convolutions and of the reg | iou
 * output -- on this library's streaming MFMA kernel (csrc/conv1x1_stream.hip: one grid row per
 * matrix, its weights in LDS); no workspace.                                                    */
int ia_batched_gemm_stream(const float *A, const float *W, float *D, int batch, int64_t rows, int k,
                           int n, void *stream);
/* The same product for the large head shapes on bf16 MFMA (csrc/wino_split_gemm.hip): every fp32
 * operand split exactly into three bf16 pieces, x = h + m + l, and the six terms hh, hm, mh, hl, lh,
 * mm summed in fp32 (hh in its own accumulators, the other five in a second set, the two added once
 * at the end): error in the fp32 class, the same bits in every run.  V is split inside the kernel;
 * U3 is U split once and packed in fragment order, (batch, k / 16, ceil(n / 128) * 4, 3, 64, 8)
 * bf16 (iouaware/winograd.py split3_pack_u).  k a multiple of 32, V and U3 16-byte aligned; no
 * workspace.                                                                                    */
int ia_batched_gemm_split3(const float *V, const void *U3, float *D, int batch, int64_t rows, int k,
                           int n, void *stream);

/* Convolutions with a stride as plain contractions with a FIXED reduction order (the library
 * convolution's fast fp32 channels-last kernels for these shapes split the reduction and add the
 * partial sums with atomics: other bits in every run).
 *   ia_im2col3x3_nhwc  3x3 / pad 1 / stride s (1..4) taps of a channels-last (B, H, W, C) tensor as
 *     the row-major matrix col[(b, yo, xo)][tap * C + c] (zeros outside the image), tap = dy * 3 + dx,
 *     Ho = (H - 1) / s + 1; C * sizeof(dtype) must be a multiple of 16.  ia_im2col3x3_bytes: its size.
 *     The convolution is then ia_linear_bias_act[_bf16] with rows = B * Ho * Wo, k = 9 * C and the
 *     weight stored (9 * C, Cout): folded BatchNorm / bias / ReLU in the GEMM epilogue.  Replaces
 *     conv2 (stride 2) of the first bottleneck of ResNet stages 2-4 (resnet.py:147-160) and the
 *     FPN's P6 / P7 (necks/fpn.py:84-99) at inference.
 *   ia_conv1x1_strided  1x1 / stride s on a channels-last (B, H, W, k) tensor -> (B, Ho, Wo, n):
 *     D = act(x[:, ::s, ::s, :] . W_kn + bias + residual) as one strided-batched library GEMM that
 *     reads the input in place (leading dimension s * k; one batch item per output row); the
 *     projection shortcut of those blocks (resnet.py:436-449).  dtype IA_F32 / IA_BF16.          */
size_t ia_im2col3x3_bytes(int B, int H, int W, int C, int stride, int dtype);
int ia_im2col3x3_nhwc(const void *x, void *col, int B, int H, int W, int C, int stride, int dtype,
                      void *stream);
int ia_conv1x1_strided(const void *x, const void *W_kn, const float *bias, const void *residual,
                       void *D, int B, int H, int W, int k, int n, int stride, int relu, int dtype,
                       void *workspace, size_t workspace_bytes, void *stream);
/* The adjoint of ia_im2col3x3_nhwc in gather form -- the input gradient of the strided 3x3
 * training node (iouaware/train_fuse.py, conv3x3_strided), after dcol = g . W_kn^T:
 *   dx[b][yi][xi][c] = sum over the taps (dy, dx), tap = dy * 3 + dx, for which (yi + 1 - dy) and
 *   (xi + 1 - dx) are multiples of `stride` and the quotients (yo, xo) lie inside Ho x Wo, of
 *   dcol[(b, yo, xo)][tap * C + c]
 * for the channels-last dx (B, H, W, C) and the (B * Ho * Wo, 9 * C) row-major dcol.  The terms are
 * added in ascending tap order, each in one fp32 add, without atomics: the same bits in every run.
 * Every element of dx is written exactly once, 0.0f where no tap reads the pixel (strides 3 / 4);
 * dx needs no initialisation.  dtype IA_F32 only, C a multiple of 4, both pointers 16-byte aligned,
 * stride 1..4; anything else: IA_E_ARG.  Reads dcol once and writes dx once
 * (9 * C * B * Ho * Wo * 4 + B * H * W * C * 4 bytes).                                           */
int ia_col2im3x3_nhwc(const void *dcol, void *dx, int B, int H, int W, int C, int stride, int dtype,
                      void *stream);

/* Deformable 3x3 convolution, DCN v1 / v2 (reference mmdet/ops/dcn), fp32 on channels-last tensors
 * (csrc/deform.hip).  Ho = (H + 2 pad - (2 dil + 1)) / stride + 1, Wo likewise; dg = deformable
 * groups, C a multiple of 4 * dg; x and col 16-byte aligned; anything else: IA_E_ARG, checked
 * before anything is enqueued.
 *   ia_deform_im2col3x3_nhwc   col[(b, ho, wo)][(i * 3 + j) * C + c] = mask * bilinear sample of
 *     x[b][.][.][c] at h = ho * stride - pad + i * dil + offset[pix][g * 18 + 2 (i * 3 + j)],
 *     w = wo * stride - pad + j * dil + offset[pix][g * 18 + 2 (i * 3 + j) + 1], g = c / (C / dg):
 *     0 unless -1 < h < H and -1 < w < W, else the four floor / floor + 1 corners, a corner outside
 *     the map contributing 0.  offset / mask are rows per output pixel (b, ho, wo) with the given
 *     pixel strides in floats (>= dg * 18 / dg * 9: channel slices of a wider channels-last tensor
 *     qualify); mask NULL: v1, no modulation; mask_logits: the mask rows hold logits, the sigmoid
 *     is taken here.  The row order is that of ia_im2col3x3_nhwc: the convolution is
 *     ia_linear_bias_act with rows = B * Ho * Wo, k = 9 * C.  ia_deform_im2col3x3_bytes: col's size.
 *   ia_deform_col2im3x3_nhwc   the adjoint, from dcol = dy . W^T (ia_linear_bias_act_wt), the
 *     derivative of the same piecewise formula (corners from floor); each output may be NULL:
 *       dx        (B, H, W, C), ZERO-FILLED HERE, then every column element added to its four
 *                 corners with fp32 atomics: NOT bit-reproducible from run to run;
 *       d_offset  dense rows (pix, dg * 18), d_mask dense rows (pix, dg * 9; needs mask): sums over
 *                 the group's channels in a fixed order, every element written, the same bits in
 *                 every run.  mask holds values here (no logits form).                            */
size_t ia_deform_im2col3x3_bytes(int B, int H, int W, int C, int stride, int pad, int dil);
int ia_deform_im2col3x3_nhwc(const float *x, const float *offset, int64_t offset_pix_stride,
                             const float *mask, int64_t mask_pix_stride, int mask_logits,
                             float *col, int B, int H, int W, int C, int stride, int pad,
                             int dil, int deformable_groups, void *stream);
int ia_deform_col2im3x3_nhwc(const float *dcol, const float *x, const float *offset,
                             int64_t offset_pix_stride, const float *mask,
                             int64_t mask_pix_stride, float *dx, float *d_offset, float *d_mask,
                             int B, int H, int W, int C, int stride, int pad, int dil,
                             int deformable_groups, void *stream);

/* How the library kernel of a new GEMM shape is chosen.
 *   2  FROZEN (default): the entry of the tuning table below, else the library heuristic's first
 *      result.  Nothing is timed at run time, so a process computes the same bits in every run
 *      (pick-by-timing made the arithmetic depend on the winner of a race).
 *   0 / 1  OFFLINE tuning (tools/tune_gemm.py writes the table with them): the first call of a
 *      shape times the heuristic's top 16 / every kernel of the library that supports the problem
 *      (~250 for fp32, ~0.3 s per shape; +2 % img/s on the R-50 inference step).
 * The environment variable IA_GEMM_TUNE = heuristic | all selects 0 / 1 at the first GEMM.  Shapes
 * already resolved keep their kernel.  Returns the previous mode; any other argument only queries. */
int ia_gemm_tuning(int mode);

/* The tuning table: (m, n, k, flags, batch, dtype) in the column-major terms of csrc/gemm.hip ->
 * the library's solution index (hipblaslt_ext::getIndexFromAlgo).  The package ships the table
 * measured on MI355X (iouaware/tuning/hipblaslt_gfx950.json, loaded by iouaware.ops at the first
 * GEMM together with the library version it was measured with; a table from another library
 * version is ignored, a solution the library no longer offers for the problem counts as stale
 * and the heuristic's first result is used).
 *   ia_gemm_table_add    one entry (a shape already resolved is resolved again);
 *   ia_gemm_table_clear  drops the table AND every resolved shape;
 *   ia_gemm_table_dump   the solution index in use for every shape resolved so far, rows of
 *                        7 x int64 {m, n, k, flags, batch, dtype, index}; returns the number of
 *                        shapes (rows7 may be NULL to query);
 *   ia_gemm_table_stats  {shapes served by the table, by the heuristic, stale entries};
 *   ia_gemm_library_version  hipblasLtGetVersion of the library mapped into this process.      */
int ia_gemm_table_add(int64_t m, int64_t n, int64_t k, int flags, int batch, int dtype,
                      int solution_index);
int ia_gemm_table_clear(void);
int ia_gemm_table_dump(int64_t *rows7, int capacity);
int ia_gemm_table_stats(int64_t *hits_misses_stale);
int ia_gemm_library_version(void);

/* Training forms of the same library GEMM (convolution autograd nodes, iouaware/train_fuse.py):
 *   ia_linear_bias_act_wt: as ia_linear_bias_act with the weight stored (n, k) row-major -- the
 *     (Cout, Cin) convolution weight as it is, read through the library's transpose flag;
 *   ia_gemm_tn: D[b] (n, k) = G[b]^T (n, rows) . X[b] (rows, k), b < batch: the weight gradient of
 *     a 1x1 convolution (G = output gradient, X = input) and, batch = 36, of the Winograd-domain
 *     product; a reduction over `rows` with a small result, the timed candidates include the
 *     library's split-K kernels (give it a workspace).                                          */
int ia_linear_bias_act_wt(const float *A, const float *W_nk, const float *bias,
                          const float *residual, float *D, int64_t rows, int k, int n, int relu,
                          void *workspace, size_t workspace_bytes, void *stream);
int ia_gemm_tn(const float *G, const float *X, float *D, int batch, int64_t rows, int n, int k,
               void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------- training
 * Per-level losses of IoUawareRetinaHead.loss_single (:221-313), computed on
 * the NCHW head outputs directly.  Each *_fwd ADDS its fp64 partial sums into
 * loss_sum[IA_LOSS_SLOTS] (device, zeroed by the caller; one fp64 atomic per
 * workgroup, spread over the slots to avoid contention); the loss numerator the
 * reference divides by avg_factor (losses.py:301-303,411,480) is the sum of the slots;
 * each *_bwd writes s * d(sum)/d(input) with the input's NCHW shape, where
 * s = gscale (host) * (gscale_dev ? *gscale_dev : 1): the upstream gradient
 * may stay on the device, so backward never synchronises with the host.       */

/* FocalLoss -> weighted_sigmoid_focal_loss -> py_sigmoid_focal_loss
 * (mmdet/core/loss/losses.py:226-247,279-303) fused with expand_binary_labels
 * (mmdet/core/anchor/anchor_target.py:247-254).  labels (B*N_l) int64,
 * label_weights (B*N_l) fp32 in anchor order n = p*A + a.                     */
int ia_focal_loss_fwd(const void *cls, int dtype, const int64_t *labels,
                      const float *label_weights, int B, int A, int C, int HW, float gamma,
                      float alpha, double *loss_sum, void *stream);
int ia_focal_loss_bwd(const void *cls, int dtype, const int64_t *labels,
                      const float *label_weights, int B, int A, int C, int HW, float gamma,
                      float alpha, float gscale, const float *gscale_dev, float *grad_cls,
                      void *stream);

/* SmoothL1Loss -> weighted_smoothl1 (losses.py:385-411).  pred NCHW
 * (B,A*4,H,W); target / weight (B,N_l,4) row-major.                           */
int ia_smooth_l1_fwd(const void *pred, int dtype, const float *target, const float *weight,
                     int B, int A, int HW, float beta, double *loss_sum, void *stream);
int ia_smooth_l1_bwd(const void *pred, int dtype, const float *target, const float *weight,
                     int B, int A, int HW, float beta, float gscale, const float *gscale_dev,
                     float *grad_pred, void *stream);

/* BalancedL1Loss -> weighted_balanced_l1_loss (losses.py:482-520), same tensors, slots and gscale as the
 * smooth-L1 pair.  With d = |pred - target| and b = e^(gamma / alpha) - 1 (formed in double, rounded once):
 * d < beta: alpha / b * (b d + 1) * log(b d / beta + 1) - alpha d, else gamma d + gamma / b - alpha beta;
 * the gradient is that of this expression (0 at pred == target, the linear branch at d == beta, a jump
 * at the knee for beta != 1).  A gradient is written for every element, exactly 0 where the weight is 0.
 * alpha, gamma or beta not > 0: IA_E_ARG.                                                             */
int ia_balanced_l1_fwd(const void *pred, int dtype, const float *target, const float *weight,
                       int B, int A, int HW, float beta, float alpha, float gamma, double *loss_sum,
                       void *stream);
int ia_balanced_l1_bwd(const void *pred, int dtype, const float *target, const float *weight,
                       int B, int A, int HW, float beta, float alpha, float gamma, float gscale,
                       const float *gscale_dev, float *grad_pred, void *stream);

/* The IoU-balanced variants (loss_cls.type='IOUbalancedSigmoidFocalLoss', losses.py:309-374;
 * loss_bbox.type='IoUbalancedSmoothL1Loss', losses.py:416-458; anchor_head.py:83-84).
 * anchor_iou (B*N_l): the IoU regression target of the level (ia_iou_bce_fwd's iou_target),
 * treated as a constant.
 * focal: the positive element of a positive anchor is weighted by iou^eta * normalizer,
 * normalizer = S1 / (S2 + 1e-6).  fwd ADDS into loss_sums3[3*IA_LOSS_SLOTS]: slots [0,64) the
 * t=0 elements, [64,128) S1 = sum_pos loss, [128,192) S2 = sum_pos loss * iou^eta; the loss is
 * S0 + normalizer*S2.  bwd reads the normalizer from a device scalar.
 * smooth-L1: weight * iou^delta.                                                          */
int ia_focal_loss_balanced_fwd(const void *cls, int dtype, const int64_t *labels,
                               const float *label_weights, const float *anchor_iou, int B, int A,
                               int C, int HW, float gamma, float alpha, float eta,
                               double *loss_sums3, void *stream);
int ia_focal_loss_balanced_bwd(const void *cls, int dtype, const int64_t *labels,
                               const float *label_weights, const float *anchor_iou, int B, int A,
                               int C, int HW, float gamma, float alpha, float eta,
                               const float *normalizer_dev, float gscale, const float *gscale_dev,
                               float *grad_cls, void *stream);
int ia_smooth_l1_balanced_fwd(const void *pred, int dtype, const float *target,
                              const float *weight, const float *anchor_iou, int B, int A, int HW,
                              float beta, float delta, double *loss_sum, void *stream);
int ia_smooth_l1_balanced_bwd(const void *pred, int dtype, const float *target,
                              const float *weight, const float *anchor_iou, int B, int A, int HW,
                              float beta, float delta, float gscale, const float *gscale_dev,
                              float *grad_pred, void *stream);

/* IoU target (delta2bbox x2 + aligned bbox_overlaps,
 * iou_aware_retina_head.py:256-259, mmdet/core/bbox/geometry.py:34-47) fused
 * with weighted_iou_regression_loss (losses.py:460-480).  `level` selects the
 * base anchors / H / W / stride of g.  iou_target (B*N_l, optional).
 * bwd: grad_iou_pred NCHW (B,A,H,W); grad_bbox_pred NCHW (B,A*4,H,W) is the
 * gradient THROUGH the IoU target (pass NULL for the detached variant).       */
int ia_iou_bce_fwd(const ia_head_geom *g, int level, const void *bbox_pred, const void *iou_pred,
                   int dtype, const float *bbox_targets, const float *bbox_weights, int B,
                   float *iou_target, double *loss_sum, void *stream);
int ia_iou_bce_bwd(const ia_head_geom *g, int level, const void *bbox_pred, const void *iou_pred,
                   int dtype, const float *bbox_targets, const float *bbox_weights, int B,
                   float gscale, const float *gscale_dev, float *grad_iou_pred,
                   float *grad_bbox_pred, void *stream);

/* Training targets for a whole batch: anchor_target -> anchor_target_single ->
 * MaxIoUAssigner.assign_wrt_overlaps + PseudoSampler + bbox2delta + unmap
 * (mmdet/core/anchor/anchor_target.py:129-242, assigners/max_iou_assigner.py:98-201,
 * bbox/geometry.py:48-64, bbox/transforms.py:6-41), gt_max_assign_all=True,
 * allowed_border < 0, no ignore regions.  gt_boxes (B,gmax,4) fp32 padded,
 * gt_labels (B,gmax) int64 or NULL (label 1), num_gt (B) >= 1, gmax <= 512;
 * valid_hw (B,L,2) int32 = valid feature rows / cols per level (from pad_shape,
 * anchor_head.py:135-146).  Outputs are level-major: for level l a (B, N_l[,4])
 * block at element offset B * anchor_off_l -- the per-level tensors of
 * images_to_levels.  counts (B,2): positives, negatives per image.
 * gt_max_scratch: (B,gmax) uint32 scratch.                                      */
int ia_anchor_targets(const ia_head_geom *g, const float *gt_boxes, const int64_t *gt_labels,
                      const int32_t *num_gt, int batch, int gmax, const int32_t *valid_hw,
                      float pos_iou_thr, float neg_iou_thr, float min_pos_iou, float pos_weight,
                      uint32_t *gt_max_scratch, int64_t *labels, float *label_weights,
                      float *bbox_targets, float *bbox_weights, int32_t *counts, void *stream);

/* The same assignment with the gt boxes where the data loader left them: HOST arrays of
 * per-image DEVICE pointers gt_boxes[b] (num_gt[b],4) fp32 / gt_labels[b] (num_gt[b]) int64 (or
 * gt_labels == NULL), host num_gt[b] in 1..512 and host valid_hw (B,L,2).  Pointers and sizes
 * travel in the kernel arguments: no padded staging tensors, no host-to-device copies.
 * batch <= IA_MAX_TARGET_BATCH.                                                    */
#define IA_MAX_TARGET_BATCH 16
int ia_anchor_targets_ptrs(const ia_head_geom *g, const float *const *gt_boxes,
                           const int64_t *const *gt_labels, const int32_t *num_gt, int batch,
                           const int32_t *valid_hw, float pos_iou_thr, float neg_iou_thr,
                           float min_pos_iou, float pos_weight, uint32_t *gt_max_scratch,
                           int64_t *labels, float *label_weights, float *bbox_targets,
                           float *bbox_weights, int32_t *counts, void *stream);

/* ------------------------------------------------------------------ IoUawareRetinaHead.loss, all levels
 * One call for the forward and one for the backward of the three losses of every pyramid level
 * (iou_aware_retina_head.py:221-313 x L, :315-387): FocalLoss(gamma = 2) on the class logits,
 * SmoothL1Loss on the deltas, IoU target + BCE on the IoU logits; 4 + 2 kernel launches.
 * Head outputs NCHW (g->layout == IA_LAYOUT_NCHW), per-level targets as ia_anchor_targets
 * writes them.  With g->cls_activation == IA_CLS_SIGMOID_NOIOU (the plain RetinaHead,
 * anchor_head.py:234-299) the same entries compute FocalLoss + SmoothL1Loss alone: NULL IoU
 * pointers, losses_iou written as 0 (see ia_head_geom.cls_activation).                */
typedef struct ia_head_targets {
    const int64_t *labels[IA_MAX_LEVELS];        /* (B, N_l) int64 in 0..C                 */
    const float *label_weights[IA_MAX_LEVELS];   /* (B, N_l)                               */
    const float *bbox_targets[IA_MAX_LEVELS];    /* (B, N_l, 4)                            */
    const float *bbox_weights[IA_MAX_LEVELS];    /* (B, N_l, 4)                            */
    /* avg_factor (num_total_samples), first non-NULL / positive of:                       */
    const int32_t *counts;                       /* (B,2) of ia_anchor_targets: sum_b max(pos_b,1) */
    const float *avg_factor_dev;                 /* device scalar                          */
    float avg_factor;                            /* host value                             */
} ia_head_targets;

typedef struct ia_head_loss_cfg {
    float gamma, alpha, loss_weight_cls;         /* FocalLoss; gamma must be 2             */
    float beta, loss_weight_bbox;                /* SmoothL1Loss                           */
    int32_t attach_iou_target;                   /* gradient through the IoU target (reference: yes) */
    int32_t exact_large_logits;                  /* class logits > 60: the loss VALUE of such a negative
                                                    element saturates at 60 unless this is set (one more
                                                    pass over the logits); gradients are exact either way */
    int32_t grad_rows_start_at_reg;              /* ia_head_loss_bwd_nhwc only.  The caller STATES that in every
                                                    level grads->reg[l] is channel 0 of its pixel row of
                                                    grad_strides->reg[l] floats and grads->iou[l] == grads->reg[l]
                                                    + 4 A in the same row; the backward then also writes the zero
                                                    gradient of the row's remaining stride - 5 A (<= 64) channels.
                                                    0 (e.g. a row laid out [X | reg | iou | pad]): only the reg /
                                                    iou slices are written, the caller clears the rest.  Nothing is
                                                    inferred from the pointers alone.  Zero-initialise
                                                    this struct: it has grown since round 4.               */
    /* IoU-balanced losses of the IoU-aware head (IOUbalancedSigmoidFocalLoss / IoUbalancedSmoothL1Loss,
     * core/loss/losses.py:309-374,416-458); all zero: the plain losses above.  With iou_n the (detached)
     * IoU of anchor n's decoded prediction with its decoded target -- the IoU branch's regression target:
     *   balanced_cls: loss_cls[l] = loss_weight_cls * (S0 + norm_l * S2) / avg_factor, S0 the focal sum over
     *     the elements with target 0, S1 over the positive elements, S2 the same with every term times
     *     iou_n^eta, norm_l = S1 / (S2 + 1e-6) (detached; 0 on a level without positives); the gradient of
     *     a positive element is the focal derivative times iou_n^eta * norm_l.  eta > 0.
     *   balanced_loc: smooth-L1 value and derivative of an anchor times iou_n^delta.  delta > 0.
     * Either flag with IA_CLS_SIGMOID_NOIOU, or with an exponent <= 0: IA_E_ARG.                        */
    float eta, delta;
    int32_t balanced_cls, balanced_loc;
} ia_head_loss_cfg;

/* workspace (256-byte aligned, ia_head_loss_workspace_bytes): the fp64 partial sums and an
 * anchor-major copy of labels / label_weights that the forward call writes and the backward
 * call reads -- keep it alive and untouched between the two.
 * result: (3L + 4) fp32 = loss_cls[L] | loss_bbox[L] | losses_iou[L] | their sums over the
 * levels [3] | avg_factor -- each loss = loss_weight * (sum / avg_factor).              */
size_t ia_head_loss_workspace_bytes(const ia_head_geom *g, int batch);
/* The size for a given cfg: with cfg->balanced_cls two more rows of fp64 partial sums per level (S1, S2)
 * -- for ia_head_loss_fwd; ia_head_loss_fwd_nhwc then takes 8 * 5 L * IA_LOSS_SLOTS bytes instead of
 * 8 * 3 L * IA_LOSS_SLOTS.  A balanced forward call with less returns IA_E_ARG before anything is
 * enqueued.  With balanced_cls the result vector is (4L + 4) fp32: the layout above, then norm_l[L],
 * which the backward calls read from it (grad_result stays 3L + 3).                              */
size_t ia_head_loss_workspace_bytes_cfg(const ia_head_geom *g, int batch, const ia_head_loss_cfg *cfg);
int ia_head_loss_fwd(const ia_head_geom *g, const ia_level_ptrs *p, int dtype, int batch,
                     const ia_head_targets *t, const ia_head_loss_cfg *cfg, void *workspace,
                     size_t workspace_bytes, float *result, void *stream);
/* grad_result: (3L + 3) fp32 upstream gradients in result's order (per-level entries and the
 * three totals add up); grads: fp32 NCHW tensors shaped like the head outputs.          */
int ia_head_loss_bwd(const ia_head_geom *g, const ia_level_ptrs *p, int dtype, int batch,
                     const ia_head_targets *t, const ia_head_loss_cfg *cfg, const void *workspace,
                     const float *result, const float *grad_result, const ia_level_ptrs *grads,
                     void *stream);

/* The same losses on CHANNELS-LAST fp32 head outputs (what the training head of
 * iouaware/winograd_train.py produces): element (b, p, a, c) of a class map at
 * (b*HW + p) * pix_stride + a*C + c -- the reference's flattened order
 * cls_score.permute(0, 2, 3, 1).reshape(-1, C) (iou_aware_retina_head.py:236-240) in place, so the
 * anchor-major targets index it directly (no packed copy; the workspace holds only the fp64 sums).
 * pix_stride (elements) may exceed the map's own channel count: reg / iou may be channel slices
 * of one wider tensor.  C % 4 == 0; cls / reg pointers and strides 16-byte aligned.  g->layout is
 * not consulted.  Gradients are written with their own pixel strides (e.g. into the slices of one
 * tensor shaped like the wider one).  With cfg->grad_rows_start_at_reg set -- reg is channel 0 of the
 * gradient's pixel row, iou right behind it (iou == reg + 4 A, equal strides; IA_E_ARG when the pointers
 * contradict the flag) -- the backward also writes the zero gradient of the row's remaining channels
 * (stride - 5 A of them, alignment padding) and the caller need not clear them; without the flag it writes
 * the reg / iou slices and nothing else. */
typedef struct ia_level_pix_strides {
    int64_t cls[IA_MAX_LEVELS], reg[IA_MAX_LEVELS], iou[IA_MAX_LEVELS];
} ia_level_pix_strides;
int ia_head_loss_fwd_nhwc(const ia_head_geom *g, const ia_level_ptrs *p,
                          const ia_level_pix_strides *strides, int batch, const ia_head_targets *t,
                          const ia_head_loss_cfg *cfg, void *workspace, size_t workspace_bytes,
                          float *result, void *stream);
int ia_head_loss_bwd_nhwc(const ia_head_geom *g, const ia_level_ptrs *p,
                          const ia_level_pix_strides *strides, int batch, const ia_head_targets *t,
                          const ia_head_loss_cfg *cfg, const float *result, const float *grad_result,
                          const ia_level_ptrs *grads, const ia_level_pix_strides *grad_strides,
                          void *stream);

/* The localisation loss of the four entries above as a choice: ia_head_loss_cfg keeps its layout, the choice
 * travels in a struct of its own.  kind IA_BOX_SMOOTH_L1: SmoothL1Loss (cfg->beta), alpha / gamma not looked at;
 * IA_BOX_BALANCED_L1: BalancedL1Loss (losses.py:482-520; ia_balanced_l1_fwd) with knee cfg->beta, weight
 * cfg->loss_weight_bbox and the alpha / gamma given here -- on every layout and dtype of the entries above, with
 * or without the IoU term (with it d(bbox_pred) = the BalancedL1 gradient + the gradient through the attached
 * IoU target, as for smooth-L1).  Focal kernels, slots, result layout and workspace size are those of the
 * entries above, which call these with box = NULL.  Contract:
 *   box == NULL or kind IA_BOX_SMOOTH_L1: the bits of the entry above;
 *   IA_E_ARG before anything is enqueued for: struct_size != sizeof(ia_box_loss_cfg); an unknown kind;
 *   IA_BOX_BALANCED_L1 together with cfg->balanced_loc (the IoU-balanced weighting belongs to smooth-L1);
 *   IA_BOX_BALANCED_L1 with alpha, gamma or cfg->beta not > 0.
 *   IA_BOX_BALANCED_L1 with cfg->balanced_cls is allowed (the focal kernels do not depend on the choice).
 * The backward call takes the struct the forward call took.                                             */
#define IA_BOX_SMOOTH_L1 0
#define IA_BOX_BALANCED_L1 1
typedef struct ia_box_loss_cfg {
    int32_t struct_size;                         /* sizeof(ia_box_loss_cfg)                           */
    int32_t kind;                                /* IA_BOX_*                                          */
    float alpha, gamma;                          /* BalancedL1Loss(alpha, gamma)                      */
} ia_box_loss_cfg;
int ia_head_loss_fwd_box(const ia_head_geom *g, const ia_level_ptrs *p, int dtype, int batch,
                         const ia_head_targets *t, const ia_head_loss_cfg *cfg, const ia_box_loss_cfg *box,
                         void *workspace, size_t workspace_bytes, float *result, void *stream);
int ia_head_loss_bwd_box(const ia_head_geom *g, const ia_level_ptrs *p, int dtype, int batch,
                         const ia_head_targets *t, const ia_head_loss_cfg *cfg, const ia_box_loss_cfg *box,
                         const void *workspace, const float *result, const float *grad_result,
                         const ia_level_ptrs *grads, void *stream);
int ia_head_loss_fwd_nhwc_box(const ia_head_geom *g, const ia_level_ptrs *p,
                              const ia_level_pix_strides *strides, int batch, const ia_head_targets *t,
                              const ia_head_loss_cfg *cfg, const ia_box_loss_cfg *box, void *workspace,
                              size_t workspace_bytes, float *result, void *stream);
int ia_head_loss_bwd_nhwc_box(const ia_head_geom *g, const ia_level_ptrs *p,
                              const ia_level_pix_strides *strides, int batch, const ia_head_targets *t,
                              const ia_head_loss_cfg *cfg, const ia_box_loss_cfg *box, const float *result,
                              const float *grad_result, const ia_level_ptrs *grads,
                              const ia_level_pix_strides *grad_strides, void *stream);

/* ------------------------------------------------------------------ ResNeXt grouped 3x3 convolution
 * conv2 of the ResNeXt bottleneck (mmdet/models/backbones/resnext.py:12-91: groups = 32 / 64,
 * 4 / 8 / 16 / 32 channels per group), channels-last fp32, pad 1, stride 1 or 2, + per-channel
 * bias (the folded BatchNorm shift) + optional ReLU, on v_mfma_f32_16x16x4_f32.
 * ia_grouped_conv3x3_pack is HOST code: weight (C, C/groups, 3, 3) and optional per-output-channel
 * scale (folded BatchNorm scale) -> wpack, C/16 * 9 * 16 * 64 floats for <= 16 channels per
 * group, C/32 * 9 * 64 * 64 for 32 (host pointers); copy wpack to the device once.        */
int ia_grouped_conv3x3_pack(const float *weight, const float *scale, int channels, int groups,
                            float *wpack);
int ia_grouped_conv3x3_nhwc(const float *x, const float *wpack, const float *bias, float *y,
                            int batch, int H, int W, int channels, int groups, int stride, int relu,
                            void *stream);

/* Training (csrc/gconv_bwd.hip): the same layout and shapes -- channels-last fp32, x / dz / dx
 * 16-byte aligned, 4 / 8 / 16 / 32 channels per group, channels % 16 == 0 (% 32 for 32 per group),
 * pad 1, stride 1 or 2, H / W the INPUT size, Ho = (H - 1) / stride + 1; anything else is IA_E_ARG
 * before the first enqueue, nothing written.  All pointers are DEVICE pointers.
 * ia_grouped_conv3x3_pack_dev: one launch; weight (C, C/groups, 3, 3) contiguous (+ optional
 *   per-output-channel scale) -> wpack in the layout of ia_grouped_conv3x3_pack.  adjoint = 0: the
 *   bits of the host pack; adjoint = 1: the weight of the input-gradient convolution (taps flipped
 *   in both directions, input and output channel swapped inside each group, scale ignored);
 *   adjoint = 2: both in one launch, wpack twice the size -- the adjoint = 0 pack, then the
 *   adjoint = 1 pack (the scale applies to the first only).
 * ia_grouped_conv3x3_bwd_data_nhwc: dz (B, Ho, Wo, C) and the ADJOINT pack -> dx (B, H, W, C),
 *   every element written; stride 1 is the forward kernel on the adjoint pack, stride 2 a gather
 *   kernel (terms whose output row / column does not exist are masked).  No atomics.
 * ia_grouped_conv3x3_bwd_weight_nhwc: x (B, H, W, C), dz (B, Ho, Wo, C) -> dw (C, C/groups, 3, 3)
 *   contiguous; the reduction over the pixels is cut into slices of output rows whose partial
 *   results go to `workspace` (ia_grouped_conv3x3_bwd_weight_workspace_bytes, 0 for a shape that
 *   is not covered; a smaller workspace is IA_E_ARG; need not be initialised) and are added in a
 *   fixed order: the same bits in every run.                                                  */
int ia_grouped_conv3x3_pack_dev(const float *weight, const float *scale, int channels, int groups,
                                int adjoint, float *wpack, void *stream);
int ia_grouped_conv3x3_bwd_data_nhwc(const float *dz, const float *wpack_adjoint, float *dx, int batch,
                                     int H, int W, int channels, int groups, int stride, void *stream);
size_t ia_grouped_conv3x3_bwd_weight_workspace_bytes(int batch, int H, int W, int channels, int groups,
                                                     int stride);
int ia_grouped_conv3x3_bwd_weight_nhwc(const float *x, const float *dz, float *dw, void *workspace,
                                       size_t workspace_bytes, int batch, int H, int W, int channels,
                                       int groups, int stride, void *stream);

/* The bf16 twin (csrc/gconv_bf16.hip): channels-last bf16 in and out, fp32 accumulation on
 * v_mfma_f32_16x16x32_bf16, fp32 bias (+ ReLU) in fp32, one round-to-nearest-even to bf16 at the
 * store.  A wavefront owns 32 consecutive channels: channels % 32 == 0, 4 / 8 / 16 / 32 channels
 * per group, stride 1 or 2, x / y / wpack 16-byte aligned, batch * Ho <= INT32_MAX; anything else
 * is IA_E_ARG before the device is touched.
 * ia_grouped_conv3x3_pack_bf16 is HOST code: fp32 weight (C, C/groups, 3, 3) and optional fp32
 * per-output-channel scale -> wpack (host pointer) of ia_grouped_conv3x3_packed_bytes_bf16 bytes
 * (0 for an unsupported shape), laid out (C/32, 9, 2, 64, 8):
 *   wpack[(((sg * 9 + t) * 2 + co) * 64 + lane) * 8 + j] = bf16(scale[o] * weight[o][in % Cg][t])
 *   with o = 32 sg + 16 co + (lane & 15), in = 32 sg + 8 (lane >> 4) + j, the product in fp32 and
 *   rounded to nearest even once; 0 where o and in lie in different groups.
 * Copy wpack to the device once.                                                            */
size_t ia_grouped_conv3x3_packed_bytes_bf16(int channels, int groups);
int ia_grouped_conv3x3_pack_bf16(const float *weight, const float *scale, int channels, int groups,
                                 uint16_t *wpack);
int ia_grouped_conv3x3_bf16_nhwc(const uint16_t *x, const uint16_t *wpack, const float *bias,
                                 uint16_t *y, int batch, int H, int W, int channels, int groups,
                                 int stride, int relu, void *stream);

/* mmdet.ops.sigmoid_focal_loss: sigmoid_focal_loss_cuda.forward / .backward
 * (mmdet/ops/sigmoid_focal_loss/src/sigmoid_focal_loss_cuda.cu:23-63,65-105;
 * binding sigmoid_focal_loss.cpp:17-43).  logits (N,C) fp32, targets (N) int64,
 * losses / d_losses / d_logits (N,C) fp32.                                    */
int ia_sigmoid_focal_loss_fwd(const float *logits, const int64_t *targets, int N, int C,
                              float gamma, float alpha, float *losses, void *stream);
int ia_sigmoid_focal_loss_bwd(const float *logits, const int64_t *targets, const float *d_losses,
                              int N, int C, float gamma, float alpha, float *d_logits,
                              void *stream);
/* The same for every storage type the reference op is instantiated for
 * (AT_DISPATCH_FLOATING_TYPES_AND_HALF: float, double, half -- sigmoid_focal_loss_cuda.cu:128,166)
 * plus bf16: dtype = IA_F32 / IA_F64 / IA_F16 / IA_BF16 is the type of logits, losses, d_losses and
 * d_logits.  Like the reference kernel (expf / powf / logf) the arithmetic is single precision
 * whatever the storage type; the result is rounded once at the store.                          */
int ia_sigmoid_focal_loss_fwd_dt(const void *logits, int dtype, const int64_t *targets, int N, int C,
                                 float gamma, float alpha, void *losses, void *stream);
int ia_sigmoid_focal_loss_bwd_dt(const void *logits, int dtype, const int64_t *targets,
                                 const void *d_losses, int N, int C, float gamma, float alpha,
                                 void *d_logits, void *stream);

/* ------------------------------------------------------------------ conv epilogues
 * In place on an NCHW tensor x (N, C, HW contiguous):
 *   x = act(x * scale[c] + shift[c] [+ residual * res_scale[c] + res_shift[c]]).
 * Any of scale / shift / res_scale / res_shift may be NULL (1 / 0).  Fuses the
 * eval-mode BatchNorm -> (+identity) -> ReLU chains of the reference Bottleneck
 * (mmdet/models/backbones/resnet.py:215-255) and ConvModule's bias -> ReLU
 * (mmdet/models/utils/conv_module.py:149-163) into one pass per convolution.   */
int ia_channel_affine_act(void *x, int dtype, const float *scale, const float *shift,
                          const void *residual, const float *res_scale, const float *res_shift,
                          int relu, int N, int C, int64_t HW, void *stream);
/* the same on a channels-last tensor: x is (N, H, W, C) in memory (NHW = N*H*W);
 * C must be a multiple of 4 (fp32) / 8 (bf16); x, residual and every per-channel
 * vector given must be 16-byte aligned (IA_E_ARG otherwise).  With ReLU a NaN
 * stays a NaN, as in torch.relu.                                               */
int ia_channel_affine_act_nhwc(void *x, int dtype, const float *scale, const float *shift,
                               const void *residual, const float *res_scale,
                               const float *res_shift, int relu, int64_t NHW, int C, void *stream);

/* (N, H*W, C) channels-last memory -> (N, C, H*W) NCHW memory (LDS-tiled transpose): lets the
 * convolutions run in MIOpen's NHWC kernels while the head kernels read NCHW.    */
int ia_nhwc_to_nchw(const void *src, void *dst, int dtype, int N, int C, int64_t HW, void *stream);

/* ResNet stem at inference (mmdet/models/backbones/resnet.py:506-512): folded BatchNorm + ReLU +
 * MaxPool2d(kernel 3, stride 2, padding 1) in one pass.  x (B,H,W,C) channels-last fp32, C % 4 == 0;
 * out (B, (H-1)/2+1, (W-1)/2+1, C).                                                          */
int ia_affine_relu_maxpool_nhwc(const float *x, const float *scale, const float *shift, int B, int H,
                                int W, int C, float *out, void *stream);
/* the same for dtype IA_F32 / IA_BF16 (C % 4 / C % 8 == 0): fp32 arithmetic, a bf16 result is
 * rounded once -- equal to eager's affine -> ReLU -> max-pool on bf16 values.  IA_F32 propagates a
 * NaN as eager does (an output is NaN exactly when a tap of its window is); IA_BF16 drops it (the
 * maximum of the other taps, or 0): a known difference, DESIGN 3.26.                              */
int ia_affine_relu_maxpool_nhwc_dt(const void *x, int dtype, const float *scale, const float *shift,
                                   int B, int H, int W, int C, void *out, void *stream);

/* FPN top-down step, in place (mmdet/models/necks/fpn.py:118-120): fine += nearest-x2(coarse);
 * channels-last fp32, H = 2*Hc, W = 2*Wc, C % 4 == 0.                                          */
int ia_upsample2x_add_nhwc(float *fine, const float *coarse, int B, int H, int W, int Hc, int Wc,
                           int C, void *stream);
/* dtype IA_F32 / IA_BF16 (C % 4 / C % 8 == 0); bf16: one rounding of the fp32 sum, like eager's add */
int ia_upsample2x_add_nhwc_dt(void *fine, const void *coarse, int dtype, int B, int H, int W, int Hc,
                              int Wc, int C, void *stream);

/* The ResNet stem convolution (resnet.py:403-414 `conv1`: 7x7 / stride 2 / pad 3, 3 -> 64, no bias;
 * forward :506-512) on a channels-last fp32 image batch as an implicit GEMM on fp32 MFMA
 * (csrc/stem.hip): x (B, H, W, 3), w_packed (148, 64) with row ky * 21 + kx * 3 + c = w[:, c, ky, kx]
 * and a zero row 147, y (B, Ho, Wo, 64) = the RAW convolution, Ho = (H - 1) / 2 + 1.  The folded
 * BatchNorm + ReLU + max-pool behind it: ia_affine_relu_maxpool_nhwc.                            */
int ia_stem_conv7x7s2(const float *x, const float *w_packed, float *y, int B, int H, int W,
                      void *stream);
/* The same convolution on bf16 (BASELINE config 3) on v_mfma_f32_16x16x16_bf16: x (B, H, W, 3) bf16,
 * y (B, Ho, Wo, 64) bf16 (fp32 accumulation, one rounding), w_packed = 11 x 4 x 64 x 4 bf16 in
 * fragment order: element [s][nb][lane][e] = w[nb * 16 + (lane & 15)][k = 16 s + 4 (lane >> 4) + e]
 * with k = ky * 24 + 1 + kx * 3 + c (zero at the other positions and for ky = 7).                                    */
int ia_stem_conv7x7s2_bf16(const void *x, const void *w_packed, void *y, int B, int H, int W,
                           void *stream);

/* 1x1 convolutions of ResNet stage 1 (resnet.py:215-255, folded BatchNorm) as a streaming MFMA
 * kernel with the weights resident in LDS (csrc/conv1x1_stream.hip): y = relu?(x . w + bias
 * (+ residual)), fp32, x (rows, k), w (k, n) row-major, (k, n) in {(64, 256), (256, 64), (64, 64)}. */
int ia_conv1x1_stream(const float *x, const float *w, const float *bias, const float *residual,
                      float *y, int64_t rows, int k, int n, int relu, void *stream);
/* The boundary between two stage-1 bottlenecks in one pass (resnet.py:215-255: conv3 + bn3 + add +
 * ReLU of a block, then conv1 + bn1 + ReLU of the next): y = relu(x . w + bias + residual) (rows, n)
 * is stored and, from the accumulators, h = relu(y . w2 + bias2) (rows, n2) -- the second product
 * does not read y back.  fp32, (k, n, n2) = (64, 256, 64), residual / biases may be NULL.      */
int ia_conv1x1_chain(const float *x, const float *w, const float *bias, const float *residual,
                     const float *w2, const float *bias2, float *y, float *h, int64_t rows, int k,
                     int n, int n2, void *stream);
/* The same streaming product for a wide output row: (k, n) = (128, 512), column blocks of 256
 * channels per workgroup (ResNet stage 2: conv3 + bn3 + identity + ReLU, resnet.py:215-255).   */
int ia_conv1x1_wide(const float *x, const float *w, const float *bias, const float *residual,
                    float *y, int64_t rows, int k, int n, int relu, void *stream);

/* ------------------------------------------------------------------ bf16 3x3 convolution
 * 3x3 / stride 1 / pad 1 convolution + bias (+ReLU) on bf16 channels-last tensors, fp32
 * accumulation: the tower / output / FPN ConvModules of BASELINE config 3 (reference
 * mmdet/models/utils/conv_module.py:149-163, iou_aware_retina_head.py:171-219) as an implicit GEMM
 * on v_mfma_f32_32x32x16_bf16 (csrc/conv3x3_bf16.hip).  One launch covers a list of feature maps
 * (the pyramid levels the head's weights are shared over) and up to two groups (the cls and the
 * reg tower: own inputs, weights, outputs).  cin % 32 == 0, cout even (per group).
 * ia_conv3x3_bf16_pack: weights (groups * cout, 3, 3, cin) bf16 (= a channels-last
 * (groups * cout, cin, 3, 3) tensor) -> the kernel's layout, ia_conv3x3_bf16_packed_bytes bytes,
 * once per model.  bias (groups * cout) fp32 or NULL.
 * ia_conv3x3_bf16_plan: the geometry ia_conv3x3_bf16_levels would launch for this descriptor, per
 * level l < num_levels (host only: launches nothing, does not look at the pointers; any output may be
 * NULL): variant[l] = 100 * MB + 10 * WM + WN of the kernel instance (414, 214, 222, 141 or 122: four
 * wavefronts as WM x WN, each 32 * MB pixels x 64 channels), the TH[l] x TW[l] pixel tile and the
 * tiles_y[l] x tiles_x[l] tiles per image.  The launcher's own code computes it (IA_CONV3_VARIANT, a
 * timing aid read on every call, included).  IA_E_ARG where the launcher would refuse the sizes.    */
typedef struct ia_conv3x3_desc {
    int32_t num_levels, batch, groups;
    int32_t cin, cout;                    /* channels per group                                   */
    int32_t x_stride, y_stride;           /* elements between pixels of x / y (>= cin / cout)     */
    int32_t H[IA_MAX_LEVELS], W[IA_MAX_LEVELS];
    const void *x[2][IA_MAX_LEVELS];      /* [group][level] -> (batch, H, W, x_stride) bf16, 16-byte aligned */
    void *y[2][IA_MAX_LEVELS];            /* [group][level] -> (batch, H, W, y_stride) bf16       */
} ia_conv3x3_desc;
size_t ia_conv3x3_bf16_packed_bytes(int cin, int cout, int groups);
int ia_conv3x3_bf16_pack(const void *w, int cin, int cout, int groups, void *wp, void *stream);
int ia_conv3x3_bf16_levels(const ia_conv3x3_desc *d, const void *wp, const float *bias, int relu, void *stream);
int ia_conv3x3_bf16_plan(const ia_conv3x3_desc *d, int32_t *variant, int32_t *TH, int32_t *TW, int32_t *tiles_y,
                         int32_t *tiles_x);

/* ------------------------------------------------------------------ bf16 training of the convolution above
 * (csrc/conv3x3_bf16_bwd.hip): bf16 activations and gradients, fp32 master weights.
 *   ia_conv3x3_bf16_wgrad_levels: the weight gradient of one weight shared by d->num_levels levels and
 *     d->groups groups.  The descriptor is the forward one with y = dy (the gradient w.r.t. the
 *     convolution's output, pixel stride y_stride >= cout):
 *       dw[g][co][ci][ky][kx] = sum_l sum_b sum_{y,x} dy_l[b,y,x,co] * x_l[b,y+ky-1,x+kx-1,ci]
 *     (zero outside the map), bf16 products accumulated in fp32 on v_mfma_f32_32x32x16_bf16; dw is fp32
 *     in the layout of an nn.Conv2d weight (groups * cout, cin, 3, 3).  cin % 32 == 0, any cout >= 1,
 *     maps down to 1 x 1; x as in the forward call (16-byte aligned, x_stride % 8 == 0); dy any 2-byte
 *     aligned pointer and any stride (16-byte loads when every dy pointer is 16-byte aligned and
 *     y_stride % 8 == 0, element loads otherwise).  IA_E_ARG outside that.
 *     The pixels of all levels and images are cut into 128-pixel tiles and the tile list into `slices`
 *     runs of `slice_tiles` tiles (ia_conv3x3_bf16_wgrad_plan reports both and the tile count; the
 *     last slice may be shorter); each slice's fp32 partial result goes to the caller's workspace
 *     (ia_conv3x3_bf16_wgrad_workspace_bytes, 16-byte aligned; 0 for a descriptor that is not covered --
 *     the query does not look at the pointers) and a second kernel adds the partials in slice order:
 *     no atomics, the same bits on every run, the workspace need not be initialised and nothing of it is
 *     read that this call did not write.
 *   ia_conv3x3_bf16_pack_f32: w fp32 (groups * cout, cin, 3, 3), dense -> rounded to bf16 (nearest even)
 *     in the packed layout of ia_conv3x3_bf16_pack, one launch.  adjoint = 0: the forward weight,
 *     ia_conv3x3_bf16_packed_bytes(cin, cout, groups) bytes.  adjoint = 1: the weight of the
 *     input-gradient convolution, w'[ci][co][ky][kx] = w[co][ci][2-ky][2-kx], a convolution with
 *     cout' = cin outputs and cin' = cout rounded up to a multiple of 32 inputs, the padded input
 *     channels being ZERO weight rows: ia_conv3x3_bf16_packed_bytes(cin', cin, groups) bytes, and
 *     dx = ia_conv3x3_bf16_levels on dy tensors of (at least) cin' channels per pixel whose padding is
 *     finite.  cin % 32 == 0, cout >= 1.
 *   ia_relu_bwd_bias_grad_bf16: the bf16 instance of ia_relu_bwd_bias_grad with row strides (elements;
 *     each >= n): g = dy where y > 0, else a zero with dy's sign (= dy * (y > 0) for finite dy);
 *     y == NULL: no mask, g = dy (g == NULL: nothing written); db[n] fp32 = column sums of g through
 *     per-strip partial rows added in a fixed order (db == NULL: not computed; then no workspace).  Any
 *     n >= 1; 16-byte accesses when n % 8 == 0 and every pointer and stride allows them.            */
size_t ia_conv3x3_bf16_wgrad_workspace_bytes(const ia_conv3x3_desc *d);
int ia_conv3x3_bf16_wgrad_plan(const ia_conv3x3_desc *d, int32_t *tiles, int32_t *slice_tiles, int32_t *slices);
int ia_conv3x3_bf16_wgrad_levels(const ia_conv3x3_desc *d, float *dw, void *workspace, size_t workspace_bytes,
                                 void *stream);
int ia_conv3x3_bf16_pack_f32(const float *w, int cin, int cout, int groups, int adjoint, void *wp, void *stream);
size_t ia_relu_bwd_bias_grad_bf16_workspace_bytes(int64_t rows, int n);
int ia_relu_bwd_bias_grad_bf16(const void *dy, int64_t dy_stride, const void *y, int64_t y_stride, int64_t rows,
                               int n, void *g, int64_t g_stride, float *db, void *workspace,
                               size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ IoU-aware FCOS
 * GroupNorm + ReLU of the FCOS head towers (reference mmdet/models/anchor_heads/
 * iou_aware_fcos_head.py:41-62: ConvModule(3x3, no bias, GN(32), ReLU); torch nn.GroupNorm:
 * biased variance, y = (x - mean) / sqrt(var + eps) * gamma + beta) at inference, on the
 * activations the Winograd output transform writes: per level x[l] (batch, H_l, W_l, channels)
 * fp32 channels-last (both towers side by side: channels = 2 * 256, groups = 2 * 32, gamma / beta
 * of the two towers concatenated).  Statistics per (level, image, group) over channels / groups
 * channels x H_l x W_l values.
 *   ia_groupnorm_stats: per workgroup (level, image, chunk of IA_GN_CHUNK pixels) fp64 sums and
 *     sums of squares per group, written to the workspace (no atomics).
 *   ia_groupnorm_apply: every workgroup sums its (level, image)'s partials in index order (fp64:
 *     mean, var = E[x^2] - mean^2 stays accurate for |mean| >> std), s = gamma * rstd,
 *     t = beta - mean * s per channel, then x = relu?(x * s + t) in place, 16-byte accesses.
 * Same bits from run to run; an image's result does not depend on the other images / levels of
 * the launch.  channels: 4 * 2^k, <= 1024; groups divides channels, channels / groups % 4 == 0;
 * x[l] 16-byte aligned.  Pairs on one stream, the workspace untouched in between.            */
#define IA_GN_CHUNK 256
size_t ia_groupnorm_workspace_bytes(const ia_wino_geom *g, int channels, int groups);
int ia_groupnorm_stats(const ia_wino_geom *g, const float *const *x, int channels, int groups,
                       void *workspace, size_t workspace_bytes, void *stream);
int ia_groupnorm_apply(const ia_wino_geom *g, float *const *x, int channels, int groups,
                       const float *gamma, const float *beta, float eps, int relu,
                       const void *workspace, size_t workspace_bytes, void *stream);
/* The inference triple for dtype IA_F32 / IA_BF16 activations (gamma, beta, eps, the workspace and
 * its contract as above).  IA_F32: the entries above, same bits.  IA_BF16: x[l] (batch, H_l, W_l,
 * channels) bf16 channels-last, normalised in place -- fp64 sums of the exactly converted values,
 * added in a fixed order (a thread's 16-byte column is 8 channels of one group); s = gamma * rstd
 * and t = beta - mean * s formed in fp64 and rounded once to fp32; y = relu?(x * s + t) in fp32 and
 * ONE round-to-nearest-even to bf16; 16-byte loads and stores.  Same bits from run to run; an
 * image's result does not depend on the other images / levels of the launch.
 * What IA_BF16 covers: channels a power of two, 8 <= channels <= 1024; 1 <= groups <= 256, groups
 * divides channels and channels / groups % 8 == 0; x[l] 16-byte aligned.  The size query returns 0
 * for anything else (and for any other dtype); the two launches then return IA_E_ARG.          */
size_t ia_groupnorm_workspace_bytes_dt(const ia_wino_geom *g, int channels, int groups, int dtype);
int ia_groupnorm_stats_dt(const ia_wino_geom *g, const void *const *x, int dtype, int channels,
                          int groups, void *workspace, size_t workspace_bytes, void *stream);
int ia_groupnorm_apply_dt(const ia_wino_geom *g, void *const *x, int dtype, int channels, int groups,
                          const float *gamma, const float *beta, float eps, int relu,
                          const void *workspace, size_t workspace_bytes, void *stream);
/* The same GroupNorm + ReLU as a training node, out of place (csrc/groupnorm.hip).  Forward:
 * ia_groupnorm_stats on x, then
 *   ia_groupnorm_apply_to: y[l] = relu?(x[l] * s + t), the bits ia_groupnorm_apply leaves in x;
 *     x is only read, y[l] != x[l].  saved (ia_groupnorm_saved_bytes, caller-owned) receives
 *     (mean, rstd) in fp64 per (level, image, group): with x, all the backward needs.
 * Backward, with xh = (x - mean) * rstd, g = dy * [x * s + t > 0] (the forward's fp32 expression,
 * so the forward's mask bit for bit; g = dy with relu == 0), n = channels / groups * H_l * W_l:
 *     dbeta_c = sum g,  dgamma_c = sum g * xh   over all pixels, images and levels
 *     dx = rstd * (gamma * g - mean_grp(gamma * g) - xh * mean_grp(gamma * g * xh))
 *   ia_groupnorm_bwd_reduce: per workgroup (level, image, chunk) fp64 partials of the two sums per
 *     channel and, weighted by gamma, per group, to workspace (ia_groupnorm_bwd_workspace_bytes).
 *   ia_groupnorm_bwd_apply: adds the group partials of a (level, image) in chunk order and writes
 *     dx[l] (dx == NULL: skipped; dx[l] != dy[l], x[l]); then adds the per-channel partials in a
 *     fixed order (16 contiguous runs of the level-major / image / chunk rows, each in index order,
 *     then the runs in index order) into dgamma / dbeta (channels) fp32, either may be NULL.
 * dy and x are only read.  No atomics: same bits from run to run, and an image's y and dx do not
 * depend on the other images / levels of the launch.  relu, gamma and beta as in the forward call.
 * All five entries: channels a power of two, 4 <= channels <= 1024; 1 <= groups <= 256, groups
 * divides channels and channels / groups % 4 == 0; x[l], y[l], dy[l], dx[l], saved and workspace
 * 16-byte aligned; the calls of a forward, and those of a backward, on one stream with the
 * workspace untouched in between.  The size queries return 0 for what the kernels do
 * not cover.                                                                                  */
size_t ia_groupnorm_saved_bytes(const ia_wino_geom *g, int channels, int groups);
int ia_groupnorm_apply_to(const ia_wino_geom *g, const float *const *x, float *const *y,
                          int channels, int groups, const float *gamma, const float *beta,
                          float eps, int relu, const void *workspace, size_t workspace_bytes,
                          void *saved, size_t saved_bytes, void *stream);
size_t ia_groupnorm_bwd_workspace_bytes(const ia_wino_geom *g, int channels, int groups);
int ia_groupnorm_bwd_reduce(const ia_wino_geom *g, const float *const *x, const float *const *dy,
                            int channels, int groups, const float *gamma, const float *beta,
                            int relu, const void *saved, size_t saved_bytes, void *workspace,
                            size_t workspace_bytes, void *stream);
int ia_groupnorm_bwd_apply(const ia_wino_geom *g, const float *const *x, const float *const *dy,
                           float *const *dx, int channels, int groups, const float *gamma,
                           const float *beta, int relu, const void *saved, size_t saved_bytes,
                           const void *workspace, size_t workspace_bytes, float *dgamma,
                           float *dbeta, void *stream);
/* The five training entries for dtype IA_F32 / IA_BF16 (everything else as above).  IA_F32: the
 * entries above, same bits.  IA_BF16: x[l], y[l], dy[l], dx[l] (batch, H_l, W_l, channels) bf16
 * channels-last; the forward pair is ia_groupnorm_stats_dt(IA_BF16) + ia_groupnorm_apply_to_dt.  A
 * thread's 16-byte column is 8 channels of one group.  x and dy widen exactly to fp32, so:
 *   y  = bf16(relu?(float(x) * s + t)): the bits ia_groupnorm_apply_dt(IA_BF16) leaves in x;
 *   g  = dy where the forward's fp32 pre-activation float(x) * s + t > 0 (y is not needed);
 *   sum g and sum g * x per channel in fp64 (exact products), the (mean, rstd), channel and group
 *     rows and the parameter-gradient pass of the fp32 node (dgamma / dbeta stay fp32);
 *   dx = bf16(s * g + (c1 + ((x - mean_hi) - mean_lo) * c2)): the fp32 entry's expression on the
 *     widened values, ONE round-to-nearest-even.
 * What IA_BF16 covers: channels a power of two, 8 <= channels <= 1024; 1 <= groups <= 256, groups
 * divides channels and channels / groups % 8 == 0; all pointers 16-byte aligned.  The size queries
 * return 0 for anything else (and for any other dtype); the launches then return IA_E_ARG.     */
size_t ia_groupnorm_saved_bytes_dt(const ia_wino_geom *g, int channels, int groups, int dtype);
int ia_groupnorm_apply_to_dt(const ia_wino_geom *g, const void *const *x, void *const *y, int dtype,
                             int channels, int groups, const float *gamma, const float *beta,
                             float eps, int relu, const void *workspace, size_t workspace_bytes,
                             void *saved, size_t saved_bytes, void *stream);
size_t ia_groupnorm_bwd_workspace_bytes_dt(const ia_wino_geom *g, int channels, int groups,
                                           int dtype);
int ia_groupnorm_bwd_reduce_dt(const ia_wino_geom *g, const void *const *x, const void *const *dy,
                               int dtype, int channels, int groups, const float *gamma,
                               const float *beta, int relu, const void *saved, size_t saved_bytes,
                               void *workspace, size_t workspace_bytes, void *stream);
int ia_groupnorm_bwd_apply_dt(const ia_wino_geom *g, const void *const *x, const void *const *dy,
                              void *const *dx, int dtype, int channels, int groups,
                              const float *gamma, const float *beta, int relu, const void *saved,
                              size_t saved_bytes, const void *workspace, size_t workspace_bytes,
                              float *dgamma, float *dbeta, void *stream);
/* The FCOS regression epilogue bbox_pred = exp(scale_l * x) (iou_aware_fcos_head.py:105) in place
 * on per-level (batch, H_l, W_l, channels) fp32 tensors (channels % 4 == 0, 16-byte aligned);
 * scales: (num_levels) fp32 device array (the head's Scale parameters).                      */
int ia_scale_exp_levels(const ia_wino_geom *g, float *const *x, int channels, const float *scales,
                        void *stream);
/* dtype IA_F32: the entry above.  IA_BF16: x[l] bf16 (channels % 4 == 0, 8-byte aligned), in place
 * bf16(exp(scale_l * float(x))): the fp32 entry's evaluation, rounded once (nearest even) -- the
 * bits of the fp32 entry on the widened tensor, converted to bf16.                             */
int ia_scale_exp_levels_dt(const ia_wino_geom *g, void *const *x, int dtype, int channels,
                           const float *scales, void *stream);

/* Point head (IoU-aware FCOS) post-processing: get_bboxes / get_bboxes_single of
 * iou_aware_fcos_head.py:248-370.  One point per position (no anchors), stored like the anchor
 * head's outputs with A = 1: cls (B, C, H, W), reg (B, 4, H, W) = the already exponentiated
 * distances (left, top, right, bottom), iou (B, 1, H, W); NCHW or channels-last (layout), fp32.
 *   score_c = powf(sigmoid(cls_c), score_alpha) * powf(sigmoid(iou), 1 - score_alpha)
 *     (:326-331, alpha = 0.3; centerness is not used, as in the reference);
 *   per level the row max over classes and the top nms_pre (score desc, index asc) (:335-345);
 *   point (x * stride + stride / 2, y * stride + stride / 2) (:379-388), distance2bbox clamped to
 *   [0, w-1] x [0, h-1] (mmdet/core/bbox/transforms.py:169-190), true division by scale_factor;
 *   the batched NMS of ia_get_bboxes (lazy: candidates >= 0, 0 = default; < 0: complete path).
 * Outputs and workspace contract as ia_get_bboxes (rows = candidate row ids; the candidate's
 * point index inside its level is cand_idx[row]).  ia_point_decode_stage: the decode stage only;
 * ia_point_workspace_layout: where it leaves rowmax, cand_idx, boxes, scores_t, keep_count,
 * keep_rows, best_score (offsets as ia_get_bboxes_workspace_layout).                        */
typedef struct ia_point_head_geom {
    int32_t num_levels;                 /* L <= IA_MAX_LEVELS */
    int32_t num_classes;                /* C (80) */
    int32_t nms_pre;                    /* <= 0: no per-level top-k */
    int32_t H[IA_MAX_LEVELS];
    int32_t W[IA_MAX_LEVELS];
    int32_t stride[IA_MAX_LEVELS];
    int32_t layout;                     /* IA_LAYOUT_* */
    float score_alpha;                  /* in [0, 1] */
} ia_point_head_geom;
size_t ia_point_workspace_bytes(const ia_point_head_geom *g, int batch);
int ia_point_workspace_layout(const ia_point_head_geom *g, int batch, size_t offsets[8]);
int ia_point_decode_stage(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                          const float *img_hw, const float *scale_factor, int rescale,
                          void *workspace, size_t workspace_bytes, void *stream);
int ia_point_get_bboxes(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                        const float *img_hw, const float *scale_factor, int rescale,
                        float score_thr, float iou_thr, int max_per_img, int candidates,
                        void *workspace, size_t workspace_bytes, float *dets, int32_t *labels,
                        int32_t *rows, int32_t *num, void *stream);

/* Plain FCOS (reference mmdet/models/anchor_heads/fcos_head.py:225-272 with multiclass_nms(...,
 * score_factors=centerness), mmdet/core/post_processing/bbox_nms.py:37-48): as the ia_point_*
 * entries above, same geometry (score_alpha ignored), workspace, outputs and tie rule, with
 * p->iou[l] = the centerness logits (B, 1, H, W) and these scores:
 *   rowmax = max_c sigmoid(cls_c) * sigmoid(ctr) (fp32 product; the per-level top nms_pre);
 *   scores_t[c] = sigmoid(cls_c) * sigmoid(ctr) where the RAW score sigmoid(cls_c) > score_thr
 *     (a product of 0 included), else a negative sentinel that no NMS stage, key or output row
 *     takes; best_score = the row maximum of what was written.
 * NMS and the final max_per_img sort use the product.  ia_point_ctr_decode_stage: the decode
 * stage only (it applies score_thr).                                                          */
int ia_point_ctr_decode_stage(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                              const float *img_hw, const float *scale_factor, int rescale,
                              float score_thr, void *workspace, size_t workspace_bytes, void *stream);
int ia_point_ctr_get_bboxes(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                            const float *img_hw, const float *scale_factor, int rescale,
                            float score_thr, float iou_thr, int max_per_img, int candidates,
                            void *workspace, size_t workspace_bytes, float *dets, int32_t *labels,
                            int32_t *rows, int32_t *num, void *stream);
/* The four point entries for dtype IA_F32 / IA_BF16 maps (one dtype for cls, reg and iou /
 * centerness; dtype after batch, as ia_get_bboxes has it).  A bf16 value converts exactly to fp32
 * when it is loaded and everything behind the load is the fp32 arithmetic: bf16 maps give the bits
 * the fp32 entries give on their widened copies.  Workspace, outputs and tie rule unchanged (scores
 * and boxes are fp32).  Channels-last bf16: C % 8 == 0 and 16-byte aligned cls pointers.        */
int ia_point_decode_stage_dt(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                             int dtype, const float *img_hw, const float *scale_factor, int rescale,
                             void *workspace, size_t workspace_bytes, void *stream);
int ia_point_get_bboxes_dt(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                           int dtype, const float *img_hw, const float *scale_factor, int rescale,
                           float score_thr, float iou_thr, int max_per_img, int candidates,
                           void *workspace, size_t workspace_bytes, float *dets, int32_t *labels,
                           int32_t *rows, int32_t *num, void *stream);
int ia_point_ctr_decode_stage_dt(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                                 int dtype, const float *img_hw, const float *scale_factor,
                                 int rescale, float score_thr, void *workspace,
                                 size_t workspace_bytes, void *stream);
int ia_point_ctr_get_bboxes_dt(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                               int dtype, const float *img_hw, const float *scale_factor,
                               int rescale, float score_thr, float iou_thr, int max_per_img,
                               int candidates, void *workspace, size_t workspace_bytes, float *dets,
                               int32_t *labels, int32_t *rows, int32_t *num, void *stream);

/* ------------------------------------------------------------------ FCOS training: point targets
 * fcos_target / fcos_target_single of fcos_head.py and iou_aware_fcos_head.py for a whole batch in
 * one launch.  Point (x * stride + stride / 2, y * stride + stride / 2) of level l; for gt g
 * left = px - x1, top = py - y1, right = x2 - px, bottom = y2 - py; g is a candidate iff
 * min(l,t,r,b) > 0 and lo_l <= max(l,t,r,b) <= hi_l (regress_ranges: HOST (L,2) fp32, both ends
 * inclusive); the candidate of minimal area (x2 - x1 + 1) * (y2 - y1 + 1) wins, equal areas: the
 * lowest gt index; an area >= 1e8 counts as no candidate (the reference's INF sentinel).  Every
 * quantity is one IEEE fp32 operation on fp32 inputs (no contraction): labels and targets are
 * bit-identical to the torch evaluation on the CPU.
 * gt_boxes / gt_labels / num_gt as ia_anchor_targets_ptrs: HOST arrays of per-image DEVICE
 * pointers (boxes 16-byte aligned), host num_gt[b] in 1..512, batch <= IA_MAX_TARGET_BATCH.
 * Geometry: ia_point_head_geom (nms_pre, layout, score_alpha ignored).
 * Outputs, level-major as ia_anchor_targets (level l a (B, N_l[,4]) block at element offset
 * B * point_off_l): labels int64 (0 = background, else gt_labels[g]); bbox_targets (l,t,r,b) of the
 * chosen gt, of gt 0 for a background point; counts (B) int32 positives per image.
 * packed (optional, ia_point_packed_labels_elems int32 elements, 16-byte aligned): the int32 copy of
 * the labels followed by fp32 weights of 1 that ia_point_head_loss_* read -- written here, the loss
 * needs no pack launch.                                                                       */
size_t ia_point_packed_labels_elems(const ia_point_head_geom *g, int batch);
int ia_point_targets_ptrs(const ia_point_head_geom *g, const float *const *gt_boxes,
                          const int64_t *const *gt_labels, const int32_t *num_gt, int batch,
                          const float *regress_ranges, int64_t *labels, float *bbox_targets,
                          int32_t *packed, int32_t *counts, void *stream);

/* ------------------------------------------------------------------ FCOS training: loss, all levels
 * The loss of IoUawareFCOSHead / FCOSHead (iou_aware_fcos_head.py:139-226, fcos_head.py:105-191)
 * for every level in <= 4 launches forward and 2 backward.  fp32 NCHW head outputs: cls
 * (B,C,H,W), reg (B,4,H,W) = the exponentiated distances, ctr (B,1,H,W), iou (B,1,H,W) or -- plain
 * FCOS -- every iou pointer NULL (mixed: IA_E_ARG).  With P the positive points (label > 0),
 * n = |P|, c_p = sqrt(min(l,r)/max(l,r) * min(t,b)/max(t,b)) of the target distances and u_p the
 * aligned (+1) IoU of distance2bbox(point, pred) and distance2bbox(point, target):
 *   loss_cls        = sum of the sigmoid focal loss (gamma = 2, class label - 1 positive) / (n + B)
 *   loss_reg        = sum_P -log(u_p) c_p / sum_P c_p
 *   loss_centerness = sum_P BCE_logits(ctr_p, c_p) / n
 *   loss_iou        = sum_P BCE_logits(iou_p, u_p) / n, u_p attached (cfg->attach_iou_target): its
 *                     gradient reaches reg
 * n = 0: the three positive-only terms are 0 with zero gradients, loss_cls = sum / B.
 * result: 6 fp32 = loss_cls | loss_reg | loss_centerness | loss_iou (0 without the branch) | n |
 * sum_P c_p.  Class logits > 60: as ia_head_loss_cfg.exact_large_logits.                    */
typedef struct ia_point_level_ptrs {
    const void *cls[IA_MAX_LEVELS];
    const void *reg[IA_MAX_LEVELS];
    const void *ctr[IA_MAX_LEVELS];
    const void *iou[IA_MAX_LEVELS];     /* all set (IoU-aware FCOS) or all NULL (plain FCOS) */
} ia_point_level_ptrs;

typedef struct ia_point_targets {
    const int64_t *labels[IA_MAX_LEVELS];        /* (B, N_l) int64 in 0..C, as ia_point_targets_ptrs */
    const float *bbox_targets[IA_MAX_LEVELS];    /* (B, N_l, 4), 16-byte aligned                    */
    const int32_t *packed;                       /* of ia_point_targets_ptrs for the same geometry and
                                                    batch, or NULL: the forward call packs the labels
                                                    into its workspace (one more launch)             */
    const int32_t *counts;                       /* (B) positives per image, or NULL: counted        */
} ia_point_targets;

typedef struct ia_point_loss_cfg {
    float gamma, alpha;                          /* focal loss; gamma must be 2                       */
    int32_t attach_iou_target;                   /* gradient of loss_iou through u_p (reference: yes) */
    int32_t exact_large_logits;                  /* as ia_head_loss_cfg                               */
} ia_point_loss_cfg;

/* workspace (256-byte aligned): fp64 partial sums, the focal kernel's normaliser / upstream
 * vector and (when t->packed is NULL) the packed labels; the forward call writes it, the backward
 * call reads it -- keep it alive and untouched between the two.  0: unsupported geometry / batch. */
size_t ia_point_head_loss_workspace_bytes(const ia_point_head_geom *g, int batch);
int ia_point_head_loss_fwd(const ia_point_head_geom *g, const ia_point_level_ptrs *p, int batch,
                           const ia_point_targets *t, const ia_point_loss_cfg *cfg,
                           void *workspace, size_t workspace_bytes, float *result, void *stream);
/* grad_result: 4 fp32 on the device, the upstream gradients of the four losses; grads: fp32 tensors
 * shaped like the head outputs, every element written (zeros at background points).          */
int ia_point_head_loss_bwd(const ia_point_head_geom *g, const ia_point_level_ptrs *p, int batch,
                           const ia_point_targets *t, const ia_point_loss_cfg *cfg,
                           void *workspace, const float *result, const float *grad_result,
                           const ia_point_level_ptrs *grads, void *stream);

/* ------------------------------------------------------------------ FCOS training: loss on channels-last rows
 * The same loss on the head outputs as the HIP tower routes leave them: fp32 or bf16 (dtype IA_F32 /
 * IA_BF16, one for all maps and gradients) pixel rows.  Element (b, p, c) of a map sits at
 * (b * H_l W_l + p) * stride + c, stride in ELEMENTS per map and level; maps may be channel slices of one
 * wider tensor (ctr == cls + C in the same row).  cls and reg pointers and their byte strides are 16-byte
 * (fp32) / 8-byte (bf16) aligned, C % 4 == 0; anything else is IA_E_ARG.  iou: all set or all NULL.
 * g->layout is not consulted.  t->packed is not read (the labels are read as they are).
 * reg_scale (device, L floats) or NULL.  Non-NULL: the reg map holds the RAW fcos_reg output x and the
 * kernels form d_k = exp(reg_scale[l] * x_k) in fp32 (the library's exp); the backward returns
 * dL/dx_k = g_k * reg_scale[l] * d_k in the reg gradient and grad_scale[l] = sum_{b,p,k} g_k d_k x_k
 * (fp64 partial sums, one fp32 rounding; exactly 0 for a level without positives).  NULL: reg holds the
 * distances and grad_scale must be NULL (one without the other: IA_E_ARG).
 * bf16: inputs widened (exact), the fp32 arithmetic of the fp32 kernels, gradients rounded to nearest
 * even once; result, grad_result, reg_scale, grad_scale are fp32.
 * workspace (256-byte aligned, ia_point_head_loss_nhwc_workspace_bytes; 0: unsupported geometry / batch):
 * written by the forward call, read and written by the backward call -- keep it between the two.
 * grad_rows_packed: the caller states that each level's gradient rows are [cls C | ctr | pad] and
 * [reg 4 | iou? | pad] (grads->ctr == grads->cls + C, grads->iou == grads->reg + 4, equal strides within a
 * row; pointers that contradict it: IA_E_ARG): the backward then also writes +0 into every remaining
 * channel of both rows.  Without it only the map slices are written.
 * Every argument error is returned before anything is enqueued.                                    */
typedef struct ia_point_pix_strides {
    int64_t cls[IA_MAX_LEVELS], reg[IA_MAX_LEVELS], ctr[IA_MAX_LEVELS], iou[IA_MAX_LEVELS];
} ia_point_pix_strides;
size_t ia_point_head_loss_nhwc_workspace_bytes(const ia_point_head_geom *g, int batch);
int ia_point_head_loss_fwd_nhwc(const ia_point_head_geom *g, const ia_point_level_ptrs *p,
                                const ia_point_pix_strides *strides, int dtype, int batch,
                                const ia_point_targets *t, const ia_point_loss_cfg *cfg,
                                const float *reg_scale, void *workspace, size_t workspace_bytes,
                                float *result, void *stream);
int ia_point_head_loss_bwd_nhwc(const ia_point_head_geom *g, const ia_point_level_ptrs *p,
                                const ia_point_pix_strides *strides, int dtype, int batch,
                                const ia_point_targets *t, const ia_point_loss_cfg *cfg,
                                const float *reg_scale, void *workspace, size_t workspace_bytes,
                                const float *result, const float *grad_result,
                                const ia_point_level_ptrs *grads, const ia_point_pix_strides *grad_strides,
                                int grad_rows_packed, float *grad_scale, void *stream);

/* ------------------------------------------------------------------ masked convolution
 * (reference mmdet/ops/masked_conv): a stride-1 convolution evaluated only where a (B, H, W) mask is
 * set, exactly 0 elsewhere.  fp32, channels-last.  Four stages; the GEMM between the gather and the
 * scatter is ia_linear_bias_act on the caller's side (its row count is a host value).
 *
 * ia_mask_compact: mask (total = B * H * W bytes, nonzero = kept) -> idx (ascending flat pixel
 *     indices b * H * W + y * W + x of the kept pixels; total entries of room), rank (total int32:
 *     the pixel's row in idx, or -1), count (1 int32: the number kept).  Wave ballots, a prefix
 *     scan over the per-workgroup counts, no atomics: the same row order in every run.
 *     Workspace: ia_mask_compact_workspace_bytes(total).
 * ia_logit_compact: the same from fp32 logits, a pixel kept where sigmoid(logit) >= thr (0 <= thr <= 1),
 *     the expression ia_guided_rowmax / ia_guided_gather_decode apply to their `loc` maps: the masked
 *     layers and the decode agree on every location.  No mask tensor, no extra launch.
 * ia_masked_im2col: col[r][tap * C + c] for the rows [row0, row0 + rows) of the compacted order --
 *     the im2col row (ksize 3: pad 1, row order of ia_im2col3x3_nhwc; ksize 1: the pixel's own C
 *     values) of pixel idx[row0 + r] for row0 + r < count, zeros from the count on.  C % 4 == 0,
 *     x and col 16-byte aligned.  count is the host's copy of ia_mask_compact's.
 * ia_masked_scatter: out (total, n) channels-last rows from the GEMM result y (rows of ld floats,
 *     row r = kept pixel r): out[p][c] = rank[p] >= 0 ? y[rank[p]][c] : +0.0f.  Every element is
 *     written exactly once; y may be NULL when nothing is kept.                                    */
size_t ia_mask_compact_workspace_bytes(int64_t total);
int ia_mask_compact(const uint8_t *mask, int64_t total, int32_t *idx, int32_t *rank, int32_t *count,
                    void *workspace, size_t workspace_bytes, void *stream);
int ia_logit_compact(const float *logits, float thr, int64_t total, int32_t *idx, int32_t *rank,
                     int32_t *count, void *workspace, size_t workspace_bytes, void *stream);
int ia_masked_im2col(const float *x, const int32_t *idx, int64_t count, int64_t row0, int64_t rows,
                     float *col, int B, int H, int W, int C, int ksize, void *stream);
int ia_masked_scatter(const float *y, int64_t ld, const int32_t *rank, float *out, int64_t total,
                      int n, void *stream);

/* ------------------------------------------------------------------ guided-anchor decode
 * Post-conv path of IoUawareGARetinaHead (reference iou_aware_ga_retina_head.py get_bboxes on
 * guided_anchor_head.py get_anchors): one square anchor per location (head.num_anchors must be 1,
 * base_anchors[l][0]), the guided anchor delta2bbox(square, [0, 0, shape], anchoring_means,
 * anchoring_stds, wh_ratio_clip 1e-6) without an image clamp, the box delta2bbox(guided anchor,
 * bbox_pred, head.means, head.stds) clamped to the image; score sigmoid(cls) * sigmoid(iou); a
 * location is kept when !use_loc_filter or sigmoid(loc) >= loc_filter_thr.  fp32 NCHW maps,
 * sigmoid classification (head.layout IA_LAYOUT_NCHW, head.cls_activation IA_CLS_SIGMOID).
 *
 * ia_guided_rowmax: rowmax (B, N): the kept location's maximum over classes of the score, +0.0f
 *     for a filtered-out one (the top-k's keys are ordered for scores >= 0); then ia_select_topk.
 * ia_guided_gather_decode: boxes (B, R, 4), scores_t (B, C, Rs), best_score (B, R) of the selected
 *     candidates; a filtered-out candidate gets a zero box, zero scores and best_score 0, which the
 *     NMS skips at any score_thr >= 0.
 * ia_guided_get_bboxes: the two kernels, ia_select_topk and ia_multiclass_nms in one call, on a
 *     workspace of ia_guided_get_bboxes_workspace_bytes (256-byte aligned; the workspace of
 *     ia_get_bboxes for the same head geometry, carved up the same way: ia_guided_workspace_layout).  score_thr < 0: IA_E_ARG.  An image without a
 *     kept location gives num = 0.                                                                */
typedef struct ia_guided_geom {
    ia_head_geom head;
    float anchoring_means[4], anchoring_stds[4];
    float loc_filter_thr;
    int32_t use_loc_filter;
} ia_guided_geom;
typedef struct ia_guided_level_ptrs {
    const void *cls[IA_MAX_LEVELS], *reg[IA_MAX_LEVELS], *iou[IA_MAX_LEVELS];
    const void *shape[IA_MAX_LEVELS], *loc[IA_MAX_LEVELS];
} ia_guided_level_ptrs;
int ia_guided_rowmax(const ia_guided_geom *g, const ia_guided_level_ptrs *p, int batch, float *rowmax,
                     void *stream);
int ia_guided_gather_decode(const ia_guided_geom *g, const ia_guided_level_ptrs *p, int batch,
                            const int32_t *cand_idx, const float *img_hw, const float *scale_factor,
                            int rescale, float *boxes, float *scores_t, float *best_score, void *stream);
size_t ia_guided_get_bboxes_workspace_bytes(const ia_guided_geom *g, int batch);
int ia_guided_workspace_layout(const ia_guided_geom *g, int batch, size_t offsets[8]);
int ia_guided_get_bboxes(const ia_guided_geom *g, const ia_guided_level_ptrs *p, int batch,
                         const float *img_hw, const float *scale_factor, int rescale, float score_thr,
                         float iou_thr, int max_per_img, void *workspace, size_t workspace_bytes,
                         float *dets, int32_t *labels, int32_t *rows, int32_t *num, void *stream);

/* ------------------------------------------------------------------ SSD: L2Norm and decode
 * ia_l2norm_nchw: the L2Norm layer of SSDVGG (reference backbones/ssd_vgg.py) on an fp32 NCHW map:
 *     norm = sqrtf(sum_c x^2) + eps, y = (weight[c] * x) / norm, the sum of squares over the channels
 *     in ascending order in fp64, rounded once.  C >= 1, B >= 1, any H * W.  x and y must not overlap
 *     (in place: IA_E_ARG).  No atomics, the same bits in every run.
 *
 * Post-conv path of SSDHead (reference anchor_heads/ssd_head.py on anchor_head.py get_bboxes,
 * use_sigmoid_cls = False, no nms_pre).  ia_ssd_geom instead of ia_head_geom: the number of anchors
 * differs per level.  LIMITS: num_levels <= IA_MAX_LEVELS (8), num_anchors[l] <= IA_MAX_ANCHORS (16);
 * no limit on the rows R = sum_l H_l * W_l * A_l per image below 2^31 (stages 1-3 are pure geometry).
 * fp32 NCHW maps only (dtype must be IA_F32): cls[l] (B, A_l * (C + 1), H_l, W_l), channel 0 of an
 * anchor = background; reg[l] (B, A_l * 4, H_l, W_l).  Rows are numbered in the reference's order:
 * level, then (y, x), then anchor.
 *
 * ia_ssd_geom_rows: R, and the prefix of the rows per level.
 * ia_ssd_rowscore: best (B, R): the largest foreground softmax score of every row, with the bits of
 *     ia_decode_fuse_rowmax under IA_CLS_SOFTMAX_NOIOU on that level alone.
 * ia_ssd_compact: per image the rows with best > score_thr in ascending order -> kept_rows
 *     (B, IA_MAX_CANDIDATES) int32 (the first IA_MAX_CANDIDATES of them; -1 behind the count),
 *     kept_count (B) the TRUE count, overflow (B) = kept_count > IA_MAX_CANDIDATES.  Ballots and a
 *     prefix scan, no atomics.  Workspace: ia_ssd_compact_workspace_bytes(batch, R), 4-byte aligned.
 * ia_ssd_gather_decode: for the rows kept_rows[b * kept_stride + r], r < kept_count[b] <= Rk (any Rk
 *     >= 1, kept_stride >= Rk): boxes (B, Rk, 4) = delta2bbox(anchor, bbox_pred, means, stds,
 *     max_shape = img_hw[b]) (/ scale_factor[b] when rescale), scores_t (B, C, Rs) the C foreground
 *     softmax scores class-major (Rs = Rk rounded up to 64), best_score (B, Rk) -- the bits of
 *     ia_gather_decode under IA_CLS_SOFTMAX_NOIOU.  Rows r >= kept_count[b], and every row of an image
 *     with kept_count[b] > Rk, get a zero box, zero scores and best_score 0.
 * ia_ssd_get_bboxes: the three stages with Rk = min(R, IA_MAX_CANDIDATES), ia_multiclass_nms on the
 *     compacted rows, and `rows` mapped back to anchor row ids.  An image with more than
 *     IA_MAX_CANDIDATES kept rows gets overflow[b] = 1 and num[b] = 0 -- never a truncated result; the
 *     caller resolves it through the stage entries.  score_thr < 0: IA_E_ARG.  Workspace:
 *     ia_ssd_get_bboxes_workspace_bytes, 256-byte aligned; ia_ssd_workspace_layout gives the byte
 *     offsets of row scores (B, R), kept_rows, kept_count, boxes, scores_t, best_score, keep_count
 *     (B, C), keep_rows (B, C, Rs).                                                                */
int ia_l2norm_nchw(const float *x, const float *weight, float eps, int B, int C, int H, int W, float *y,
                   void *stream);
typedef struct ia_ssd_geom {
    int32_t num_levels;                       /* <= IA_MAX_LEVELS */
    int32_t num_classes;                      /* C foreground classes; cls has A_l*(C+1) channels, channel 0 = background */
    int32_t H[IA_MAX_LEVELS], W[IA_MAX_LEVELS], stride[IA_MAX_LEVELS];
    int32_t num_anchors[IA_MAX_LEVELS];       /* A_l <= IA_MAX_ANCHORS, may differ per level */
    float base_anchors[IA_MAX_LEVELS][IA_MAX_ANCHORS][4];
    float means[4], stds[4];
} ia_ssd_geom;
typedef struct ia_ssd_level_ptrs {
    const void *cls[IA_MAX_LEVELS], *reg[IA_MAX_LEVELS];
} ia_ssd_level_ptrs;
int ia_ssd_geom_rows(const ia_ssd_geom *g, int32_t *R, int32_t level_off[IA_MAX_LEVELS + 1]);
int ia_ssd_rowscore(const ia_ssd_geom *g, const ia_ssd_level_ptrs *p, int batch, int dtype, float *best,
                    void *stream);
size_t ia_ssd_compact_workspace_bytes(int batch, int R);
int ia_ssd_compact(const float *best, int batch, int R, float score_thr, int32_t *kept_rows, int32_t *kept_count,
                   int32_t *overflow, void *workspace, size_t workspace_bytes, void *stream);
int ia_ssd_gather_decode(const ia_ssd_geom *g, const ia_ssd_level_ptrs *p, int batch, int dtype,
                         const int32_t *kept_rows, int kept_stride, const int32_t *kept_count, int Rk,
                         const float *img_hw, const float *scale_factor, int rescale, float *boxes,
                         float *scores_t, float *best_score, void *stream);
size_t ia_ssd_get_bboxes_workspace_bytes(const ia_ssd_geom *g, int batch);
int ia_ssd_workspace_layout(const ia_ssd_geom *g, int batch, size_t offsets[8]);
int ia_ssd_get_bboxes(const ia_ssd_geom *g, const ia_ssd_level_ptrs *p, int batch, int dtype,
                      const float *img_hw, const float *scale_factor, int rescale, float score_thr,
                      float iou_thr, int max_per_img, void *workspace, size_t workspace_bytes, float *dets,
                      int32_t *labels, int32_t *rows, int32_t *num, int32_t *overflow, void *stream);

/* ------------------------------------------------------------------ SSD: training loss (csrc/ssdloss.hip)
 * SSDHead.loss / loss_single of the reference (anchor_heads/ssd_head.py, IoU_balanced_* off) for a whole
 * batch: softmax cross-entropy of every anchor row, hard-negative mining, smooth-L1 on the positives.
 * Geometry, level pointers and row order are those of the decode entries above (fp32 NCHW maps consumed
 * in place, dtype must be IA_F32; batch * num_levels <= 65535).  Targets are image-major:
 * labels (B, R) int64 in 0..C (0 = background; a negative value is neither positive nor negative),
 * label_weights (B, R) fp32, bbox_targets / bbox_weights (B, R, 4) fp32, 16-byte aligned.
 * avg_factor: *avg_factor_dev (a device scalar) when non-NULL, else the host value avg_factor (> 0) --
 * the convention of ia_head_targets.
 *
 * ia_ssd_loss_rows (stage 1): lse = max + log(sum exp(x - max)) through the softmax statistics of the
 *     decode, ce = (lse - x[label]) * label_weight -> ce, lse (B, R).  box_partials (may be NULL):
 *     (B, nparts) fp64, nparts from ia_ssd_loss_partials: every workgroup's sum over its rows of
 *     sum_k bbox_weight_k * smoothl1(pred_k - target_k, beta) (|d| < beta: 0.5 d^2 / beta, else
 *     |d| - 0.5 beta), each slot written by exactly one workgroup.  beta <= 0: IA_E_ARG.
 * ia_ssd_mine (stage 2): per image num_pos = #(label > 0), num_neg = #(label == 0),
 *     k = min(neg_pos_ratio * num_pos, num_neg), formed on the device; the k-th largest ce among the
 *     negatives by an exact radix select (any R < 2^31; the keys stay in LDS for
 *     R <= ia_ssd_mine_lds_rows()).  TIE RULE: with t the k-th largest value, a negative is selected
 *     when ce > t, or when ce == t and it is among the first k - #(ce > t) such rows in ascending row
 *     order (-0.0 counts as +0.0).  sel (B, R) uint8: 1 for positives and selected negatives;
 *     counts (B, 2) int32 = (num_pos, k); losses (B, 2) fp32 = ((sum_pos ce + sum_selected ce) /
 *     avg_factor, sum of the box partials / avg_factor): fp64 sums in a fixed order, rounded once.
 *     k = 0 gives a classification loss of 0.  neg_pos_ratio < 0: IA_E_ARG.
 * ia_ssd_loss_bwd: every element of every gradient map, exactly once (no memset needed): the C + 1 class
 *     gradients of a row are grad_losses[b][0] / avg_factor * label_weight * (exp(x - lse) - [c == label])
 *     when sel (exp(x - lse) is evaluated as exp(x - max) / sum on the row's softmax statistics, formed
 *     again: lse rounded to fp32 would cost up to half an ulp of lse in the exponent), else +0.0; the box gradients grad_losses[b][1] / avg_factor * bbox_weight_k *
 *     d smoothl1 (+0.0 where the weight is 0).  grads: the gradient maps, shaped like the head outputs,
 *     not the head outputs themselves (IA_E_ARG).  grad_losses (B, 2) fp32 on the device.
 * ia_ssd_head_loss_fwd / _bwd: the node: stage 1 + stage 2 (2 launches), and the backward (1 launch) on
 *     the workspace the forward filled.  Workspace: ia_ssd_head_loss_workspace_bytes (0: unsupported
 *     geometry / batch), 256-byte aligned, a smaller one is IA_E_ARG;
 *     ia_ssd_head_loss_workspace_layout gives the byte offsets of ce (B, R) fp32, lse (B, R) fp32,
 *     sel (B, R) uint8, counts (B, 2) int32 and the box partials (B, nparts) fp64.
 * No floating-point atomics and none on global memory (the digit counters of the radix select are
 * integer LDS atomics): the same bits in every run.  No host synchronisation.                          */
int ia_ssd_mine_lds_rows(void);
int ia_ssd_loss_partials(const ia_ssd_geom *g, int32_t *nparts);
int ia_ssd_loss_rows(const ia_ssd_geom *g, const ia_ssd_level_ptrs *p, int batch, int dtype, const int64_t *labels,
                     const float *label_weights, const float *bbox_targets, const float *bbox_weights, float beta,
                     float *ce, float *lse, double *box_partials, void *stream);
int ia_ssd_mine(const float *ce, const int64_t *labels, int batch, int R, int neg_pos_ratio,
                const double *box_partials, int nparts, const float *avg_factor_dev, float avg_factor, uint8_t *sel,
                int32_t *counts, float *losses, void *stream);
int ia_ssd_loss_bwd(const ia_ssd_geom *g, const ia_ssd_level_ptrs *p, int batch, int dtype, const int64_t *labels,
                    const float *label_weights, const float *bbox_targets, const float *bbox_weights, float beta,
                    const uint8_t *sel, const float *grad_losses, const float *avg_factor_dev, float avg_factor,
                    const ia_ssd_level_ptrs *grads, void *stream);
size_t ia_ssd_head_loss_workspace_bytes(const ia_ssd_geom *g, int batch);
int ia_ssd_head_loss_workspace_layout(const ia_ssd_geom *g, int batch, size_t offsets[5]);
int ia_ssd_head_loss_fwd(const ia_ssd_geom *g, const ia_ssd_level_ptrs *p, int batch, int dtype,
                         const int64_t *labels, const float *label_weights, const float *bbox_targets,
                         const float *bbox_weights, const float *avg_factor_dev, float avg_factor, int neg_pos_ratio,
                         float beta, void *workspace, size_t workspace_bytes, float *losses, void *stream);
int ia_ssd_head_loss_bwd(const ia_ssd_geom *g, const ia_ssd_level_ptrs *p, int batch, int dtype,
                         const int64_t *labels, const float *label_weights, const float *bbox_targets,
                         const float *bbox_weights, const float *avg_factor_dev, float avg_factor, float beta,
                         const void *workspace, size_t workspace_bytes, const float *grad_losses,
                         const ia_ssd_level_ptrs *grads, void *stream);

/* ------------------------------------------------------------------ self-test
 * Elementwise fp32 math used by the kernels, exposed so tests can pin the
 * device implementation bit-for-bit: op 0 exp, 1 log, 2 sigmoid, 3 sqrt,
 * 4 x/y (y = second input), 5 sqrt(sigmoid(x)).                               */
int ia_test_math(int op, const float *x, const float *y, float *out, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* IOUAWARE_H */
