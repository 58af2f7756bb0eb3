// Decode stage of the IoU-aware guided-anchor RetinaNet head (reference
// mmdet/models/anchor_heads/iou_aware_ga_retina_head.py get_bboxes / get_bboxes_single on
// guided_anchor_head.py get_anchors / get_guided_anchors_single).  One square anchor per location;
// the head predicts the anchor's shape (2 channels), whether the location is kept (1 channel), and
// the usual class / box / IoU maps against the guided anchor.
//
//   k_guided_rowmax   one thread per (image, location): keep = !use_loc_filter ||
//                     sigmoid(loc) >= loc_filter_thr; a kept location's row score is
//                     max_c(sigmoid(cls_c) * sigmoid(iou)) (a plain fp32 product, not the sqrt * sqrt
//                     fusion of IoUawareRetinaHead), a filtered-out one's is +0.0f: the top-k
//                     (select.hip) orders the raw bits of scores >= 0, ties to the ascending index,
//                     so a level of mostly zeros ranks its kept locations first and fills the rest of
//                     its quota with the lowest filtered-out indices.
//   k_guided_gather   one thread per (image, candidate): the keep decision again from `loc` by the
//                     same expression; the square from base_anchors[l][0] and the position; the
//                     guided anchor = delta2bbox(square, [0, 0, shape], anchoring means / stds) with
//                     the clip |log(1e-6)| and no clamp; the box = delta2bbox(guided anchor, bbox_pred,
//                     target means / stds) with the clip |log(16 / 1000)|, clamped to the image,
//                     divided by scale_factor when rescaling.  A filtered-out candidate: zero box,
//                     zero scores, best_score 0 -- the NMS stages (score > score_thr >= 0) skip it.
//
// The top-k between the two kernels and the NMS behind them are the anchor head's, on the level
// table of the A = 1 geometry (the row-max array is then in location order).  fp32 NCHW maps.
#include "ia_internal.hpp"
#include "ia_math.hpp"

namespace ia {

struct GuidedArgs {
    LevelTable t;
    ia_guided_level_ptrs p;
    float base[IA_MAX_LEVELS][4];            // base_anchors[l][0]
    float a_means[4], a_stds[4];             // anchoring
    float t_means[4], t_stds[4];             // target
    float loc_thr;
    int32_t use_filter;
    float *rowmax;                           // (B, N)
    const int32_t *cand_idx;                 // (B, R)
    const float *img_hw, *scale_factor;
    float *boxes, *scores_t, *best_score;
    int32_t R, Rs, rescale, batch;
};

struct GuidedLevel { int l, base, H, W, stride; const float *cls, *reg, *iou, *shape, *loc; };

// level of an index into a prefix table; the per-level scalars through selects (scalar kernarg
// loads, no per-lane indexing of the argument block)
__device__ __forceinline__ GuidedLevel guided_level(const GuidedArgs &a, const int32_t *off, int i)
{
    GuidedLevel s;
    s.l = 0;
#pragma unroll
    for (int k = 1; k < IA_MAX_LEVELS; ++k) s.l += (k < a.t.num_levels && i >= off[k]) ? 1 : 0;
    s.base = off[0]; s.H = a.t.H[0]; s.W = a.t.W[0]; s.stride = a.t.stride[0];
    s.cls = static_cast<const float *>(a.p.cls[0]);
    s.reg = static_cast<const float *>(a.p.reg[0]);
    s.iou = static_cast<const float *>(a.p.iou[0]);
    s.shape = static_cast<const float *>(a.p.shape[0]);
    s.loc = static_cast<const float *>(a.p.loc[0]);
#pragma unroll
    for (int k = 1; k < IA_MAX_LEVELS; ++k) {
        const bool m = s.l == k;
        s.base = m ? off[k] : s.base;
        s.H = m ? a.t.H[k] : s.H; s.W = m ? a.t.W[k] : s.W; s.stride = m ? a.t.stride[k] : s.stride;
        s.cls = m ? static_cast<const float *>(a.p.cls[k]) : s.cls;
        s.reg = m ? static_cast<const float *>(a.p.reg[k]) : s.reg;
        s.iou = m ? static_cast<const float *>(a.p.iou[k]) : s.iou;
        s.shape = m ? static_cast<const float *>(a.p.shape[k]) : s.shape;
        s.loc = m ? static_cast<const float *>(a.p.loc[k]) : s.loc;
    }
    return s;
}

// the keep decision of both kernels (false for a NaN logit, like the reference's >=)
__device__ __forceinline__ bool guided_keep(const GuidedArgs &a, float loc)
{
    return !a.use_filter || sigmoidf_(loc) >= a.loc_thr;
}

// delta2bbox (reference mmdet/core/bbox/transforms.py) of one box without clamp: the operation
// order of decode_box (ia_gather_dev.hpp), the clip as a parameter
__device__ __forceinline__ float4 guided_delta2bbox(float ax1, float ay1, float ax2, float ay2, float r0,
                                                    float r1, float r2, float r3, const float *means,
                                                    const float *stds, float max_ratio)
{
    float dx = r0 * stds[0] + means[0];
    float dy = r1 * stds[1] + means[1];
    float dw = r2 * stds[2] + means[2];
    float dh = r3 * stds[3] + means[3];
    dw = (dw < -max_ratio) ? -max_ratio : dw;  dw = (dw > max_ratio) ? max_ratio : dw;
    dh = (dh < -max_ratio) ? -max_ratio : dh;  dh = (dh > max_ratio) ? max_ratio : dh;
    const float px = (ax1 + ax2) * 0.5f;
    const float py = (ay1 + ay2) * 0.5f;
    const float pw = (ax2 - ax1) + 1.0f;
    const float ph = (ay2 - ay1) + 1.0f;
    const float gw = pw * expf_(dw);
    const float gh = ph * expf_(dh);
    const float gx = px + pw * dx;
    const float gy = py + ph * dy;
    return make_float4((gx - gw * 0.5f) + 0.5f, (gy - gh * 0.5f) + 0.5f, (gx + gw * 0.5f) - 0.5f,
                       (gy + gh * 0.5f) - 0.5f);
}

constexpr float kGuidedAnchorClip = 13.815510557964274f;    // |log(1e-6)|
constexpr float kGuidedBoxClip = 4.135166556742356f;        // |log(16 / 1000)|

__global__ void __launch_bounds__(256) k_guided_rowmax(GuidedArgs a)
{
    const int N = a.t.anchor_off[a.t.num_levels];
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)a.batch * N) return;
    const int b = (int)(gid / N), i = (int)(gid - (int64_t)b * N);
    const GuidedLevel lv = guided_level(a, a.t.anchor_off, i);
    const int pos = i - lv.base, HW = lv.H * lv.W, C = a.t.C;
    float best = 0.0f;                       // scores are >= 0; the filtered-out location's +0.0f
    if (guided_keep(a, lv.loc[(size_t)b * HW + pos])) {
        const float fi = sigmoidf_(lv.iou[(size_t)b * HW + pos]);
        const float *cls = lv.cls + (size_t)b * C * HW + pos;
        for (int c = 0; c < C; ++c) {
            const float sc = sigmoidf_(cls[(size_t)c * HW]) * fi;
            best = (best < sc) ? sc : best;
        }
    }
    a.rowmax[(size_t)b * N + i] = best;
}

__global__ void __launch_bounds__(256) k_guided_gather(GuidedArgs a)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (r >= a.R) return;
    const GuidedLevel lv = guided_level(a, a.t.cand_off, r);
    const int HW = lv.H * lv.W, C = a.t.C;
    const int pos = a.cand_idx[(size_t)b * a.R + r];
    float *so = a.scores_t + (size_t)b * C * a.Rs + r;
    float4 *box = reinterpret_cast<float4 *>(a.boxes) + (size_t)b * a.R + r;
    if (!guided_keep(a, lv.loc[(size_t)b * HW + pos])) {
        for (int c = 0; c < C; ++c) so[(size_t)c * a.Rs] = 0.0f;
        if (a.best_score) a.best_score[(size_t)b * a.R + r] = 0.0f;
        *box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float fi = sigmoidf_(lv.iou[(size_t)b * HW + pos]);
    const float *cls = lv.cls + (size_t)b * C * HW + pos;
    float best = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float sc = sigmoidf_(cls[(size_t)c * HW]) * fi;
        so[(size_t)c * a.Rs] = sc;
        best = (best < sc) ? sc : best;
    }
    if (a.best_score) a.best_score[(size_t)b * a.R + r] = best;
    const int y = pos / lv.W, x = pos - y * lv.W;
    const float sx = (float)(x * lv.stride), sy = (float)(y * lv.stride);
    // per-lane level index into the small kernarg table: four loads per candidate
    const float *ba = a.base[lv.l];
    const float *sh = lv.shape + (size_t)b * 2 * HW + pos;
    const float4 ga = guided_delta2bbox(ba[0] + sx, ba[1] + sy, ba[2] + sx, ba[3] + sy, 0.0f, 0.0f, sh[0],
                                        sh[HW], a.a_means, a.a_stds, kGuidedAnchorClip);
    const float *reg = lv.reg + (size_t)b * 4 * HW + pos;
    const float4 q = guided_delta2bbox(ga.x, ga.y, ga.z, ga.w, reg[0], reg[HW], reg[2 * (size_t)HW],
                                       reg[3 * (size_t)HW], a.t_means, a.t_stds, kGuidedBoxClip);
    float x1 = q.x, y1 = q.y, x2 = q.z, y2 = q.w;
    // clamp(min=0, max=w-1): comparisons, so a NaN stays NaN like torch.clamp
    const float mx = a.img_hw[2 * b + 1] - 1.0f, my = a.img_hw[2 * b] - 1.0f;
    x1 = (x1 < 0.0f) ? 0.0f : x1;  x1 = (x1 > mx) ? mx : x1;
    y1 = (y1 < 0.0f) ? 0.0f : y1;  y1 = (y1 > my) ? my : y1;
    x2 = (x2 < 0.0f) ? 0.0f : x2;  x2 = (x2 > mx) ? mx : x2;
    y2 = (y2 < 0.0f) ? 0.0f : y2;  y2 = (y2 > my) ? my : y2;
    if (a.rescale) {
        const float *sf = a.scale_factor + 4 * b;
        x1 = x1 / sf[0]; y1 = y1 / sf[1]; x2 = x2 / sf[2]; y2 = y2 / sf[3];
    }
    *box = make_float4(x1, y1, x2, y2);
}

// argument check shared by the entries -> level table and the kernels' argument block
static int guided_args(const ia_guided_geom *g, const ia_guided_level_ptrs *p, int batch, LevelTable &t,
                       GuidedArgs &a)
{
    if (!g || !p || batch < 1) return IA_E_ARG;
    int rc = make_level_table(&g->head, t);
    if (rc) return rc;
    if (t.A != 1 || t.layout != IA_LAYOUT_NCHW || t.act != IA_CLS_SIGMOID) return IA_E_ARG;
    if (!(g->loc_filter_thr >= 0.0f && g->loc_filter_thr <= 1.0f)) return IA_E_ARG;
    if ((int64_t)batch * t.anchor_off[t.num_levels] > 2147483647LL) return IA_E_ARG;
    for (int l = 0; l < t.num_levels; ++l)
        if (!p->cls[l] || !p->reg[l] || !p->iou[l] || !p->shape[l] || !p->loc[l]) return IA_E_ARG;
    a.t = t; a.p = *p;
    for (int l = 0; l < IA_MAX_LEVELS; ++l)
        for (int k = 0; k < 4; ++k) a.base[l][k] = g->head.base_anchors[l][0][k];
    for (int k = 0; k < 4; ++k) {
        a.a_means[k] = g->anchoring_means[k]; a.a_stds[k] = g->anchoring_stds[k];
        a.t_means[k] = g->head.means[k]; a.t_stds[k] = g->head.stds[k];
    }
    a.loc_thr = g->loc_filter_thr; a.use_filter = g->use_loc_filter ? 1 : 0;
    a.rowmax = nullptr; a.cand_idx = nullptr; a.img_hw = nullptr; a.scale_factor = nullptr;
    a.boxes = nullptr; a.scores_t = nullptr; a.best_score = nullptr;
    a.R = t.cand_off[t.num_levels]; a.Rs = (a.R + 63) / 64 * 64; a.rescale = 0; a.batch = batch;
    return 0;
}

static int launch_guided_rowmax(GuidedArgs &a, float *rowmax, hipStream_t s)
{
    if (!rowmax) return IA_E_ARG;
    a.rowmax = rowmax;
    const int64_t n = (int64_t)a.batch * a.t.anchor_off[a.t.num_levels];
    hipLaunchKernelGGL(k_guided_rowmax, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return hip_status(hipGetLastError());
}

static int launch_guided_gather(GuidedArgs &a, const int32_t *cand_idx, const float *img_hw,
                                const float *scale_factor, int rescale, float *boxes, float *scores_t,
                                float *best_score, hipStream_t s)
{
    if (!cand_idx || !img_hw || !boxes || !scores_t || (rescale && !scale_factor)) return IA_E_ARG;
    if (a.batch > 65535) return IA_E_ARG;
    a.cand_idx = cand_idx; a.img_hw = img_hw; a.scale_factor = scale_factor; a.rescale = rescale ? 1 : 0;
    a.boxes = boxes; a.scores_t = scores_t; a.best_score = best_score;
    hipLaunchKernelGGL(k_guided_gather, dim3((unsigned)((a.R + 255) / 256), (unsigned)a.batch), dim3(256), 0,
                       s, a);
    return hip_status(hipGetLastError());
}

}  // namespace ia

extern "C" {

int ia_guided_rowmax(const ia_guided_geom *g, const ia_guided_level_ptrs *p, int batch, float *rowmax,
                     void *stream)
{
    ia::LevelTable t;
    ia::GuidedArgs a;
    int rc = ia::guided_args(g, p, batch, t, a);
    if (rc) return rc;
    return ia::launch_guided_rowmax(a, rowmax, (hipStream_t)stream);
}

int ia_guided_gather_decode(const ia_guided_geom *g, const ia_guided_level_ptrs *p, int batch,
                            const int32_t *cand_idx, const float *img_hw, const float *scale_factor,
                            int rescale, float *boxes, float *scores_t, float *best_score, void *stream)
{
    ia::LevelTable t;
    ia::GuidedArgs a;
    int rc = ia::guided_args(g, p, batch, t, a);
    if (rc) return rc;
    return ia::launch_guided_gather(a, cand_idx, img_hw, scale_factor, rescale, boxes, scores_t, best_score,
                                    (hipStream_t)stream);
}

// the workspace of ia_get_bboxes for the A = 1 geometry (carve_bboxes), used piece by piece as that
// entry uses it
size_t ia_guided_get_bboxes_workspace_bytes(const ia_guided_geom *g, int batch)
{
    if (!g) return 0;
    return ia_get_bboxes_workspace_bytes(&g->head, batch);
}

int ia_guided_workspace_layout(const ia_guided_geom *g, int batch, size_t offsets[8])
{
    if (!g || !offsets) return IA_E_ARG;
    return ia_get_bboxes_workspace_layout(&g->head, batch, offsets);
}

int ia_guided_get_bboxes(const ia_guided_geom *g, const ia_guided_level_ptrs *p, int batch,
                         const float *img_hw, const float *scale_factor, int rescale, float score_thr,
                         float iou_thr, int max_per_img, void *workspace, size_t workspace_bytes,
                         float *dets, int32_t *labels, int32_t *rows, int32_t *num, void *stream)
{
    ia::LevelTable t;
    ia::GuidedArgs a;
    int rc = ia::guided_args(g, p, batch, t, a);
    if (rc) return rc;
    if (!(score_thr >= 0.0f)) return IA_E_ARG;      // the zero rows of filtered-out candidates must not pass
    if (!workspace || !dets || !labels || !rows || !num || !img_hw) return IA_E_ARG;
    if (((uintptr_t)workspace & 255u) != 0) return IA_E_ARG;
    ia::BboxWorkspace w;
    if ((rc = ia::carve_bboxes(&g->head, batch, workspace, w))) return rc;
    if (workspace_bytes < w.bytes) return IA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = ia::launch_guided_rowmax(a, w.rowmax, s))) return rc;
    if ((rc = ia::launch_select(t, w.rowmax, batch, w.cand_idx, w.select, s, false))) return rc;
    if ((rc = ia::launch_guided_gather(a, w.cand_idx, img_hw, scale_factor, rescale, w.boxes, w.scores_t,
                                       w.best_score, s)))
        return rc;
    return ia::launch_bboxes_nms(w, score_thr, iou_thr, max_per_img, -1, dets, labels, rows, num, s);
}

}  // extern "C"
