// Decode stage of the point heads (IoU-aware FCOS, reference
// mmdet/models/anchor_heads/iou_aware_fcos_head.py:310-350, and plain FCOS, fcos_head.py:225-272):
// scores, per-level row max, candidate gather and distance2bbox.  The top-k between the two kernels and the NMS behind them
// are the anchor head's (select.hip, nms.hip, lazynms.hip), run on the level table of the same
// feature maps with one "anchor" per position -- the row-max array is then in point order in
// either memory layout, the tie rule (score desc, index asc) and the workspace contract are shared.
//
//   k_point_rowmax   one thread per (image, point): max over classes of
//                    powf(sigmoid(x_c), alpha) * powf(sigmoid(iou), 1 - alpha) (ia_math.hpp
//                    restatements, each product evaluated exactly as the gather evaluates it, so
//                    the selection sees the very scores the NMS does).  NCHW: class planes read
//                    coalesced across threads; channels-last: the row in 16-byte vectors.
//   k_point_gather   one thread per (image, candidate): the C fused scores into the class-major
//                    (B, C, Rs) array, their maximum into best_score, and the box
//                    (px - l, py - t, px + r, py + b) with px = x * stride + stride / 2, clamped to
//                    [0, w-1] x [0, h-1], divided by scale_factor when rescaling.
//
// Both kernels are templates on the storage type of the three maps (float, or uint16_t = bf16 raw
// bits: a load converts exactly to fp32 and everything behind it is the fp32 arithmetic, so bf16
// maps give the bits of their fp32 copies; the channels-last class row is then 8 values per
// 16-byte vector) and on the score kind (launch-uniform):
//   kPointIouAware   the fused score above (the third map is the IoU logit);
//   kPointCtr        plain FCOS: the third map is the centerness logit.  Row max
//                    max_c(sigmoid(x_c) * sigmoid(ctr)) (fp32 product, the reference's max_scores);
//                    the gather writes sigmoid(x_c) * sigmoid(ctr) where the RAW score
//                    sigmoid(x_c) > score_thr and kPointCtrSentinel (< 0) elsewhere
//                    (multiclass_nms with score_factors, bbox_nms.py:37-48: threshold on the raw
//                    score, NMS / final sort on the product).  The shared NMS stages then run with
//                    the threshold kPointCtrStageThr, between the sentinel and 0: every product
//                    (>= 0, an underflowed 0 included) passes it, no sentinel does.
#include "ia_internal.hpp"
#include "ia_math.hpp"

namespace ia {

struct PointArgs {
    LevelTable t;
    ia_level_ptrs p;
    float alpha, beta;                       // beta = 1 - alpha
    float *rowmax;                           // (B, N)
    const int32_t *cand_idx;                 // (B, R)
    const float *img_hw, *scale_factor;
    float *boxes, *scores_t, *best_score;
    int32_t R, Rs, rescale, batch;
    float score_thr;                         // kPointCtr: the raw-score threshold of the gather
};

// score kinds (template parameter of the two kernels)
constexpr int kPointIouAware = 0, kPointCtr = 1;

template <typename T>
struct PointLevel { int l, base, H, W, stride; const T *cls, *reg, *iou; };   // iou: or centerness

// level of an index into a prefix table (the per-level scalars through selects: scalar kernarg
// loads, no per-lane indexing of the argument block)
template <typename T>
__device__ __forceinline__ PointLevel<T> point_level(const PointArgs &a, const int32_t *off, int i)
{
    PointLevel<T> s;
    s.l = 0;
#pragma unroll
    for (int k = 1; k < IA_MAX_LEVELS; ++k) s.l += (k < a.t.num_levels && i >= off[k]) ? 1 : 0;
    s.base = off[0]; s.H = a.t.H[0]; s.W = a.t.W[0]; s.stride = a.t.stride[0];
    s.cls = static_cast<const T *>(a.p.cls[0]);
    s.reg = static_cast<const T *>(a.p.reg[0]);
    s.iou = static_cast<const T *>(a.p.iou[0]);
#pragma unroll
    for (int k = 1; k < IA_MAX_LEVELS; ++k) {
        const bool m = s.l == k;
        s.base = m ? off[k] : s.base;
        s.H = m ? a.t.H[k] : s.H; s.W = m ? a.t.W[k] : s.W; s.stride = m ? a.t.stride[k] : s.stride;
        s.cls = m ? static_cast<const T *>(a.p.cls[k]) : s.cls;
        s.reg = m ? static_cast<const T *>(a.p.reg[k]) : s.reg;
        s.iou = m ? static_cast<const T *>(a.p.iou[k]) : s.iou;
    }
    return s;
}

// a stored value as fp32 (bf16: exact)
__device__ __forceinline__ float point_f32(float v) { return v; }
__device__ __forceinline__ float point_f32(uint16_t v) { return bf16_to_f32(v); }

// the per-point factor of the score: powf(sigmoid(iou), 1 - alpha), or sigmoid(centerness)
template <int KIND>
__device__ __forceinline__ float point_factor(float x, float beta)
{
    return KIND == kPointCtr ? sigmoidf_(x) : powf_pos_(sigmoidf_(x), beta);
}

template <int KIND>
__device__ __forceinline__ float point_score(float x, float fi, float alpha)
{
    return KIND == kPointCtr ? sigmoidf_(x) * fi : powf_pos_(sigmoidf_(x), alpha) * fi;
}

template <int KIND, typename T>
__global__ void __launch_bounds__(256) k_point_rowmax(PointArgs a)
{
    const int N = a.t.anchor_off[a.t.num_levels];
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)a.batch * N) return;
    const int b = (int)(gid / N), i = (int)(gid - (int64_t)b * N);
    const PointLevel<T> lv = point_level<T>(a, a.t.anchor_off, i);
    const int pos = i - lv.base, HW = lv.H * lv.W, C = a.t.C;
    const float fi = point_factor<KIND>(point_f32(lv.iou[(size_t)b * HW + pos]), a.beta);
    float best = 0.0f;                       // scores are >= 0
    if (a.t.layout == IA_LAYOUT_NHWC) {
        if constexpr (sizeof(T) == 2) {
            const uint4 *row = reinterpret_cast<const uint4 *>(lv.cls + ((size_t)b * HW + pos) * C);
            for (int v = 0; v < C / 8; ++v) {
                float f[8];
                bf16x8_to_f32(row[v], f);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float sc = point_score<KIND>(f[j], fi, a.alpha);
                    best = (best < sc) ? sc : best;
                }
            }
        } else {
            const float4 *row = reinterpret_cast<const float4 *>(lv.cls + ((size_t)b * HW + pos) * C);
            for (int v = 0; v < C / 4; ++v) {
                const float4 q = row[v];
                float sc = point_score<KIND>(q.x, fi, a.alpha); best = (best < sc) ? sc : best;
                sc = point_score<KIND>(q.y, fi, a.alpha); best = (best < sc) ? sc : best;
                sc = point_score<KIND>(q.z, fi, a.alpha); best = (best < sc) ? sc : best;
                sc = point_score<KIND>(q.w, fi, a.alpha); best = (best < sc) ? sc : best;
            }
        }
    } else {
        const T *cls = lv.cls + (size_t)b * C * HW + pos;
        for (int c = 0; c < C; ++c) {
            const float sc = point_score<KIND>(point_f32(cls[(size_t)c * HW]), fi, a.alpha);
            best = (best < sc) ? sc : best;
        }
    }
    a.rowmax[(size_t)b * N + i] = best;
}

template <int KIND, typename T>
__global__ void __launch_bounds__(256) k_point_gather(PointArgs a)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (r >= a.R) return;
    const PointLevel<T> lv = point_level<T>(a, a.t.cand_off, r);
    const int HW = lv.H * lv.W, C = a.t.C;
    const int pos = a.cand_idx[(size_t)b * a.R + r];
    const bool nhwc = a.t.layout == IA_LAYOUT_NHWC;
    const size_t cs = nhwc ? (size_t)1 : (size_t)HW;
    const float fi = point_factor<KIND>(point_f32(lv.iou[(size_t)b * HW + pos]), a.beta);
    const T *cls = lv.cls + (nhwc ? ((size_t)b * HW + pos) * C : (size_t)b * C * HW + pos);
    float *so = a.scores_t + (size_t)b * C * a.Rs + r;
    bool done = false;                       // fp32: constant, the loops below are all there is
    if constexpr (sizeof(T) == 2) {
        if (nhwc) {
            // bf16 channels-last: the candidate's class row in 16-byte vectors of 8, the classes
            // in index order through the expressions of the loops below
            float best = KIND == kPointCtr ? kPointCtrSentinel : 0.0f;
            const uint4 *row = reinterpret_cast<const uint4 *>(cls);
            for (int v = 0; v < C / 8; ++v) {
                float f[8];
                bf16x8_to_f32(row[v], f);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float sc;
                    if (KIND == kPointCtr) {
                        const float s = sigmoidf_(f[j]);
                        sc = (s > a.score_thr) ? s * fi : kPointCtrSentinel;
                    } else {
                        sc = point_score<KIND>(f[j], fi, a.alpha);
                    }
                    so[(size_t)(8 * v + j) * a.Rs] = sc;
                    best = (best < sc) ? sc : best;
                }
            }
            if (a.best_score) a.best_score[(size_t)b * a.R + r] = best;
            done = true;
        }
    }
    if (done) {
    } else if (KIND == kPointCtr) {
        // raw-score threshold, then the product; best = max of what was written (the sentinel
        // when no class passes: the row then stays out of k_adj's relation)
        float best = kPointCtrSentinel;
        for (int c = 0; c < C; ++c) {
            const float s = sigmoidf_(point_f32(cls[(size_t)c * cs]));
            const float sc = (s > a.score_thr) ? s * fi : kPointCtrSentinel;
            so[(size_t)c * a.Rs] = sc;
            best = (best < sc) ? sc : best;
        }
        if (a.best_score) a.best_score[(size_t)b * a.R + r] = best;
    } else {
        float best = 0.0f;
        for (int c = 0; c < C; ++c) {
            const float sc = point_score<KIND>(point_f32(cls[(size_t)c * cs]), fi, a.alpha);
            so[(size_t)c * a.Rs] = sc;
            best = (best < sc) ? sc : best;
        }
        if (a.best_score) a.best_score[(size_t)b * a.R + r] = best;
    }
    const T *reg = lv.reg + (nhwc ? ((size_t)b * HW + pos) * 4 : (size_t)b * 4 * HW + pos);
    const int y = pos / lv.W, x = pos - y * lv.W;
    const float px = (float)(x * lv.stride + lv.stride / 2), py = (float)(y * lv.stride + lv.stride / 2);
    float x1 = px - point_f32(reg[0]), y1 = py - point_f32(reg[cs]);
    float x2 = px + point_f32(reg[2 * cs]), y2 = py + point_f32(reg[3 * cs]);
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
    reinterpret_cast<float4 *>(a.boxes)[(size_t)b * a.R + r] = make_float4(x1, y1, x2, y2);
}

// the anchor-head geometry of the same feature maps with one anchor per position: what the
// shared stages (top-k, NMS) and the workspace carve-up are computed from
int point_head_geom(const ia_point_head_geom *pg, ia_head_geom &g)
{
    if (!pg) return IA_E_ARG;
    if (!(pg->score_alpha >= 0.0f && pg->score_alpha <= 1.0f)) return IA_E_ARG;
    g = ia_head_geom{};
    g.num_levels = pg->num_levels;
    g.num_anchors = 1;
    g.num_classes = pg->num_classes;
    g.nms_pre = pg->nms_pre;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        g.H[l] = pg->H[l]; g.W[l] = pg->W[l]; g.stride[l] = pg->stride[l];
    }
    for (int k = 0; k < 4; ++k) { g.means[k] = 0.0f; g.stds[k] = 1.0f; }
    g.layout = pg->layout;
    g.cls_activation = IA_CLS_SIGMOID;
    LevelTable t;
    int rc = make_level_table(&g, t);
    if (rc) return rc;
    if (g.layout == IA_LAYOUT_NHWC && g.num_classes % 4 != 0) return IA_E_ARG;
    return 0;
}

int launch_point_decode(const ia_point_head_geom *pg, const LevelTable &t, const ia_level_ptrs &p,
                        int batch, const float *img_hw, const float *scale_factor, int rescale,
                        float *rowmax, int32_t *cand_idx, void *select_ws, float *boxes,
                        float *scores_t, float *best_score, int Rs, int kind, float score_thr,
                        int dtype, hipStream_t s)
{
    if (batch < 1 || !img_hw || (rescale && !scale_factor)) return IA_E_ARG;
    if (kind != kPointIouAware && kind != kPointCtr) return IA_E_ARG;
    if (dtype != IA_F32 && dtype != IA_BF16) return IA_E_ARG;
    const bool bf = dtype == IA_BF16;
    // channels-last bf16: the class row in whole 16-byte vectors
    if (bf && t.layout == IA_LAYOUT_NHWC && t.C % 8 != 0) return IA_E_ARG;
    PointArgs a;
    a.t = t; a.p = p;
    a.alpha = pg->score_alpha; a.beta = 1.0f - pg->score_alpha;
    a.rowmax = rowmax; a.cand_idx = cand_idx; a.img_hw = img_hw; a.scale_factor = scale_factor;
    a.boxes = boxes; a.scores_t = scores_t; a.best_score = best_score;
    a.R = t.cand_off[t.num_levels]; a.Rs = Rs; a.rescale = rescale ? 1 : 0; a.batch = batch;
    a.score_thr = score_thr;
    for (int l = 0; l < t.num_levels; ++l) {
        if (!p.cls[l] || !p.reg[l] || !p.iou[l]) return IA_E_ARG;
        if (t.layout == IA_LAYOUT_NHWC && ((uintptr_t)p.cls[l] & 15u)) return IA_E_ARG;
    }
    const int64_t n = (int64_t)batch * t.anchor_off[t.num_levels];
    const dim3 rgrid((unsigned)((n + 255) / 256));
    if (kind == kPointCtr) {
        if (bf) hipLaunchKernelGGL((k_point_rowmax<kPointCtr, uint16_t>), rgrid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_point_rowmax<kPointCtr, float>), rgrid, dim3(256), 0, s, a);
    } else {
        if (bf) hipLaunchKernelGGL((k_point_rowmax<kPointIouAware, uint16_t>), rgrid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_point_rowmax<kPointIouAware, float>), rgrid, dim3(256), 0, s, a);
    }
    int rc = hip_status(hipGetLastError());
    if (rc) return rc;
    if ((rc = launch_select(t, rowmax, batch, cand_idx, select_ws, s, false))) return rc;
    const dim3 grid((unsigned)((a.R + 255) / 256), (unsigned)batch);
    if (kind == kPointCtr) {
        if (bf) hipLaunchKernelGGL((k_point_gather<kPointCtr, uint16_t>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_point_gather<kPointCtr, float>), grid, dim3(256), 0, s, a);
    } else {
        if (bf) hipLaunchKernelGGL((k_point_gather<kPointIouAware, uint16_t>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_point_gather<kPointIouAware, float>), grid, dim3(256), 0, s, a);
    }
    return hip_status(hipGetLastError());
}

}  // namespace ia
