// C-ABI entry points of the inference half (see include/iouaware.h) and the
// whole-path driver ia_get_bboxes: five launches on the caller's stream, no
// host synchronisation, no allocation.
#include <string.h>
#include <atomic>
#include <mutex>
#include "ia_internal.hpp"
#include "ia_math.hpp"

namespace ia {

static void base_from_geom(const ia_head_geom *g, BaseAnchors &ba)
{
    memcpy(ba.v, g->base_anchors, sizeof(ba.v));
}

int carve_bboxes(const ia_head_geom *g, int batch, void *base, BboxWorkspace &w)
{
    LevelTable &t = w.t;
    int rc = make_level_table(g, t);
    if (rc) return rc;
    if (batch < 1) return IA_E_ARG;
    w.batch = batch;
    w.N = t.anchor_off[t.num_levels];
    w.R = t.cand_off[t.num_levels];
    if (w.R > IA_MAX_CANDIDATES) return IA_E_LIMIT_BOXES;
    w.Rs = (w.R + 63) / 64 * 64;
    const size_t B = (size_t)batch, C = (size_t)t.C;
    Carver c(base);
    w.off[0] = c.take(w.rowmax, B * w.N * sizeof(float));
    w.off[1] = c.take(w.cand_idx, B * w.R * sizeof(int32_t));
    w.off[2] = c.take(w.boxes, B * w.R * 4 * sizeof(float));
    w.off[3] = c.take(w.scores_t, B * C * w.Rs * sizeof(float));
    w.off[4] = c.take(w.keep_count, B * C * sizeof(int32_t));
    w.off[5] = c.take(w.keep_rows, B * C * w.Rs * sizeof(int32_t));
    w.off[6] = c.take(w.best_score, B * w.R * sizeof(float));
    w.off[7] = c.take(w.nms, nms_tail_workspace_bytes(batch, w.R, t.C));
    w.select_off = c.take(w.select, select_workspace_bytes(t, batch));
    c.take(w.lazy, lazy_workspace_bytes(batch, w.Rs, t.C));
    c.take(w.need_full, B * sizeof(int32_t));
    w.bytes = c.bytes;
    return 0;
}

int launch_bboxes_nms(const BboxWorkspace &w, float score_thr, float iou_thr, int max_per_img,
                      int candidates, float *dets, int32_t *labels, int32_t *rows, int32_t *num,
                      hipStream_t s)
{
    const NmsLazy lazy = {w.lazy, w.need_full, candidates};
    return launch_nms_tail(w.boxes, w.scores_t, w.best_score, w.batch, w.R, w.Rs, w.t.C, score_thr,
                           iou_thr, max_per_img, w.nms, candidates >= 0 ? &lazy : nullptr,
                           w.keep_count, w.keep_rows, dets, labels, rows, num, s);
}

// the workspace of ia_multiclass_nms_lazy: the complete path's | lazy NMS | need_full (B) |
// keep_count (B, C) | keep_rows (B, C, Rs)
struct LazyNmsWorkspace { void *full, *lazy; int32_t *need_full, *keep_count, *keep_rows; size_t bytes; };

static LazyNmsWorkspace carve_nms_lazy(int batch, int R, int C, void *base)
{
    const int Rs = (R + 63) / 64 * 64;
    LazyNmsWorkspace w;
    Carver c(base);
    c.take(w.full, nms_tail_workspace_bytes(batch, R, C));
    c.take(w.lazy, lazy_workspace_bytes(batch, Rs, C));
    c.take(w.need_full, (size_t)batch * sizeof(int32_t));
    c.take(w.keep_count, (size_t)batch * C * sizeof(int32_t));
    c.take(w.keep_rows, (size_t)batch * C * Rs * sizeof(int32_t));
    w.bytes = c.bytes;
    return w;
}

__global__ void k_test_math(int op, const float *x, const float *y, float *out, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        float v = x[i], r;
        switch (op) {
        case 0: r = expf_(v); break;
        case 1: r = logf_(v); break;
        case 2: r = sigmoidf_(v); break;
        case 3: r = __builtin_sqrtf(v); break;
        case 4: r = v / y[i]; break;
        case 6: r = (float)exp_f64_((double)(v / y[i])); break;
        default: r = sqrt_sigmoidf_(v); break;
        }
        out[i] = r;
    }
}

}  // namespace ia

extern "C" {

const char *ia_version(void) { return "iouaware-hip 0.1 (gfx950)"; }

int ia_geom_sizes(const ia_head_geom *g, int32_t *N, int32_t *R, int32_t *Rs)
{
    // pure geometry: valid for any head, also when R exceeds what ia_get_bboxes supports
    // (the training losses use a geometry with nms_pre <= 0, i.e. R = N)
    ia::LevelTable t;
    int rc = ia::make_level_table(g, t);
    if (rc) return rc;
    const int32_t r = t.cand_off[t.num_levels];
    if (N) *N = t.anchor_off[t.num_levels];
    if (R) *R = r;
    if (Rs) *Rs = (r + 63) / 64 * 64;
    return 0;
}

int ia_decode_fuse_rowmax(const ia_head_geom *g, const ia_level_ptrs *p, int batch, int dtype,
                          float *rowmax, void *stream)
{
    ia::LevelTable t;
    int rc = ia::make_level_table(g, t);
    if (rc) return rc;
    if (!p) return IA_E_ARG;
    return ia::launch_rowmax(t, *p, batch, dtype, rowmax, (hipStream_t)stream);
}

size_t ia_select_topk_workspace_bytes(const ia_head_geom *g, int batch)
{
    ia::LevelTable t;
    if (ia::make_level_table(g, t) || batch < 1) return 0;
    return ia::select_workspace_bytes(t, batch);
}

int ia_select_topk(const ia_head_geom *g, const float *rowmax, int batch, int32_t *cand_idx,
                   void *workspace, size_t workspace_bytes, void *stream)
{
    ia::LevelTable t;
    int rc = ia::make_level_table(g, t);
    if (rc) return rc;
    if (batch < 1 || !workspace) return IA_E_ARG;
    if (workspace_bytes < ia::select_workspace_bytes(t, batch)) return IA_E_WORKSPACE;
    return ia::launch_select(t, rowmax, batch, cand_idx, workspace, (hipStream_t)stream);
}

int ia_decode_fuse_rowmax_grouped(const ia_head_geom *g, const ia_level_ptrs *p, int batch,
                                  int dtype, float *rowmax, void *select_workspace,
                                  size_t workspace_bytes, void *stream)
{
    ia::LevelTable t;
    int rc = ia::make_level_table(g, t);
    if (rc) return rc;
    if (!p || batch < 1 || !select_workspace) return IA_E_ARG;
    if (workspace_bytes < ia::select_workspace_bytes(t, batch)) return IA_E_WORKSPACE;
    float *groupmax = ia::select_workspace_groupmax(t, batch, select_workspace);
    rc = ia::launch_rowmax(t, *p, batch, dtype, rowmax, (hipStream_t)stream, groupmax);
    if (!rc && t.softmax())     // the softmax row-score kernel does not emit the group maxima
        rc = ia::launch_groupmax(t, rowmax, batch, select_workspace, (hipStream_t)stream);
    return rc;
}

int ia_select_topk_grouped(const ia_head_geom *g, const float *rowmax, int batch,
                           int32_t *cand_idx, void *select_workspace, size_t workspace_bytes,
                           void *stream)
{
    ia::LevelTable t;
    int rc = ia::make_level_table(g, t);
    if (rc) return rc;
    if (batch < 1 || !select_workspace) return IA_E_ARG;
    if (workspace_bytes < ia::select_workspace_bytes(t, batch)) return IA_E_WORKSPACE;
    return ia::launch_select(t, rowmax, batch, cand_idx, select_workspace, (hipStream_t)stream,
                             true);
}

int ia_gather_decode(const ia_head_geom *g, const ia_level_ptrs *p, int batch, int dtype,
                     const int32_t *cand_idx, const float *img_hw, const float *scale_factor,
                     int rescale, float *boxes, float *scores_t, float *best_score, void *stream)
{
    // pure geometry like the row-max and top-k entries: any number of candidates per image (the
    // IA_MAX_CANDIDATES capacity belongs to the batched NMS behind ia_get_bboxes, not to this stage)
    ia::LevelTable t;
    int rc = ia::make_level_table(g, t);
    if (rc) return rc;
    if (!p || batch < 1) return IA_E_ARG;
    const int Rs = (t.cand_off[t.num_levels] + 63) / 64 * 64;
    ia::BaseAnchors ba;
    ia::base_from_geom(g, ba);
    return ia::launch_gather(t, ba, g->means, g->stds, *p, batch, dtype, cand_idx, img_hw,
                             scale_factor, rescale, boxes, scores_t, best_score, Rs,
                             (hipStream_t)stream);
}

size_t ia_multiclass_nms_workspace_bytes(int batch, int R, int C)
{
    if (batch < 1 || R < 1 || R > IA_MAX_CANDIDATES || C < 1) return 0;
    return ia::nms_tail_workspace_bytes(batch, R, C);
}

int ia_multiclass_nms(const float *boxes, const float *scores_t, const float *best_score,
                      int batch, int R, int C, float score_thr, float iou_thr, int max_per_img,
                      void *workspace, size_t workspace_bytes, float *dets, int32_t *labels,
                      int32_t *rows, int32_t *num, int32_t *keep_count, int32_t *keep_rows,
                      void *stream)
{
    const int Rs = (R + 63) / 64 * 64;
    if (!workspace) return IA_E_ARG;
    if (workspace_bytes < ia_multiclass_nms_workspace_bytes(batch, R, C) || workspace_bytes == 0)
        return IA_E_WORKSPACE;
    return ia::launch_nms_tail(boxes, scores_t, best_score, batch, R, Rs, C, score_thr, iou_thr,
                               max_per_img, workspace, nullptr, keep_count, keep_rows, dets, labels,
                               rows, num, (hipStream_t)stream);
}

// stage-level lazy NMS: lazy walk first, the complete path (gated) for the images it cannot finish
size_t ia_multiclass_nms_lazy_workspace_bytes(int batch, int R, int C)
{
    if (ia_multiclass_nms_workspace_bytes(batch, R, C) == 0) return 0;
    return ia::carve_nms_lazy(batch, R, C, nullptr).bytes;
}

int ia_multiclass_nms_lazy(const float *boxes, const float *scores_t, const float *best_score,
                           int batch, int R, int C, float score_thr, float iou_thr,
                           int max_per_img, int candidates, void *workspace,
                           size_t workspace_bytes, float *dets, int32_t *labels, int32_t *rows,
                           int32_t *num, void *stream)
{
    const int Rs = (R + 63) / 64 * 64;
    if (!workspace || candidates < 0) return IA_E_ARG;
    const size_t need = ia_multiclass_nms_lazy_workspace_bytes(batch, R, C);
    if (need == 0 || workspace_bytes < need) return IA_E_WORKSPACE;
    const ia::LazyNmsWorkspace w = ia::carve_nms_lazy(batch, R, C, workspace);
    const ia::NmsLazy lazy = {w.lazy, w.need_full, candidates};
    return ia::launch_nms_tail(boxes, scores_t, best_score, batch, R, Rs, C, score_thr, iou_thr,
                               max_per_img, w.full, &lazy, w.keep_count, w.keep_rows, dets, labels,
                               rows, num, (hipStream_t)stream);
}

size_t ia_multiclass_soft_nms_workspace_bytes(int batch, int R, int C)
{
    if (batch < 1 || R < 1 || R > IA_MAX_CANDIDATES || C < 1) return 0;
    const int Rs = (R + 63) / 64 * 64;
    return ia::align256((size_t)batch * C * Rs * sizeof(float)) +
           ia::finalize_workspace_bytes(batch, Rs, C);
}

int ia_multiclass_soft_nms(const float *boxes, const float *scores_t, int batch, int R, int C,
                           float score_thr, float iou_thr, int method, float sigma,
                           float min_score, int max_per_img, void *workspace,
                           size_t workspace_bytes, float *dets, int32_t *labels, int32_t *rows,
                           int32_t *num, int32_t *keep_count, int32_t *keep_rows, void *stream)
{
    const int Rs = (R + 63) / 64 * 64;
    if (!workspace) return IA_E_ARG;
    if (workspace_bytes < ia_multiclass_soft_nms_workspace_bytes(batch, R, C) || workspace_bytes == 0)
        return IA_E_WORKSPACE;
    float *soft = static_cast<float *>(workspace);
    int rc = ia::launch_soft_nms(boxes, scores_t, batch, R, Rs, C, score_thr, iou_thr, method,
                                 sigma, min_score, keep_count, keep_rows, soft,
                                 (hipStream_t)stream);
    if (rc) return rc;
    char *fin_ws = static_cast<char *>(workspace) +
                   ia::align256((size_t)batch * C * Rs * sizeof(float));
    return ia::launch_finalize(boxes, soft, keep_count, keep_rows, batch, R, Rs, C, max_per_img,
                               fin_ws, dets, labels, rows, num, (hipStream_t)stream);
}

int ia_soft_nms(const float *dets, int n, float iou_thr, int method, float sigma, float min_score,
                float *out_dets, int32_t *out_inds, int32_t *count, void *stream)
{
    return ia::launch_soft_nms_single(dets, n, iou_thr, method, sigma, min_score, out_dets,
                                      out_inds, count, (hipStream_t)stream);
}

size_t ia_get_bboxes_workspace_bytes(const ia_head_geom *g, int batch)
{
    ia::BboxWorkspace w;
    if (ia::carve_bboxes(g, batch, nullptr, w)) return 0;
    return w.bytes;
}

size_t ia_get_bboxes_status_offset(const ia_head_geom *g, int batch)
{
    ia::BboxWorkspace w;
    if (ia::carve_bboxes(g, batch, nullptr, w)) return 0;
    return w.select_off + ia::select_workspace_status_offset(w.t, batch);
}

int ia_get_bboxes_workspace_layout(const ia_head_geom *g, int batch, size_t offsets[8])
{
    ia::BboxWorkspace w;
    int rc = ia::carve_bboxes(g, batch, nullptr, w);
    if (rc) return rc;
    for (int i = 0; i < 8; ++i) offsets[i] = w.off[i];
    return 0;
}

// ia_profile_stage_events: a pair of caller-owned HIP events recorded on the call's stream right
// before the stage's first launch and right behind its last one (bench.py: the decode stage timed
// INSIDE the steps of the timed region).  Both null (the default): nothing is recorded.
// The hook is scoped to ONE stream (the stream current when it was installed is not known to the
// library, so the first stage call after installation binds it; ia_profile_stage_events(NULL,
// NULL) unbinds): calls on other streams / from other models in the process do not record into the
// same events.  The caller clears the hook before releasing the events.
// (events, binding flag and bound stream were four separate atomics -- a caller on another
// stream could compare with a stale stream, or see the old begin event with the new end event.  One small
// mutex around the whole record: the hook is read once per stage call, ~20 ns uncontended.)
static std::mutex g_stage_mu;
static struct { void *ev[2]; void *stream; bool bound; } g_stage = {{nullptr, nullptr}, nullptr, false};

// what the decode stages of the anchor and point entries check alike, in this order: geometry and
// batch (the layout), the pointers, the workspace's size, its 256-byte alignment
static int carve_checked(const ia_head_geom *g, const ia_level_ptrs *p, int batch, void *workspace,
                         size_t workspace_bytes, ia::BboxWorkspace &w)
{
    int rc = ia::carve_bboxes(g, batch, workspace, w);
    if (rc) return rc;
    if (!p || !workspace) return IA_E_ARG;
    if (workspace_bytes < w.bytes) return IA_E_WORKSPACE;
    if (((uintptr_t)workspace & 255u) != 0) return IA_E_ARG;
    return 0;
}

static int decode_stage_launches(const ia_head_geom *g, const ia_level_ptrs *p, int dtype,
                                 const float *img_hw, const float *scale_factor, int rescale,
                                 hipStream_t s, const ia::BboxWorkspace &w);

static int decode_stage_impl(const ia_head_geom *g, const ia_level_ptrs *p, int batch, int dtype,
                             const float *img_hw, const float *scale_factor, int rescale,
                             void *workspace, size_t workspace_bytes, hipStream_t s,
                             ia::BboxWorkspace &w)
{
    int rc = carve_checked(g, p, batch, workspace, workspace_bytes, w);
    if (rc) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_stage_mu);
        if (g_stage.ev[0]) {
            if (!g_stage.bound) { g_stage.bound = true; g_stage.stream = (void *)s; }
            if (g_stage.stream == (void *)s) { e0 = (hipEvent_t)g_stage.ev[0]; e1 = (hipEvent_t)g_stage.ev[1]; }
        }                                                           // else: another stream's call records nothing
    }
    if (e0 && (rc = ia::hip_status(hipEventRecord(e0, s)))) return rc;
    rc = decode_stage_launches(g, p, dtype, img_hw, scale_factor, rescale, s, w);
    if (!rc && e1) rc = ia::hip_status(hipEventRecord(e1, s));
    return rc;
}

static int decode_stage_launches(const ia_head_geom *g, const ia_level_ptrs *p, int dtype,
                                 const float *img_hw, const float *scale_factor, int rescale,
                                 hipStream_t s, const ia::BboxWorkspace &w)
{
    int rc;
    ia::BaseAnchors ba;
    ia::base_from_geom(g, ba);
    // row-max (+ group maxima) and the top-k's filter in one launch where the layout allows
    if ((rc = ia::launch_rowmax_select(w.t, *p, w.batch, dtype, w.rowmax, w.cand_idx, w.select, s))) return rc;
    return ia::launch_gather(w.t, ba, g->means, g->stds, *p, w.batch, dtype, w.cand_idx, img_hw, scale_factor,
                             rescale, w.boxes, w.scores_t, w.best_score, w.Rs, s);
}

// lazy_candidates < 0: the complete NMS for every image (keep_count / keep_rows of all classes
// are produced); >= 0: lazy NMS first (0 = default candidate count), complete path only for the
// images it could not finish
static int get_bboxes_impl(const ia_head_geom *g, const ia_level_ptrs *p, int batch, int dtype,
                           const float *img_hw, const float *scale_factor, int rescale,
                           float score_thr, float iou_thr, int max_per_img, int lazy_candidates,
                           void *workspace, size_t workspace_bytes, float *dets, int32_t *labels,
                           int32_t *rows, int32_t *num, void *stream)
{
    ia::BboxWorkspace w;
    hipStream_t s = (hipStream_t)stream;
    int rc = decode_stage_impl(g, p, batch, dtype, img_hw, scale_factor, rescale, workspace,
                               workspace_bytes, s, w);
    if (rc) return rc;
    return ia::launch_bboxes_nms(w, score_thr, iou_thr, max_per_img, lazy_candidates, dets, labels,
                                 rows, num, s);
}

int ia_profile_stage_events(void *begin, void *end)
{
    if ((begin == nullptr) != (end == nullptr)) return IA_E_ARG;
    std::lock_guard<std::mutex> lk(g_stage_mu);
    g_stage.ev[0] = begin; g_stage.ev[1] = end;
    g_stage.bound = false; g_stage.stream = nullptr;                // the next stage call binds its stream
    return 0;
}

int ia_decode_stage(const ia_head_geom *g, const ia_level_ptrs *p, int batch, int dtype,
                    const float *img_hw, const float *scale_factor, int rescale, void *workspace,
                    size_t workspace_bytes, void *stream)
{
    ia::BboxWorkspace w;
    return decode_stage_impl(g, p, batch, dtype, img_hw, scale_factor, rescale, workspace,
                             workspace_bytes, (hipStream_t)stream, w);
}

int ia_get_bboxes(const ia_head_geom *g, const ia_level_ptrs *p, int batch, int dtype,
                  const float *img_hw, const float *scale_factor, int rescale, float score_thr,
                  float iou_thr, int max_per_img, void *workspace, size_t workspace_bytes,
                  float *dets, int32_t *labels, int32_t *rows, int32_t *num, void *stream)
{
    return get_bboxes_impl(g, p, batch, dtype, img_hw, scale_factor, rescale, score_thr, iou_thr,
                           max_per_img, -1, workspace, workspace_bytes, dets, labels, rows, num,
                           stream);
}

int ia_get_bboxes_lazy(const ia_head_geom *g, const ia_level_ptrs *p, int batch, int dtype,
                       const float *img_hw, const float *scale_factor, int rescale,
                       float score_thr, float iou_thr, int max_per_img, int candidates,
                       void *workspace, size_t workspace_bytes, float *dets, int32_t *labels,
                       int32_t *rows, int32_t *num, void *stream)
{
    if (candidates < 0) return IA_E_ARG;
    return get_bboxes_impl(g, p, batch, dtype, img_hw, scale_factor, rescale, score_thr, iou_thr,
                           max_per_img, candidates, workspace, workspace_bytes, dets, labels, rows,
                           num, stream);
}

// point head (IoU-aware FCOS): the ia_get_bboxes workspace of the A = 1 geometry, its own decode
// stage, the shared NMS stages
size_t ia_point_workspace_bytes(const ia_point_head_geom *g, int batch)
{
    ia_head_geom hg;
    if (ia::point_head_geom(g, hg)) return 0;
    return ia_get_bboxes_workspace_bytes(&hg, batch);
}

int ia_point_workspace_layout(const ia_point_head_geom *g, int batch, size_t offsets[8])
{
    ia_head_geom hg;
    int rc = ia::point_head_geom(g, hg);
    if (rc) return rc;
    return ia_get_bboxes_workspace_layout(&hg, batch, offsets);
}

static int point_decode_impl(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                             const float *img_hw, const float *scale_factor, int rescale,
                             void *workspace, size_t workspace_bytes, hipStream_t s,
                             ia::BboxWorkspace &w, int kind, float score_thr, int dtype)
{
    ia_head_geom hg;
    int rc = ia::point_head_geom(g, hg);
    if (rc) return rc;
    if ((rc = carve_checked(&hg, p, batch, workspace, workspace_bytes, w))) return rc;
    return ia::launch_point_decode(g, w.t, *p, batch, img_hw, scale_factor, rescale, w.rowmax,
                                   w.cand_idx, w.select, w.boxes, w.scores_t, w.best_score, w.Rs,
                                   kind, score_thr, dtype, s);
}

int ia_point_decode_stage_dt(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                             int dtype, const float *img_hw, const float *scale_factor, int rescale,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    ia::BboxWorkspace w;
    return point_decode_impl(g, p, batch, img_hw, scale_factor, rescale, workspace, workspace_bytes,
                             (hipStream_t)stream, w, 0, 0.0f, dtype);
}

int ia_point_decode_stage(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                          const float *img_hw, const float *scale_factor, int rescale,
                          void *workspace, size_t workspace_bytes, void *stream)
{
    return ia_point_decode_stage_dt(g, p, batch, IA_F32, img_hw, scale_factor, rescale, workspace,
                                    workspace_bytes, stream);
}

int ia_point_ctr_decode_stage_dt(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                                 int dtype, const float *img_hw, const float *scale_factor,
                                 int rescale, float score_thr, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    ia::BboxWorkspace w;
    return point_decode_impl(g, p, batch, img_hw, scale_factor, rescale, workspace, workspace_bytes,
                             (hipStream_t)stream, w, 1, score_thr, dtype);
}

int ia_point_ctr_decode_stage(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                              const float *img_hw, const float *scale_factor, int rescale,
                              float score_thr, void *workspace, size_t workspace_bytes, void *stream)
{
    return ia_point_ctr_decode_stage_dt(g, p, batch, IA_F32, img_hw, scale_factor, rescale,
                                        score_thr, workspace, workspace_bytes, stream);
}

// decode stage of `kind`, then the shared NMS stages at `stage_thr` (the IoU-aware head: its
// score_thr; plain FCOS: kPointCtrStageThr, the raw threshold having been applied by the gather)
static int point_get_bboxes_impl(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                                 int dtype, const float *img_hw, const float *scale_factor, int rescale,
                                 int kind, float score_thr, float stage_thr, float iou_thr,
                                 int max_per_img, int candidates, void *workspace,
                                 size_t workspace_bytes, float *dets, int32_t *labels,
                                 int32_t *rows, int32_t *num, hipStream_t s)
{
    ia::BboxWorkspace w;
    if (!dets || !labels || !rows || !num) return IA_E_ARG;
    int rc = point_decode_impl(g, p, batch, img_hw, scale_factor, rescale, workspace,
                               workspace_bytes, s, w, kind, score_thr, dtype);
    if (rc) return rc;
    return ia::launch_bboxes_nms(w, stage_thr, iou_thr, max_per_img, candidates, dets, labels, rows,
                                 num, s);
}

int ia_point_get_bboxes_dt(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                           int dtype, const float *img_hw, const float *scale_factor, int rescale,
                           float score_thr, float iou_thr, int max_per_img, int candidates,
                           void *workspace, size_t workspace_bytes, float *dets, int32_t *labels,
                           int32_t *rows, int32_t *num, void *stream)
{
    return point_get_bboxes_impl(g, p, batch, dtype, img_hw, scale_factor, rescale, 0, 0.0f,
                                 score_thr, iou_thr, max_per_img, candidates, workspace,
                                 workspace_bytes, dets, labels, rows, num, (hipStream_t)stream);
}

int ia_point_get_bboxes(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                        const float *img_hw, const float *scale_factor, int rescale,
                        float score_thr, float iou_thr, int max_per_img, int candidates,
                        void *workspace, size_t workspace_bytes, float *dets, int32_t *labels,
                        int32_t *rows, int32_t *num, void *stream)
{
    return ia_point_get_bboxes_dt(g, p, batch, IA_F32, img_hw, scale_factor, rescale, score_thr,
                                  iou_thr, max_per_img, candidates, workspace, workspace_bytes,
                                  dets, labels, rows, num, stream);
}

int ia_point_ctr_get_bboxes_dt(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                               int dtype, const float *img_hw, const float *scale_factor,
                               int rescale, float score_thr, float iou_thr, int max_per_img,
                               int candidates, void *workspace, size_t workspace_bytes, float *dets,
                               int32_t *labels, int32_t *rows, int32_t *num, void *stream)
{
    return point_get_bboxes_impl(g, p, batch, dtype, img_hw, scale_factor, rescale, 1, score_thr,
                                 ia::kPointCtrStageThr, iou_thr, max_per_img, candidates, workspace,
                                 workspace_bytes, dets, labels, rows, num, (hipStream_t)stream);
}

int ia_point_ctr_get_bboxes(const ia_point_head_geom *g, const ia_level_ptrs *p, int batch,
                            const float *img_hw, const float *scale_factor, int rescale,
                            float score_thr, float iou_thr, int max_per_img, int candidates,
                            void *workspace, size_t workspace_bytes, float *dets, int32_t *labels,
                            int32_t *rows, int32_t *num, void *stream)
{
    return ia_point_ctr_get_bboxes_dt(g, p, batch, IA_F32, img_hw, scale_factor, rescale,
                                      score_thr, iou_thr, max_per_img, candidates, workspace,
                                      workspace_bytes, dets, labels, rows, num, stream);
}

size_t ia_nms_workspace_bytes(int n)
{
    return n > IA_MAX_CANDIDATES ? ia::nms_big_workspace_bytes(n) : ia::nms_single_workspace_bytes(n);
}

int ia_nms(const float *dets, int n, float iou_thr, int32_t *keep, int32_t *count, void *workspace,
           size_t workspace_bytes, void *stream)
{
    if (n > IA_MAX_CANDIDATES)              // no size limit, like nms_cpu.cpp: chunked (bignms.hip)
        return ia::launch_nms_big(dets, n, iou_thr, keep, count, workspace, workspace_bytes,
                                  (hipStream_t)stream);
    return ia::launch_nms_single(dets, n, iou_thr, keep, count, workspace, workspace_bytes,
                                 (hipStream_t)stream);
}

int ia_test_math(int op, const float *x, const float *y, float *out, int64_t n, void *stream)
{
    if (n < 0 || op < 0 || op > 6) return IA_E_ARG;
    if (n == 0) return 0;
    if (!x || !out || ((op == 4 || op == 6) && !y)) return IA_E_ARG;
    int64_t blocks = (n + 255) / 256;
    unsigned grid = (unsigned)(blocks > 8192 ? 8192 : blocks);
    hipLaunchKernelGGL(ia::k_test_math, dim3(grid), dim3(256), 0, (hipStream_t)stream, op, x, y,
                       out, n);
    return ia::hip_status(hipGetLastError());
}

}  // extern "C"
