// Post-conv path of SSDHead (reference mmdet/models/anchor_heads/ssd_head.py on anchor_head.py
// get_bboxes / get_bboxes_single, use_sigmoid_cls = False, no nms_pre): softmax over the C + 1 class
// logits of every anchor row, delta2bbox on the regenerated anchor, multiclass_nms over ALL rows of
// the image.  The number of anchors differs per level (4 / 6 / 6 / 6 / 4 / 4), so the geometry is
// ia_ssd_geom, not ia_head_geom; the 8 732 (SSD300) or 24 564 (SSD512) rows exceed the batched NMS
// (IA_MAX_CANDIDATES rows), but nearly all of them lie under score_thr in every class and the
// reference's multiclass_nms never looks at such a row.  Four stages, fp32 NCHW maps:
//
//   k_ssd_rowscore   one lane per (image, level, anchor, pixel), lanes along the pixels of one channel
//                    plane (coalesced): softmax_row_stats (ia_softmax_dev.hpp, the device function of
//                    the softmax kernels of decode.hip) -> best foreground score e_fg / s, written in
//                    the reference's row order: level, then (y, x), then anchor.
//   compaction       per image the rows with best > score_thr in ascending row order: wave ballots,
//                    a prefix scan over the per-workgroup counts, the ballots again
//                    (ia_compact_dev.hpp, the scheme of masked_conv.hip); no atomics.  kept_count is
//                    the true count; more than IA_MAX_CANDIDATES sets overflow and keeps the first
//                    IA_MAX_CANDIDATES row ids; the slots behind the count hold -1.
//   k_ssd_gather     one lane per (image, compacted row): the C foreground scores
//                    exp(x_c - m) / s class-major, their maximum, and the box through decode_box
//                    (ia_gather_dev.hpp, the device function of k_gather_softmax).  Rows behind the
//                    count (and every row of an image whose count exceeds the row capacity of the
//                    call) get a zero box, zero scores and best_score 0, which the NMS stages skip
//                    at any score_thr >= 0.
//   NMS              launch_nms / launch_finalize on the compacted rows, then k_ssd_map_rows turns
//                    the compacted row ids of the detections into anchor row ids.
//
// Compaction keeps the rows' relative order and drops only rows that take part in no class problem,
// so the detections are those of the uncompacted evaluation, canonical tie order included.
#include <string.h>
#include "ia_internal.hpp"
#include "ia_math.hpp"
#include "ia_ssd.hpp"
#include "ia_softmax_dev.hpp"
#include "ia_compact_dev.hpp"
#include "ia_gather_dev.hpp"

namespace ia {

// ------------------------------------------------------------------ stage 1: row scores
struct SsdRowArgs {
    SsdTable t;
    float *best;                             // (B, R)
};

__global__ void __launch_bounds__(256) k_ssd_rowscore(SsdRowArgs a)
{
    const int l = (int)blockIdx.y % a.t.num_levels, b = (int)blockIdx.y / a.t.num_levels;
    const int A = a.t.A[l], Cin = a.t.C + 1, HW = a.t.H[l] * a.t.W[l];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (anchor, pixel): pixels along the lanes
    if (i >= (int64_t)HW * A) return;
    const int an = (int)(i / HW), pos = (int)(i - (int64_t)an * HW);
    const float *cls = a.t.cls[l] + ((size_t)b * A + an) * Cin * HW + pos;
    float m, s, e;
    softmax_row_stats<float>(cls, (size_t)HW, Cin, m, s, e);
    const int R = a.t.row_off[a.t.num_levels];
    a.best[(size_t)b * R + a.t.row_off[l] + (size_t)pos * A + an] = e / s;
}

static int launch_ssd_rowscore(const SsdTable &t, int batch, float *best, hipStream_t s)
{
    if (!best || batch < 1) return IA_E_ARG;
    if ((int64_t)batch * t.num_levels > 65535) return IA_E_ARG;
    if ((int64_t)batch * t.row_off[t.num_levels] > 2147483647LL) return IA_E_ARG;
    SsdRowArgs a;
    a.t = t; a.best = best;
    int64_t nmax = 1;
    for (int l = 0; l < t.num_levels; ++l) {
        const int64_t n = t.row_off[l + 1] - t.row_off[l];
        nmax = n > nmax ? n : nmax;
    }
    const dim3 grid((unsigned)((nmax + 255) / 256), (unsigned)(batch * t.num_levels));
    hipLaunchKernelGGL(k_ssd_rowscore, grid, dim3(256), 0, s, a);
    return hip_status(hipGetLastError());
}

// ------------------------------------------------------------------ stage 2: compaction per image
static int ssd_row_blocks(int R) { return (R + kMaskBlock - 1) / kMaskBlock; }

// grid (row blocks, batch): kept rows of each workgroup
__global__ void __launch_bounds__(kMaskBlock) k_ssd_count(const float *best, int R, float thr, int32_t *block_count)
{
    __shared__ int s_wave[kMaskBlock / 64];
    const int r = blockIdx.x * kMaskBlock + threadIdx.x, b = blockIdx.y;
    const bool keep = r < R && best[(size_t)b * R + r] > thr;
    const int n = block_keep_count(keep, s_wave);
    if (threadIdx.x == 0) block_count[(size_t)b * gridDim.x + blockIdx.x] = n;
}

// one workgroup per image: prefix over its row blocks, the count, the overflow flag, and -1 in the
// slots of kept_rows that k_ssd_write will not fill
__global__ void __launch_bounds__(256) k_ssd_scan(const int32_t *block_count, int32_t *block_off, int nb,
                                                  int32_t *kept_rows, int32_t *kept_count, int32_t *overflow)
{
    __shared__ int s_v[256];
    __shared__ int s_carry;
    const int b = blockIdx.x;
    const int total = scan_block_counts(block_count + (size_t)b * nb, block_off + (size_t)b * nb, nb, s_v, &s_carry);
    if (threadIdx.x == 0) {
        kept_count[b] = total;
        overflow[b] = total > IA_MAX_CANDIDATES ? 1 : 0;
    }
    for (int i = total + (int)threadIdx.x; i < IA_MAX_CANDIDATES; i += 256)
        kept_rows[(size_t)b * IA_MAX_CANDIDATES + i] = -1;
}

__global__ void __launch_bounds__(kMaskBlock) k_ssd_write(const float *best, int R, float thr, const int32_t *block_off,
                                                          int32_t *kept_rows)
{
    __shared__ int s_wave[kMaskBlock / 64];
    const int r = blockIdx.x * kMaskBlock + threadIdx.x, b = blockIdx.y;
    const bool keep = r < R && best[(size_t)b * R + r] > thr;
    const int k = block_off[(size_t)b * gridDim.x + blockIdx.x] + block_keep_rank(keep, s_wave);
    if (keep && k < IA_MAX_CANDIDATES) kept_rows[(size_t)b * IA_MAX_CANDIDATES + k] = r;
}

static size_t ssd_compact_bytes(int batch, int R)
{
    return (size_t)2 * batch * ssd_row_blocks(R) * sizeof(int32_t);
}

static int launch_ssd_compact(const float *best, int batch, int R, float thr, int32_t *kept_rows, int32_t *kept_count,
                              int32_t *overflow, void *workspace, hipStream_t s)
{
    if (!best || !kept_rows || !kept_count || !overflow || !workspace) return IA_E_ARG;
    if (batch < 1 || batch > 65535 || R < 1) return IA_E_ARG;
    if ((uintptr_t)workspace & 3u) return IA_E_ARG;
    const int nb = ssd_row_blocks(R);
    int32_t *block_count = static_cast<int32_t *>(workspace), *block_off = block_count + (size_t)batch * nb;
    const dim3 grid((unsigned)nb, (unsigned)batch);
    hipLaunchKernelGGL(k_ssd_count, grid, dim3(kMaskBlock), 0, s, best, R, thr, block_count);
    hipLaunchKernelGGL(k_ssd_scan, dim3((unsigned)batch), dim3(256), 0, s, block_count, block_off, nb, kept_rows,
                       kept_count, overflow);
    hipLaunchKernelGGL(k_ssd_write, grid, dim3(kMaskBlock), 0, s, best, R, thr, block_off, kept_rows);
    return hip_status(hipGetLastError());
}

// ------------------------------------------------------------------ stage 3: gather / decode
struct SsdGatherArgs {
    SsdTable t;
    BaseAnchors ba;
    float means[4], stds[4];                 // decode_box reads these four members
    const float *img_hw, *scale_factor;
    int32_t rescale;
    const int32_t *kept_rows, *kept_count;
    int32_t kept_stride, Rk, Rs;
    float *boxes, *scores_t, *best_score;
};

__global__ void __launch_bounds__(64) k_ssd_gather(SsdGatherArgs a)
{
    const int b = blockIdx.y;
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= a.Rk) return;
    const int C = a.t.C, Cin = C + 1;
    float *so = a.scores_t + (size_t)b * C * a.Rs + r;
    float4 *box = reinterpret_cast<float4 *>(a.boxes) + (size_t)b * a.Rk + r;
    const int cnt = a.kept_count[b];
    const int n = cnt > a.Rk ? 0 : cnt;      // an image beyond the capacity takes part in nothing
    const int row = r < n ? a.kept_rows[(size_t)b * a.kept_stride + r] : -1;
    if (row < 0 || row >= a.t.row_off[a.t.num_levels]) {
        for (int c = 0; c < C; ++c) so[(size_t)c * a.Rs] = 0.0f;
        a.best_score[(size_t)b * a.Rk + r] = 0.0f;
        *box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    // level of the row: compares and selects on the scalar tables (ia_gather_dev.hpp, level_of_candidate)
    int l = 0;
#pragma unroll
    for (int k = 1; k < IA_MAX_LEVELS; ++k) l += (k < a.t.num_levels && row >= a.t.row_off[k]) ? 1 : 0;
    int base = a.t.row_off[0], H = a.t.H[0], W = a.t.W[0], stride = a.t.stride[0], A = a.t.A[0];
    const float *clsl = a.t.cls[0], *regl = a.t.reg[0];
#pragma unroll
    for (int k = 1; k < IA_MAX_LEVELS; ++k) {
        const bool m = l == k;
        base = m ? a.t.row_off[k] : base;
        H = m ? a.t.H[k] : H; W = m ? a.t.W[k] : W; stride = m ? a.t.stride[k] : stride; A = m ? a.t.A[k] : A;
        clsl = m ? a.t.cls[k] : clsl; regl = m ? a.t.reg[k] : regl;
    }
    const int HW = H * W;
    const int idx = row - base;
    const int pos = idx / A, an = idx - pos * A;
    const size_t cs = (size_t)HW;
    const float *cls = clsl + ((size_t)b * A + an) * Cin * HW + pos;
    float m, s, e_fg;
    softmax_row_stats<float>(cls, cs, Cin, m, s, e_fg);
    float best = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float p = expf_(cls[(size_t)(c + 1) * cs] - m) / s;
        so[(size_t)c * a.Rs] = p;
        best = (best < p) ? p : best;
    }
    a.best_score[(size_t)b * a.Rk + r] = best;
    const float *reg = regl + ((size_t)b * A + an) * 4 * HW + pos;
    const float *ba = a.ba.v[l][an];
    *box = decode_box(a, b, ba[0], ba[1], ba[2], ba[3], W, stride, pos, reg[0], reg[cs], reg[2 * cs], reg[3 * cs]);
}

static int launch_ssd_gather(const ia_ssd_geom *g, const SsdTable &t, int batch, const int32_t *kept_rows,
                             int kept_stride, const int32_t *kept_count, int Rk, const float *img_hw,
                             const float *scale_factor, int rescale, float *boxes, float *scores_t, float *best_score,
                             hipStream_t s)
{
    if (!kept_rows || !kept_count || !img_hw || !boxes || !scores_t || !best_score) return IA_E_ARG;
    if (rescale && !scale_factor) return IA_E_ARG;
    if (batch < 1 || batch > 65535 || Rk < 1 || kept_stride < Rk) return IA_E_ARG;
    if (((uintptr_t)boxes & 15u) != 0) return IA_E_ARG;
    SsdGatherArgs a;
    a.t = t;
    memcpy(a.ba.v, g->base_anchors, sizeof(a.ba.v));
    for (int k = 0; k < 4; ++k) { a.means[k] = g->means[k]; a.stds[k] = g->stds[k]; }
    a.img_hw = img_hw; a.scale_factor = scale_factor; a.rescale = rescale ? 1 : 0;
    a.kept_rows = kept_rows; a.kept_count = kept_count; a.kept_stride = kept_stride;
    a.Rk = Rk; a.Rs = (Rk + 63) / 64 * 64;
    a.boxes = boxes; a.scores_t = scores_t; a.best_score = best_score;
    hipLaunchKernelGGL(k_ssd_gather, dim3((unsigned)((Rk + 63) / 64), (unsigned)batch), dim3(64), 0, s, a);
    return hip_status(hipGetLastError());
}

// ------------------------------------------------------------------ stage 4: rows back to anchor rows
__global__ void __launch_bounds__(256) k_ssd_map_rows(const int32_t *kept_rows, const int32_t *overflow, int max_per_img,
                                                      int32_t *rows, int32_t *num)
{
    const int b = blockIdx.x;
    const bool over = overflow[b] != 0;
    const int n = over ? 0 : num[b];
    for (int i = threadIdx.x; i < n; i += 256) {
        const int r = rows[(size_t)b * max_per_img + i];
        if (r >= 0 && r < IA_MAX_CANDIDATES) rows[(size_t)b * max_per_img + i] = kept_rows[(size_t)b * IA_MAX_CANDIDATES + r];
    }
    if (over && threadIdx.x == 0) num[b] = 0;
}

// workspace of ia_ssd_get_bboxes, in this order; off: the byte offsets of the first eight pieces
// (ia_ssd_workspace_layout)
struct SsdWorkspace {
    float *row_score;         // (B, R)
    int32_t *kept_rows;       // (B, IA_MAX_CANDIDATES)
    int32_t *kept_count;      // (B)
    float *boxes;             // (B, Rk, 4)
    float *scores_t;          // (B, C, Rs)
    float *best_score;        // (B, Rk)
    int32_t *keep_count;      // (B, C)
    int32_t *keep_rows;       // (B, C, Rs)
    void *compact;            // compaction parts
    void *nms;                // NMS stage | final keys (launch_nms_tail)
    size_t off[8];
    size_t bytes;
    int32_t R, Rk, Rs;
};

static int carve_ssd(const SsdTable &t, int batch, void *base, SsdWorkspace &w)
{
    if (batch < 1 || batch > 65535) return IA_E_ARG;
    w.R = t.row_off[t.num_levels];
    w.Rk = w.R < IA_MAX_CANDIDATES ? w.R : IA_MAX_CANDIDATES;
    w.Rs = (w.Rk + 63) / 64 * 64;
    const size_t B = (size_t)batch, C = (size_t)t.C;
    Carver c(base);
    w.off[0] = c.take(w.row_score, B * w.R * sizeof(float));
    w.off[1] = c.take(w.kept_rows, B * IA_MAX_CANDIDATES * sizeof(int32_t));
    w.off[2] = c.take(w.kept_count, B * sizeof(int32_t));
    w.off[3] = c.take(w.boxes, B * w.Rk * 4 * sizeof(float));
    w.off[4] = c.take(w.scores_t, B * C * w.Rs * sizeof(float));
    w.off[5] = c.take(w.best_score, B * w.Rk * sizeof(float));
    w.off[6] = c.take(w.keep_count, B * C * sizeof(int32_t));
    w.off[7] = c.take(w.keep_rows, B * C * w.Rs * sizeof(int32_t));
    c.take(w.compact, ssd_compact_bytes(batch, w.R));
    c.take(w.nms, nms_tail_workspace_bytes(batch, w.Rk, t.C));
    w.bytes = c.bytes;
    return 0;
}

}  // namespace ia

extern "C" {

int ia_ssd_geom_rows(const ia_ssd_geom *g, int32_t *R, int32_t level_off[IA_MAX_LEVELS + 1])
{
    ia::SsdTable t;
    int rc = ia::make_ssd_table(g, nullptr, t);
    if (rc) return rc;
    if (R) *R = t.row_off[t.num_levels];
    if (level_off)
        for (int l = 0; l <= IA_MAX_LEVELS; ++l) level_off[l] = t.row_off[l < t.num_levels ? l : t.num_levels];
    return 0;
}

int ia_ssd_rowscore(const ia_ssd_geom *g, const ia_ssd_level_ptrs *p, int batch, int dtype, float *best, void *stream)
{
    ia::SsdTable t;
    if (!p || dtype != IA_F32) return IA_E_ARG;
    int rc = ia::make_ssd_table(g, p, t);
    if (rc) return rc;
    return ia::launch_ssd_rowscore(t, batch, best, (hipStream_t)stream);
}

size_t ia_ssd_compact_workspace_bytes(int batch, int R)
{
    if (batch < 1 || batch > 65535 || R < 1) return 0;
    return ia::ssd_compact_bytes(batch, R);
}

int ia_ssd_compact(const float *best, int batch, int R, float score_thr, int32_t *kept_rows, int32_t *kept_count,
                   int32_t *overflow, void *workspace, size_t workspace_bytes, void *stream)
{
    const size_t need = ia_ssd_compact_workspace_bytes(batch, R);
    if (need == 0) return IA_E_ARG;
    if (workspace && workspace_bytes < need) return IA_E_WORKSPACE;
    return ia::launch_ssd_compact(best, batch, R, score_thr, kept_rows, kept_count, overflow, workspace,
                                  (hipStream_t)stream);
}

int ia_ssd_gather_decode(const ia_ssd_geom *g, const ia_ssd_level_ptrs *p, int batch, int dtype,
                         const int32_t *kept_rows, int kept_stride, const int32_t *kept_count, int Rk,
                         const float *img_hw, const float *scale_factor, int rescale, float *boxes, float *scores_t,
                         float *best_score, void *stream)
{
    ia::SsdTable t;
    if (!p || dtype != IA_F32) return IA_E_ARG;
    int rc = ia::make_ssd_table(g, p, t);
    if (rc) return rc;
    return ia::launch_ssd_gather(g, t, batch, kept_rows, kept_stride, kept_count, Rk, img_hw, scale_factor, rescale,
                                 boxes, scores_t, best_score, (hipStream_t)stream);
}

size_t ia_ssd_get_bboxes_workspace_bytes(const ia_ssd_geom *g, int batch)
{
    ia::SsdTable t;
    ia::SsdWorkspace w;
    if (ia::make_ssd_table(g, nullptr, t) || ia::carve_ssd(t, batch, nullptr, w)) return 0;
    return w.bytes;
}

int ia_ssd_workspace_layout(const ia_ssd_geom *g, int batch, size_t offsets[8])
{
    ia::SsdTable t;
    ia::SsdWorkspace w;
    if (!offsets) return IA_E_ARG;
    int rc = ia::make_ssd_table(g, nullptr, t);
    if (rc) return rc;
    if ((rc = ia::carve_ssd(t, batch, nullptr, w))) return rc;
    for (int i = 0; i < 8; ++i) offsets[i] = w.off[i];
    return 0;
}

int ia_ssd_get_bboxes(const ia_ssd_geom *g, const ia_ssd_level_ptrs *p, int batch, int dtype, const float *img_hw,
                      const float *scale_factor, int rescale, float score_thr, float iou_thr, int max_per_img,
                      void *workspace, size_t workspace_bytes, float *dets, int32_t *labels, int32_t *rows,
                      int32_t *num, int32_t *overflow, void *stream)
{
    ia::SsdTable t;
    ia::SsdWorkspace w;
    if (!p || dtype != IA_F32) return IA_E_ARG;
    int rc = ia::make_ssd_table(g, p, t);
    if (rc) return rc;
    if (!(score_thr >= 0.0f)) return IA_E_ARG;      // the zero rows behind the kept count must not pass
    if (!workspace || !dets || !labels || !rows || !num || !overflow || !img_hw) return IA_E_ARG;
    if (((uintptr_t)workspace & 255u) != 0) return IA_E_ARG;
    if (max_per_img > IA_MAX_PER_IMG) return IA_E_LIMIT_PER_IMG;
    if (max_per_img < 1) return IA_E_ARG;
    if ((rc = ia::carve_ssd(t, batch, workspace, w))) return rc;
    if (workspace_bytes < w.bytes) return IA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = ia::launch_ssd_rowscore(t, batch, w.row_score, s))) return rc;
    if ((rc = ia::launch_ssd_compact(w.row_score, batch, w.R, score_thr, w.kept_rows, w.kept_count, overflow,
                                     w.compact, s)))
        return rc;
    if ((rc = ia::launch_ssd_gather(g, t, batch, w.kept_rows, IA_MAX_CANDIDATES, w.kept_count, w.Rk, img_hw,
                                    scale_factor, rescale, w.boxes, w.scores_t, w.best_score, s)))
        return rc;
    if ((rc = ia::launch_nms_tail(w.boxes, w.scores_t, w.best_score, batch, w.Rk, w.Rs, t.C, score_thr, iou_thr,
                                  max_per_img, w.nms, nullptr, w.keep_count, w.keep_rows, dets, labels, rows, num, s)))
        return rc;
    hipLaunchKernelGGL(ia::k_ssd_map_rows, dim3((unsigned)batch), dim3(256), 0, s, w.kept_rows, overflow, max_per_img,
                       rows, num);
    return ia::hip_status(hipGetLastError());
}

}  // extern "C"
