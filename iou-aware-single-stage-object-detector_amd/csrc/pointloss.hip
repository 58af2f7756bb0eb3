// Training side of the FCOS heads (IoUawareFCOSHead, FCOSHead): point targets and the loss of
// every pyramid level (reference fcos_head.py:105-191 / iou_aware_fcos_head.py:139-226 `loss`,
// `fcos_target`, `fcos_target_single`, `centerness_target`; core/loss/losses.py:636-646 iou_loss;
// core/bbox/geometry.py aligned bbox_overlaps; core/bbox/transforms.py distance2bbox).
//
//   targets : k_point_targets                                               (1 launch)
//   forward : [k_point_pack]  k_focal_ml<fwd>  k_point_box<fwd>  k_point_finalize   (3-4 launches)
//   backward: k_point_box<bwd>  k_focal_ml<bwd>                             (2 launches)
//
// * k_point_targets -- a workgroup owns 256 points of one (level, image), stages that image's gt
//   boxes and areas in LDS once and every thread scans them.  Every quantity is one IEEE fp32
//   operation on fp32 inputs, the area's product is not contracted (-ffp-contract=off is part of
//   the build): labels and targets are bit-identical to the torch evaluation on the CPU.  It also
//   writes the int32 label copy (+ weights of 1) the focal kernel reads: with A = 1 the kernel's
//   anchor-major (B, A, HW) order IS the level-major (B, N_l) order of the targets.
// * focal term -- k_focal_ml<float> of headloss.hip with A = 1, through launch_focal_ml_f32.  Its
//   backward reads upstream gradient and normaliser in the (3L + 4) layout of the anchor node:
//   k_point_finalize writes an internal vector in that layout (normaliser n + B), and
//   k_point_box<bwd>, which runs before it, copies the upstream gradient of loss_cls into it.
// * k_point_box -- one pass over the labels; only a positive point (< 2 % of them) reads targets,
//   distances, centerness and IoU logits; exact-math helpers of ia_math.hpp there.  Forward: five
//   fp64 sums into the IA_LOSS_SLOTS scheme; backward: d bbox_pred (IoU-loss part + the part
//   through the attached IoU target in one store), d centerness, d iou for every point.
// * k_point_finalize -- slots -> the six result floats; n = 0 decided here, on the device.
//
// Channels-last rows (ia_point_head_loss_*_nhwc): the head outputs as the two HIP tower routes leave
// them, fp32 or bf16 pixel rows [cls C | ctr | pad] and [reg 4 | iou? | pad] addressed by pixel strides,
// the reg row optionally raw (d = exp(scale_l * x) formed here).
//   forward : k_focal_nhwc<fwd, T, unit weights>  k_point_box_nhwc<T, fwd>  k_point_finalize   (3 launches)
//   backward: k_point_box_nhwc<T, bwd>  k_focal_nhwc<bwd, T, unit weights>  [k_point_scale_finalize]
// The labels are read from the int64 targets (low words), no packed copy; the finalize kernel and the
// slot layout are those of the NCHW node; the box kernel's backward also writes the zero gradient of a
// row's padding channels and adds g * d * x into fp64 slots per level (d scale_l).
//
// One body per step of the box loss.  The box kernels of the two layouts (k_point_box: NCHW planes;
// k_point_box_nhwc: pixel rows of T, optional exp(scale x)) keep block location, the positive test,
// their loads, their stores and the padding-channel zeros; the rest is shared: point_centre (also the
// targets kernel's), point_elem, point_fwd_terms (the five sums), point_bwd_terms (the whole chain down
// to the four distance gradients, exactly 0 at the minimum) and point_block_reduce (early-out, wave
// sums, fixed tree, one fp64 atomic per term; its one-term form adds d scale_l).  With the same result
// and upstream vectors the two backward kernels give the same bits (tests/test_gpu_point_loss_nhwc.py).
// Host: both workspaces come off one Carver head (carve_point_head), both forwards end in
// clear_point_slots ... launch_point_finalize, both box kernels are picked from a table.
#include <string.h>
#include "ia_loss.hpp"
#include "ia_headloss.hpp"

namespace ia {

constexpr int kPtMaxGt = 512;             // gt boxes per image held in LDS
constexpr float kPtInf = 1e8f;            // the reference's INF sentinel (fcos_head.py:11)
constexpr int kPtSums = 5;                // sum -log(u) c | sum c | sum BCE_ctr | sum BCE_iou | n
constexpr int kPtSlotMask = IA_LOSS_SLOTS - 1;

// packed: the NCHW node's focal kernel reads the packed labels (the channels-last node does not)
static int point_levels(const ia_point_head_geom *pg, int B, HLLevels &lv, bool packed = true,
                        ia_head_geom *out = nullptr)
{
    if (!pg) return IA_E_ARG;
    ia_head_geom g = ia_head_geom{};
    g.num_levels = pg->num_levels;
    g.num_anchors = 1;
    g.num_classes = pg->num_classes;
    if (g.num_levels < 1 || g.num_levels > IA_MAX_LEVELS) return IA_E_ARG;
    for (int l = 0; l < g.num_levels; ++l) {
        g.H[l] = pg->H[l]; g.W[l] = pg->W[l]; g.stride[l] = pg->stride[l];
        if (g.stride[l] < 1) return IA_E_ARG;
    }
    g.layout = IA_LAYOUT_NCHW;
    g.cls_activation = IA_CLS_SIGMOID_NOIOU;
    int rc = fill_levels(&g, B, lv);
    if (rc) return rc;
    if (out) *out = g;
    if (!packed) return 0;
    // the focal kernel reads the packed labels of a level with HW % 4 == 0 in 16-byte pieces
    for (int l = 0; l < lv.L; ++l)
        if (((lv.H[l] * lv.W[l]) & 3) == 0 && (lv.pack_off[l] & 3)) return IA_E_ARG;
    return 0;
}

// packed labels: int32 labels [padded] | fp32 weights [padded]
static size_t packed_pad(const HLLevels &lv) { return ((size_t)lv.pack_off[lv.L] + 63) / 64 * 64; }

struct PtBlock { int l, b, p0; };
__device__ __forceinline__ PtBlock locate_point_block(const HLLevels &lv, int bid)
{
    int o = 0;
    while (bid >= lv.blk_off[o + 1]) ++o;                 // launch order: small levels first
    PtBlock r;
    r.l = lv.L - 1 - o;
    const int q = bid - lv.blk_off[o];
    const int tiles = (lv.H[r.l] * lv.W[r.l] + 255) / 256;
    r.b = q / tiles;
    r.p0 = (q - r.b * tiles) * 256;
    return r;
}

// the image coordinates of point p of a level (targets and both box kernels)
__device__ __forceinline__ void point_centre(int p, int W, int stride, float &px, float &py)
{
    const int y = p / W, x = p - y * W;
    px = (float)(x * stride) + (float)(stride / 2);
    py = (float)(y * stride) + (float)(stride / 2);
}

// ------------------------------------------------------------------ targets
struct PtTargetArgs {
    HLLevels lv;
    const float *gt_ptr[IA_MAX_TARGET_BATCH];
    const int64_t *gl_ptr[IA_MAX_TARGET_BATCH];
    int16_t num_gt[IA_MAX_TARGET_BATCH];
    float lo[IA_MAX_LEVELS], hi[IA_MAX_LEVELS];
    int64_t *labels;                      // level-major (B, N_l) blocks
    float *bbox_targets;                  // level-major (B, N_l, 4) blocks
    int32_t *lab32;                       // packed copy or NULL
    float *w32;
    int32_t *counts;                      // (B), zero-initialised
};

__global__ void __launch_bounds__(256) k_point_targets(PtTargetArgs a)
{
    __shared__ float4 s_gt[kPtMaxGt];
    __shared__ float s_area[kPtMaxGt];
    __shared__ uint32_t s_cnt;
    const PtBlock r = locate_point_block(a.lv, blockIdx.x);
    const int G = a.num_gt[r.b];
    const float4 *gsrc = reinterpret_cast<const float4 *>(a.gt_ptr[r.b]);
    for (int g = threadIdx.x; g < G; g += 256) {
        const float4 q = gsrc[g];
        s_gt[g] = q;
        s_area[g] = ((q.z - q.x) + 1.0f) * ((q.w - q.y) + 1.0f);
    }
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const int W = a.lv.W[r.l], HW = a.lv.H[r.l] * W, s = a.lv.stride[r.l];
    const int p = r.p0 + threadIdx.x;
    bool is_pos = false;
    if (p < HW) {
        float px, py;
        point_centre(p, W, s, px, py);
        const float lo = a.lo[r.l], hi = a.hi[r.l];
        // areas.min(dim=1) over the row with non-candidates set to INF: the first minimum
        float best = 0.0f;
        int arg = 0;
        float4 bt = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int g = 0; g < G; ++g) {
            const float4 q = s_gt[g];
            const float dl = px - q.x, dt = py - q.y, dr = q.z - px, db = q.w - py;
            const float mn = __builtin_fminf(__builtin_fminf(dl, dt), __builtin_fminf(dr, db));
            const float mx = __builtin_fmaxf(__builtin_fmaxf(dl, dt), __builtin_fmaxf(dr, db));
            const bool cand = (mn > 0.0f) && (mx >= lo) && (mx <= hi);
            const float ar = cand ? s_area[g] : kPtInf;
            if (g == 0 || ar < best) { best = ar; arg = g; bt = make_float4(dl, dt, dr, db); }
        }
        int64_t label = 0;
        if (best != kPtInf) { label = a.gl_ptr[r.b][arg]; is_pos = label != 0; }
        const size_t out = (size_t)a.lv.pack_off[r.l] + (size_t)r.b * HW + p;   // A = 1: B * point_off_l + b * N_l + p
        a.labels[out] = label;
        reinterpret_cast<float4 *>(a.bbox_targets)[out] = bt;
        if (a.lab32) { a.lab32[out] = (int32_t)label; a.w32[out] = 1.0f; }
    }
    const uint64_t mp = __ballot(is_pos);
    if ((threadIdx.x & 63) == 0 && mp) atomicAdd(&s_cnt, (uint32_t)__builtin_popcountll(mp));
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&a.counts[r.b], (int32_t)s_cnt);
}

// ------------------------------------------------------------------ labels -> packed copy
struct PtPackArgs {
    HLLevels lv;
    const int64_t *labels[IA_MAX_LEVELS];
    int32_t *lab32;
    float *w32;
};

__global__ void __launch_bounds__(256) k_point_pack(PtPackArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.lv.pack_off[a.lv.L]) return;
    int l = 0;
    while (i >= a.lv.pack_off[l + 1]) ++l;
    a.lab32[i] = (int32_t)a.labels[l][i - a.lv.pack_off[l]];
    a.w32[i] = 1.0f;
}

// ------------------------------------------------------------------ regression / centerness / IoU terms
struct PtBoxArgs {
    HLLevels lv;
    const float *reg[IA_MAX_LEVELS], *ctr[IA_MAX_LEVELS], *iou[IA_MAX_LEVELS];
    const float *bt[IA_MAX_LEVELS];
    const int32_t *lab32;
    float *g_reg[IA_MAX_LEVELS], *g_ctr[IA_MAX_LEVELS], *g_iou[IA_MAX_LEVELS];
    double *sums;                         // fwd: [kPtSums][IA_LOSS_SLOTS] behind the focal slots
    const float *res, *gin;               // bwd: the six result floats, the four upstream gradients
    float *fgin;                          // bwd: the focal kernel's upstream vector (entry 3L)
    int32_t attach;
};

// sx1 .. sy2: the share of d ov / d (intersection edge) that the predicted edge takes -- 1 inside the
// target's, 0 outside, 0.5 on it (what torch.max / torch.min and the anchor kernels of ia_loss.hpp do)
struct PtElem { float c, u, ov, un, w, h, pw, ph, sx1, sy1, sx2, sy2; };

__device__ __forceinline__ float tie_share(bool in, bool on) { return in ? 1.0f : (on ? 0.5f : 0.0f); }

// centerness target, the two boxes and their aligned IoU (+1 widths) of one positive point
__device__ __forceinline__ PtElem point_elem(float px, float py, const float (&d)[4], const float4 &t)
{
    PtElem e;
    const float lrmin = __builtin_fminf(t.x, t.z), lrmax = __builtin_fmaxf(t.x, t.z);
    const float tbmin = __builtin_fminf(t.y, t.w), tbmax = __builtin_fmaxf(t.y, t.w);
    e.c = __builtin_sqrtf((lrmin / lrmax) * (tbmin / tbmax));
    const float px1 = px - d[0], py1 = py - d[1], px2 = px + d[2], py2 = py + d[3];
    const float tx1 = px - t.x, ty1 = py - t.y, tx2 = px + t.z, ty2 = py + t.w;
    const bool x1in = px1 > tx1, y1in = py1 > ty1, x2in = px2 < tx2, y2in = py2 < ty2;
    e.sx1 = tie_share(x1in, px1 == tx1); e.sy1 = tie_share(y1in, py1 == ty1);
    e.sx2 = tie_share(x2in, px2 == tx2); e.sy2 = tie_share(y2in, py2 == ty2);
    const float ltx = x1in ? px1 : tx1, lty = y1in ? py1 : ty1;
    const float rbx = x2in ? px2 : tx2, rby = y2in ? py2 : ty2;
    const float w0 = (rbx - ltx) + 1.0f, h0 = (rby - lty) + 1.0f;
    e.w = (w0 < 0.0f) ? 0.0f : w0; e.h = (h0 < 0.0f) ? 0.0f : h0;
    e.ov = e.w * e.h;
    e.pw = (px2 - px1) + 1.0f; e.ph = (py2 - py1) + 1.0f;
    const float ap = e.pw * e.ph;
    const float at = ((tx2 - tx1) + 1.0f) * ((ty2 - ty1) + 1.0f);
    e.un = (ap + at) - e.ov;
    e.u = e.ov / e.un;
    return e;
}

// ---- one body per step of the box loss: what k_point_box and k_point_box_nhwc share ----
// forward: -log(u) c | c | BCE_ctr | BCE_iou | 1 of one positive point
template <bool IOU>
__device__ __forceinline__ void point_fwd_terms(const PtElem &q, float xc, float xi, double (&acc)[kPtSums])
{
    acc[0] = (double)(-logf_(q.u) * q.c);
    acc[1] = (double)q.c;
    acc[2] = (double)bce_logits_(xc, q.c);
    if constexpr (IOU) acc[3] = (double)bce_logits_(xi, q.u);
    acc[4] = 1.0;
}

// backward of one positive point with respect to the four distances, the centerness and the IoU logit
template <bool IOU>
__device__ __forceinline__ void point_bwd_terms(const PtElem &q, float xc, float xi, const float *res,
                                                const float *gin, int attach, float (&g_box)[4],
                                                float &g_ctr, float &g_iou)
{
    const float n = res[4], sc = res[5];
    const float gs_reg = gin[1] / sc, gs_ctr = gin[2] / n;
    g_ctr = (sigmoidf_(xc) - q.c) * gs_ctr;
    float gu = -(q.c / q.u) * gs_reg;                    // d(-log(u) c) / du
    if constexpr (IOU) {
        const float gs_iou = gin[3] / n;
        g_iou = (sigmoidf_(xi) - q.u) * gs_iou;
        if (attach) gu += (-xi) * gs_iou;                // d BCE(xi, u) / du = -xi
    }
    // u = ov / un, un = ap + at - ov; both factors are formed as (v / un) / un, so that at
    // ov == un (prediction == target) d/d ov is -2 d/d ap to the bit and the two halves below
    // cancel it: the gradient at the loss's minimum is exactly 0
    const float inv_un = 1.0f / q.un;
    const float g_ov = gu * (((q.un + q.ov) * inv_un) * inv_un);
    const float g_ap = gu * (-(q.ov * inv_un) * inv_un);
    const float g_w = g_ov * q.h, g_h = g_ov * q.w;      // w0, h0 > 0: both boxes hold the point
    const float g_pw = g_ap * q.ph, g_ph = g_ap * q.pw;
    // x1 = px - left, x2 = px + right: d/d left = -d/d x1
    g_box[0] = g_pw + q.sx1 * g_w;
    g_box[1] = g_ph + q.sy1 * g_h;
    g_box[2] = g_pw + q.sx2 * g_w;
    g_box[3] = g_ph + q.sy2 * g_h;
}

// NT fp64 terms of a 256-thread block into their slots: wave sums, the fixed ((r0 + r1) + r2) + r3
// order, one atomic per term (term k at sums + k * IA_LOSS_SLOTS).  Positives are rare: a block
// without one adds nothing.  SKIP: a term left out (-1: none).
template <int NT, int SKIP>
__device__ __forceinline__ void point_block_reduce(double *sums, const double (&acc)[NT], bool pos,
                                                   double (&red)[kPtSums][4])
{
    if (!__syncthreads_or(pos)) return;
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        if (k == SKIP) continue;
        const double s = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0) red[k][w] = s;
    }
    __syncthreads();
    if (threadIdx.x < NT && (int)threadIdx.x != SKIP) {
        const int k = threadIdx.x;
        const double s = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
        atomicAdd(sums + (size_t)k * IA_LOSS_SLOTS + (blockIdx.x & kPtSlotMask), s);
    }
}

template <bool BWD, bool IOU>
__global__ void __launch_bounds__(256) k_point_box(PtBoxArgs a)
{
    __shared__ double red[kPtSums][4];
    const PtBlock r = locate_point_block(a.lv, blockIdx.x);
    const int W = a.lv.W[r.l], HW = a.lv.H[r.l] * W;
    const int p = r.p0 + threadIdx.x;
    if (BWD && blockIdx.x == 0 && threadIdx.x == 0) a.fgin[3 * a.lv.L] = a.gin[0];
    double acc[kPtSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    bool pos = false;
    if (p < HW) {
        const size_t e1 = (size_t)r.b * HW + p;
        pos = a.lab32[(size_t)a.lv.pack_off[r.l] + e1] > 0;
        float g_box[4] = {0.0f, 0.0f, 0.0f, 0.0f}, g_ctr = 0.0f, g_iou = 0.0f;
        if (pos) {
            const float *bp = a.reg[r.l] + (size_t)r.b * 4 * HW + p;
            const float d[4] = {bp[0], bp[(size_t)HW], bp[(size_t)2 * HW], bp[(size_t)3 * HW]};
            const float4 t = reinterpret_cast<const float4 *>(a.bt[r.l])[e1];
            float px, py;
            point_centre(p, W, a.lv.stride[r.l], px, py);
            const PtElem q = point_elem(px, py, d, t);
            const float xc = a.ctr[r.l][e1];
            float xi = 0.0f;
            if constexpr (IOU) xi = a.iou[r.l][e1];
            if (!BWD) point_fwd_terms<IOU>(q, xc, xi, acc);
            else point_bwd_terms<IOU>(q, xc, xi, a.res, a.gin, a.attach, g_box, g_ctr, g_iou);
        }
        if (BWD) {
            float *go = a.g_reg[r.l] + (size_t)r.b * 4 * HW + p;
            go[0] = g_box[0];
            go[(size_t)HW] = g_box[1];
            go[(size_t)2 * HW] = g_box[2];
            go[(size_t)3 * HW] = g_box[3];
            a.g_ctr[r.l][e1] = g_ctr;
            if constexpr (IOU) a.g_iou[r.l][e1] = g_iou;
        }
    }
    if (!BWD) point_block_reduce<kPtSums, IOU ? -1 : 3>(a.sums, acc, pos, red);
}

// ------------------------------------------------------------------ channels-last rows, fp32 / bf16
struct PtBoxNhwcArgs {
    HLLevels lv;
    const void *reg[IA_MAX_LEVELS], *ctr[IA_MAX_LEVELS], *iou[IA_MAX_LEVELS];
    int64_t ps_reg[IA_MAX_LEVELS], ps_ctr[IA_MAX_LEVELS], ps_iou[IA_MAX_LEVELS];   // pixel strides (elements)
    const int64_t *labels[IA_MAX_LEVELS];
    const float *bt[IA_MAX_LEVELS];
    void *g_reg[IA_MAX_LEVELS], *g_ctr[IA_MAX_LEVELS], *g_iou[IA_MAX_LEVELS];
    int64_t pg_reg[IA_MAX_LEVELS], pg_ctr[IA_MAX_LEVELS], pg_iou[IA_MAX_LEVELS];
    // bwd, packed gradient rows: zero-gradient channels behind d(ctr), and behind d(iou) (d(reg) without it)
    int32_t pad_cls[IA_MAX_LEVELS], pad_reg[IA_MAX_LEVELS];
    const float *reg_scale;               // L floats or NULL: reg holds the distances
    double *sums;                         // fwd: as PtBoxArgs
    double *scale_sums;                   // bwd with reg_scale: [L][IA_LOSS_SLOTS]
    const float *res, *gin;
    float *fgin;
    int32_t attach;
};

// k_point_box on pixel rows of T, the reg row optionally raw (d = exp(scale_l x)); every point's gradient
// row is written whole (maps, and the padding the host counted)
template <typename T, bool BWD, bool IOU>
__global__ void __launch_bounds__(256) k_point_box_nhwc(PtBoxNhwcArgs a)
{
    __shared__ double red[kPtSums][4];
    const PtBlock r = locate_point_block(a.lv, blockIdx.x);
    const int W = a.lv.W[r.l], HW = a.lv.H[r.l] * W;
    const int p = r.p0 + threadIdx.x;
    if (BWD && blockIdx.x == 0 && threadIdx.x == 0) a.fgin[3 * a.lv.L] = a.gin[0];
    const bool raw = a.reg_scale != nullptr;              // uniform
    double acc[kPtSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double acc_s[1] = {0.0};
    bool pos = false;
    if (p < HW) {
        const int64_t e1 = (int64_t)r.b * HW + p;
        pos = reinterpret_cast<const int32_t *>(a.labels[r.l])[2 * e1] > 0;      // low word: labels < 2^31
        float g_box[4] = {0.0f, 0.0f, 0.0f, 0.0f}, g_ctr = 0.0f, g_iou = 0.0f;
        if (pos) {
            float x[4], d[4];
            Elems<T, 4>::load(static_cast<const T *>(a.reg[r.l]) + e1 * a.ps_reg[r.l], x);
            const float sc = raw ? a.reg_scale[r.l] : 1.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = raw ? expf_(sc * x[k]) : x[k];
            const float4 t = reinterpret_cast<const float4 *>(a.bt[r.l])[e1];
            float px, py;
            point_centre(p, W, a.lv.stride[r.l], px, py);
            const PtElem q = point_elem(px, py, d, t);
            const float xc = load_f32<T>(static_cast<const T *>(a.ctr[r.l]) + e1 * a.ps_ctr[r.l]);
            float xi = 0.0f;
            if constexpr (IOU) xi = load_f32<T>(static_cast<const T *>(a.iou[r.l]) + e1 * a.ps_iou[r.l]);
            if (!BWD) {
                point_fwd_terms<IOU>(q, xc, xi, acc);
            } else {
                point_bwd_terms<IOU>(q, xc, xi, a.res, a.gin, a.attach, g_box, g_ctr, g_iou);
                if (raw) {
                    // d = exp(scale x): dL/dx = (g d) scale, dL/dscale += (g d) x
                    float ts = 0.0f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float gd = g_box[k] * d[k];
                        ts += gd * x[k];
                        g_box[k] = gd * sc;
                    }
                    acc_s[0] = (double)ts;
                }
            }
        }
        if (BWD) {
            T *gr = static_cast<T *>(a.g_reg[r.l]) + e1 * a.pg_reg[r.l];
            T *gc = static_cast<T *>(a.g_ctr[r.l]) + e1 * a.pg_ctr[r.l];
            Elems<T, 4>::store(gr, g_box);                           // bf16: one round-to-nearest-even each
            store_f32<T>(gc, g_ctr);
            T *tail = gr + 4;                                        // behind d(reg), or behind d(iou)
            if constexpr (IOU) {
                T *gi = static_cast<T *>(a.g_iou[r.l]) + e1 * a.pg_iou[r.l];
                store_f32<T>(gi, g_iou);
                tail = gi + 1;
            }
            for (int k = 0; k < a.pad_cls[r.l]; ++k) gc[1 + k] = (T)0;      // +0 in both storage types
            for (int k = 0; k < a.pad_reg[r.l]; ++k) tail[k] = (T)0;
        }
    }
    if (!BWD) point_block_reduce<kPtSums, IOU ? -1 : 3>(a.sums, acc, pos, red);
    // a block is one level's: its g d x sum into that level's slots
    else if (raw) point_block_reduce<1, -1>(a.scale_sums + (size_t)r.l * IA_LOSS_SLOTS, acc_s, pos, red);
}

// slots -> d scale_l (fp32); a level without positives has nothing but the memset's zeros: exactly 0
__global__ void __launch_bounds__(64) k_point_scale_finalize(const double *scale_sums, int L, float *grad_scale)
{
    const int i = threadIdx.x;
    if (i < L) {
        double s = 0.0;
        for (int k = 0; k < IA_LOSS_SLOTS; ++k) s += scale_sums[(size_t)i * IA_LOSS_SLOTS + k];
        grad_scale[i] = (float)s;
    }
}

// ------------------------------------------------------------------ slots -> losses
struct PtFinArgs {
    const double *sums;                   // [L + kPtSums][IA_LOSS_SLOTS]
    const int32_t *counts;                // (B) or NULL
    int32_t L, B, iou;
    float *res;                           // 6
    float *fgin, *fres;                   // (3L + 4) each: what k_focal_ml<bwd> reads
};

__global__ void __launch_bounds__(64) k_point_finalize(PtFinArgs a)
{
    __shared__ double s_q[IA_MAX_LEVELS + kPtSums];
    const int i = threadIdx.x;
    if (i < a.L + kPtSums) {
        double s = 0.0;
        for (int k = 0; k < IA_LOSS_SLOTS; ++k) s += a.sums[(size_t)i * IA_LOSS_SLOTS + k];
        s_q[i] = s;
    }
    if (i < 3 * a.L + 4) { a.fgin[i] = 0.0f; a.fres[i] = 0.0f; }
    __syncthreads();
    if (i == 0) {
        double cls = 0.0;
        for (int l = 0; l < a.L; ++l) cls += s_q[l];
        const double *q = s_q + a.L;
        double n = q[4];
        if (a.counts) {
            int tot = 0;
            for (int b = 0; b < a.B; ++b) tot += a.counts[b];
            n = (double)tot;
        }
        const bool any = n > 0.0;                 // n = 0: the reference's empty.sum() = 0
        a.res[0] = (float)(cls / (n + (double)a.B));
        a.res[1] = any ? (float)(q[0] / q[1]) : 0.0f;
        a.res[2] = any ? (float)(q[2] / n) : 0.0f;
        a.res[3] = (any && a.iou) ? (float)(q[3] / n) : 0.0f;
        a.res[4] = (float)n;
        a.res[5] = (float)q[1];
        a.fres[3 * a.L + 3] = (float)(n + (double)a.B);
    }
}

// the workspaces of the two nodes: fp64 slots [L + kPtSums] | the focal kernel's two (3L + 4) vectors, then
// NCHW: the packed labels | their weights; channels-last: fp64 slots [L] of d scale
struct PtWorkspace {
    double *sums;
    float *fgin, *fres;
    int32_t *lab32; float *w32;           // NCHW node
    double *scale_sums;                   // channels-last node
    size_t bytes;
};

static Carver carve_point_head(int L, void *workspace, PtWorkspace &r)
{
    Carver c(workspace);
    r.lab32 = nullptr; r.w32 = nullptr; r.scale_sums = nullptr;
    c.take(r.sums, sizeof(double) * (L + kPtSums) * IA_LOSS_SLOTS);
    c.take(r.fgin, sizeof(float) * 2 * (3 * L + 4));
    r.fres = r.fgin ? r.fgin + (3 * L + 4) : nullptr;
    return c;
}

static PtWorkspace carve_point(const HLLevels &lv, void *workspace)
{
    PtWorkspace r;
    Carver c = carve_point_head(lv.L, workspace, r);
    c.take(r.lab32, packed_pad(lv) * 4);
    c.take(r.w32, packed_pad(lv) * 4);
    r.bytes = c.bytes;
    return r;
}

static PtWorkspace carve_point_nhwc(int L, void *workspace)
{
    PtWorkspace r;
    Carver c = carve_point_head(L, workspace, r);
    c.take(r.scale_sums, sizeof(double) * L * IA_LOSS_SLOTS);
    r.bytes = c.bytes;
    return r;
}

// the tail of the two forward entries: clear the slots before the first kernel, reduce them after the last
static int clear_point_slots(double *sums, int L, hipStream_t s)
{
    return hip_status(hipMemsetAsync(sums, 0, sizeof(double) * (size_t)(L + kPtSums) * IA_LOSS_SLOTS, s));
}

static int launch_point_finalize(const double *sums, const ia_point_targets *t, int L, int batch, bool with_iou,
                                 float *result, float *fgin, float *fres, hipStream_t s)
{
    PtFinArgs f;
    f.sums = sums; f.counts = t->counts; f.L = L; f.B = batch; f.iou = with_iou ? 1 : 0;
    f.res = result; f.fgin = fgin; f.fres = fres;
    hipLaunchKernelGGL(k_point_finalize, dim3(1), dim3(64), 0, s, f);
    return hip_status(hipGetLastError());
}

static int launch_point_box(bool bwd, bool with_iou, const PtBoxArgs &ba, hipStream_t s)
{
    static void (*const k[2][2])(PtBoxArgs) = {{k_point_box<false, false>, k_point_box<false, true>},
                                               {k_point_box<true, false>, k_point_box<true, true>}};
    hipLaunchKernelGGL(k[bwd][with_iou], dim3((unsigned)ba.lv.blk_off[ba.lv.L]), dim3(256), 0, s, ba);
    return hip_status(hipGetLastError());
}

// what forward and backward check alike; fills the focal and box arguments except the outputs
static int point_loss_args(const ia_point_head_geom *g, const ia_point_level_ptrs *p, int batch,
                           const ia_point_targets *t, const ia_point_loss_cfg *cfg, void *workspace,
                           FocalMLArgs &fa, PtBoxArgs &ba, PtWorkspace &ws, bool &with_iou)
{
    if (!p || !t || !cfg || !workspace || ((uintptr_t)workspace & 255u)) return IA_E_ARG;
    int rc = point_levels(g, batch, fa.lv);
    if (rc) return rc;
    if (cfg->gamma != 2.0f) return IA_E_ARG;
    const int L = fa.lv.L;
    with_iou = p->iou[0] != nullptr;
    ws = carve_point(fa.lv, workspace);
    if (t->packed) {
        if ((uintptr_t)t->packed & 15u) return IA_E_ARG;
        ws.lab32 = const_cast<int32_t *>(t->packed);
        ws.w32 = reinterpret_cast<float *>(ws.lab32 + packed_pad(fa.lv));
    }
    ba.lv = fa.lv;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        const bool on = l < L;
        if (on && (!p->cls[l] || !p->reg[l] || !p->ctr[l] || !t->labels[l] || !t->bbox_targets[l]))
            return IA_E_ARG;
        if (on && ((p->iou[l] != nullptr) != with_iou)) return IA_E_ARG;
        if (on && ((uintptr_t)t->bbox_targets[l] & 15u)) return IA_E_ARG;
        if (on && ((uintptr_t)p->cls[l] & 15u)) return IA_E_ARG;                // 16-byte class loads
        fa.cls[l] = on ? p->cls[l] : nullptr;
        fa.grad[l] = nullptr;
        ba.reg[l] = on ? static_cast<const float *>(p->reg[l]) : nullptr;
        ba.ctr[l] = on ? static_cast<const float *>(p->ctr[l]) : nullptr;
        ba.iou[l] = on ? static_cast<const float *>(p->iou[l]) : nullptr;
        ba.bt[l] = on ? t->bbox_targets[l] : nullptr;
        ba.g_reg[l] = ba.g_ctr[l] = ba.g_iou[l] = nullptr;
    }
    fa.lab_am = ws.lab32; fa.w_am = ws.w32;
    fa.tail = focal_tail(cfg->alpha, 1.0f, false, nullptr, nullptr, nullptr);
    ba.lab32 = ws.lab32;
    ba.sums = nullptr; ba.res = ba.gin = nullptr; ba.fgin = nullptr;
    ba.attach = cfg->attach_iou_target ? 1 : 0;
    return 0;
}

// ------------------------------------------------------------------ channels-last rows: host
static int point_levels_nhwc(const ia_point_head_geom *g, int batch, HLLevels &lv, NhwcLevels &nl)
{
    ia_head_geom hg;
    int rc = point_levels(g, batch, lv, false, &hg);
    if (rc) return rc;
    return fill_levels_nhwc(&hg, batch, nl);                // C % 4 == 0: class quads
}

// one set of maps (head outputs, or gradients): pointers, strides and the alignment of the vector pieces
static int point_rows_ok(int L, int C, int esize, const ia_point_level_ptrs *p, const ia_point_pix_strides *st,
                         bool with_iou)
{
    const uintptr_t amask = (uintptr_t)(4 * esize - 1);     // 16 bytes fp32, 8 bytes bf16
    for (int l = 0; l < L; ++l) {
        if (!p->cls[l] || !p->reg[l] || !p->ctr[l] || ((p->iou[l] != nullptr) != with_iou)) return IA_E_ARG;
        if (st->cls[l] < C || st->reg[l] < 4 || st->ctr[l] < 1 || (with_iou && st->iou[l] < 1)) return IA_E_ARG;
        if ((st->cls[l] & 3) || (st->reg[l] & 3)) return IA_E_ARG;
        if (((uintptr_t)p->cls[l] & amask) || ((uintptr_t)p->reg[l] & amask)) return IA_E_ARG;
        const uintptr_t emask = (uintptr_t)(esize - 1);
        if (((uintptr_t)p->ctr[l] & emask) || (with_iou && ((uintptr_t)p->iou[l] & emask))) return IA_E_ARG;
    }
    return 0;
}

// what forward and backward check alike (backward = forward + gradient maps); no launch before it returns 0
static int point_nhwc_args(const ia_point_head_geom *g, const ia_point_level_ptrs *p,
                           const ia_point_pix_strides *strides, int dtype, int batch, const ia_point_targets *t,
                           const ia_point_loss_cfg *cfg, const float *reg_scale, void *workspace,
                           size_t workspace_bytes, bool bwd, const ia_point_level_ptrs *grads,
                           const ia_point_pix_strides *grad_strides, int grad_rows_packed,
                           FocalNhwcArgs &fa, PtBoxNhwcArgs &ba, PtWorkspace &ws, bool &with_iou)
{
    if (!p || !strides || !t || !cfg || !workspace || ((uintptr_t)workspace & 255u)) return IA_E_ARG;
    if (dtype != IA_F32 && dtype != IA_BF16) return IA_E_ARG;
    if (bwd && (!grads || !grad_strides)) return IA_E_ARG;
    int rc = point_levels_nhwc(g, batch, ba.lv, fa.lv);
    if (rc) return rc;
    if (cfg->gamma != 2.0f) return IA_E_ARG;
    const int L = ba.lv.L, C = ba.lv.C, esize = dtype == IA_BF16 ? 2 : 4;
    with_iou = p->iou[0] != nullptr;
    if ((rc = point_rows_ok(L, C, esize, p, strides, with_iou))) return rc;
    if (bwd && (rc = point_rows_ok(L, C, esize, grads, grad_strides, with_iou))) return rc;
    ws = carve_point_nhwc(L, workspace);
    if (workspace_bytes < ws.bytes) return IA_E_WORKSPACE;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        const bool on = l < L, gon = on && bwd;
        if (on && (!t->labels[l] || !t->bbox_targets[l] || ((uintptr_t)t->bbox_targets[l] & 15u))) return IA_E_ARG;
        fa.cls[l] = on ? p->cls[l] : nullptr;
        fa.ps_cls[l] = on ? strides->cls[l] : 0;
        fa.labels[l] = on ? t->labels[l] : nullptr;
        fa.lw[l] = nullptr;                                  // unit weights: never read
        fa.grad[l] = gon ? const_cast<void *>(grads->cls[l]) : nullptr;
        fa.ps_grad[l] = gon ? grad_strides->cls[l] : 0;
        ba.reg[l] = on ? p->reg[l] : nullptr; ba.ctr[l] = on ? p->ctr[l] : nullptr;
        ba.iou[l] = (on && with_iou) ? p->iou[l] : nullptr;
        ba.ps_reg[l] = on ? strides->reg[l] : 0; ba.ps_ctr[l] = on ? strides->ctr[l] : 0;
        ba.ps_iou[l] = (on && with_iou) ? strides->iou[l] : 0;
        ba.labels[l] = on ? t->labels[l] : nullptr;
        ba.bt[l] = on ? t->bbox_targets[l] : nullptr;
        ba.g_reg[l] = gon ? const_cast<void *>(grads->reg[l]) : nullptr;
        ba.g_ctr[l] = gon ? const_cast<void *>(grads->ctr[l]) : nullptr;
        ba.g_iou[l] = (gon && with_iou) ? const_cast<void *>(grads->iou[l]) : nullptr;
        ba.pg_reg[l] = gon ? grad_strides->reg[l] : 0; ba.pg_ctr[l] = gon ? grad_strides->ctr[l] : 0;
        ba.pg_iou[l] = (gon && with_iou) ? grad_strides->iou[l] : 0;
        ba.pad_cls[l] = ba.pad_reg[l] = 0;
        if (gon && grad_rows_packed) {
            // the caller states rows [cls C | ctr | pad] and [reg 4 | iou? | pad]: the channels left up to
            // each row's end get their zero gradient in the box kernel
            const char *gc = static_cast<const char *>(grads->cls[l]), *gr = static_cast<const char *>(grads->reg[l]);
            if (static_cast<const char *>(grads->ctr[l]) != gc + (size_t)C * esize ||
                grad_strides->ctr[l] != grad_strides->cls[l] || grad_strides->cls[l] < C + 1)
                return IA_E_ARG;
            const int nreg = with_iou ? 5 : 4;
            if (with_iou && (static_cast<const char *>(grads->iou[l]) != gr + (size_t)4 * esize ||
                             grad_strides->iou[l] != grad_strides->reg[l]))
                return IA_E_ARG;
            if (grad_strides->reg[l] < nreg || grad_strides->cls[l] - (C + 1) > 1024 ||
                grad_strides->reg[l] - nreg > 1024)
                return IA_E_ARG;
            ba.pad_cls[l] = (int32_t)(grad_strides->cls[l] - (C + 1));
            ba.pad_reg[l] = (int32_t)(grad_strides->reg[l] - nreg);
        }
    }
    fa.tail = focal_tail(cfg->alpha, 1.0f, false, nullptr, nullptr, nullptr);
    ba.reg_scale = reg_scale;
    ba.sums = nullptr; ba.scale_sums = ws.scale_sums;
    ba.res = ba.gin = nullptr; ba.fgin = nullptr;
    ba.attach = cfg->attach_iou_target ? 1 : 0;
    return 0;
}

static int launch_point_box_nhwc(int dtype, bool bwd, bool with_iou, const PtBoxNhwcArgs &ba, hipStream_t s)
{
    static void (*const k[2][2][2])(PtBoxNhwcArgs) = {
        {{k_point_box_nhwc<float, false, false>, k_point_box_nhwc<float, false, true>},
         {k_point_box_nhwc<float, true, false>, k_point_box_nhwc<float, true, true>}},
        {{k_point_box_nhwc<uint16_t, false, false>, k_point_box_nhwc<uint16_t, false, true>},
         {k_point_box_nhwc<uint16_t, true, false>, k_point_box_nhwc<uint16_t, true, true>}}};
    hipLaunchKernelGGL(k[dtype == IA_BF16][bwd][with_iou], dim3((unsigned)ba.lv.blk_off[ba.lv.L]), dim3(256), 0, s, ba);
    return hip_status(hipGetLastError());
}

}  // namespace ia

extern "C" {

size_t ia_point_packed_labels_elems(const ia_point_head_geom *g, int batch)
{
    ia::HLLevels lv;
    if (ia::point_levels(g, batch, lv)) return 0;
    return 2 * ia::packed_pad(lv);
}

int ia_point_targets_ptrs(const ia_point_head_geom *g, const float *const *gt_boxes,
                          const int64_t *const *gt_labels, const int32_t *num_gt, int batch,
                          const float *regress_ranges, int64_t *labels, float *bbox_targets,
                          int32_t *packed, int32_t *counts, void *stream)
{
    using namespace ia;
    if (!g || !gt_boxes || !gt_labels || !num_gt || !regress_ranges || !labels || !bbox_targets ||
        !counts || batch < 1 || batch > IA_MAX_TARGET_BATCH)
        return IA_E_ARG;
    if (((uintptr_t)bbox_targets & 15u) || ((uintptr_t)packed & 15u)) return IA_E_ARG;
    PtTargetArgs a;
    memset(&a, 0, sizeof(a));
    int rc = point_levels(g, batch, a.lv);
    if (rc) return rc;
    for (int b = 0; b < batch; ++b) {
        if (!gt_boxes[b] || !gt_labels[b] || num_gt[b] < 1 || num_gt[b] > kPtMaxGt) return IA_E_ARG;
        if (((uintptr_t)gt_boxes[b]) & 15u) return IA_E_ARG;          // float4 loads
        a.gt_ptr[b] = gt_boxes[b];
        a.gl_ptr[b] = gt_labels[b];
        a.num_gt[b] = (int16_t)num_gt[b];
    }
    for (int l = 0; l < a.lv.L; ++l) {
        a.lo[l] = regress_ranges[2 * l]; a.hi[l] = regress_ranges[2 * l + 1];
        if (!(a.lo[l] <= a.hi[l])) return IA_E_ARG;
    }
    a.labels = labels; a.bbox_targets = bbox_targets; a.counts = counts;
    a.lab32 = packed;
    a.w32 = packed ? reinterpret_cast<float *>(packed + packed_pad(a.lv)) : nullptr;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)batch, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_point_targets, dim3((unsigned)a.lv.blk_off[a.lv.L]), dim3(256), 0, s, a);
    return hip_status(hipGetLastError());
}

size_t ia_point_head_loss_workspace_bytes(const ia_point_head_geom *g, int batch)
{
    ia::HLLevels lv;
    if (ia::point_levels(g, batch, lv)) return 0;
    return ia::carve_point(lv, nullptr).bytes;
}

int ia_point_head_loss_fwd(const ia_point_head_geom *g, const ia_point_level_ptrs *p, int batch,
                           const ia_point_targets *t, const ia_point_loss_cfg *cfg,
                           void *workspace, size_t workspace_bytes, float *result, void *stream)
{
    using namespace ia;
    if (!result) return IA_E_ARG;
    FocalMLArgs fa;
    PtBoxArgs ba;
    PtWorkspace ws;
    bool with_iou;
    int rc = point_loss_args(g, p, batch, t, cfg, workspace, fa, ba, ws, with_iou);
    if (rc) return rc;
    if (workspace_bytes < ws.bytes) return IA_E_WORKSPACE;
    const int L = fa.lv.L;
    fa.tail.sums = ws.sums;
    fa.tail.big_logits = cfg->exact_large_logits ? 1 : 0;
    ba.sums = ws.sums + (size_t)L * IA_LOSS_SLOTS;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = clear_point_slots(ws.sums, L, s))) return rc;
    if (!t->packed) {
        PtPackArgs pa;
        pa.lv = fa.lv;
        for (int l = 0; l < IA_MAX_LEVELS; ++l) pa.labels[l] = l < L ? t->labels[l] : nullptr;
        pa.lab32 = ws.lab32; pa.w32 = ws.w32;
        hipLaunchKernelGGL(k_point_pack, dim3((unsigned)((fa.lv.pack_off[L] + 255) / 256)), dim3(256), 0, s, pa);
    }
    if ((rc = launch_focal_ml_f32(fa, false, s))) return rc;
    if ((rc = launch_point_box(false, with_iou, ba, s))) return rc;
    return launch_point_finalize(ws.sums, t, L, batch, with_iou, result, ws.fgin, ws.fres, s);
}

int ia_point_head_loss_bwd(const ia_point_head_geom *g, const ia_point_level_ptrs *p, int batch,
                           const ia_point_targets *t, const ia_point_loss_cfg *cfg,
                           void *workspace, const float *result, const float *grad_result,
                           const ia_point_level_ptrs *grads, void *stream)
{
    using namespace ia;
    if (!result || !grad_result || !grads) return IA_E_ARG;
    FocalMLArgs fa;
    PtBoxArgs ba;
    PtWorkspace ws;
    bool with_iou;
    int rc = point_loss_args(g, p, batch, t, cfg, workspace, fa, ba, ws, with_iou);
    if (rc) return rc;
    const int L = fa.lv.L;
    for (int l = 0; l < L; ++l) {
        if (!grads->cls[l] || !grads->reg[l] || !grads->ctr[l]) return IA_E_ARG;
        if ((grads->iou[l] != nullptr) != with_iou) return IA_E_ARG;
        if ((uintptr_t)grads->cls[l] & 15u) return IA_E_ARG;
        fa.grad[l] = (float *)grads->cls[l];
        ba.g_reg[l] = (float *)grads->reg[l];
        ba.g_ctr[l] = (float *)grads->ctr[l];
        ba.g_iou[l] = (float *)grads->iou[l];
    }
    fa.tail.gin = ws.fgin; fa.tail.res = ws.fres;
    ba.res = result; ba.gin = grad_result; ba.fgin = ws.fgin;
    hipStream_t s = (hipStream_t)stream;
    // the box kernel first: it hands the upstream gradient of loss_cls to the focal kernel
    if ((rc = launch_point_box(true, with_iou, ba, s))) return rc;
    return launch_focal_ml_f32(fa, true, s);
}

size_t ia_point_head_loss_nhwc_workspace_bytes(const ia_point_head_geom *g, int batch)
{
    ia::HLLevels lv;
    ia::NhwcLevels nl;
    if (ia::point_levels_nhwc(g, batch, lv, nl)) return 0;
    return ia::carve_point_nhwc(lv.L, nullptr).bytes;
}

int ia_point_head_loss_fwd_nhwc(const ia_point_head_geom *g, const ia_point_level_ptrs *p,
                                const ia_point_pix_strides *strides, int dtype, int batch,
                                const ia_point_targets *t, const ia_point_loss_cfg *cfg,
                                const float *reg_scale, void *workspace, size_t workspace_bytes,
                                float *result, void *stream)
{
    using namespace ia;
    if (!result) return IA_E_ARG;
    FocalNhwcArgs fa;
    PtBoxNhwcArgs ba;
    PtWorkspace ws;
    bool with_iou;
    int rc = point_nhwc_args(g, p, strides, dtype, batch, t, cfg, reg_scale, workspace, workspace_bytes, false,
                             nullptr, nullptr, 0, fa, ba, ws, with_iou);
    if (rc) return rc;
    const int L = ba.lv.L;
    fa.tail.sums = ws.sums;
    fa.tail.big_logits = cfg->exact_large_logits ? 1 : 0;
    ba.sums = ws.sums + (size_t)L * IA_LOSS_SLOTS;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = clear_point_slots(ws.sums, L, s))) return rc;
    if ((rc = launch_focal_nhwc_unit(fa, dtype, false, s))) return rc;
    if ((rc = launch_point_box_nhwc(dtype, false, with_iou, ba, s))) return rc;
    return launch_point_finalize(ws.sums, t, L, batch, with_iou, result, ws.fgin, ws.fres, s);
}

int ia_point_head_loss_bwd_nhwc(const ia_point_head_geom *g, const ia_point_level_ptrs *p,
                                const ia_point_pix_strides *strides, int dtype, int batch,
                                const ia_point_targets *t, const ia_point_loss_cfg *cfg,
                                const float *reg_scale, void *workspace, size_t workspace_bytes,
                                const float *result, const float *grad_result,
                                const ia_point_level_ptrs *grads, const ia_point_pix_strides *grad_strides,
                                int grad_rows_packed, float *grad_scale, void *stream)
{
    using namespace ia;
    if (!result || !grad_result) return IA_E_ARG;
    if ((reg_scale != nullptr) != (grad_scale != nullptr)) return IA_E_ARG;
    FocalNhwcArgs fa;
    PtBoxNhwcArgs ba;
    PtWorkspace ws;
    bool with_iou;
    int rc = point_nhwc_args(g, p, strides, dtype, batch, t, cfg, reg_scale, workspace, workspace_bytes, true,
                             grads, grad_strides, grad_rows_packed, fa, ba, ws, with_iou);
    if (rc) return rc;
    const int L = ba.lv.L;
    fa.tail.gin = ws.fgin; fa.tail.res = ws.fres;
    ba.res = result; ba.gin = grad_result; ba.fgin = ws.fgin;
    hipStream_t s = (hipStream_t)stream;
    if (reg_scale) {
        hipError_t e = hipMemsetAsync(ws.scale_sums, 0, sizeof(double) * (size_t)L * IA_LOSS_SLOTS, s);
        if (e != hipSuccess) return (int)e;
    }
    // the box kernel first: it hands the upstream gradient of loss_cls to the focal kernel
    if ((rc = launch_point_box_nhwc(dtype, true, with_iou, ba, s))) return rc;
    if ((rc = launch_focal_nhwc_unit(fa, dtype, true, s))) return rc;
    if (reg_scale) {
        hipLaunchKernelGGL(k_point_scale_finalize, dim3(1), dim3(64), 0, s, ws.scale_sums, L, grad_scale);
        return hip_status(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
