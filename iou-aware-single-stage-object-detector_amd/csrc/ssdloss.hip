// Training loss of SSDHead (reference mmdet/models/anchor_heads/ssd_head.py, loss / loss_single with
// its IoU_balanced_* switches off): per image the softmax cross-entropy of every anchor row, hard
// negative mining (the neg_pos_ratio * num_pos largest losses among the rows with label 0), and
// smooth-L1 on the box deltas.  fp32 NCHW head outputs consumed in place, rows numbered as in
// ssddecode.hip (level, then (y, x), then anchor); targets image-major: labels (B, R) int64 in 0..C,
// label_weights (B, R), bbox_targets / bbox_weights (B, R, 4).
//
//   k_ssdloss_rows   one lane per (image, level, anchor, pixel), lanes along the pixels of a channel
//                    plane (the access pattern of k_ssd_rowscore): softmax_row_stats -> lse = m + log(s),
//                    ce = (lse - x[label]) * label_weight; ce and lse (B, R).  The same lane forms
//                    sum_k bbox_weight_k * smoothl1(pred_k - target_k); the workgroup adds its rows in
//                    fp64 (wave tree, then the waves in order) into one partial of its own.
//   k_ssd_mine       one workgroup of 1024 lanes per image: num_pos, num_neg, k = min(ratio * num_pos,
//                    num_neg); the k-th largest negative ce through a radix select on ordered_key
//                    (8-bit digits from the top, four passes); keys in LDS when R <= kSsdMineLdsRows,
//                    formed again from ce / labels in global memory otherwise.  A negative is selected
//                    when its key is above the threshold key t, or equal to it and among the first
//                    k - #(key > t) such rows in ascending row order (ballots + a running carry: the tie
//                    rule).  sel (B, R) uint8 (positives 1), counts (B, 2) = (num_pos, k), losses (B, 2)
//                    = (sum_pos ce + sum_selected ce) / avg_factor, sum box / avg_factor: fp64 sums in
//                    a fixed order, rounded once.
//   k_ssdloss_bwd    the lanes of k_ssdloss_rows: the C + 1 class gradients g_cls[b] / avg_factor *
//                    label_weight * (exp(x - lse) - [c == label]) of a selected row (as exp(x - m) / s on
//                    the row's statistics, formed again), +0.0 of any other, and the four smooth-L1
//                    derivatives: every element of every gradient map is written exactly once, so the
//                    maps need no memset.
//
// No floating-point atomics and no atomics on global memory: the only atomic operations are the
// integer digit counters of the radix select in LDS, whose sums do not depend on the order.  Every
// run gives the same bits.
#include "ia_internal.hpp"
#include "ia_math.hpp"
#include "ia_ssd.hpp"
#include "ia_softmax_dev.hpp"
#include "ia_compact_dev.hpp"
#include "ia_loss.hpp"

namespace ia {

constexpr int kSsdMineBlock = 1024;          // lanes of k_ssd_mine (16 wavefronts)
constexpr int kSsdMineLdsRows = 12288;       // keys kept in LDS up to this many rows (48 KiB)

struct SsdTargets {
    const int64_t *labels;                   // (B, R)
    const float *label_weights;              // (B, R)
    const float *bbox_targets, *bbox_weights;// (B, R, 4)
};

__device__ __forceinline__ float ssd_avg(const float *dev, float host) { return dev ? dev[0] : host; }

// sum over the workgroup, the same value in every lane: wave tree, then the waves in order.
// lds: one double per wavefront; may be used again right after the call.
__device__ __forceinline__ double block_sum_all(double v, double *lds)
{
    const int tid = threadIdx.x, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    if ((tid & 63) == 0) lds[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < nw; ++w) s += lds[w];
    __syncthreads();
    return s;
}

__device__ __forceinline__ int block_sum_all_int(int v, int *lds)
{
    const int tid = threadIdx.x, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((tid & 63) == 0) lds[tid >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < nw; ++w) s += lds[w];
    __syncthreads();
    return s;
}

// ------------------------------------------------------------------ stage 1: rows
struct SsdLossRowArgs {
    SsdTable t;
    SsdTargets tg;
    float beta;
    float *ce, *lse;                         // (B, R)
    double *partials;                        // (B, num_levels * gridDim.x) or NULL
};

__global__ void __launch_bounds__(256) k_ssdloss_rows(SsdLossRowArgs a)
{
    __shared__ double s_part[4];
    const int l = (int)blockIdx.y % a.t.num_levels, b = (int)blockIdx.y / a.t.num_levels;
    const int A = a.t.A[l], Cin = a.t.C + 1, HW = a.t.H[l] * a.t.W[l];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (anchor, pixel): pixels along the lanes
    double box = 0.0;
    if (i < (int64_t)HW * A) {
        const int an = (int)(i / HW), pos = (int)(i - (int64_t)an * HW);
        const int R = a.t.row_off[a.t.num_levels];
        const size_t row = (size_t)b * R + a.t.row_off[l] + (size_t)pos * A + an;
        const float *cls = a.t.cls[l] + ((size_t)b * A + an) * Cin * HW + pos;
        float m, s, e;
        softmax_row_stats<float>(cls, (size_t)HW, Cin, m, s, e);
        const float lse = m + logf_(s);
        const int64_t lab = a.tg.labels[row];
        // a label outside 0..C reads nothing and poisons the row
        const float xl = (lab >= 0 && lab < Cin) ? cls[(size_t)lab * HW] : __builtin_nanf("");
        a.ce[row] = (lse - xl) * a.tg.label_weights[row];
        a.lse[row] = lse;
        const float *reg = a.t.reg[l] + ((size_t)b * A + an) * 4 * HW + pos;
        const float4 bt = reinterpret_cast<const float4 *>(a.tg.bbox_targets)[row];
        const float4 bw = reinterpret_cast<const float4 *>(a.tg.bbox_weights)[row];
        box = (double)(smooth_l1_val(reg[0] - bt.x, a.beta) * bw.x);
        box += (double)(smooth_l1_val(reg[(size_t)HW] - bt.y, a.beta) * bw.y);
        box += (double)(smooth_l1_val(reg[(size_t)2 * HW] - bt.z, a.beta) * bw.z);
        box += (double)(smooth_l1_val(reg[(size_t)3 * HW] - bt.w, a.beta) * bw.w);
    }
    if (a.partials) {                        // uniform: every lane of the workgroup takes part
        const double sum = block_sum_all(box, s_part);
        if (threadIdx.x == 0)
            a.partials[((size_t)b * a.t.num_levels + l) * gridDim.x + blockIdx.x] = sum;
    }
}

static int check_targets(const SsdTargets &tg)
{
    if (!tg.labels || !tg.label_weights || !tg.bbox_targets || !tg.bbox_weights) return IA_E_ARG;
    if (((uintptr_t)tg.bbox_targets & 15u) || ((uintptr_t)tg.bbox_weights & 15u)) return IA_E_ARG;
    if ((uintptr_t)tg.labels & 7u) return IA_E_ARG;
    return 0;
}

static int check_rows_batch(const SsdTable &t, int batch)
{
    if (batch < 1 || (int64_t)batch * t.num_levels > 65535) return IA_E_ARG;
    return 0;
}

static int launch_ssdloss_rows(const SsdTable &t, int batch, const SsdTargets &tg, float beta, float *ce, float *lse,
                               double *partials, hipStream_t s)
{
    int rc;
    if (!ce || !lse || !(beta > 0.0f)) return IA_E_ARG;
    if ((rc = check_targets(tg)) || (rc = check_rows_batch(t, batch))) return rc;
    if (((uintptr_t)partials & 7u) != 0) return IA_E_ARG;
    SsdLossRowArgs a;
    a.t = t; a.tg = tg; a.beta = beta; a.ce = ce; a.lse = lse; a.partials = partials;
    const dim3 grid((unsigned)ssd_row_grid_x(t), (unsigned)(batch * t.num_levels));
    hipLaunchKernelGGL(k_ssdloss_rows, grid, dim3(256), 0, s, a);
    return hip_status(hipGetLastError());
}

// ------------------------------------------------------------------ stage 2: mining
// key of a row in the selection: 0 for a row that is no negative, else the order-preserving key of
// its ce (>= 1; -0.0 counts as +0.0)
__device__ __forceinline__ uint32_t mine_key(int64_t label, float ce)
{
    if (label != 0) return 0u;
    const uint32_t k = ordered_key(ce + 0.0f);
    return k ? k : 1u;
}

struct SsdMineArgs {
    const float *ce;                         // (B, R)
    const int64_t *labels;                   // (B, R)
    int32_t R, neg_pos_ratio, nparts;
    const double *partials;                  // (B, nparts) or NULL
    const float *avg_dev;
    float avg;
    uint8_t *sel;                            // (B, R)
    int32_t *counts;                         // (B, 2)
    float *losses;                           // (B, 2)
};

template <bool kLds>
__global__ void __launch_bounds__(kSsdMineBlock) k_ssd_mine(SsdMineArgs a)
{
    __shared__ uint32_t s_keys[kLds ? kSsdMineLdsRows : 1];
    __shared__ int s_hist[256], s_scan[256];
    __shared__ int s_wave[kSsdMineBlock / 64];
    __shared__ double s_dsum[kSsdMineBlock / 64];
    __shared__ int s_digit, s_rem;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t R = a.R;
    const float *ce = a.ce + (size_t)b * R;
    const int64_t *labels = a.labels + (size_t)b * R;

    // counts (and the keys into LDS)
    int npos = 0, nneg = 0;
    for (int64_t r = tid; r < R; r += kSsdMineBlock) {
        const int64_t lab = labels[r];
        npos += lab > 0 ? 1 : 0;
        nneg += lab == 0 ? 1 : 0;
        if (kLds) s_keys[r] = mine_key(lab, ce[r]);
    }
    npos = block_sum_all_int(npos, s_wave);
    nneg = block_sum_all_int(nneg, s_wave);
    const int64_t want = (int64_t)a.neg_pos_ratio * npos;
    const int k = (int)(want < nneg ? want : nneg);

    // radix select: after the four passes `prefix` is the k-th largest key, `rem` the number of rows
    // with that key to take
    uint32_t prefix = 0xffffffffu;
    int rem = 0;
    if (k > 0) {                             // uniform
        prefix = 0u; rem = k;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const uint32_t mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            for (int64_t r = tid; r < R; r += kSsdMineBlock) {
                const uint32_t key = kLds ? s_keys[r] : mine_key(labels[r], ce[r]);
                if (key != 0u && (key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
            }
            __syncthreads();
            // s_scan[t] = number of keys with digit >= 255 - t (Hillis-Steele over 256 lanes)
            if (tid < 256) s_scan[tid] = s_hist[255 - tid];
            __syncthreads();
            for (int o = 1; o < 256; o <<= 1) {
                const int add = (tid < 256 && tid >= o) ? s_scan[tid - o] : 0;
                __syncthreads();
                if (tid < 256) s_scan[tid] += add;
                __syncthreads();
            }
            if (tid < 256) {
                const int incl = s_scan[tid], excl = incl - s_hist[255 - tid];
                if (excl < rem && rem <= incl) { s_digit = 255 - tid; s_rem = rem - excl; }
            }
            __syncthreads();
            prefix |= (uint32_t)s_digit << shift;
            rem = s_rem;
            __syncthreads();
        }
    }

    // selection in ascending row order, and the classification sum
    double acc = 0.0;
    int carry = 0;                           // rows with the threshold key in the chunks before this one
    for (int64_t base = 0; base < R; base += kSsdMineBlock) {
        const int64_t r = base + tid;
        const bool in = r < R;
        const int64_t lab = in ? labels[r] : -1;
        const float v = in ? ce[r] : 0.0f;
        const uint32_t key = in ? mine_key(lab, v) : 0u;
        const bool eq = key != 0u && key == prefix;
        const int rank = carry + block_keep_rank(eq, s_wave);
        int total = 0;
        for (int w = 0; w < kSsdMineBlock / 64; ++w) total += s_wave[w];
        carry += total;
        const bool take = lab > 0 || (key != 0u && key > prefix) || (eq && rank < rem);
        if (in) a.sel[(size_t)b * R + r] = take ? 1 : 0;
        if (take) acc += (double)v;
        __syncthreads();                     // s_wave is written again in the next chunk
    }
    const double cls_sum = block_sum_all(acc, s_dsum);
    double box = 0.0;
    if (a.partials)
        for (int i = tid; i < a.nparts; i += kSsdMineBlock) box += a.partials[(size_t)b * a.nparts + i];
    const double box_sum = block_sum_all(box, s_dsum);
    if (tid == 0) {
        const double avg = (double)ssd_avg(a.avg_dev, a.avg);
        a.counts[2 * b] = npos; a.counts[2 * b + 1] = k;
        a.losses[2 * b] = (float)(cls_sum / avg);
        a.losses[2 * b + 1] = (float)(box_sum / avg);
    }
}

static int launch_ssd_mine(const float *ce, const int64_t *labels, int batch, int R, int neg_pos_ratio,
                           const double *partials, int nparts, const float *avg_dev, float avg, uint8_t *sel,
                           int32_t *counts, float *losses, hipStream_t s)
{
    if (!ce || !labels || !sel || !counts || !losses) return IA_E_ARG;
    if (batch < 1 || batch > 65535 || R < 1 || neg_pos_ratio < 0 || nparts < 0) return IA_E_ARG;
    if (!avg_dev && !(avg > 0.0f)) return IA_E_ARG;
    if (((uintptr_t)labels & 7u) || ((uintptr_t)partials & 7u)) return IA_E_ARG;
    SsdMineArgs a;
    a.ce = ce; a.labels = labels; a.R = R; a.neg_pos_ratio = neg_pos_ratio;
    a.nparts = partials ? nparts : 0; a.partials = partials;
    a.avg_dev = avg_dev; a.avg = avg; a.sel = sel; a.counts = counts; a.losses = losses;
    if (R <= kSsdMineLdsRows)
        hipLaunchKernelGGL(k_ssd_mine<true>, dim3((unsigned)batch), dim3(kSsdMineBlock), 0, s, a);
    else
        hipLaunchKernelGGL(k_ssd_mine<false>, dim3((unsigned)batch), dim3(kSsdMineBlock), 0, s, a);
    return hip_status(hipGetLastError());
}

// ------------------------------------------------------------------ backward
struct SsdLossBwdArgs {
    SsdTable t;
    SsdTargets tg;
    float beta;
    const uint8_t *sel;                      // (B, R)
    const float *grad_losses;                // (B, 2): upstream gradients of loss_cls[b], loss_bbox[b]
    const float *avg_dev;
    float avg;
    float *gcls[IA_MAX_LEVELS], *greg[IA_MAX_LEVELS];
};

__global__ void __launch_bounds__(256) k_ssdloss_bwd(SsdLossBwdArgs a)
{
    const int l = (int)blockIdx.y % a.t.num_levels, b = (int)blockIdx.y / a.t.num_levels;
    const int A = a.t.A[l], Cin = a.t.C + 1, HW = a.t.H[l] * a.t.W[l];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)HW * A) return;
    const int an = (int)(i / HW), pos = (int)(i - (int64_t)an * HW);
    const int R = a.t.row_off[a.t.num_levels];
    const size_t row = (size_t)b * R + a.t.row_off[l] + (size_t)pos * A + an;
    const float avg = ssd_avg(a.avg_dev, a.avg);
    const size_t coff = ((size_t)b * A + an) * Cin * HW + pos;
    const float *cls = a.t.cls[l] + coff;
    float *gc = a.gcls[l] + coff;
    if (a.sel[row]) {
        const float g = (a.grad_losses[2 * b] / avg) * a.tg.label_weights[row];
        const int64_t lab = a.tg.labels[row];
        // exp(x - lse) as exp(x - m) / s on the statistics of stage 1, formed again: lse rounded to
        // fp32 would put up to half an ulp of lse into the exponent
        float m, s, e;
        softmax_row_stats<float>(cls, (size_t)HW, Cin, m, s, e);
        for (int c = 0; c < Cin; ++c) {
            const float p = expf_(cls[(size_t)c * HW] - m) / s;
            gc[(size_t)c * HW] = g * (p - (c == lab ? 1.0f : 0.0f));
        }
    } else {
        for (int c = 0; c < Cin; ++c) gc[(size_t)c * HW] = 0.0f;
    }
    const size_t roff = ((size_t)b * A + an) * 4 * HW + pos;
    const float *reg = a.t.reg[l] + roff;
    float *gr = a.greg[l] + roff;
    const float gb = a.grad_losses[2 * b + 1] / avg;
    const float4 bt = reinterpret_cast<const float4 *>(a.tg.bbox_targets)[row];
    const float4 bw = reinterpret_cast<const float4 *>(a.tg.bbox_weights)[row];
    const float t4[4] = {bt.x, bt.y, bt.z, bt.w}, w4[4] = {bw.x, bw.y, bw.z, bw.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float d = smooth_l1_der(reg[(size_t)k * HW] - t4[k], a.beta);
        gr[(size_t)k * HW] = w4[k] != 0.0f ? (gb * w4[k]) * d : 0.0f;      // a row without weight: +0.0
    }
}

static int launch_ssdloss_bwd(const SsdTable &t, int batch, const SsdTargets &tg, float beta, const uint8_t *sel, const float *grad_losses, const float *avg_dev, float avg,
                              const ia_ssd_level_ptrs *grads, hipStream_t s)
{
    int rc;
    if (!sel || !grad_losses || !grads || !(beta > 0.0f)) return IA_E_ARG;
    if (!avg_dev && !(avg > 0.0f)) return IA_E_ARG;
    if ((rc = check_targets(tg)) || (rc = check_rows_batch(t, batch))) return rc;
    SsdLossBwdArgs a;
    a.t = t; a.tg = tg; a.beta = beta; a.sel = sel; a.grad_losses = grad_losses;
    a.avg_dev = avg_dev; a.avg = avg;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        const bool on = l < t.num_levels;
        a.gcls[l] = on ? static_cast<float *>(const_cast<void *>(grads->cls[l])) : nullptr;
        a.greg[l] = on ? static_cast<float *>(const_cast<void *>(grads->reg[l])) : nullptr;
        if (on && (!a.gcls[l] || !a.greg[l])) return IA_E_ARG;
        if (on && (a.gcls[l] == t.cls[l] || a.greg[l] == t.reg[l])) return IA_E_ARG;     // not in place
    }
    const dim3 grid((unsigned)ssd_row_grid_x(t), (unsigned)(batch * t.num_levels));
    hipLaunchKernelGGL(k_ssdloss_bwd, grid, dim3(256), 0, s, a);
    return hip_status(hipGetLastError());
}

// ------------------------------------------------------------------ workspace of the node
// in this order; off: the pieces' byte offsets (ia_ssd_head_loss_workspace_layout)
struct SsdLossWorkspace {
    float *ce, *lse;          // (B, R) each
    uint8_t *sel;             // (B, R)
    int32_t *counts;          // (B, 2)
    double *parts;            // box partials (B, nparts)
    size_t off[5];
    size_t bytes;
    int32_t R, nparts;
};

static int carve_ssdloss(const SsdTable &t, int batch, const void *base, SsdLossWorkspace &w)
{
    int rc;
    if ((rc = check_rows_batch(t, batch))) return rc;
    w.R = t.row_off[t.num_levels];
    const int64_t np = (int64_t)t.num_levels * ssd_row_grid_x(t);
    if (np > 2147483647LL) return IA_E_ARG;
    w.nparts = (int32_t)np;
    const size_t B = (size_t)batch;
    Carver c(base);
    w.off[0] = c.take(w.ce, B * w.R * sizeof(float));
    w.off[1] = c.take(w.lse, B * w.R * sizeof(float));
    w.off[2] = c.take(w.sel, B * w.R);
    w.off[3] = c.take(w.counts, B * 2 * sizeof(int32_t));
    w.off[4] = c.take(w.parts, B * w.nparts * sizeof(double));
    w.bytes = c.bytes;
    return 0;
}

}  // namespace ia

extern "C" {

int ia_ssd_mine_lds_rows(void) { return ia::kSsdMineLdsRows; }

int ia_ssd_loss_partials(const ia_ssd_geom *g, int32_t *nparts)
{
    ia::SsdTable t;
    int rc = ia::make_ssd_table(g, nullptr, t);
    if (rc) return rc;
    if (!nparts) return IA_E_ARG;
    const int64_t np = (int64_t)t.num_levels * ia::ssd_row_grid_x(t);
    if (np > 2147483647LL) return IA_E_ARG;
    *nparts = (int32_t)np;
    return 0;
}

int ia_ssd_loss_rows(const ia_ssd_geom *g, const ia_ssd_level_ptrs *p, int batch, int dtype, const int64_t *labels,
                     const float *label_weights, const float *bbox_targets, const float *bbox_weights, float beta,
                     float *ce, float *lse, double *box_partials, void *stream)
{
    ia::SsdTable t;
    if (!p || dtype != IA_F32) return IA_E_ARG;
    int rc = ia::make_ssd_table(g, p, t);
    if (rc) return rc;
    const ia::SsdTargets tg = {labels, label_weights, bbox_targets, bbox_weights};
    return ia::launch_ssdloss_rows(t, batch, tg, beta, ce, lse, box_partials, (hipStream_t)stream);
}

int ia_ssd_mine(const float *ce, const int64_t *labels, int batch, int R, int neg_pos_ratio,
                const double *box_partials, int nparts, const float *avg_factor_dev, float avg_factor, uint8_t *sel,
                int32_t *counts, float *losses, void *stream)
{
    return ia::launch_ssd_mine(ce, labels, batch, R, neg_pos_ratio, box_partials, nparts, avg_factor_dev, avg_factor,
                               sel, counts, losses, (hipStream_t)stream);
}

int ia_ssd_loss_bwd(const ia_ssd_geom *g, const ia_ssd_level_ptrs *p, int batch, int dtype, const int64_t *labels,
                    const float *label_weights, const float *bbox_targets, const float *bbox_weights, float beta,
                    const uint8_t *sel, const float *grad_losses, const float *avg_factor_dev, float avg_factor,
                    const ia_ssd_level_ptrs *grads, void *stream)
{
    ia::SsdTable t;
    if (!p || dtype != IA_F32) return IA_E_ARG;
    int rc = ia::make_ssd_table(g, p, t);
    if (rc) return rc;
    const ia::SsdTargets tg = {labels, label_weights, bbox_targets, bbox_weights};
    return ia::launch_ssdloss_bwd(t, batch, tg, beta, sel, grad_losses, avg_factor_dev, avg_factor, grads,
                                  (hipStream_t)stream);
}

size_t ia_ssd_head_loss_workspace_bytes(const ia_ssd_geom *g, int batch)
{
    ia::SsdTable t;
    ia::SsdLossWorkspace w;
    if (ia::make_ssd_table(g, nullptr, t) || ia::carve_ssdloss(t, batch, nullptr, w)) return 0;
    return w.bytes;
}

int ia_ssd_head_loss_workspace_layout(const ia_ssd_geom *g, int batch, size_t offsets[5])
{
    ia::SsdTable t;
    ia::SsdLossWorkspace w;
    if (!offsets) return IA_E_ARG;
    int rc = ia::make_ssd_table(g, nullptr, t);
    if (rc) return rc;
    if ((rc = ia::carve_ssdloss(t, batch, nullptr, w))) return rc;
    for (int i = 0; i < 5; ++i) offsets[i] = w.off[i];
    return 0;
}

int ia_ssd_head_loss_fwd(const ia_ssd_geom *g, const ia_ssd_level_ptrs *p, int batch, int dtype,
                         const int64_t *labels, const float *label_weights, const float *bbox_targets,
                         const float *bbox_weights, const float *avg_factor_dev, float avg_factor, int neg_pos_ratio,
                         float beta, void *workspace, size_t workspace_bytes, float *losses, void *stream)
{
    ia::SsdTable t;
    ia::SsdLossWorkspace w;
    if (!p || dtype != IA_F32) return IA_E_ARG;
    int rc = ia::make_ssd_table(g, p, t);
    if (rc) return rc;
    if (neg_pos_ratio < 0 || !(beta > 0.0f)) return IA_E_ARG;
    if (!avg_factor_dev && !(avg_factor > 0.0f)) return IA_E_ARG;
    if (!workspace || !losses || ((uintptr_t)workspace & 255u) != 0) return IA_E_ARG;
    if ((rc = ia::carve_ssdloss(t, batch, workspace, w))) return rc;
    if (workspace_bytes < w.bytes) return IA_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const ia::SsdTargets tg = {labels, label_weights, bbox_targets, bbox_weights};
    if ((rc = ia::launch_ssdloss_rows(t, batch, tg, beta, w.ce, w.lse, w.parts, s))) return rc;
    return ia::launch_ssd_mine(w.ce, labels, batch, w.R, neg_pos_ratio, w.parts, w.nparts, avg_factor_dev, avg_factor,
                               w.sel, w.counts, losses, s);
}

int ia_ssd_head_loss_bwd(const ia_ssd_geom *g, const ia_ssd_level_ptrs *p, int batch, int dtype,
                         const int64_t *labels, const float *label_weights, const float *bbox_targets,
                         const float *bbox_weights, const float *avg_factor_dev, float avg_factor, float beta,
                         const void *workspace, size_t workspace_bytes, const float *grad_losses,
                         const ia_ssd_level_ptrs *grads, void *stream)
{
    ia::SsdTable t;
    ia::SsdLossWorkspace w;
    if (!p || dtype != IA_F32) return IA_E_ARG;
    int rc = ia::make_ssd_table(g, p, t);
    if (rc) return rc;
    if (!workspace || ((uintptr_t)workspace & 255u) != 0) return IA_E_ARG;
    if ((rc = ia::carve_ssdloss(t, batch, workspace, w))) return rc;
    if (workspace_bytes < w.bytes) return IA_E_ARG;
    const ia::SsdTargets tg = {labels, label_weights, bbox_targets, bbox_weights};
    return ia::launch_ssdloss_bwd(t, batch, tg, beta, w.sel, grad_losses, avg_factor_dev, avg_factor, grads,
                                  (hipStream_t)stream);
}

}  // extern "C"
