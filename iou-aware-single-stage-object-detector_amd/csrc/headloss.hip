// IoUawareRetinaHead.loss for ALL pyramid levels at once
// (reference iou_aware_retina_head.py:221-313 `loss_single` x 5 levels, :315-387 `loss`;
// core/loss/losses.py:226-247,279-303 focal, :385-411 smooth-L1, :460-480 IoU BCE).
//
// The per-level kernels of loss.hip cost one launch per (loss, level, direction): 30 launches,
// the four small levels running far below the HBM stream of P3, plus ~140 scalar torch kernels
// of autograd glue around them.  Here one training iteration's loss part is
//
//   forward : k_pack_targets  k_focal_ml<fwd>  k_box_ml<fwd>  k_headloss_finalize   (4 launches)
//   backward: k_focal_ml<bwd>  k_box_ml<bwd>                                        (2 launches)
//
// * k_focal_ml -- focal loss (gamma = 2) over the class logits of every level: the wavefront
//   tiling of k_rowmax / k_focal (wavefront = anchor x 256 positions, every class-plane access one
//   contiguous 1 KiB segment), blocks of the SMALL levels first so that their latency-bound
//   tails overlap the P3 stream.  All elements are evaluated as negatives (no per-element label
//   compare / select; the per-anchor weight is applied once per position after the class loop)
//   and the rare positive element of a positive anchor is corrected afterwards: five plain VALU
//   operations + exp + rcp + log per element, evaluated eight elements abreast so that the
//   transcendental unit is fed back to back, class planes double-buffered in registers.
//   MI355X, B = 4 (rocprofv3): forward 52.5 us = 5.1 TB/s, backward 105 us = 5.0 TB/s of
//   algorithmic bytes (0.64 / 0.63 of the 8 TB/s peak); what it took, in measured steps
//   (forward): one wavefront per (anchor, tile) running all 80 classes on every level 99.5 us ->
//   class range of the small levels split 71 -> counted-wait ping-pong pipeline 66 -> labels
//   from an anchor-major copy instead of 72-byte-stride gathers 55 -> split target 4096: 52.5.
// * k_box_ml  -- smooth-L1 + IoU target + IoU BCE of every level in one pass over the box
//   deltas; anchors whose bbox_weights are zero (all negatives: > 99 %) contribute exactly 0
//   and skip the exact-math decode; backward writes d(bbox_pred) = smooth-L1 part + the part
//   through the attached IoU target in one store, and d(iou_pred).
// * k_headloss_finalize -- the 64 fp64 partial slots per (loss, level) -> fp32 losses
//   (sum / avg_factor) * loss_weight, avg_factor = sum_b max(n_pos_b, 1) read from the
//   assignment kernel's counts: the normaliser never visits the host.
//
// The plain RetinaHead (IA_CLS_SIGMOID_NOIOU, reference anchor_head.py:234-299) takes the same
// entries: the box kernels carry the kind as a template parameter (IOU), and their IOU = false
// instances are smooth-L1 alone -- no anchor, no decode, no IoU map read, no IoU gradient written;
// the losses_iou entries of the result are 0.  Focal kernels, packed targets and slots are shared.
//
// The IoU-balanced losses of the IoU-aware head (IOUbalancedSigmoidFocalLoss / IoUbalancedSmoothL1Loss,
// core/loss/losses.py:309-374,416-458) are two more compile-time switches on the same kernels and the
// same launches: BAL_CLS on the focal kernels (the rare positive correction goes to two slot rows of its
// own, S1 and S2 = S1 weighted by iou^eta, and recomputes the anchor's IoU with the box kernel's code),
// BAL_LOC on box_elem (smooth-L1 weights times iou^delta); k_headloss_finalize forms
// norm_l = S1 / (S2 + 1e-6) and leaves it behind the plain result for the backward kernels.
//
// BalancedL1Loss (core/loss/losses.py:482-520) in place of smooth-L1 is the box kernels' last template
// parameter, LOC (0 smooth-L1, 1 balanced L1: balanced_l1_val / _der of ia_loss.hpp), with or without the IoU
// term; its constants ride behind the smooth-L1 argument blocks (BoxSel), so every LOC = 0 instance keeps
// its kernel arguments and its code.  Focal kernels, packed targets, slots, finalize and workspace are shared.
//
// The box kernels of the two layouts (k_box_ml: NCHW planes, k_box_nhwc: pixel rows with a stride)
// keep block location, the `live` test, loads and stores; the per-anchor math is box_elem, the
// fp64 block reduction box_block_reduce.  Host: ml_loss_args / nhwc_loss_args validate and fill
// for forward and backward alike (backward = forward + gradient pointers); carve() alone knows
// the workspace layout; a forward call is refused before its first enqueue.
#include <stddef.h>
#include <string.h>
#include "ia_loss.hpp"
#include "ia_headloss.hpp"

namespace ia {

struct BlockRef { int l, b, an, p0, chunk; };

template <bool SPLIT>
__device__ __forceinline__ BlockRef locate_block(const HLLevels &lv, int bid)
{
    const int32_t *off = SPLIT ? lv.fblk_off : lv.blk_off;
    int o = 0;
    while (bid >= off[o + 1]) ++o;
    BlockRef r;
    r.l = lv.L - 1 - o;
    int q = bid - off[o];
    const int tiles = (lv.H[r.l] * lv.W[r.l] + 255) / 256;
    const int tile = q % tiles; q /= tiles;
    r.chunk = 0;
    r.p0 = tile * 256;
    if (SPLIT) { r.chunk = q % lv.csplit[r.l]; q /= lv.csplit[r.l]; }
    r.an = q % lv.A;
    r.b = q / lv.A;
    return r;
}

constexpr int kSlotMask = IA_LOSS_SLOTS - 1;
constexpr int64_t kFocalLevelWaves = 4096;
constexpr int kNumLoss = 3;               // cls, bbox, iou
// layout of the fp32 result / upstream-gradient vector: [k * L + l] per-level, [3L + k] totals,
// [3L + 3] avg_factor
__device__ __forceinline__ float upstream(const float *gin, const float *res, int L, int k, int l,
                                          float lw)
{
    return ((gin[k * L + l] + gin[3 * L + k]) * lw) / res[3 * L + 3];
}

// ------------------------------------------------------------------ focal, all levels
// ---- element math.  With t = exp(x), s = 1 + t:   sigmoid(x) = t/s,  1 - sigmoid(x) = 1/s,
// BCE(x, 0) = softplus(x) = log(s),  BCE(x, 1) = softplus(-x) = log(s) - x.
// One v_exp_f32, one v_rcp_f32, one v_log_f32 per element (the transcendental unit issues at an
// eighth of the plain VALU rate on gfx950: these three are 48 of the ~60 issue cycles of an
// element) and five plain operations; the factor ln 2 of log2 -> log and the anchor's weight are
// applied once per position after the class loop.  x is clamped to kXMax before the exponential
// (exp(88.8) overflows fp32); above it sigmoid = 1 and softplus(x) = x hold to the last bit, and
// the (never observed) logits beyond it take the exact branch below.
constexpr float kXMax = 60.0f;
constexpr float kLog2e = 1.44269504088896341f, kLn2 = 0.693147180559945309f;

struct Sig { float p, q, lg; };          // sigmoid, 1 - sigmoid, log2(1 + exp(x))
__device__ __forceinline__ Sig sig_parts(float x)
{
    const float t = __builtin_amdgcn_exp2f(__builtin_fminf(x, kXMax) * kLog2e);
    const float s = 1.0f + t;
    Sig r;
    r.q = __builtin_amdgcn_rcpf(s);
    r.lg = __builtin_amdgcn_logf(s);
    r.p = t * r.q;
    return r;
}
// UNWEIGHTED negative element  p^2 * BCE(x, 0), in units of ln 2, and its x-derivative (natural units)
__device__ __forceinline__ float neg_val2(const Sig &g) { return (g.p * g.p) * g.lg; }
__device__ __forceinline__ float neg_der(const Sig &g)
{
    return (g.p * g.p) * __builtin_fmaf(2.0f * kLn2, g.lg * g.q, g.p);
}
// positive element  q^2 * BCE(x, 1) (natural units) and its derivative
__device__ __forceinline__ float pos_val(const Sig &g, float x)
{
    return (g.q * g.q) * __builtin_fmaf(kLn2, g.lg, -x);
}
__device__ __forceinline__ float pos_der(const Sig &g, float x)
{
    return -((g.q * g.q) * __builtin_fmaf(2.0f * __builtin_fmaf(kLn2, g.lg, -x), g.p, g.q));
}

// the anchor of position p of a W-wide level: base anchor + grid shift (regenerated, never stored)
__device__ __forceinline__ void grid_anchor(const BaseAnchors &ba, int l, int an, int p, int W, int stride,
                                            float (&anc)[4])
{
    const int y = p / W, x = p - y * W;
    const float sx = (float)(x * stride), sy = (float)(y * stride);
    const float *b4 = ba.v[l][an];
    anc[0] = b4[0] + sx; anc[1] = b4[1] + sy; anc[2] = b4[2] + sx; anc[3] = b4[3] + sy;
}

// ---- IoU-balanced focal loss (BAL_CLS; reference core/loss/losses.py:309-374).  The positive element of
// a positive anchor goes to two sums of its own, S1 = sum of the focal terms and S2 = the same terms
// times iou^eta; the class row keeps S0, the negatives.  loss = S0 + norm * S2 with norm = S1 / (S2 + 1e-6)
// formed by the finalize kernel; backward scales the positive derivative by iou^eta * norm.  iou is the
// (detached) IoU of the anchor's decoded prediction with its decoded target, recomputed here by the
// code the box kernel runs: positives are < 1 % of the anchors and one class chunk owns each, so
// there is no per-anchor map and no ordering between the two kernels.
// iou^x as k_focal of loss.hip forms it; iou = 0: log2 = -inf, exp2(-inf) = 0 for x > 0 -- no NaN
__device__ __forceinline__ float iou_pow(float iou, float x)
{
    return __builtin_amdgcn_exp2f(x * __builtin_amdgcn_logf(iou));
}
__device__ __forceinline__ float bal_weight(const FocalBal &c, int l, int an, int p, int W, int stride,
                                            const float (&dp)[4], const float4 tq)
{
    const float dt[4] = {tq.x, tq.y, tq.z, tq.w};
    float anc[4];
    grid_anchor(c.ba, l, an, p, W, stride, anc);
    return iou_pow(iou_target_elem(anc, dp, dt, c.means, c.stds).t, c.eta);
}

// S1 / S2 of one wavefront -> the level's slots in the two rows behind the three losses' (wave-uniform
// branch: positives are rare, most wavefronts have nothing to add)
__device__ __forceinline__ void bal_wave_sums(double *sums, int L, int l, double s1, double s2)
{
    if (__ballot((s1 != 0.0) | (s2 != 0.0))) {
        const double d1 = wave_sum(s1), d2 = wave_sum(s2);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(sums + (size_t)(kNumLoss * L + l) * IA_LOSS_SLOTS + (blockIdx.x & kSlotMask), d1);
            atomicAdd(sums + (size_t)((kNumLoss + 1) * L + l) * IA_LOSS_SLOTS + (blockIdx.x & kSlotMask), d2);
        }
    }
}

template <typename T, bool BWD, bool BAL_CLS = false>
__global__ void __launch_bounds__(64) k_focal_ml(typename FocalSel<BAL_CLS>::ML a)
{
    const int lane = threadIdx.x;
    const BlockRef r = locate_block<true>(a.lv, blockIdx.x);
    const int A = a.lv.A, C = a.lv.C, HW = a.lv.H[r.l] * a.lv.W[r.l];
    const int cbeg = r.chunk * a.lv.cchunk[r.l];
    const int cend = (cbeg + a.lv.cchunk[r.l] < C) ? (cbeg + a.lv.cchunk[r.l]) : C;
    const T *cls = static_cast<const T *>(a.cls[r.l]) + ((size_t)r.b * A + r.an) * C * HW;
    float *grad = BWD ? a.grad[r.l] + ((size_t)r.b * A + r.an) * C * HW : nullptr;
    const float gs = BWD ? upstream(a.tail.gin, a.tail.res, a.lv.L, 0, r.l, a.tail.loss_weight) : 1.0f;
    const bool vec = (HW & 3) == 0;
    // labels / weights of this anchor's 256 positions from the anchor-major packed copy
    // (k_pack_targets): two coalesced 16-byte loads per lane instead of eight 64-line gathers
    const size_t am = (size_t)a.lv.pack_off[r.l] + ((size_t)r.b * A + r.an) * HW;
    int pos[4], pc[4], lab[4];
    float wn[4], wp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        pos[j] = vec ? (r.p0 + lane * 4 + j) : (r.p0 + lane + 64 * j);
        pc[j] = (pos[j] < HW) ? pos[j] : (vec ? (HW - 4 + j) : (HW - 1));   // clamped: loads unconditional
    }
    if (vec) {
        const int4 l4 = *reinterpret_cast<const int4 *>(a.lab_am + am + pc[0]);
        const float4 w4 = *reinterpret_cast<const float4 *>(a.w_am + am + pc[0]);
        lab[0] = l4.x; lab[1] = l4.y; lab[2] = l4.z; lab[3] = l4.w;
        wn[0] = w4.x; wn[1] = w4.y; wn[2] = w4.z; wn[3] = w4.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) { lab[j] = a.lab_am[am + pc[j]]; wn[j] = a.w_am[am + pc[j]]; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float w0 = (pos[j] < HW) ? wn[j] : 0.0f;                      // padding lanes weigh 0
        if (pos[j] >= HW) lab[j] = 0;
        wn[j] = (a.tail.alpha_neg * w0) * gs;
        wp[j] = (a.tail.alpha_pos * w0) * gs;
    }
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    constexpr int K = 8;                                   // class planes in flight per wavefront
    if (vec) {
        // Software pipeline over groups of K class planes with two register buffers in ping-pong
        // (no register copies, so the waits stay counted): while one group is evaluated the next
        // group's 8 KiB per wavefront are in flight.
        using V = typename Elems<T, 4>::XV;
        const T *src = cls + pc[0];
        auto issue = [&](V (&q)[K], int c0) {
#pragma unroll
            for (int i = 0; i < K; ++i) {                  // unconditional, clamped: no branches
                const int c = (c0 + i < cend) ? (c0 + i) : (cend - 1);
                q[i] = __builtin_nontemporal_load(reinterpret_cast<const V *>(src + (size_t)c * HW));
            }
        };
        // two class planes (8 elements per lane) at a time, stage by stage: the eight
        // exponentials, then the eight reciprocals and logarithms, issue back to back instead
        // of waiting on one element's dependent chain
        auto eval = [&](const V (&q)[K], int c0) {
#pragma unroll
            for (int i = 0; i < K; i += 2) {
                if (c0 + i < cend) {                       // wave-uniform
                    float v[8], t[8], rq[8], lg[8];
                    Elems<T, 4>::unpack(q[i], *reinterpret_cast<float (*)[4]>(&v[0]));
                    Elems<T, 4>::unpack(q[i + 1], *reinterpret_cast<float (*)[4]>(&v[4]));
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        t[k] = __builtin_amdgcn_exp2f(__builtin_fminf(v[k], kXMax) * kLog2e);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const float sk = 1.0f + t[k];
                        rq[k] = __builtin_amdgcn_rcpf(sk);
                        lg[k] = __builtin_amdgcn_logf(sk);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    const bool second = c0 + i + 1 < cend;
                    float o[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        Sig g; g.q = rq[k]; g.lg = lg[k]; g.p = t[k] * rq[k];
                        if (BWD) o[k] = neg_der(g) * wn[k & 3];
                        else if (k < 4 || second) acc[k & 3] += neg_val2(g);
                    }
                    if (BWD && pos[0] < HW) {
                        typedef float F4 __attribute__((ext_vector_type(4)));
                        F4 g0, g1;
                        g0.x = o[0]; g0.y = o[1]; g0.z = o[2]; g0.w = o[3];
                        g1.x = o[4]; g1.y = o[5]; g1.z = o[6]; g1.w = o[7];
                        F4 *d0 = reinterpret_cast<F4 *>(grad + (size_t)(c0 + i) * HW + pc[0]);
                        F4 *d1 = reinterpret_cast<F4 *>(grad + (size_t)(c0 + i + 1) * HW + pc[0]);
                        *d0 = g0;              // (non-temporal stores: no difference, 104.9 vs 105.5 us)
                        if (second) *d1 = g1;
                    }
                }
            }
        };
        V qa[K], qb[K];
        issue(qa, cbeg);
        for (int c0 = cbeg; c0 < cend; c0 += 2 * K) {
            issue(qb, c0 + K);
            eval(qa, c0);
            issue(qa, c0 + 2 * K);
            eval(qb, c0 + K);
        }
    } else {                                               // plane bases only 4-byte aligned
        for (int c0 = cbeg; c0 < cend; c0 += K) {
            float v[K][4];
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const int c = (c0 + i < cend) ? (c0 + i) : (cend - 1);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[i][j] = load_f32<T>(cls + (size_t)c * HW + pc[j]);
            }
#pragma unroll
            for (int i = 0; i < K; ++i) {
                if (c0 + i < cend) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const Sig g = sig_parts(v[i][j]);
                        if (BWD) {
                            if (pos[j] < HW) grad[(size_t)(c0 + i) * HW + pos[j]] = neg_der(g) * wn[j];
                        } else acc[j] += neg_val2(g);
                    }
                }
            }
        }
    }
    // Corrections, all rare: (1) the positive element of a positive anchor replaces its
    // negative-form contribution (the same lane wrote the negative-form gradient above, so the
    // overwrite is ordered); (2) logits above kXMax: softplus(x) = x there, the clamp gave kXMax.
    float total = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float fix = 0.0f;
        if (lab[j] > cbeg && lab[j] <= cend && pos[j] < HW) {      // class lab-1 in [cbeg, cend)
            const size_t e = (size_t)(lab[j] - 1) * HW + pos[j];
            const float x = load_f32<T>(cls + e);
            const Sig g = sig_parts(x);
            float iw = 1.0f;
            if constexpr (BAL_CLS) {
                const T *bp = static_cast<const T *>(a.bal.reg[r.l]) + ((size_t)r.b * A + r.an) * 4 * HW + pos[j];
                const float dp[4] = {load_f32<T>(bp), load_f32<T>(bp + (size_t)HW),
                                     load_f32<T>(bp + (size_t)2 * HW), load_f32<T>(bp + (size_t)3 * HW)};
                iw = bal_weight(a.bal, r.l, r.an, pos[j], a.lv.W[r.l], a.lv.stride[r.l], dp,
                                reinterpret_cast<const float4 *>(a.bal.bt[r.l])[((size_t)r.b * HW + pos[j]) * A + r.an]);
            }
            if (BWD) {
                const float d = pos_der(g, __builtin_fminf(x, kXMax)) * wp[j];
                // norm_l = S1 / (S2 + 1e-6) of the forward call, behind the plain result entries
                grad[e] = BAL_CLS ? d * (iw * a.tail.res[3 * a.lv.L + 4 + r.l]) : d;
            } else {
                acc[j] -= neg_val2(g);
                fix = pos_val(g, __builtin_fminf(x, kXMax)) * wp[j];
                if constexpr (BAL_CLS) { s1 += fix; s2 += fix * iw; fix = 0.0f; }
            }
        }
        if (!BWD) total += __builtin_fmaf(acc[j] * kLn2, wn[j], fix);
    }
    if (!BWD && __builtin_expect(a.tail.big_logits != 0, 0)) {
        // exact tail for logits > kXMax (requested by the host when it cannot exclude them):
        // add (x - kXMax) per such negative element
        for (int c = cbeg; c < cend; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (pos[j] < HW) {
                    const float x = load_f32<T>(cls + (size_t)c * HW + pos[j]);
                    if (x > kXMax && lab[j] != c + 1) total += (x - kXMax) * wn[j];
                }
    }
    if (!BWD) {
        const double d = wave_sum((double)total);
        if (lane == 0) atomicAdd(a.tail.sums + (size_t)(0 * a.lv.L + r.l) * IA_LOSS_SLOTS +
                                     (blockIdx.x & kSlotMask), d);
        if constexpr (BAL_CLS) bal_wave_sums(a.tail.sums, a.lv.L, r.l, (double)s1, (double)s2);
    }
}

// ------------------------------------------------------------------ targets -> anchor-major
// labels / label_weights arrive position-major (n = p*A + a, the reference's order): read per
// anchor they are 8-byte gathers at a 72-byte stride, 64 cache lines per load instruction -- as
// many L1 line requests as the class stream itself.  One small pass transposes them (through LDS,
// both sides coalesced) to (B, A, HW) int32 / fp32; forward and backward read that copy.
struct PackArgs {
    HLLevels lv;
    const int64_t *labels[IA_MAX_LEVELS];
    const float *lw[IA_MAX_LEVELS];
    int32_t *lab_am;
    float *w_am;
    int32_t tile_off[IA_MAX_LEVELS + 1];  // prefix of B * tiles_l
};

__global__ void __launch_bounds__(256) k_pack_targets(PackArgs a)
{
    __shared__ int32_t s_lab[IA_MAX_ANCHORS * 257];
    __shared__ float s_w[IA_MAX_ANCHORS * 257];
    int l = 0;
    while ((int)blockIdx.x >= a.tile_off[l + 1]) ++l;
    int q = blockIdx.x - a.tile_off[l];
    const int A = a.lv.A, HW = a.lv.H[l] * a.lv.W[l];
    const int tiles = (HW + 255) / 256;
    const int b = q / tiles, p0 = (q - b * tiles) * 256;
    const int npos = (HW - p0 < 256) ? (HW - p0) : 256;
    const size_t base = ((size_t)b * HW + p0) * A;
    for (int k = threadIdx.x; k < npos * A; k += 256) {
        const int p = k / A, an = k - p * A;
        s_lab[an * 257 + p] = (int32_t)a.labels[l][base + k];
        s_w[an * 257 + p] = a.lw[l][base + k];
    }
    __syncthreads();
    const size_t out = (size_t)a.lv.pack_off[l] + (size_t)b * A * HW + p0;
    for (int k = threadIdx.x; k < 256 * A; k += 256) {
        const int an = k >> 8, p = k & 255;
        if (p < npos) {
            a.lab_am[out + (size_t)an * HW + p] = s_lab[an * 257 + p];
            a.w_am[out + (size_t)an * HW + p] = s_w[an * 257 + p];
        }
    }
}

// ------------------------------------------------------------------ smooth-L1 + IoU BCE, all levels
// what the box kernels of both layouts share behind their own addressing: targets, gradient maps
// and scalars (the base anchors stay in front of the head-output pointers, where they have always
// been in both argument blocks)
struct BoxTail {
    const float *bt[IA_MAX_LEVELS], *bw[IA_MAX_LEVELS];
    float *g_reg[IA_MAX_LEVELS], *g_iou[IA_MAX_LEVELS];
    double *sums;
    const float *gin, *res;
    float means[4], stds[4];
    float beta, lw_bbox, lw_iou;
    int32_t attach;
    float delta;                          // BAL_LOC: smooth-L1 weights times iou^delta
};

struct BoxMLArgs {
    HLLevels lv;
    BaseAnchors ba;
    const void *reg[IA_MAX_LEVELS], *iou[IA_MAX_LEVELS];
    BoxTail tail;
};
// LOC = 1: the balanced-L1 constants BEHIND the block of either layout (as FocalBal rides behind the focal
// blocks); loc_consts hands them to box_elem, nothing for LOC = 0
struct BoxMLBl1Args : BoxMLArgs { BalL1 bl; };
struct BoxNhwcArgs;
struct BoxNhwcBl1Args;
template <int LOC> struct BoxSel { typedef BoxMLArgs ML; typedef BoxNhwcArgs Nhwc; };
template <> struct BoxSel<1> { typedef BoxMLBl1Args ML; typedef BoxNhwcBl1Args Nhwc; };
template <int LOC, class Args>
__device__ __forceinline__ BalL1 loc_consts(const Args &a)
{
    if constexpr (LOC == 1) return a.bl;
    else return BalL1();
}

// One live anchor (an, position p of level l) of either layout.  Forward: its two loss terms;
// backward: d(bbox_pred) = smooth-L1 part + the part through the attached IoU target, and
// d(iou_pred).  xl is the IoU logit (not looked at without IOU).
// BAL_LOC (IoU-balanced smooth-L1, reference core/loss/losses.py:416-458): the anchor's weights times
// iou^delta, iou the (detached) IoU target this function holds anyway -- powf_pos_ on the weights like
// k_smooth_l1 of loss.hip, so both routes round alike; IoU BCE and the gradient through the attached
// target are unchanged.
// LOC: the localisation loss of a coordinate -- 0 smooth-L1, 1 balanced L1 (constants bl, c.beta its knee).
template <bool BWD, bool IOU, bool BAL_LOC = false, int LOC = 0>
__device__ __forceinline__ void box_elem(const BoxTail &c, const BalL1 &bl, const BaseAnchors &ba, int L, int l, int an, int p, int W, int stride,
                                         const float (&wv)[4], const float (&dp)[4],
                                         const float (&dt)[4], float xl, double &acc_l1,
                                         double &acc_iou, float (&g_box)[4], float &g_iou)
{
    static_assert(IOU || !BAL_LOC, "the IoU-balanced smooth-L1 needs the IoU branch");
    static_assert(LOC == 0 || (LOC == 1 && !BAL_LOC), "balanced L1 has no IoU-balanced variant");
    auto loc_val = [&](float df) { if constexpr (LOC == 1) return balanced_l1_val(df, c.beta, bl); else return smooth_l1_val(df, c.beta); };
    auto loc_der = [&](float df) { if constexpr (LOC == 1) return balanced_l1_der(df, c.beta, bl); else return smooth_l1_der(df, c.beta); };
    IouElem q;
    if constexpr (IOU) {
        float anc[4];
        grid_anchor(ba, l, an, p, W, stride, anc);
        q = iou_target_elem(anc, dp, dt, c.means, c.stds);
    }
    float wl[4] = {wv[0], wv[1], wv[2], wv[3]};           // the smooth-L1 term's weights
    if constexpr (BAL_LOC) {
        const float pw = powf_pos_(q.t, c.delta);
#pragma unroll
        for (int k = 0; k < 4; ++k) wl[k] = wv[k] * pw;
    }
    if (!BWD) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) s += loc_val(dp[k] - dt[k]) * wl[k];
        acc_l1 = (double)s;
        if constexpr (IOU) acc_iou = (double)(bce_logits_(xl, q.t) * wv[0]);
    } else {
        const float gs1 = upstream(c.gin, c.res, L, 1, l, c.lw_bbox);
        float gv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (IOU) {
            const float gs2 = upstream(c.gin, c.res, L, 2, l, c.lw_iou);
            g_iou = ((sigmoidf_(xl) - q.t) * wv[0]) * gs2;
            if (c.attach) iou_bce_box_grad(q, xl, wv[0], gs2, c.stds, gv);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float g = (loc_der(dp[k] - dt[k]) * wl[k]) * gs1;
            // with the IoU term the add is unconditional (attach off: gv = 0, and x + 0.0f turns
            // -0.0f into +0.0f); the plain RetinaHead kind (smooth-L1 alone) has no add
            g_box[k] = IOU ? g + gv[k] : g;
        }
    }
}

// the workgroup's two fp64 sums -> slots of (loss, level); positives are rare: most workgroups
// have nothing to add
template <bool IOU>
__device__ __forceinline__ void box_block_reduce(double *sums, int L, int l, double acc_l1, double acc_iou)
{
    __shared__ double red[2][4];
    const bool any = __syncthreads_or((acc_l1 != 0.0) | (acc_iou != 0.0));
    if (any) {
        const double s1 = wave_sum(acc_l1), s2 = wave_sum(acc_iou);
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { red[0][w] = s1; red[1][w] = s2; }
        __syncthreads();
        if (threadIdx.x < (IOU ? 2 : 1)) {
            const double s = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) +
                             red[threadIdx.x][3];
            if (s != 0.0)
                atomicAdd(sums + (size_t)((1 + threadIdx.x) * L + l) * IA_LOSS_SLOTS +
                              (blockIdx.x & kSlotMask), s);
        }
    }
}

template <typename T, bool BWD, bool IOU, bool BAL_LOC = false, int LOC = 0>
__global__ void __launch_bounds__(256) k_box_ml(typename BoxSel<LOC>::ML a)
{
    const BlockRef r = locate_block<false>(a.lv, blockIdx.x);
    const int A = a.lv.A, W = a.lv.W[r.l], HW = a.lv.H[r.l] * W;
    const int p = r.p0 + threadIdx.x;
    double acc_l1 = 0.0, acc_iou = 0.0;
    if (p < HW) {
        const size_t ba = (size_t)r.b * A + r.an;
        const size_t e = ba * HW + p;
        const size_t n = ((size_t)r.b * HW + p) * A + r.an;
        const float4 wt4 = reinterpret_cast<const float4 *>(a.tail.bw[r.l])[n];
        const float wv[4] = {wt4.x, wt4.y, wt4.z, wt4.w};
        const bool live = (wv[0] != 0.0f) | (wv[1] != 0.0f) | (wv[2] != 0.0f) | (wv[3] != 0.0f);
        float g_box[4] = {0.0f, 0.0f, 0.0f, 0.0f}, g_iou = 0.0f;
        if (live) {
            const T *bp = static_cast<const T *>(a.reg[r.l]) + ba * 4 * HW + p;
            const float dp[4] = {load_f32<T>(bp), load_f32<T>(bp + (size_t)HW),
                                 load_f32<T>(bp + (size_t)2 * HW), load_f32<T>(bp + (size_t)3 * HW)};
            const float4 tq = reinterpret_cast<const float4 *>(a.tail.bt[r.l])[n];
            const float dt[4] = {tq.x, tq.y, tq.z, tq.w};
            const float xl = IOU ? load_f32<T>(static_cast<const T *>(a.iou[r.l]) + e) : 0.0f;
            box_elem<BWD, IOU, BAL_LOC, LOC>(a.tail, loc_consts<LOC>(a), a.ba, a.lv.L, r.l, r.an, p, W, a.lv.stride[r.l],
                                             wv, dp, dt, xl, acc_l1, acc_iou, g_box, g_iou);
        }
        if (BWD) {
            float *go = a.tail.g_reg[r.l] + ba * 4 * HW + p;
            go[0] = g_box[0];
            go[(size_t)HW] = g_box[1];
            go[(size_t)2 * HW] = g_box[2];
            go[(size_t)3 * HW] = g_box[3];
            if constexpr (IOU) a.tail.g_iou[r.l][e] = g_iou;
        }
    }
    if (!BWD) box_block_reduce<IOU>(a.tail.sums, a.lv.L, r.l, acc_l1, acc_iou);
}

// ------------------------------------------------------------------ channels-last head outputs
// The training head (winograd_train.py) produces channels-last tensors: element (b, p, a, c) of a
// class map sits at (b*HW + p) * pix_stride + a*C + c, i.e. in the reference's flattened order
// (cls_score.permute(0, 2, 3, 1).reshape(-1, C), iou_aware_retina_head.py:236-240) -- the targets
// (anchor-major n = (b, p, a)) index it directly, no packed copy, and every load / store is a
// 16-byte piece of a contiguous run.  reg / iou may be channel slices of one wider tensor
// (pix_stride > A*4 / A).  The anchor heads' entries are fp32 only; the point heads (pointloss.hip) run
// the focal kernel on fp32 or bf16 rows with unit label weights.
// T: storage type of logits and gradient (float, or uint16_t = bf16 widened on load, the fp32 gradient
// rounded to nearest even once on store); UNITW: every label weight is 1, a.lw is not read (the point
// heads, A = 1)
template <bool BWD, typename T, bool UNITW, bool BAL_CLS = false>
__global__ void __launch_bounds__(256) k_focal_nhwc(typename FocalSel<BAL_CLS>::Nhwc a)
{
    static_assert(!BAL_CLS || (sizeof(T) == 4 && !UNITW), "IoU-balanced: the anchor heads' fp32 rows");
    __shared__ double red[4];
    int o = 0;
    while ((int)blockIdx.x >= a.lv.fblk_off[o + 1]) ++o;
    const int l = a.lv.L - 1 - o;
    const int A = a.lv.A, C = a.lv.C, C4 = C >> 2, AC4 = A * C4;
    const int64_t HW = (int64_t)a.lv.H[l] * a.lv.W[l];
    const int64_t nchunks = (int64_t)a.lv.B * HW * AC4;
    // chunk -> (pixel, anchor, class quad) without per-chunk integer divisions (a 64-bit division
    // per chunk cost as many issue slots as the loss math of its four elements): one division
    // per workgroup for its first chunk, then offsets < AC4 + 1024 divided through the float
    // reciprocal ((n + 0.5) / d is at least 0.5 / d away from an integer, far above fp32
    // rounding for n, d < 2^14)
    const int64_t base0 = (int64_t)(blockIdx.x - a.lv.fblk_off[o]) * kFocalChunks;
    const int64_t pix0 = base0 / AC4;
    const int r0 = (int)(base0 - pix0 * AC4);
    const float inv_ac4 = 1.0f / (float)AC4, inv_c4 = 1.0f / (float)C4;
    const float gs = BWD ? upstream(a.tail.gin, a.tail.res, a.lv.L, 0, l, a.tail.loss_weight) : 1.0f;
    const T *cls = static_cast<const T *>(a.cls[l]);
    const int64_t ps = a.ps_cls[l], pg = BWD ? a.ps_grad[l] : 0;
    // every load of the thread is issued before the first use (addresses clamped, no predicate):
    // a load next to its use, or under `on ? load : 0`, compiles to load + s_waitcnt vmcnt(0)
    // per piece, i.e. eight dependent memory round trips per thread instead of one
    float4 v[kFocalU];
    int32_t labv[kFocalU];
    float lwv[kFocalU];
    int cq[kFocalU];
    int64_t goff[kFocalU];
    bool on[kFocalU];
    const int32_t *labels = reinterpret_cast<const int32_t *>(a.labels[l]);   // low words: labels < 2^31
    const float *lwp = UNITW ? nullptr : a.lw[l];
#pragma unroll
    for (int u = 0; u < kFocalU; ++u) {
        int j = (int)threadIdx.x + 256 * u;
        on[u] = base0 + j < nchunks;
        if (!on[u]) j = (int)(nchunks - 1 - base0);         // clamped: loads unconditional
        const int rr = r0 + j;
        const int dp = (int)(((float)rr + 0.5f) * inv_ac4);
        const int64_t pix = pix0 + dp;                      // (b, p)
        const int r = rr - dp * AC4;                        // a * C4 + class quad
        const int an = (int)(((float)r + 0.5f) * inv_c4);
        const int64_t anchor = pix * A + an;
        cq[u] = r - an * C4;
        using V = typename Elems<T, 4>::XV;
        const V q = __builtin_nontemporal_load(reinterpret_cast<const V *>(cls + pix * ps + 4 * r));
        float x4[4];
        Elems<T, 4>::unpack(q, x4);
        v[u] = make_float4(x4[0], x4[1], x4[2], x4[3]);
        labv[u] = labels[2 * anchor];
        lwv[u] = UNITW ? 1.0f : lwp[anchor];
        goff[u] = pix * pg + 4 * r;
    }
    double total = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int u = 0; u < kFocalU; ++u) {
        const int lab = labv[u];
        const float w0 = on[u] ? lwv[u] : 0.0f;
        const float wn = (a.tail.alpha_neg * w0) * gs, wp = (a.tail.alpha_pos * w0) * gs;
        const float x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
        float t[4], rq[4], lg[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = __builtin_amdgcn_exp2f(__builtin_fminf(x[k], kXMax) * kLog2e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float sk = 1.0f + t[k];
            rq[k] = __builtin_amdgcn_rcpf(sk);
            lg[k] = __builtin_amdgcn_logf(sk);
        }
        // every element in its negative form first (no per-element select: the forward kernel is
        // VALU-bound -- 3 transcendentals + the plain operations of an element are ~60 us of
        // issue time at batch 4, against 41 us of HBM time); the one positive element of a
        // positive anchor (0.1 % of the anchors) is corrected after, under a rare branch
        float o4[4], acc = 0.0f, fix = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            Sig g; g.q = rq[k]; g.lg = lg[k]; g.p = t[k] * rq[k];
            if (BWD) o4[k] = neg_der(g) * wn;
            else acc += neg_val2(g);
        }
        const int jp = lab - 1 - 4 * cq[u];                 // the positive class's slot in this quad
        if (jp >= 0 && jp < 4) {
            float iw = 1.0f;
            if constexpr (BAL_CLS) {
                // the chunk's (pixel, anchor) once more (not kept across the loads above), then the
                // anchor's deltas and target as the box kernel reads them; a clamped chunk weighs 0
                const int rr = r0 + (int)threadIdx.x + 256 * u;
                const int dpx = (int)(((float)rr + 0.5f) * inv_ac4);
                const int an = (int)(((float)(rr - dpx * AC4) + 0.5f) * inv_c4);
                const int64_t pix = pix0 + dpx;
                iw = 0.0f;
                if (on[u]) {
                    const float4 d4 = *reinterpret_cast<const float4 *>(
                        static_cast<const float *>(a.bal.reg[l]) + pix * a.bal.ps_reg[l] + 4 * an);
                    const float dp[4] = {d4.x, d4.y, d4.z, d4.w};
                    iw = bal_weight(a.bal, l, an, (int)(pix % HW), a.lv.W[l], a.lv.stride[l], dp,
                                    reinterpret_cast<const float4 *>(a.bal.bt[l])[pix * A + an]);
                    if (BWD) iw *= a.tail.res[3 * a.lv.L + 4 + l];          // norm_l of the forward call
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k == jp) {
                    Sig g; g.q = rq[k]; g.lg = lg[k]; g.p = t[k] * rq[k];
                    if (BWD) {
                        const float d = pos_der(g, __builtin_fminf(x[k], kXMax)) * wp;
                        o4[k] = BAL_CLS ? d * iw : d;
                    } else {
                        acc -= neg_val2(g);
                        fix = pos_val(g, __builtin_fminf(x[k], kXMax)) * wp;
                        if constexpr (BAL_CLS) { s1 += (double)fix; s2 += (double)(fix * iw); fix = 0.0f; }
                    }
                }
        }
        if (!BWD && a.tail.big_logits) {                         // exact tail, on request (wave-uniform)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x[k] > kXMax && k != jp) fix += (x[k] - kXMax) * wn;
        }
        if (BWD) {
            if constexpr (sizeof(T) == 4) {
                if (on[u]) *reinterpret_cast<float4 *>(static_cast<float *>(a.grad[l]) + goff[u]) = make_float4(o4[0], o4[1], o4[2], o4[3]);
            } else {
                if (on[u]) *reinterpret_cast<uint2 *>(static_cast<uint16_t *>(a.grad[l]) + goff[u]) =
                    make_uint2(f32_to_bf16(o4[0]) | (f32_to_bf16(o4[1]) << 16), f32_to_bf16(o4[2]) | (f32_to_bf16(o4[3]) << 16));
            }
        } else total += (double)__builtin_fmaf(acc * kLn2, wn, fix);
    }
    if (!BWD) {
        const double d = wave_sum(total);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
        __syncthreads();
        if (threadIdx.x == 0)
            atomicAdd(a.tail.sums + (size_t)(0 * a.lv.L + l) * IA_LOSS_SLOTS + (blockIdx.x & kSlotMask),
                      (red[0] + red[1]) + (red[2] + red[3]));
        if constexpr (BAL_CLS) bal_wave_sums(a.tail.sums, a.lv.L, l, s1, s2);
    }
}

struct BoxNhwcArgs {
    NhwcLevels lv;
    BaseAnchors ba;
    const float *reg[IA_MAX_LEVELS], *iou[IA_MAX_LEVELS];
    int64_t ps_reg[IA_MAX_LEVELS], ps_iou[IA_MAX_LEVELS], pg_reg[IA_MAX_LEVELS], pg_iou[IA_MAX_LEVELS];
    BoxTail tail;
    int32_t g_pad[IA_MAX_LEVELS];         // bwd: zero-gradient channels behind d(iou) in the same pixel row
};

struct BoxNhwcBl1Args : BoxNhwcArgs { BalL1 bl; };
// the LOC = 0 launches pass the base part of one such block (launch_box_ml / launch_box_nhwc): the base must
// sit at the block's front with the constants behind it
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"   // single inheritance: a base at offset 0, asserted here
static_assert(offsetof(BoxMLBl1Args, bl) >= sizeof(BoxMLArgs), "the constants ride behind the smooth-L1 block");
static_assert(offsetof(BoxNhwcBl1Args, bl) >= sizeof(BoxNhwcArgs), "the constants ride behind the smooth-L1 block");
#pragma clang diagnostic pop

template <bool BWD, bool IOU, bool BAL_LOC = false, int LOC = 0>
__global__ void __launch_bounds__(256) k_box_nhwc(typename BoxSel<LOC>::Nhwc a)
{
    int o = 0;
    while ((int)blockIdx.x >= a.lv.bblk_off[o + 1]) ++o;
    const int l = a.lv.L - 1 - o;
    const int A = a.lv.A, W = a.lv.W[l];
    const int64_t HW = (int64_t)a.lv.H[l] * W, N = (int64_t)a.lv.B * HW * A;
    const int64_t n = (int64_t)(blockIdx.x - a.lv.bblk_off[o]) * 256 + threadIdx.x;   // (b, p, a)
    double acc_l1 = 0.0, acc_iou = 0.0;
    if (n < N) {
        const int64_t pix = n / A;
        const int an = (int)(n - pix * A);
        const int p = (int)(pix % HW);
        const float4 wt4 = reinterpret_cast<const float4 *>(a.tail.bw[l])[n];
        const float wv[4] = {wt4.x, wt4.y, wt4.z, wt4.w};
        const bool live = (wv[0] != 0.0f) | (wv[1] != 0.0f) | (wv[2] != 0.0f) | (wv[3] != 0.0f);
        float g_box[4] = {0.0f, 0.0f, 0.0f, 0.0f}, g_iou = 0.0f;
        if (live) {
            const float4 d4 = *reinterpret_cast<const float4 *>(a.reg[l] + pix * a.ps_reg[l] + 4 * an);
            const float dp[4] = {d4.x, d4.y, d4.z, d4.w};
            const float4 tq = reinterpret_cast<const float4 *>(a.tail.bt[l])[n];
            const float dt[4] = {tq.x, tq.y, tq.z, tq.w};
            const float xl = IOU ? a.iou[l][pix * a.ps_iou[l] + an] : 0.0f;
            box_elem<BWD, IOU, BAL_LOC, LOC>(a.tail, loc_consts<LOC>(a), a.ba, a.lv.L, l, an, p, W, a.lv.stride[l], wv, dp, dt,
                                             xl, acc_l1, acc_iou, g_box, g_iou);
        }
        if (BWD) {
            *reinterpret_cast<float4 *>(a.tail.g_reg[l] + pix * a.pg_reg[l] + 4 * an) =
                make_float4(g_box[0], g_box[1], g_box[2], g_box[3]);
            if constexpr (IOU) {
                a.tail.g_iou[l][pix * a.pg_iou[l] + an] = g_iou;
                // d(reg) | d(iou) as slices of one wider tensor: its alignment channels behind the IoU
                // slice get their zero gradient here (the last anchor's thread), not from a fill per level
                if (an == A - 1)
                    for (int k = 0; k < a.g_pad[l]; ++k) a.tail.g_iou[l][pix * a.pg_iou[l] + A + k] = 0.0f;
            } else {
                // no IoU slice: the row is [reg 4A | padding], zeroed behind the reg slice
                if (an == A - 1)
                    for (int k = 0; k < a.g_pad[l]; ++k) a.tail.g_reg[l][pix * a.pg_reg[l] + 4 * A + k] = 0.0f;
            }
        }
    }
    if (!BWD) box_block_reduce<IOU>(a.tail.sums, a.lv.L, l, acc_l1, acc_iou);
}

// ------------------------------------------------------------------ slots -> losses
struct FinArgs {
    const double *sums;
    const int32_t *counts;                // (B, 2) from ia_anchor_targets, or NULL
    const float *avg_dev;                 // device scalar, or NULL
    float avg_host;
    float lw[kNumLoss];
    int32_t L, B;
    float *res;                           // 3L + 4 (+ L: norm_l, balanced_cls)
    int32_t bal_cls;                      // loss_cls[l] = lw * (S0 + norm_l * S2) / avg, norm_l = S1 / (S2 + 1e-6)
};

__global__ void __launch_bounds__(64) k_headloss_finalize(FinArgs a)
{
    __shared__ float s_loss[kNumLoss * IA_MAX_LEVELS];
    float avg = a.avg_host;
    if (a.counts) {                       // sum_i max(n_pos_i, 1)   (anchor_target.py:94)
        int tot = 0;
        for (int b = 0; b < a.B; ++b) tot += (a.counts[2 * b] > 1) ? a.counts[2 * b] : 1;
        avg = (float)tot;
    } else if (a.avg_dev) avg = a.avg_dev[0];
    const int i = threadIdx.x;
    if (i < kNumLoss * a.L) {
        double s = 0.0;
        for (int k = 0; k < IA_LOSS_SLOTS; ++k) s += a.sums[(size_t)i * IA_LOSS_SLOTS + k];
        float sv = (float)s;
        if (a.bal_cls && i < a.L) {
            // iou_balanced_sigmoid_focal_loss (losses.py:363-374) in fp32 like the per-level route
            // (ops._FocalBalancedFn): the class row is S0; a level without positives has S1 = S2 = 0,
            // norm_l = 0 and loss = lw * S0 / avg
            double d1 = 0.0, d2 = 0.0;
            for (int k = 0; k < IA_LOSS_SLOTS; ++k) {
                d1 += a.sums[(size_t)(kNumLoss * a.L + i) * IA_LOSS_SLOTS + k];
                d2 += a.sums[(size_t)((kNumLoss + 1) * a.L + i) * IA_LOSS_SLOTS + k];
            }
            const float S1 = (float)d1, S2 = (float)d2;
            const float norm = S1 / (S2 + 1e-6f);
            sv = sv + norm * S2;
            a.res[kNumLoss * a.L + kNumLoss + 1 + i] = norm;
        }
        // weighted_*: sum()[None] / avg_factor, then * loss_weight (losses.py:303,411,480)
        const float v = a.lw[i / a.L] * (sv / avg);
        s_loss[i] = v;
        a.res[i] = v;
    }
    __syncthreads();
    if (i < kNumLoss) {                   // parse_losses: sum over the levels, in level order
        float t = 0.0f;
        for (int l = 0; l < a.L; ++l) t += s_loss[i * a.L + l];
        a.res[kNumLoss * a.L + i] = t;
    }
    if (i == 0) a.res[kNumLoss * a.L + kNumLoss] = avg;
}

// ------------------------------------------------------------------ host: checks and arguments
// the two kinds the node covers: sigmoid focal loss with (IoU-aware head) or without (plain
// RetinaHead) the IoU term; the softmax kinds have no fused loss
static bool sigmoid_kind(const ia_head_geom *g)
{
    return g->cls_activation == IA_CLS_SIGMOID || g->cls_activation == IA_CLS_SIGMOID_NOIOU;
}
// IoU maps (head outputs or gradients): all present with the IoU-aware kind, all NULL without it
static bool iou_ptrs_ok(const ia_level_ptrs *p, int L, bool with_iou)
{
    for (int l = 0; l < L; ++l)
        if ((p->iou[l] != nullptr) != with_iou) return false;
    return true;
}

// the geometry step of both level tables (HLLevels, NhwcLevels): ranges, kind, H / W / stride
template <class LV>
static int level_geometry(const ia_head_geom *g, int B, LV &lv)
{
    if (!g || B < 1) return IA_E_ARG;
    if (g->num_levels < 1 || g->num_levels > IA_MAX_LEVELS) return IA_E_ARG;
    if (g->num_anchors < 1 || g->num_anchors > IA_MAX_ANCHORS || g->num_classes < 1) return IA_E_ARG;
    if (!sigmoid_kind(g)) return IA_E_ARG;                       // sigmoid focal loss only
    lv.L = g->num_levels; lv.B = B; lv.A = g->num_anchors; lv.C = g->num_classes;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        const bool on = l < lv.L;
        if (on && (g->H[l] < 1 || g->W[l] < 1)) return IA_E_ARG;
        lv.H[l] = on ? g->H[l] : 0; lv.W[l] = on ? g->W[l] : 0; lv.stride[l] = on ? g->stride[l] : 0;
    }
    return 0;
}

int fill_levels(const ia_head_geom *g, int B, HLLevels &lv)
{
    const int rc = level_geometry(g, B, lv);
    if (rc) return rc;
    if (g->layout != IA_LAYOUT_NCHW) return IA_E_ARG;            // training kernels: NCHW only
    int64_t off = 0, foff = 0, poff = 0;
    lv.blk_off[0] = lv.fblk_off[0] = 0;
    for (int l = 0; l <= IA_MAX_LEVELS; ++l) {
        lv.pack_off[l] = (int32_t)poff;
        if (l < lv.L) poff += (int64_t)B * lv.A * lv.H[l] * lv.W[l];
        if (poff > 2147483647LL) return IA_E_ARG;
    }
    for (int l = 0; l < IA_MAX_LEVELS; ++l) { lv.csplit[l] = 1; lv.cchunk[l] = lv.C; }
    for (int o = 0; o < IA_MAX_LEVELS; ++o) {
        if (o < lv.L) {
            const int l = lv.L - 1 - o;
            const int64_t blocks = (int64_t)B * lv.A * (((int64_t)lv.H[l] * lv.W[l] + 255) / 256);
            // >= ~4 wavefronts per SIMD per level, chunks of whole 8-class load groups (MI355X,
            // B = 4: target 1 / 1024 / 2048 / 4096 wavefronts -> fwd 51.9 / 53.3 / 55.6 / 52.5 us,
            // bwd 110.9 / 112.2 / 112.2 / 108.2 us)
            int split = (int)((kFocalLevelWaves + blocks - 1) / blocks);   // blocks = wavefronts of the level
            if (split > (lv.C + 7) / 8) split = (lv.C + 7) / 8;
            if (split < 1) split = 1;
            lv.cchunk[l] = ((lv.C + split - 1) / split + 7) / 8 * 8;
            lv.csplit[l] = (lv.C + lv.cchunk[l] - 1) / lv.cchunk[l];
            off += blocks;
            foff += blocks * lv.csplit[l];
            if (foff > 2147483647LL) return IA_E_ARG;
        }
        lv.blk_off[o + 1] = (int32_t)off;
        lv.fblk_off[o + 1] = (int32_t)foff;
    }
    return 0;
}

int fill_levels_nhwc(const ia_head_geom *g, int B, NhwcLevels &lv)
{
    const int rc = level_geometry(g, B, lv);
    if (rc) return rc;
    if (lv.C & 3) return IA_E_ARG;                               // class quads: C % 4 == 0
    if ((int64_t)lv.A * (lv.C / 4) > 8192) return IA_E_ARG;      // float-reciprocal division
    int64_t foff = 0, boff = 0;
    lv.fblk_off[0] = lv.bblk_off[0] = 0;
    for (int o = 0; o < IA_MAX_LEVELS; ++o) {
        if (o < lv.L) {
            const int l = lv.L - 1 - o;
            const int64_t anchors = (int64_t)B * lv.H[l] * lv.W[l] * lv.A;
            foff += (anchors * (lv.C / 4) + kFocalChunks - 1) / kFocalChunks;
            boff += (anchors + 255) / 256;
            if (foff > 2147483647LL || boff > 2147483647LL) return IA_E_ARG;
        }
        lv.fblk_off[o + 1] = (int32_t)foff;
        lv.bblk_off[o + 1] = (int32_t)boff;
    }
    return 0;
}

static int check_strides(const NhwcLevels &lv, const ia_level_pix_strides *st, const ia_level_ptrs *p,
                         bool with_iou)
{
    for (int l = 0; l < lv.L; ++l) {
        if (st->cls[l] < (int64_t)lv.A * lv.C || st->reg[l] < (int64_t)lv.A * 4) return IA_E_ARG;
        if ((st->cls[l] & 3) || (st->reg[l] & 3)) return IA_E_ARG;          // 16-byte pieces
        if (((uintptr_t)p->cls[l] & 15u) || ((uintptr_t)p->reg[l] & 15u)) return IA_E_ARG;
        // the IoU strides are not looked at without the branch
        if (with_iou && (st->iou[l] < lv.A || ((uintptr_t)p->iou[l] & 3u))) return IA_E_ARG;
    }
    return 0;
}

// What the four entries check alike, after the geometry (g is valid).  Backward is forward plus
// the gradient pointers: grads / grad_result are NULL in a forward call.
static int check_common(const ia_head_geom *g, const ia_level_ptrs *p, const ia_head_targets *t,
                        const ia_head_loss_cfg *cfg, const float *result, bool bwd,
                        const float *grad_result, const ia_level_ptrs *grads, bool &with_iou)
{
    if (!p || !t || !cfg || !result || (bwd && (!grad_result || !grads))) return IA_E_ARG;
    if (cfg->gamma != 2.0f || !(cfg->beta > 0.0f)) return IA_E_ARG;      // other gammas: per-level path
    const int L = g->num_levels;
    with_iou = g->cls_activation == IA_CLS_SIGMOID;
    // the IoU-balanced losses weigh by the IoU target: the IoU-aware kind only, positive exponents
    if ((cfg->balanced_cls || cfg->balanced_loc) && !with_iou) return IA_E_ARG;
    if ((cfg->balanced_cls && !(cfg->eta > 0.0f)) || (cfg->balanced_loc && !(cfg->delta > 0.0f))) return IA_E_ARG;
    if (!iou_ptrs_ok(p, L, with_iou) || (bwd && !iou_ptrs_ok(grads, L, with_iou))) return IA_E_ARG;
    for (int l = 0; l < L; ++l) {
        if (!p->cls[l] || !p->reg[l] || !t->labels[l] || !t->label_weights[l] ||
            !t->bbox_targets[l] || !t->bbox_weights[l])
            return IA_E_ARG;
        if (bwd && (!grads->cls[l] || !grads->reg[l])) return IA_E_ARG;
    }
    return 0;
}
// forward: the normaliser comes from the assignment's counts, a device scalar or the host
static bool normaliser_ok(const ia_head_targets *t)
{
    return t->counts || t->avg_factor_dev || t->avg_factor > 0.0f;
}

FocalTail focal_tail(float alpha, float loss_weight, bool exact_large_logits, double *sums,
                     const float *gin, const float *res)
{
    FocalTail f;
    f.sums = sums; f.gin = gin; f.res = res;
    f.alpha_pos = alpha;
    f.alpha_neg = (float)(1.0 - (double)alpha);   // python: (1 - alpha) in double, then fp32
    f.loss_weight = loss_weight;
    f.big_logits = exact_large_logits ? 1 : 0;
    return f;
}
// grads is NULL in a forward call
static void fill_box_tail(BoxTail &b, BaseAnchors &ba, const ia_head_geom *g, const ia_head_targets *t,
                          const ia_head_loss_cfg *cfg, const ia_level_ptrs *grads, double *sums,
                          const float *gin, const float *res)
{
    memcpy(ba.v, g->base_anchors, sizeof(ba.v));
        for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        const bool on = l < g->num_levels;
        b.bt[l] = on ? t->bbox_targets[l] : nullptr; b.bw[l] = on ? t->bbox_weights[l] : nullptr;
        b.g_reg[l] = (on && grads) ? (float *)grads->reg[l] : nullptr;
        b.g_iou[l] = (on && grads) ? (float *)grads->iou[l] : nullptr;
    }
    b.sums = sums; b.gin = gin; b.res = res;
    for (int k = 0; k < 4; ++k) { b.means[k] = g->means[k]; b.stds[k] = g->stds[k]; }
    b.beta = cfg->beta; b.lw_bbox = cfg->loss_weight_bbox; b.lw_iou = 1.0f;
    b.attach = cfg->attach_iou_target ? 1 : 0;
    b.delta = cfg->delta;
}
// the balanced focal kernels' extra block; st is NULL for the NCHW kernels
static void fill_focal_bal(FocalBal &f, const ia_head_geom *g, const ia_level_ptrs *p, const ia_head_targets *t,
                           const ia_head_loss_cfg *cfg, const ia_level_pix_strides *st)
{
    memcpy(f.ba.v, g->base_anchors, sizeof(f.ba.v));
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        const bool on = l < g->num_levels;
        f.reg[l] = on ? p->reg[l] : nullptr; f.bt[l] = on ? t->bbox_targets[l] : nullptr;
        f.ps_reg[l] = (on && st) ? st->reg[l] : 0;
    }
    for (int k = 0; k < 4; ++k) { f.means[k] = g->means[k]; f.stds[k] = g->stds[k]; }
    f.eta = cfg->eta;
}

// the workspace of the NCHW entries: fp64 slots | packed labels (int32) | packed weights (fp32),
// 256-byte aligned pieces; the channels-last entries use the slots alone
struct HLWorkspace { double *sums; int32_t *lab_am; float *w_am; size_t bytes; };
// (balanced_cls: two more slot rows per level, S1 and S2, behind the three losses')
static size_t slot_bytes(int L, bool bal_cls)
{
    return sizeof(double) * (kNumLoss + (bal_cls ? 2 : 0)) * (size_t)L * IA_LOSS_SLOTS;
}
static HLWorkspace carve(const HLLevels &lv, const void *workspace, bool bal_cls)
{
    const size_t slots = align256(slot_bytes(lv.L, bal_cls));
    const size_t pk = align256((size_t)lv.pack_off[lv.L] * 4);
    char *w = static_cast<char *>(const_cast<void *>(workspace));
    HLWorkspace r;
    r.sums = reinterpret_cast<double *>(w);
    r.lab_am = reinterpret_cast<int32_t *>(w + slots);
    r.w_am = reinterpret_cast<float *>(w + slots + pk);
    r.bytes = slots + 2 * pk;
    return r;
}

// NCHW: what forward and backward check alike, and every kernel argument (backward reads the
// forward call's packed targets from the same workspace)
static int ml_loss_args(const ia_head_geom *g, const ia_level_ptrs *p, int dtype, int batch,
                        const ia_head_targets *t, const ia_head_loss_cfg *cfg, const void *workspace,
                        const float *result, bool bwd, const float *grad_result,
                        const ia_level_ptrs *grads, FocalMLBalArgs &fa, BoxMLArgs &ba, HLWorkspace &ws,
                        bool &with_iou)
{
    if (!workspace || (dtype != IA_F32 && dtype != IA_BF16)) return IA_E_ARG;
    int rc = fill_levels(g, batch, fa.lv);
    if (rc || (rc = check_common(g, p, t, cfg, result, bwd, grad_result, grads, with_iou))) return rc;
    ws = carve(fa.lv, workspace, cfg->balanced_cls != 0);
    if (cfg->balanced_cls) fill_focal_bal(fa.bal, g, p, t, cfg, nullptr);
    ba.lv = fa.lv;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        const bool on = l < fa.lv.L;
        fa.cls[l] = on ? p->cls[l] : nullptr;
        fa.grad[l] = (on && bwd) ? (float *)grads->cls[l] : nullptr;
        ba.reg[l] = on ? p->reg[l] : nullptr; ba.iou[l] = on ? p->iou[l] : nullptr;
    }
    fa.lab_am = ws.lab_am; fa.w_am = ws.w_am;
    double *sums = bwd ? nullptr : ws.sums;
    fa.tail = focal_tail(cfg->alpha, cfg->loss_weight_cls, !bwd && cfg->exact_large_logits, sums, grad_result,
                         bwd ? result : nullptr);
    fill_box_tail(ba.tail, ba.ba, g, t, cfg, grads, sums, grad_result, bwd ? result : nullptr);
    return 0;
}

// channels-last: the same, plus the pixel strides and the zero-gradient channels of a shared row
static int nhwc_loss_args(const ia_head_geom *g, const ia_level_ptrs *p,
                          const ia_level_pix_strides *strides, int batch, const ia_head_targets *t,
                          const ia_head_loss_cfg *cfg, double *sums, const float *result, bool bwd,
                          const float *grad_result, const ia_level_ptrs *grads,
                          const ia_level_pix_strides *grad_strides, FocalNhwcBalArgs &fa,
                          BoxNhwcArgs &ba, bool &with_iou)
{
    if (!strides || (bwd && !grad_strides)) return IA_E_ARG;
    int rc = fill_levels_nhwc(g, batch, fa.lv);
    if (rc || (rc = check_common(g, p, t, cfg, result, bwd, grad_result, grads, with_iou))) return rc;
    if ((rc = check_strides(fa.lv, strides, p, with_iou)) ||
        (bwd && (rc = check_strides(fa.lv, grad_strides, grads, with_iou))))
        return rc;
    if (cfg->balanced_cls) fill_focal_bal(fa.bal, g, p, t, cfg, strides);
    ba.lv = fa.lv;
    fa.tail = focal_tail(cfg->alpha, cfg->loss_weight_cls, !bwd && cfg->exact_large_logits, sums, grad_result,
                         bwd ? result : nullptr);
    fill_box_tail(ba.tail, ba.ba, g, t, cfg, grads, sums, grad_result, bwd ? result : nullptr);
    const int A = fa.lv.A;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        const bool on = l < fa.lv.L, gon = on && bwd;
        fa.cls[l] = on ? p->cls[l] : nullptr;
        fa.ps_cls[l] = on ? strides->cls[l] : 0;
        fa.grad[l] = gon ? const_cast<void *>(grads->cls[l]) : nullptr;
        fa.ps_grad[l] = gon ? grad_strides->cls[l] : 0;
        fa.labels[l] = on ? t->labels[l] : nullptr; fa.lw[l] = on ? t->label_weights[l] : nullptr;
        ba.reg[l] = on ? (const float *)p->reg[l] : nullptr; ba.iou[l] = on ? (const float *)p->iou[l] : nullptr;
        ba.ps_reg[l] = on ? strides->reg[l] : 0; ba.ps_iou[l] = (on && with_iou) ? strides->iou[l] : 0;
        ba.pg_reg[l] = gon ? grad_strides->reg[l] : 0; ba.pg_iou[l] = (gon && with_iou) ? grad_strides->iou[l] : 0;
        // both gradients in one pixel row that STARTS at reg (the caller says so: cfg->grad_rows_start_at_reg;
        // a row [X | reg | iou | pad] looks the same from here, and zero-filling behind iou would run into the
        // next pixel's X): the channels left up to the row's end get their zero gradient here
        ba.g_pad[l] = 0;
        if (gon && cfg->grad_rows_start_at_reg && with_iou) {
            if (ba.tail.g_iou[l] != ba.tail.g_reg[l] + 4 * A || ba.pg_reg[l] != ba.pg_iou[l] ||
                ba.pg_reg[l] < 5 * A || ba.pg_reg[l] - 5 * A > 64)
                return IA_E_ARG;
            ba.g_pad[l] = (int32_t)(ba.pg_reg[l] - 5 * A);
        } else if (gon && cfg->grad_rows_start_at_reg) {
            // without the IoU slice the row is [reg 4A | padding]
            if (ba.pg_reg[l] - 4 * A > 64) return IA_E_ARG;                 // (>= 4A: check_strides)
            ba.g_pad[l] = (int32_t)(ba.pg_reg[l] - 4 * A);
        }
    }
    return 0;
}

// ------------------------------------------------------------------ host: launches
// the instantiation switches: [dtype == IA_BF16][bwd] and [..][bwd][kind], kind = no IoU term / IoU
// term / IoU term + balanced smooth-L1 (the balanced losses exist with the IoU term only: check_common)
static int launch_focal_ml(int dtype, bool bwd, const FocalMLArgs &fa, hipStream_t s)
{
    static void (*const k[2][2])(FocalMLArgs) = {{k_focal_ml<float, false>, k_focal_ml<float, true>},
                                                 {k_focal_ml<uint16_t, false>, k_focal_ml<uint16_t, true>}};
    hipLaunchKernelGGL(k[dtype == IA_BF16][bwd], dim3((unsigned)fa.lv.fblk_off[fa.lv.L]), dim3(64), 0, s, fa);
    return hip_status(hipGetLastError());
}
int launch_focal_ml_f32(const FocalMLArgs &fa, bool bwd, hipStream_t s) { return launch_focal_ml(IA_F32, bwd, fa, s); }
// bal_cls: the IoU-balanced instances on the whole block; else the plain ones on its plain part
static int launch_focal_ml(int dtype, bool bwd, bool bal_cls, const FocalMLBalArgs &fa, hipStream_t s)
{
    if (!bal_cls) return launch_focal_ml(dtype, bwd, static_cast<const FocalMLArgs &>(fa), s);
    static void (*const k[2][2])(FocalMLBalArgs) = {
        {k_focal_ml<float, false, true>, k_focal_ml<float, true, true>},
        {k_focal_ml<uint16_t, false, true>, k_focal_ml<uint16_t, true, true>}};
    hipLaunchKernelGGL(k[dtype == IA_BF16][bwd], dim3((unsigned)fa.lv.fblk_off[fa.lv.L]), dim3(64), 0, s, fa);
    return hip_status(hipGetLastError());
}
static int launch_focal_nhwc(bool bwd, bool bal_cls, const FocalNhwcBalArgs &fa, hipStream_t s)
{
    const dim3 grid((unsigned)fa.lv.fblk_off[fa.lv.L]);
    if (!bal_cls) {
        const FocalNhwcArgs &f = fa;
        if (bwd) hipLaunchKernelGGL((k_focal_nhwc<true, float, false>), grid, dim3(256), 0, s, f);
        else hipLaunchKernelGGL((k_focal_nhwc<false, float, false>), grid, dim3(256), 0, s, f);
    } else if (bwd) hipLaunchKernelGGL((k_focal_nhwc<true, float, false, true>), grid, dim3(256), 0, s, fa);
    else hipLaunchKernelGGL((k_focal_nhwc<false, float, false, true>), grid, dim3(256), 0, s, fa);
    return hip_status(hipGetLastError());
}
static int box_kind(bool with_iou, const ia_head_loss_cfg *cfg) { return with_iou ? (cfg->balanced_loc ? 2 : 1) : 0; }
static int launch_box_ml(int dtype, bool bwd, int kind, const BoxMLArgs &ba, hipStream_t s)
{
    static void (*const k[2][2][3])(BoxMLArgs) = {
        {{k_box_ml<float, false, false>, k_box_ml<float, false, true>, k_box_ml<float, false, true, true>},
         {k_box_ml<float, true, false>, k_box_ml<float, true, true>, k_box_ml<float, true, true, true>}},
        {{k_box_ml<uint16_t, false, false>, k_box_ml<uint16_t, false, true>, k_box_ml<uint16_t, false, true, true>},
         {k_box_ml<uint16_t, true, false>, k_box_ml<uint16_t, true, true>, k_box_ml<uint16_t, true, true, true>}}};
    hipLaunchKernelGGL(k[dtype == IA_BF16][bwd][kind], dim3((unsigned)ba.lv.blk_off[ba.lv.L]), dim3(256), 0, s, ba);
    return hip_status(hipGetLastError());
}
static int launch_box_nhwc(bool bwd, int kind, const BoxNhwcArgs &ba, hipStream_t s)
{
    static void (*const k[2][3])(BoxNhwcArgs) = {
        {k_box_nhwc<false, false>, k_box_nhwc<false, true>, k_box_nhwc<false, true, true>},
        {k_box_nhwc<true, false>, k_box_nhwc<true, true>, k_box_nhwc<true, true, true>}};
    hipLaunchKernelGGL(k[bwd][kind], dim3((unsigned)ba.lv.bblk_off[ba.lv.L]), dim3(256), 0, s, ba);
    return hip_status(hipGetLastError());
}
// bl1: the balanced-L1 instances (kind 0 / 1) on the whole block; else the smooth-L1 ones on its front part
static int launch_box_ml(int dtype, bool bwd, int kind, bool bl1, const BoxMLBl1Args &ba, hipStream_t s)
{
    if (bl1) {
        static void (*const k[2][2][2])(BoxMLBl1Args) = {
            {{k_box_ml<float, false, false, false, 1>, k_box_ml<float, false, true, false, 1>},
             {k_box_ml<float, true, false, false, 1>, k_box_ml<float, true, true, false, 1>}},
            {{k_box_ml<uint16_t, false, false, false, 1>, k_box_ml<uint16_t, false, true, false, 1>},
             {k_box_ml<uint16_t, true, false, false, 1>, k_box_ml<uint16_t, true, true, false, 1>}}};
        hipLaunchKernelGGL(k[dtype == IA_BF16][bwd][kind], dim3((unsigned)ba.lv.blk_off[ba.lv.L]), dim3(256), 0, s, ba);
        return hip_status(hipGetLastError());
    }
    return launch_box_ml(dtype, bwd, kind, static_cast<const BoxMLArgs &>(ba), s);
}
static int launch_box_nhwc(bool bwd, int kind, bool bl1, const BoxNhwcBl1Args &ba, hipStream_t s)
{
    if (bl1) {
        static void (*const k[2][2])(BoxNhwcBl1Args) = {
            {k_box_nhwc<false, false, false, 1>, k_box_nhwc<false, true, false, 1>},
            {k_box_nhwc<true, false, false, 1>, k_box_nhwc<true, true, false, 1>}};
        hipLaunchKernelGGL(k[bwd][kind], dim3((unsigned)ba.lv.bblk_off[ba.lv.L]), dim3(256), 0, s, ba);
        return hip_status(hipGetLastError());
    }
    return launch_box_nhwc(bwd, kind, static_cast<const BoxNhwcArgs &>(ba), s);
}
// ia_box_loss_cfg -> bl1 and the kernels' constants.  NULL / IA_BOX_SMOOTH_L1: the smooth-L1 of cfg alone.
static int box_loss_consts(const ia_box_loss_cfg *box, const ia_head_loss_cfg *cfg, bool &bl1, BalL1 &bl)
{
    bl1 = false;
    if (!box) return 0;
    if (box->struct_size != (int32_t)sizeof(ia_box_loss_cfg)) return IA_E_ARG;
    if (box->kind == IA_BOX_SMOOTH_L1) return 0;
    if (box->kind != IA_BOX_BALANCED_L1 || !cfg || cfg->balanced_loc) return IA_E_ARG;
    if (!balanced_l1_consts(box->alpha, box->gamma, cfg->beta, bl)) return IA_E_ARG;
    bl1 = true;
    return 0;
}
int launch_focal_nhwc_unit(const FocalNhwcArgs &fa, int dtype, bool bwd, hipStream_t s)
{
    static void (*const k[2][2])(FocalNhwcArgs) = {
        {k_focal_nhwc<false, float, true>, k_focal_nhwc<true, float, true>},
        {k_focal_nhwc<false, uint16_t, true>, k_focal_nhwc<true, uint16_t, true>}};
    hipLaunchKernelGGL(k[dtype == IA_BF16][bwd], dim3((unsigned)fa.lv.fblk_off[fa.lv.L]), dim3(256), 0, s, fa);
    return hip_status(hipGetLastError());
}
static int launch_finalize(const double *sums, const ia_head_targets *t, const ia_head_loss_cfg *cfg,
                           int L, int batch, float *result, hipStream_t s)
{
    FinArgs f;
    f.sums = sums; f.counts = t->counts; f.avg_dev = t->avg_factor_dev; f.avg_host = t->avg_factor;
    f.lw[0] = cfg->loss_weight_cls; f.lw[1] = cfg->loss_weight_bbox; f.lw[2] = 1.0f;
    f.L = L; f.B = batch; f.res = result; f.bal_cls = cfg->balanced_cls ? 1 : 0;
    hipLaunchKernelGGL(k_headloss_finalize, dim3(1), dim3(64), 0, s, f);
    return hip_status(hipGetLastError());
}

}  // namespace ia

extern "C" {

size_t ia_head_loss_workspace_bytes(const ia_head_geom *g, int batch)
{
    ia::HLLevels lv;
    if (ia::fill_levels(g, batch, lv)) return 0;
    return ia::carve(lv, nullptr, false).bytes;
}

size_t ia_head_loss_workspace_bytes_cfg(const ia_head_geom *g, int batch, const ia_head_loss_cfg *cfg)
{
    ia::HLLevels lv;
    if (!cfg || ia::fill_levels(g, batch, lv)) return 0;
    return ia::carve(lv, nullptr, cfg->balanced_cls != 0).bytes;
}

int ia_head_loss_fwd(const ia_head_geom *g, const ia_level_ptrs *p, int dtype, int batch,
                     const ia_head_targets *t, const ia_head_loss_cfg *cfg, void *workspace,
                     size_t workspace_bytes, float *result, void *stream)
{
    return ia_head_loss_fwd_box(g, p, dtype, batch, t, cfg, nullptr, workspace, workspace_bytes, result, stream);
}

int ia_head_loss_fwd_box(const ia_head_geom *g, const ia_level_ptrs *p, int dtype, int batch,
                         const ia_head_targets *t, const ia_head_loss_cfg *cfg, const ia_box_loss_cfg *box,
                         void *workspace, size_t workspace_bytes, float *result, void *stream)
{
    using namespace ia;
    if ((uintptr_t)workspace & 255u) return IA_E_ARG;
    FocalMLBalArgs fa;
    BoxMLBl1Args ba;
    HLWorkspace ws;
    bool with_iou, bl1;
    int rc = box_loss_consts(box, cfg, bl1, ba.bl);
    if (rc) return rc;
    rc = ml_loss_args(g, p, dtype, batch, t, cfg, workspace, result, false, nullptr, nullptr, fa, ba,
                          ws, with_iou);
    if (rc) return rc;
    const bool bal_cls = cfg->balanced_cls != 0;
    // (a balanced call is sized by ia_head_loss_workspace_bytes_cfg: the plain size is a wrong argument)
    if (workspace_bytes < ws.bytes) return bal_cls ? IA_E_ARG : IA_E_WORKSPACE;
    if (!normaliser_ok(t)) return IA_E_ARG;              // before the first enqueue
    const int L = fa.lv.L;
    PackArgs pa;
    pa.lv = fa.lv;
    pa.lab_am = ws.lab_am; pa.w_am = ws.w_am;
    pa.tile_off[0] = 0;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        const bool on = l < L;
        pa.labels[l] = on ? t->labels[l] : nullptr;
        pa.lw[l] = on ? t->label_weights[l] : nullptr;
        pa.tile_off[l + 1] = pa.tile_off[l] + (on ? batch * ((fa.lv.H[l] * fa.lv.W[l] + 255) / 256) : 0);
    }
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(ws.sums, 0, slot_bytes(L, bal_cls), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_pack_targets, dim3((unsigned)pa.tile_off[L]), dim3(256), 0, s, pa);
    if ((rc = launch_focal_ml(dtype, false, bal_cls, fa, s)) ||
        (rc = launch_box_ml(dtype, false, box_kind(with_iou, cfg), bl1, ba, s)))
        return rc;
    return launch_finalize(ws.sums, t, cfg, L, batch, result, s);
}

int ia_head_loss_bwd(const ia_head_geom *g, const ia_level_ptrs *p, int dtype, int batch,
                     const ia_head_targets *t, const ia_head_loss_cfg *cfg, const void *workspace,
                     const float *result, const float *grad_result, const ia_level_ptrs *grads,
                     void *stream)
{
    return ia_head_loss_bwd_box(g, p, dtype, batch, t, cfg, nullptr, workspace, result, grad_result, grads, stream);
}

int ia_head_loss_bwd_box(const ia_head_geom *g, const ia_level_ptrs *p, int dtype, int batch,
                         const ia_head_targets *t, const ia_head_loss_cfg *cfg, const ia_box_loss_cfg *box,
                         const void *workspace, const float *result, const float *grad_result,
                         const ia_level_ptrs *grads, void *stream)
{
    using namespace ia;
    FocalMLBalArgs fa;
    BoxMLBl1Args ba;
    HLWorkspace ws;
    bool with_iou, bl1;
    int rc = box_loss_consts(box, cfg, bl1, ba.bl);
    if (rc) return rc;
    rc = ml_loss_args(g, p, dtype, batch, t, cfg, workspace, result, true, grad_result, grads, fa, ba,
                          ws, with_iou);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = launch_focal_ml(dtype, true, cfg->balanced_cls != 0, fa, s))) return rc;
    return launch_box_ml(dtype, true, box_kind(with_iou, cfg), bl1, ba, s);
}

int ia_head_loss_fwd_nhwc(const ia_head_geom *g, const ia_level_ptrs *p,
                          const ia_level_pix_strides *strides, int batch, const ia_head_targets *t,
                          const ia_head_loss_cfg *cfg, void *workspace, size_t workspace_bytes,
                          float *result, void *stream)
{
    return ia_head_loss_fwd_nhwc_box(g, p, strides, batch, t, cfg, nullptr, workspace, workspace_bytes, result, stream);
}

int ia_head_loss_fwd_nhwc_box(const ia_head_geom *g, const ia_level_ptrs *p,
                              const ia_level_pix_strides *strides, int batch, const ia_head_targets *t,
                              const ia_head_loss_cfg *cfg, const ia_box_loss_cfg *box, void *workspace,
                              size_t workspace_bytes, float *result, void *stream)
{
    using namespace ia;
    if (!workspace || ((uintptr_t)workspace & 255u)) return IA_E_ARG;
    double *sums = static_cast<double *>(workspace);
    FocalNhwcBalArgs fa;
    BoxNhwcBl1Args ba;
    bool with_iou, bl1;
    int rc = box_loss_consts(box, cfg, bl1, ba.bl);
    if (rc) return rc;
    rc = nhwc_loss_args(g, p, strides, batch, t, cfg, sums, result, false, nullptr, nullptr, nullptr,
                            fa, ba, with_iou);
    if (rc) return rc;
    const int L = fa.lv.L;
    const bool bal_cls = cfg->balanced_cls != 0;
    if (workspace_bytes < slot_bytes(L, bal_cls)) return bal_cls ? IA_E_ARG : IA_E_WORKSPACE;   // as ia_head_loss_fwd
    if (!normaliser_ok(t)) return IA_E_ARG;              // before the first enqueue
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(sums, 0, slot_bytes(L, bal_cls), s);
    if (e != hipSuccess) return (int)e;
    if ((rc = launch_focal_nhwc(false, bal_cls, fa, s)) || (rc = launch_box_nhwc(false, box_kind(with_iou, cfg), bl1, ba, s)))
        return rc;
    return launch_finalize(sums, t, cfg, L, batch, result, s);
}

int ia_head_loss_bwd_nhwc(const ia_head_geom *g, const ia_level_ptrs *p,
                          const ia_level_pix_strides *strides, int batch, const ia_head_targets *t,
                          const ia_head_loss_cfg *cfg, const float *result, const float *grad_result,
                          const ia_level_ptrs *grads, const ia_level_pix_strides *grad_strides,
                          void *stream)
{
    return ia_head_loss_bwd_nhwc_box(g, p, strides, batch, t, cfg, nullptr, result, grad_result, grads, grad_strides,
                                     stream);
}

int ia_head_loss_bwd_nhwc_box(const ia_head_geom *g, const ia_level_ptrs *p,
                              const ia_level_pix_strides *strides, int batch, const ia_head_targets *t,
                              const ia_head_loss_cfg *cfg, const ia_box_loss_cfg *box, const float *result,
                              const float *grad_result, const ia_level_ptrs *grads,
                              const ia_level_pix_strides *grad_strides, void *stream)
{
    using namespace ia;
    FocalNhwcBalArgs fa;
    BoxNhwcBl1Args ba;
    bool with_iou, bl1;
    int rc = box_loss_consts(box, cfg, bl1, ba.bl);
    if (rc) return rc;
    rc = nhwc_loss_args(g, p, strides, batch, t, cfg, nullptr, result, true, grad_result, grads,
                            grad_strides, fa, ba, with_iou);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = launch_focal_nhwc(true, cfg->balanced_cls != 0, fa, s))) return rc;
    return launch_box_nhwc(true, box_kind(with_iou, cfg), bl1, ba, s);
}

}  // extern "C"
