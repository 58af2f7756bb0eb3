// Device helpers shared by the per-level loss kernels (loss.hip) and the all-levels head-loss
// kernels (headloss.hip): wave / block reductions into fp64 slots, the hardware-transcendental
// helpers of the focal kernels, and the exact-math box decode + aligned IoU + BCE element that
// keeps IoU targets and their gradients bit-identical to the oracle
// (reference iou_aware_retina_head.py:256-259,276-281; core/bbox/transforms.py:44-78;
// core/bbox/geometry.py:34-47; core/loss/losses.py:385-411,460-480).
#pragma once
#include <math.h>
#include "ia_internal.hpp"
#include "ia_math.hpp"
#include "ia_block.hpp"

namespace ia {

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// every thread of the workgroup calls; one atomic per workgroup
__device__ __forceinline__ void block_sum_to(double v, double *dst, double *lds /* >= 16 */)
{
    const uint32_t tid = threadIdx.y * blockDim.x + threadIdx.x;
    const uint32_t nw = (blockDim.x * blockDim.y + kWave - 1) / kWave;
    v = wave_sum(v);
    if ((tid & (kWave - 1)) == 0) lds[tid / kWave] = v;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (uint32_t w = 0; w < nw; ++w) s += lds[w];
        atomicAdd(dst + (blockIdx.x & (IA_LOSS_SLOTS - 1)), s);   // IA_LOSS_SLOTS partial sums
    }
}

// upstream gradient: host scalar times an optional device scalar (autograd's
// grad_output stays on the device: no host synchronisation in backward)
__device__ __forceinline__ float eff_scale(float host, const float *dev)
{
    return dev ? host * dev[0] : host;
}

// Hardware transcendentals (v_exp_f32 / v_log_f32 / v_rcp_f32, ~1 ulp).  The loss kernels
// stream 80 logits per anchor and must stay HBM-bound: the bit-reproducible software
// exp/log/divide of ia_math.hpp (needed on the inference path for index parity) costs ~200
// VALU slots per element here, 3x the budget of an 8 TB/s stream.  Losses have no index
// outputs; their parity bar is the north star's 1e-4, checked against the oracle and the
// reference's autograd.
namespace fastm {
__device__ __forceinline__ float exp_(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }
__device__ __forceinline__ float log_(float x) { return __builtin_amdgcn_logf(x) * 0.693147180559945309f; }
__device__ __forceinline__ float rcp_(float x) { return __builtin_amdgcn_rcpf(x); }
}  // namespace fastm

struct Dec { float x1, y1, x2, y2, gw, gh, pw, ph; bool win, hin; };

__device__ __forceinline__ Dec decode_free(const float (&anc)[4], const float (&d)[4],
                                           const float *means, const float *stds)
{
    const float max_ratio = 4.135166556742356f;
    Dec r;
    float dx = d[0] * stds[0] + means[0];
    float dy = d[1] * stds[1] + means[1];
    float dw = d[2] * stds[2] + means[2];
    float dh = d[3] * stds[3] + means[3];
    r.win = (dw >= -max_ratio) && (dw <= max_ratio);
    r.hin = (dh >= -max_ratio) && (dh <= max_ratio);
    dw = (dw < -max_ratio) ? -max_ratio : dw;  dw = (dw > max_ratio) ? max_ratio : dw;
    dh = (dh < -max_ratio) ? -max_ratio : dh;  dh = (dh > max_ratio) ? max_ratio : dh;
    float px = (anc[0] + anc[2]) * 0.5f;
    float py = (anc[1] + anc[3]) * 0.5f;
    r.pw = (anc[2] - anc[0]) + 1.0f;
    r.ph = (anc[3] - anc[1]) + 1.0f;
    r.gw = r.pw * expf_(dw);
    r.gh = r.ph * expf_(dh);
    float gx = px + r.pw * dx;
    float gy = py + r.ph * dy;
    r.x1 = (gx - r.gw * 0.5f) + 0.5f;
    r.y1 = (gy - r.gh * 0.5f) + 0.5f;
    r.x2 = (gx + r.gw * 0.5f) - 0.5f;
    r.y2 = (gy + r.gh * 0.5f) - 0.5f;
    return r;
}


// ---- one anchor of the IoU-regression branch: decode prediction and target with the same
// anchor, aligned IoU with the +1 convention (the regression target of the IoU head)
struct IouElem {
    Dec pb, tb;
    float w0, h0, w, h, ov, un, t;
};

__device__ __forceinline__ IouElem iou_target_elem(const float (&anc)[4], const float (&dp)[4],
                                                   const float (&dt)[4], const float *means,
                                                   const float *stds)
{
    IouElem r;
    r.pb = decode_free(anc, dp, means, stds);
    r.tb = decode_free(anc, dt, means, stds);
    const Dec &pb = r.pb, &tb = r.tb;
    float ltx = (tb.x1 < pb.x1) ? pb.x1 : tb.x1;
    float lty = (tb.y1 < pb.y1) ? pb.y1 : tb.y1;
    float rbx = (pb.x2 < tb.x2) ? pb.x2 : tb.x2;
    float rby = (pb.y2 < tb.y2) ? pb.y2 : tb.y2;
    r.w0 = (rbx - ltx) + 1.0f; r.h0 = (rby - lty) + 1.0f;
    r.w = (r.w0 < 0.0f) ? 0.0f : r.w0; r.h = (r.h0 < 0.0f) ? 0.0f : r.h0;
    r.ov = r.w * r.h;
    float a1 = ((tb.x2 - tb.x1) + 1.0f) * ((tb.y2 - tb.y1) + 1.0f);
    float a2 = ((pb.x2 - pb.x1) + 1.0f) * ((pb.y2 - pb.y1) + 1.0f);
    r.un = (a1 + a2) - r.ov;
    r.t = r.ov / r.un;
    return r;
}

// gradient of BCE(xl, t(bbox_pred)) * wt w.r.t. the four deltas of bbox_pred, THROUGH the IoU
// target (the reference leaves the target attached, iou_aware_retina_head.py:256-259)
__device__ __forceinline__ void iou_bce_box_grad(const IouElem &q, float xl, float wt, float gs,
                                                 const float *stds, float (&go)[4])
{
    const Dec &pb = q.pb, &tb = q.tb;
    float gt = ((-xl) * wt) * gs;
    float inv_un = 1.0f / q.un;
    float g_ov = gt * ((q.un + q.ov) * inv_un) * inv_un;
    float g_a2 = gt * (-(q.ov * inv_un) * inv_un);
    float g_w = (q.w0 >= 0.0f) ? g_ov * q.h : 0.0f;
    float g_h = (q.h0 >= 0.0f) ? g_ov * q.w : 0.0f;
    float pw2 = (pb.x2 - pb.x1) + 1.0f, ph2 = (pb.y2 - pb.y1) + 1.0f;
    float gx1 = -g_a2 * ph2, gx2 = g_a2 * ph2;
    float gy1 = -g_a2 * pw2, gy2 = g_a2 * pw2;
    float sx1 = (pb.x1 > tb.x1) ? 1.0f : ((pb.x1 == tb.x1) ? 0.5f : 0.0f);
    float sy1 = (pb.y1 > tb.y1) ? 1.0f : ((pb.y1 == tb.y1) ? 0.5f : 0.0f);
    float sx2 = (pb.x2 < tb.x2) ? 1.0f : ((pb.x2 == tb.x2) ? 0.5f : 0.0f);
    float sy2 = (pb.y2 < tb.y2) ? 1.0f : ((pb.y2 == tb.y2) ? 0.5f : 0.0f);
    gx1 = gx1 - g_w * sx1;  gx2 = gx2 + g_w * sx2;
    gy1 = gy1 - g_h * sy1;  gy2 = gy2 + g_h * sy2;
    float g_gx = gx1 + gx2, g_gy = gy1 + gy2;
    float g_gw = (gx2 - gx1) * 0.5f, g_gh = (gy2 - gy1) * 0.5f;
    go[0] = (g_gx * pb.pw) * stds[0];
    go[1] = (g_gy * pb.ph) * stds[1];
    go[2] = pb.win ? (g_gw * pb.gw) * stds[2] : 0.0f;
    go[3] = pb.hin ? (g_gh * pb.gh) * stds[3] : 0.0f;
}

// smooth-L1 of one coordinate (losses.py:385-400) and its derivative
__device__ __forceinline__ float smooth_l1_val(float df, float beta)
{
    const float d = __builtin_fabsf(df);
    return (d < beta) ? ((0.5f * d) * d) / beta : d - 0.5f * beta;
}
__device__ __forceinline__ float smooth_l1_der(float df, float beta)
{
    const float d = __builtin_fabsf(df);
    const float sgn = (df > 0.0f) ? 1.0f : ((df < 0.0f) ? -1.0f : 0.0f);
    return (d < beta) ? df / beta : sgn;
}

// BalancedL1Loss of one coordinate (losses.py:482-507) and its derivative.  With d = |df| and
// b = e^(gamma / alpha) - 1:  d < beta: alpha / b * (b d + 1) * log(b d / beta + 1) - alpha d,  else
// gamma d + gamma / b - alpha beta.  The constants are the fp32 values the reference's python scalars
// round to (b in double first); the derivative is that of this expression, jump at the knee for
// beta != 1 included: alpha log(b d / beta + 1) + alpha (1 - beta) / (b d + beta) inside, gamma outside.
struct BalL1 { float alpha, gamma, b, a_b, g_b, ab, a1mb; };   // ., ., b, alpha/b, gamma/b, alpha*beta, alpha*(1-beta)

// host: false for alpha, gamma or beta not > 0 (or a b beyond fp32)
inline bool balanced_l1_consts(float alpha, float gamma, float beta, BalL1 &k)
{
    if (!(alpha > 0.0f) || !(gamma > 0.0f) || !(beta > 0.0f)) return false;
    const double b = pow(2.718281828459045, (double)gamma / (double)alpha) - 1.0;   // np.e ** (gamma / alpha) - 1
    if (!(b > 0.0) || !(b < 3.0e38)) return false;
    k.alpha = alpha; k.gamma = gamma; k.b = (float)b;
    k.a_b = (float)((double)alpha / b); k.g_b = (float)((double)gamma / b);
    k.ab = (float)((double)alpha * (double)beta);
    k.a1mb = (float)((double)alpha * (1.0 - (double)beta));
    return true;
}
__device__ __forceinline__ float balanced_l1_val(float df, float beta, const BalL1 &k)
{
    const float d = __builtin_fabsf(df);
    const float bd = k.b * d;
    return (d < beta) ? (k.a_b * (bd + 1.0f)) * fastm::log_(bd / beta + 1.0f) - k.alpha * d
                      : (k.gamma * d + k.g_b) - k.ab;
}
__device__ __forceinline__ float balanced_l1_der(float df, float beta, const BalL1 &k)
{
    const float d = __builtin_fabsf(df);
    const float sgn = (df > 0.0f) ? 1.0f : ((df < 0.0f) ? -1.0f : 0.0f);
    const float bd = k.b * d;
    const float in = k.alpha * fastm::log_(bd / beta + 1.0f) + k.a1mb / (bd + beta);
    return sgn * ((d < beta) ? in : k.gamma);
}

}  // namespace ia
