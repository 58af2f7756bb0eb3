// GroupNorm + ReLU of the IoU-aware FCOS head towers (reference
// mmdet/models/anchor_heads/iou_aware_fcos_head.py:41-62, ConvModule(3x3, GN(32), ReLU); torch
// nn.GroupNorm semantics: biased variance, eps inside the square root): the in-place inference pair
// and the training node (out-of-place forward, backward), each algorithm written once for fp32 and
// bf16 activations.
//
// Input: per level (B, H_l, W_l, channels) channels-last activations, fp32 (what the Winograd output
// transform writes) or bf16 (conv3x3_bf16.hip in front and behind); all levels and images of a tower
// layer in one launch per kernel.  One workgroup per (level, image, chunk of IA_GN_CHUNK pixels);
// every thread owns one 16-byte column of channels (GnCol: 4 floats or 8 bf16, inside one group:
// channels / groups % N == 0) and a strided subset of the chunk's pixels.  bf16 values widen exactly
// to fp32 / fp64, so every expression below is evaluated on the stored numbers in the same way for
// both dtypes, and what is written as bf16 (y, dx) is rounded ONCE, nearest even.
//
//   stats        fp64 sum and sum of squares per thread (x * x is exact in fp64); the threads of a
//                group are added in a fixed order through LDS and the workgroup writes (sum, sumsq)
//                per group to its own slot of the workspace.
//   apply        the first `groups` threads add their group's partials over the (level, image)'s
//                chunks in index order (fp64), mean = S / n, var = max(SS / n - mean^2, 0) -- fp64
//                keeps E[x^2] - E[x]^2 exact enough for |mean| >> std (a one-pass fp32 form loses
//                ~(mean/std)^2 * 2^-24 of the variance) --, then per channel s = gamma * rstd,
//                t = beta - mean * s (fp64, rounded once), and every thread writes its column
//                y = relu?(x * s + t) with 16-byte loads and stores: over x itself (k_gn_apply, the
//                inference pair), or to a second tensor with chunk 0 of every (level, image) leaving
//                (mean, rstd) per group in fp64 for the backward (k_gn_apply_to, the training node).
//
// Backward of the training node.  With xh = (x - mean) * rstd, g = dy * [x * s + t > 0] (the
// forward's fp32 expression re-evaluated from the saved statistics: the same mask bit for bit; y is
// not kept) and n = channels / groups * H_l * W_l:
//     dbeta_c = sum g,  dgamma_c = sum g * xh  (all pixels, images, levels)
//     dx = rstd * (gamma * g - mean_grp(gamma * g) - xh * mean_grp(gamma * g * xh))
//   bwd_reduce   sum g and sum g * x per channel in fp64 per thread (the product of two floats is
//                exact there); the threads of a column are added in a fixed order through LDS,
//                sum g * xh = rstd * (sum g * x - mean * sum g), and the workgroup writes
//                (sum g, sum g * xh) per channel and, weighted by gamma and added over a group's
//                channels in index order, per group to its own workspace rows.
//   bwd_apply    the first `groups` threads add the group partials of the (level, image) over its
//                chunks in index order; dx = s * g + (c1 + xc * c2) per element with s = gamma * rstd
//                as in the forward, c1 = -rstd * m1, c2 = -rstd^2 * m2 and xc = (x - mean_hi) -
//                mean_lo: the mean as two floats, so that |mean| >> std costs nothing (x - mean_hi
//                is exact there).
//   k_gn_bwd_params   per channel the (sum g, sum g * xh) rows in a fixed order: kGnSeg contiguous
//                runs of rows (level-major / image / chunk), each in index order by one thread, then
//                the runs in index order.
//
// No atomics anywhere: the bits do not depend on scheduling.  The partials of an (image, level) come
// from that image's pixels only and are summed in the same order whatever else shares the launch: an
// image alone gives the same bits as inside a batch.  dy is only read.
#include "ia_internal.hpp"
#include "ia_math.hpp"

namespace ia {

constexpr int kGnThreads = 256;

__device__ __forceinline__ void gn_put(const float4 q, float *f)
{
    f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
}

// A thread's 16-byte column of N channels, as floats in registers.
template <int N> struct GnCol;

template <> struct GnCol<4> {
    using vec = float4;
    static constexpr int kShift = 2;            // log2 N
    static constexpr int kUnroll = 1;           // pixels in flight per thread in the training node
    static __device__ __forceinline__ void load(const vec &q, float (&f)[4]) { gn_put(q, f); }
    static __device__ __forceinline__ vec store(const float (&f)[4])
    {
        return make_float4(f[0], f[1], f[2], f[3]);
    }
    static __device__ __forceinline__ const vec *image(const void *base, int b, int HW, int channels)
    {
        return reinterpret_cast<const vec *>(static_cast<const float *>(base) +
                                             (size_t)b * HW * channels);
    }
};

template <> struct GnCol<8> {
    using vec = uint4;
    static constexpr int kShift = 3;
    static constexpr int kUnroll = 2;
    static __device__ __forceinline__ void load(const vec &q, float (&f)[8]) { bf16x8_to_f32(q, f); }
    static __device__ __forceinline__ vec store(const float (&f)[8]) { return f32_to_bf16x8(f); }
    static __device__ __forceinline__ const vec *image(const void *base, int b, int HW, int channels)
    {
        return reinterpret_cast<const vec *>(static_cast<const uint16_t *>(base) +
                                             (size_t)b * HW * channels);
    }
};

struct GnArgs {
    int32_t num_levels, batch, channels, groups;
    int32_t HW[IA_MAX_LEVELS];
    int32_t nch[IA_MAX_LEVELS];                 // chunks per image of level l
    int32_t blk_off[IA_MAX_LEVELS + 1];         // prefix over levels of batch * nch[l] (= slab rows)
    const void *x[IA_MAX_LEVELS];
    const void *dy[IA_MAX_LEVELS];              // backward only
    void *out[IA_MAX_LEVELS];                   // y (k_gn_apply_to) / dx (k_gn_bwd_apply)
    const float *gamma, *beta;
    float eps;
    int32_t relu;
    double2 *part;                              // (slab rows, groups) (sum, sumsq)
    double2 *saved;                             // (num_levels * batch, groups) (mean, rstd)
    double2 *gpart;                             // (slab rows, groups)   (sum gamma g, sum gamma g xh)
    double2 *cpart;                             // (slab rows, channels) (sum g, sum g xh)
};

struct GnBlock { int l, b, chunk, HW, nch, row0; const void *x, *dy; void *out; };

// The per-level pointer tables are selected one table after the other, and only those a kernel uses.
template <bool kDy, bool kOut>
__device__ __forceinline__ GnBlock gn_block(const GnArgs &a, int blk)
{
    GnBlock k;
    int l = 0;
#pragma unroll
    for (int i = 1; i < IA_MAX_LEVELS; ++i) l += (i < a.num_levels && blk >= a.blk_off[i]) ? 1 : 0;
    k.l = l;
    k.HW = a.HW[0]; k.nch = a.nch[0];
    int off = a.blk_off[0];
#pragma unroll
    for (int i = 1; i < IA_MAX_LEVELS; ++i) {
        const bool m = l == i;
        k.HW = m ? a.HW[i] : k.HW; k.nch = m ? a.nch[i] : k.nch;
        off = m ? a.blk_off[i] : off;
    }
    k.x = a.x[0];
#pragma unroll
    for (int i = 1; i < IA_MAX_LEVELS; ++i) k.x = (l == i) ? a.x[i] : k.x;
    k.dy = nullptr;
    if (kDy) {
        k.dy = a.dy[0];
#pragma unroll
        for (int i = 1; i < IA_MAX_LEVELS; ++i) k.dy = (l == i) ? a.dy[i] : k.dy;
    }
    k.out = nullptr;
    if (kOut) {
        k.out = a.out[0];
#pragma unroll
        for (int i = 1; i < IA_MAX_LEVELS; ++i) k.out = (l == i) ? a.out[i] : k.out;
    }
    const int rem = blk - off;
    k.b = rem / k.nch;
    k.chunk = rem - k.b * k.nch;
    k.row0 = off + k.b * k.nch;                 // slab row of chunk 0 of this (level, image)
    return k;
}

// a column's N values added pairwise: ((d0 + d1) + (d2 + d3)) [+ ((d4 + d5) + (d6 + d7))]
template <int N> __device__ __forceinline__ double gn_tree(const double (&d)[N])
{
    double t = (d[0] + d[1]) + (d[2] + d[3]);
    if constexpr (N == 8) t = t + ((d[4] + d[5]) + (d[6] + d[7]));
    return t;
}

template <int N> __device__ __forceinline__ void gn_stats(const GnArgs &a)
{
    using C = GnCol<N>;
    __shared__ double s_sum[kGnThreads], s_sq[kGnThreads];
    const GnBlock k = gn_block<false, false>(a, blockIdx.x);
    const int tid = threadIdx.x;
    const int vc = a.channels >> C::kShift;     // 16-byte columns per pixel (divides kGnThreads)
    const int rows = kGnThreads / vc;           // pixels per pass
    const int v = tid % vc, r = tid / vc;
    const int p0 = k.chunk * IA_GN_CHUNK;
    const int p1 = min(p0 + IA_GN_CHUNK, k.HW);
    const typename C::vec *x = C::image(k.x, k.b, k.HW, a.channels) + v;
    double s = 0.0, ss = 0.0;
    for (int p = p0 + r; p < p1; p += rows) {
        float f[N];
        C::load(x[(size_t)p * vc], f);
        double d[N], dd[N];
#pragma unroll
        for (int j = 0; j < N; ++j) d[j] = f[j];
        s += gn_tree(d);
#pragma unroll
        for (int j = 0; j < N; ++j) dd[j] = d[j] * d[j];
        ss += gn_tree(dd);
    }
    s_sum[tid] = s;
    s_sq[tid] = ss;
    __syncthreads();
    const int vpg = (a.channels / a.groups) >> C::kShift;   // columns per group
    for (int g = tid; g < a.groups; g += kGnThreads) {
        double ts = 0.0, tss = 0.0;
        for (int rr = 0; rr < rows; ++rr)
            for (int j = 0; j < vpg; ++j) {
                const int t = rr * vc + g * vpg + j;
                ts += s_sum[t];
                tss += s_sq[t];
            }
        a.part[(size_t)(k.row0 + k.chunk) * a.groups + g] = make_double2(ts, tss);
    }
}

// per channel s = gamma * rstd, t = beta - mean * s: fp64, rounded once; quad q = channels 4 q ..
__device__ __forceinline__ void gn_scale_shift(const float *gamma, const float *beta, int q,
                                               double mean, double rstd, float4 &sc, float4 &sh)
{
    float s[4], t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * q + j;
        s[j] = (float)((double)gamma[c] * rstd);
        t[j] = (float)((double)beta[c] - mean * (double)s[j]);
    }
    sc = make_float4(s[0], s[1], s[2], s[3]);
    sh = make_float4(t[0], t[1], t[2], t[3]);
}

// column v's N per-channel (s, t): quads (N / 4) v .. of gn_scale_shift
template <int N>
__device__ __forceinline__ void gn_scale_shift_col(const float *gamma, const float *beta, int v,
                                                   double mean, double rstd, float (&sc)[N],
                                                   float (&sh)[N])
{
#pragma unroll
    for (int h = 0; h < N / 4; ++h) {
        float4 s4, t4;
        gn_scale_shift(gamma, beta, (N / 4) * v + h, mean, rstd, s4, t4);
        gn_put(s4, sc + 4 * h);
        gn_put(t4, sh + 4 * h);
    }
}

// kTo: y goes to a.out and chunk 0 leaves (mean, rstd) in a.saved; otherwise x is rewritten.
template <int N, bool kTo> __device__ __forceinline__ void gn_apply(const GnArgs &a)
{
    using C = GnCol<N>;
    __shared__ double s_mean[256], s_rstd[256];
    __shared__ float4 s_scale[256], s_shift[256];      // per 4 channels
    const GnBlock k = gn_block<false, kTo>(a, blockIdx.x);
    const int tid = threadIdx.x;
    const int cpg = a.channels / a.groups;
    for (int g = tid; g < a.groups; g += kGnThreads) {
        double ts = 0.0, tss = 0.0;
        const double2 *pp = a.part + (size_t)k.row0 * a.groups + g;
        for (int c = 0; c < k.nch; ++c) {
            const double2 q = pp[(size_t)c * a.groups];
            ts += q.x;
            tss += q.y;
        }
        const double n = (double)k.HW * cpg;
        const double mean = ts / n;
        double var = tss / n - mean * mean;
        var = var > 0.0 ? var : 0.0;
        const double rstd = 1.0 / sqrt(var + (double)a.eps);
        s_mean[g] = mean;
        s_rstd[g] = rstd;
        if (kTo && k.chunk == 0)
            a.saved[(size_t)(k.l * a.batch + k.b) * a.groups + g] = make_double2(mean, rstd);
    }
    __syncthreads();
    for (int q = tid; q < (a.channels >> 2); q += kGnThreads) {
        const int g = (4 * q) / cpg;
        float4 sc, sh;
        gn_scale_shift(a.gamma, a.beta, q, s_mean[g], s_rstd[g], sc, sh);
        s_scale[q] = sc;
        s_shift[q] = sh;
    }
    __syncthreads();
    const int vc = a.channels >> C::kShift;
    const int rows = kGnThreads / vc;
    const int v = tid % vc, r = tid / vc;
    float sc[N], sh[N];
#pragma unroll
    for (int h = 0; h < N / 4; ++h) gn_put(s_scale[(N / 4) * v + h], sc + 4 * h);
#pragma unroll
    for (int h = 0; h < N / 4; ++h) gn_put(s_shift[(N / 4) * v + h], sh + 4 * h);
    const int p0 = k.chunk * IA_GN_CHUNK;
    const int p1 = min(p0 + IA_GN_CHUNK, k.HW);
    const typename C::vec *x = C::image(k.x, k.b, k.HW, a.channels) + v;
    typename C::vec *y =
        const_cast<typename C::vec *>(kTo ? C::image(k.out, k.b, k.HW, a.channels) + v : x);
    constexpr int kUnroll = kTo ? C::kUnroll : 1;       // the inference pair: one pixel in flight
#pragma unroll kUnroll
    for (int p = p0 + r; p < p1; p += rows) {
        float f[N];
        C::load(x[(size_t)p * vc], f);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            f[j] = f[j] * sc[j] + sh[j];
            if (a.relu) f[j] = f[j] > 0.0f ? f[j] : 0.0f;
        }
        y[(size_t)p * vc] = C::store(f);
    }
}

// g = dy where the forward's fp32 pre-activation is positive (all of dy without the ReLU)
template <int N>
__device__ __forceinline__ void gn_masked(const float (&x)[N], float (&g)[N], const float (&sc)[N],
                                          const float (&sh)[N], int relu)
{
    if (relu) {
#pragma unroll
        for (int j = 0; j < N; ++j) g[j] = (x[j] * sc[j] + sh[j]) > 0.0f ? g[j] : 0.0f;
    }
}

// LDS: the threads of a column are added four channels at a time (channels 0..3, then 4..7 of every
// 8-wide column) through 16 KB of per-thread sums next to s_ch's 16 KB: all N channels of a bf16
// column at once would take 32 KB for the sums alone and leave three workgroups per CU instead of
// five.  The order per channel is the same fixed one; a second half costs one more barrier pair.
template <int N> __device__ __forceinline__ void gn_bwd_reduce(const GnArgs &a)
{
    using C = GnCol<N>;
    __shared__ double s_acc[8][kGnThreads];     // [2 * j + (0: g, 1: g x)][thread], j = channel & 3
    __shared__ double2 s_ch[1024];              // per channel gamma * (sum g, sum g xh)
    const GnBlock k = gn_block<true, false>(a, blockIdx.x);
    const int tid = threadIdx.x;
    const int cpg = a.channels / a.groups;
    const int vc = a.channels >> C::kShift;
    const int rows = kGnThreads / vc;
    const int v = tid % vc, r = tid / vc;
    const double2 *saved = a.saved + (size_t)(k.l * a.batch + k.b) * a.groups;
    float sc[N], sh[N];
    {
        const double2 mr = saved[(N * v) / cpg];
        gn_scale_shift_col(a.gamma, a.beta, v, mr.x, mr.y, sc, sh);
    }
    const int p0 = k.chunk * IA_GN_CHUNK;
    const int p1 = min(p0 + IA_GN_CHUNK, k.HW);
    const typename C::vec *x = C::image(k.x, k.b, k.HW, a.channels) + v;
    const typename C::vec *dy = C::image(k.dy, k.b, k.HW, a.channels) + v;
    double sg[N], sx[N];
#pragma unroll
    for (int j = 0; j < N; ++j) sg[j] = sx[j] = 0.0;
#pragma unroll C::kUnroll
    for (int p = p0 + r; p < p1; p += rows) {
        float q[N], g[N];
        C::load(x[(size_t)p * vc], q);
        C::load(dy[(size_t)p * vc], g);
        gn_masked(q, g, sc, sh, a.relu);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const double gj = g[j];
            sg[j] += gj;
            sx[j] += gj * (double)q[j];
        }
    }
    const size_t row = (size_t)(k.row0 + k.chunk);
#pragma unroll
    for (int h = 0; h < N / 4; ++h) {
        if (h) __syncthreads();                 // the previous half's sums are read
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s_acc[2 * j][tid] = sg[4 * h + j];
            s_acc[2 * j + 1][tid] = sx[4 * h + j];
        }
        __syncthreads();
        for (int i = tid; i < (a.channels >> (C::kShift - 2)); i += kGnThreads) {
            const int cv = i >> 2, j = i & 3;
            const int c = N * cv + 4 * h + j;
            double tg = 0.0, tx = 0.0;
            for (int rr = 0; rr < rows; ++rr) {
                tg += s_acc[2 * j][rr * vc + cv];
                tx += s_acc[2 * j + 1][rr * vc + cv];
            }
            const double2 mr = saved[c / cpg];
            const double th = mr.y * (tx - mr.x * tg);          // sum g * xh
            a.cpart[row * a.channels + c] = make_double2(tg, th);
            const double gm = (double)a.gamma[c];
            s_ch[c] = make_double2(gm * tg, gm * th);
        }
    }
    __syncthreads();
    for (int g = tid; g < a.groups; g += kGnThreads) {
        double t1 = 0.0, t2 = 0.0;
        for (int j = 0; j < cpg; ++j) {
            const double2 q = s_ch[g * cpg + j];
            t1 += q.x;
            t2 += q.y;
        }
        a.gpart[row * a.groups + g] = make_double2(t1, t2);
    }
}

template <int N> __device__ __forceinline__ void gn_bwd_apply(const GnArgs &a)
{
    using C = GnCol<N>;
    __shared__ double2 s_mr[256];
    __shared__ float4 s_k[256];                 // per group (mean_hi, mean_lo, c1, c2)
    const GnBlock k = gn_block<true, true>(a, blockIdx.x);
    const int tid = threadIdx.x;
    const int cpg = a.channels / a.groups;
    const double2 *saved = a.saved + (size_t)(k.l * a.batch + k.b) * a.groups;
    for (int g = tid; g < a.groups; g += kGnThreads) {
        double t1 = 0.0, t2 = 0.0;
        const double2 *pp = a.gpart + (size_t)k.row0 * a.groups + g;
        for (int c = 0; c < k.nch; ++c) {
            const double2 q = pp[(size_t)c * a.groups];
            t1 += q.x;
            t2 += q.y;
        }
        const double n = (double)k.HW * cpg;
        const double2 mr = saved[g];
        const float mh = (float)mr.x;
        s_mr[g] = mr;
        s_k[g] = make_float4(mh, (float)(mr.x - (double)mh), (float)(-mr.y * (t1 / n)),
                             (float)(-mr.y * mr.y * (t2 / n)));
    }
    __syncthreads();
    const int vc = a.channels >> C::kShift;
    const int rows = kGnThreads / vc;
    const int v = tid % vc, r = tid / vc;
    const int grp = (N * v) / cpg;
    float sc[N], sh[N];
    gn_scale_shift_col(a.gamma, a.beta, v, s_mr[grp].x, s_mr[grp].y, sc, sh);
    const float4 kk = s_k[grp];
    const int p0 = k.chunk * IA_GN_CHUNK;
    const int p1 = min(p0 + IA_GN_CHUNK, k.HW);
    const typename C::vec *x = C::image(k.x, k.b, k.HW, a.channels) + v;
    const typename C::vec *dy = C::image(k.dy, k.b, k.HW, a.channels) + v;
    typename C::vec *dx =
        const_cast<typename C::vec *>(C::image(k.out, k.b, k.HW, a.channels)) + v;
#pragma unroll C::kUnroll
    for (int p = p0 + r; p < p1; p += rows) {
        float q[N], g[N], o[N];
        C::load(x[(size_t)p * vc], q);
        C::load(dy[(size_t)p * vc], g);
        gn_masked(q, g, sc, sh, a.relu);
#pragma unroll
        for (int j = 0; j < N; ++j) o[j] = sc[j] * g[j] + (kk.z + ((q[j] - kk.x) - kk.y) * kk.w);
        dx[(size_t)p * vc] = C::store(o);
    }
}

// The entry points: fp32 (4 floats per column) and bf16 (8 values per column) of every body.
__global__ void __launch_bounds__(kGnThreads) k_gn_stats(GnArgs a) { gn_stats<4>(a); }
__global__ void __launch_bounds__(kGnThreads) k_gn_stats_bf16(GnArgs a) { gn_stats<8>(a); }
__global__ void __launch_bounds__(kGnThreads) k_gn_apply(GnArgs a) { gn_apply<4, false>(a); }
__global__ void __launch_bounds__(kGnThreads) k_gn_apply_bf16(GnArgs a) { gn_apply<8, false>(a); }
__global__ void __launch_bounds__(kGnThreads) k_gn_apply_to(GnArgs a) { gn_apply<4, true>(a); }
__global__ void __launch_bounds__(kGnThreads) k_gn_apply_to_bf16(GnArgs a) { gn_apply<8, true>(a); }
__global__ void __launch_bounds__(kGnThreads) k_gn_bwd_reduce(GnArgs a) { gn_bwd_reduce<4>(a); }
__global__ void __launch_bounds__(kGnThreads) k_gn_bwd_reduce_bf16(GnArgs a) { gn_bwd_reduce<8>(a); }
__global__ void __launch_bounds__(kGnThreads) k_gn_bwd_apply(GnArgs a) { gn_bwd_apply<4>(a); }
__global__ void __launch_bounds__(kGnThreads) k_gn_bwd_apply_bf16(GnArgs a) { gn_bwd_apply<8>(a); }

constexpr int kGnSeg = 16;                      // runs of rows per channel in k_gn_bwd_params

// one workgroup per 16 channels: thread (seg, c) adds its run of rows in index order
__global__ void __launch_bounds__(kGnThreads) k_gn_bwd_params(const double2 *cpart, int rows,
                                                              int channels, float *dgamma,
                                                              float *dbeta)
{
    __shared__ double2 s_p[kGnSeg][16];
    const int tid = threadIdx.x;
    const int cl = tid & 15, seg = tid >> 4;
    const int c = blockIdx.x * 16 + cl;
    const int per = (rows + kGnSeg - 1) / kGnSeg;
    const int r0 = seg * per, r1 = min(r0 + per, rows);
    double tg = 0.0, th = 0.0;
    if (c < channels)
        for (int r = r0; r < r1; ++r) {
            const double2 q = cpart[(size_t)r * channels + c];
            tg += q.x;
            th += q.y;
        }
    s_p[seg][cl] = make_double2(tg, th);
    __syncthreads();
    if (seg == 0 && c < channels) {
        double ug = 0.0, uh = 0.0;
        for (int s = 0; s < kGnSeg; ++s) {
            ug += s_p[s][cl].x;
            uh += s_p[s][cl].y;
        }
        if (dbeta) dbeta[c] = (float)ug;
        if (dgamma) dgamma[c] = (float)uh;
    }
}

static int gn_args(const ia_wino_geom *g, int channels, int groups, GnArgs &a)
{
    if (!g || g->num_levels < 1 || g->num_levels > IA_MAX_LEVELS || g->batch < 1) return IA_E_ARG;
    if (channels < 4 || channels > 1024 || (channels & (channels - 1)) != 0) return IA_E_ARG;
    if (groups < 1 || groups > 256 || channels % groups != 0 || (channels / groups) % 4 != 0)
        return IA_E_ARG;
    a.num_levels = g->num_levels; a.batch = g->batch; a.channels = channels; a.groups = groups;
    a.blk_off[0] = 0;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        int64_t hw = 0;
        if (l < g->num_levels) {
            if (g->H[l] < 1 || g->W[l] < 1) return IA_E_ARG;
            hw = (int64_t)g->H[l] * g->W[l];
            if (hw * channels > (1LL << 31)) return IA_E_ARG;
        }
        a.HW[l] = (int32_t)hw;
        a.nch[l] = (int32_t)((hw + IA_GN_CHUNK - 1) / IA_GN_CHUNK);
        const int64_t next = (int64_t)a.blk_off[l] + (int64_t)g->batch * a.nch[l];
        if (next > (1LL << 30)) return IA_E_ARG;
        a.blk_off[l + 1] = (int32_t)next;
        a.x[l] = nullptr; a.dy[l] = nullptr; a.out[l] = nullptr;
    }
    a.gamma = a.beta = nullptr; a.eps = 0.0f; a.relu = 0;
    a.part = nullptr; a.saved = nullptr; a.gpart = nullptr; a.cpart = nullptr;
    return 0;
}

// what bf16 takes on top of gn_args: whole 16-byte columns inside a group
static int gn_args_dt(const ia_wino_geom *g, int channels, int groups, int dtype, GnArgs &a)
{
    if (dtype != IA_F32 && dtype != IA_BF16) return IA_E_ARG;
    int rc = gn_args(g, channels, groups, a);
    if (rc) return rc;
    if (dtype == IA_BF16 && (channels < 8 || (channels / groups) % 8 != 0)) return IA_E_ARG;
    return 0;
}

// a level list's base pointers: all there and 16-byte aligned
template <class P> static bool gn_level_ptrs(int n, P *const *p, P **out)
{
    if (!p) return false;
    for (int l = 0; l < n; ++l) {
        if (!p[l] || ((uintptr_t)p[l] & 15u)) return false;
        out[l] = p[l];
    }
    return true;
}

// the fp32 or the bf16 kernel of a body on the common grid: one workgroup per (level, image, chunk)
static int gn_launch(int dtype, void (*f32)(GnArgs), void (*bf16)(GnArgs), const GnArgs &a,
                     void *stream)
{
    hipLaunchKernelGGL(dtype == IA_BF16 ? bf16 : f32, dim3((unsigned)a.blk_off[IA_MAX_LEVELS]),
                       dim3(kGnThreads), 0, (hipStream_t)stream, a);
    return hip_status(hipGetLastError());
}

// the FCOS regression epilogue bbox_pred = exp(scale_l * x) (iou_aware_fcos_head.py:105), in place
// on per-level channels-last tensors; the scales stay on the device (no host read of a parameter)
struct ScaleExpArgs {
    int32_t num_levels;
    int64_t vec_off[IA_MAX_LEVELS + 1];         // prefix of counts of groups of four values
    void *x[IA_MAX_LEVELS];
    const float *scales;
};

// a thread's four values: 16 bytes of fp32, or 8 bytes of bf16 (widened exactly, rounded once)
__device__ __forceinline__ void quad_load(const float4 &q, float (&f)[4]) { gn_put(q, f); }
__device__ __forceinline__ void quad_load(const uint2 &q, float (&f)[4])
{
    f[0] = from_bits(q.x << 16); f[1] = from_bits(q.x & 0xffff0000u);
    f[2] = from_bits(q.y << 16); f[3] = from_bits(q.y & 0xffff0000u);
}
__device__ __forceinline__ void quad_store(const float (&f)[4], float4 &q)
{
    q = make_float4(f[0], f[1], f[2], f[3]);
}
__device__ __forceinline__ void quad_store(const float (&f)[4], uint2 &q)
{
    q.x = f32_to_bf16(f[0]) | (f32_to_bf16(f[1]) << 16);
    q.y = f32_to_bf16(f[2]) | (f32_to_bf16(f[3]) << 16);
}

template <class V> __device__ __forceinline__ void scale_exp(const ScaleExpArgs &a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.vec_off[a.num_levels]) return;
    int l = 0;
#pragma unroll
    for (int k = 1; k < IA_MAX_LEVELS; ++k) l += (k < a.num_levels && i >= a.vec_off[k]) ? 1 : 0;
    V *x = static_cast<V *>(a.x[0]);
    int64_t base = a.vec_off[0];
#pragma unroll
    for (int k = 1; k < IA_MAX_LEVELS; ++k) {
        x = (l == k) ? static_cast<V *>(a.x[k]) : x;
        base = (l == k) ? a.vec_off[k] : base;
    }
    const float s = a.scales[l];
    V q = x[i - base];
    float f[4];
    quad_load(q, f);
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = expf_(f[j] * s);
    quad_store(f, q);
    x[i - base] = q;
}

__global__ void __launch_bounds__(256) k_scale_exp(ScaleExpArgs a) { scale_exp<float4>(a); }
__global__ void __launch_bounds__(256) k_scale_exp_bf16(ScaleExpArgs a) { scale_exp<uint2>(a); }

}  // namespace ia

extern "C" {

// dtype IA_F32: 16-byte groups of four floats; IA_BF16: 8-byte groups of four bf16
static int scale_exp_impl(const ia_wino_geom *g, void *const *x, int channels, int dtype,
                          const float *scales, void *stream)
{
    if (!g || g->num_levels < 1 || g->num_levels > IA_MAX_LEVELS || g->batch < 1 || !x || !scales)
        return IA_E_ARG;
    if (channels < 4 || (channels & 3)) return IA_E_ARG;
    if (dtype != IA_F32 && dtype != IA_BF16) return IA_E_ARG;
    const uintptr_t align = dtype == IA_BF16 ? 7u : 15u;
    ia::ScaleExpArgs a;
    a.num_levels = g->num_levels;
    a.scales = scales;
    a.vec_off[0] = 0;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        int64_t n = 0;
        a.x[l] = nullptr;
        if (l < g->num_levels) {
            if (g->H[l] < 1 || g->W[l] < 1 || !x[l] || ((uintptr_t)x[l] & align)) return IA_E_ARG;
            n = (int64_t)g->batch * g->H[l] * g->W[l] * (channels / 4);
            a.x[l] = x[l];
        }
        a.vec_off[l + 1] = a.vec_off[l] + n;
    }
    const int64_t n = a.vec_off[IA_MAX_LEVELS];
    if (n > (1LL << 40)) return IA_E_ARG;
    hipLaunchKernelGGL(dtype == IA_BF16 ? ia::k_scale_exp_bf16 : ia::k_scale_exp,
                       dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
}

int ia_scale_exp_levels(const ia_wino_geom *g, float *const *x, int channels, const float *scales,
                        void *stream)
{
    return scale_exp_impl(g, reinterpret_cast<void *const *>(x), channels, IA_F32, scales, stream);
}

int ia_scale_exp_levels_dt(const ia_wino_geom *g, void *const *x, int dtype, int channels,
                           const float *scales, void *stream)
{
    return scale_exp_impl(g, x, channels, dtype, scales, stream);
}

size_t ia_groupnorm_workspace_bytes_dt(const ia_wino_geom *g, int channels, int groups, int dtype)
{
    ia::GnArgs a;
    if (ia::gn_args_dt(g, channels, groups, dtype, a)) return 0;
    return ia::align256((size_t)a.blk_off[IA_MAX_LEVELS] * groups * sizeof(double2));
}

int ia_groupnorm_stats_dt(const ia_wino_geom *g, const void *const *x, int dtype, int channels,
                          int groups, void *workspace, size_t workspace_bytes, void *stream)
{
    ia::GnArgs a;
    int rc = ia::gn_args_dt(g, channels, groups, dtype, a);
    if (rc) return rc;
    if (!x || !workspace) return IA_E_ARG;
    if (workspace_bytes < ia_groupnorm_workspace_bytes_dt(g, channels, groups, dtype))
        return IA_E_WORKSPACE;
    if (!ia::gn_level_ptrs(a.num_levels, x, a.x)) return IA_E_ARG;
    a.part = static_cast<double2 *>(workspace);
    return ia::gn_launch(dtype, ia::k_gn_stats, ia::k_gn_stats_bf16, a, stream);
}

int ia_groupnorm_apply_dt(const ia_wino_geom *g, void *const *x, int dtype, int channels, int groups,
                          const float *gamma, const float *beta, float eps, int relu,
                          const void *workspace, size_t workspace_bytes, void *stream)
{
    ia::GnArgs a;
    int rc = ia::gn_args_dt(g, channels, groups, dtype, a);
    if (rc) return rc;
    if (!x || !workspace || !gamma || !beta || !(eps >= 0.0f)) return IA_E_ARG;
    if (workspace_bytes < ia_groupnorm_workspace_bytes_dt(g, channels, groups, dtype))
        return IA_E_WORKSPACE;
    if (!ia::gn_level_ptrs<const void>(a.num_levels, x, a.x)) return IA_E_ARG;
    a.gamma = gamma; a.beta = beta; a.eps = eps; a.relu = relu ? 1 : 0;
    a.part = const_cast<double2 *>(static_cast<const double2 *>(workspace));
    return ia::gn_launch(dtype, ia::k_gn_apply, ia::k_gn_apply_bf16, a, stream);
}

size_t ia_groupnorm_workspace_bytes(const ia_wino_geom *g, int channels, int groups)
{
    return ia_groupnorm_workspace_bytes_dt(g, channels, groups, IA_F32);
}

int ia_groupnorm_stats(const ia_wino_geom *g, const float *const *x, int channels, int groups,
                       void *workspace, size_t workspace_bytes, void *stream)
{
    return ia_groupnorm_stats_dt(g, reinterpret_cast<const void *const *>(x), IA_F32, channels,
                                 groups, workspace, workspace_bytes, stream);
}

int ia_groupnorm_apply(const ia_wino_geom *g, float *const *x, int channels, int groups,
                       const float *gamma, const float *beta, float eps, int relu,
                       const void *workspace, size_t workspace_bytes, void *stream)
{
    return ia_groupnorm_apply_dt(g, reinterpret_cast<void *const *>(x), IA_F32, channels, groups,
                                 gamma, beta, eps, relu, workspace, workspace_bytes, stream);
}

// The training entries for dtype IA_F32 / IA_BF16: one body each, the non-_dt names forward IA_F32.
size_t ia_groupnorm_saved_bytes_dt(const ia_wino_geom *g, int channels, int groups, int dtype)
{
    ia::GnArgs a;
    if (ia::gn_args_dt(g, channels, groups, dtype, a)) return 0;
    return ia::align256((size_t)a.num_levels * a.batch * groups * sizeof(double2));
}

size_t ia_groupnorm_saved_bytes(const ia_wino_geom *g, int channels, int groups)
{
    return ia_groupnorm_saved_bytes_dt(g, channels, groups, IA_F32);
}

int ia_groupnorm_apply_to_dt(const ia_wino_geom *g, const void *const *x, void *const *y, int dtype,
                             int channels, int groups, const float *gamma, const float *beta,
                             float eps, int relu, const void *workspace, size_t workspace_bytes,
                             void *saved, size_t saved_bytes, void *stream)
{
    ia::GnArgs a;
    int rc = ia::gn_args_dt(g, channels, groups, dtype, a);
    if (rc) return rc;
    if (!workspace || !saved || !gamma || !beta || !(eps >= 0.0f)) return IA_E_ARG;
    if (((uintptr_t)workspace & 15u) || ((uintptr_t)saved & 15u)) return IA_E_ARG;
    if (!ia::gn_level_ptrs(a.num_levels, x, a.x) || !ia::gn_level_ptrs(a.num_levels, y, a.out))
        return IA_E_ARG;
    for (int l = 0; l < a.num_levels; ++l)
        if (x[l] == y[l]) return IA_E_ARG;             // out of place: ia_groupnorm_apply otherwise
    if (workspace_bytes < ia_groupnorm_workspace_bytes_dt(g, channels, groups, dtype) ||
        saved_bytes < ia_groupnorm_saved_bytes_dt(g, channels, groups, dtype))
        return IA_E_WORKSPACE;
    a.gamma = gamma; a.beta = beta; a.eps = eps; a.relu = relu ? 1 : 0;
    a.part = const_cast<double2 *>(static_cast<const double2 *>(workspace));
    a.saved = static_cast<double2 *>(saved);
    return ia::gn_launch(dtype, ia::k_gn_apply_to, ia::k_gn_apply_to_bf16, a, stream);
}

int ia_groupnorm_apply_to(const ia_wino_geom *g, const float *const *x, float *const *y,
                          int channels, int groups, const float *gamma, const float *beta,
                          float eps, int relu, const void *workspace, size_t workspace_bytes,
                          void *saved, size_t saved_bytes, void *stream)
{
    return ia_groupnorm_apply_to_dt(g, reinterpret_cast<const void *const *>(x),
                                    reinterpret_cast<void *const *>(y), IA_F32, channels, groups,
                                    gamma, beta, eps, relu, workspace, workspace_bytes, saved,
                                    saved_bytes, stream);
}

size_t ia_groupnorm_bwd_workspace_bytes_dt(const ia_wino_geom *g, int channels, int groups,
                                           int dtype)
{
    ia::GnArgs a;
    if (ia::gn_args_dt(g, channels, groups, dtype, a)) return 0;
    const size_t rows = (size_t)a.blk_off[IA_MAX_LEVELS];
    return ia::align256(rows * ((size_t)groups + channels) * sizeof(double2));
}

size_t ia_groupnorm_bwd_workspace_bytes(const ia_wino_geom *g, int channels, int groups)
{
    return ia_groupnorm_bwd_workspace_bytes_dt(g, channels, groups, IA_F32);
}

static int gn_bwd_args(const ia_wino_geom *g, const void *const *x, const void *const *dy, int dtype,
                       int channels, int groups, const float *gamma, const float *beta,
                       const void *saved, size_t saved_bytes, int relu, void *workspace,
                       size_t workspace_bytes, ia::GnArgs &a)
{
    int rc = ia::gn_args_dt(g, channels, groups, dtype, a);
    if (rc) return rc;
    if (!workspace || !saved || !gamma || !beta) return IA_E_ARG;
    if (((uintptr_t)workspace & 15u) || ((uintptr_t)saved & 15u)) return IA_E_ARG;
    if (!ia::gn_level_ptrs(a.num_levels, x, a.x) || !ia::gn_level_ptrs(a.num_levels, dy, a.dy))
        return IA_E_ARG;
    if (workspace_bytes < ia_groupnorm_bwd_workspace_bytes_dt(g, channels, groups, dtype) ||
        saved_bytes < ia_groupnorm_saved_bytes_dt(g, channels, groups, dtype))
        return IA_E_WORKSPACE;
    a.gamma = gamma; a.beta = beta; a.relu = relu ? 1 : 0;
    a.saved = const_cast<double2 *>(static_cast<const double2 *>(saved));
    a.gpart = static_cast<double2 *>(workspace);
    a.cpart = a.gpart + (size_t)a.blk_off[IA_MAX_LEVELS] * groups;
    return 0;
}

int ia_groupnorm_bwd_reduce_dt(const ia_wino_geom *g, const void *const *x, const void *const *dy,
                               int dtype, int channels, int groups, const float *gamma,
                               const float *beta, int relu, const void *saved, size_t saved_bytes,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    ia::GnArgs a;
    int rc = gn_bwd_args(g, x, dy, dtype, channels, groups, gamma, beta, saved, saved_bytes, relu,
                         workspace, workspace_bytes, a);
    if (rc) return rc;
    return ia::gn_launch(dtype, ia::k_gn_bwd_reduce, ia::k_gn_bwd_reduce_bf16, a, stream);
}

int ia_groupnorm_bwd_reduce(const ia_wino_geom *g, const float *const *x, const float *const *dy,
                            int channels, int groups, const float *gamma, const float *beta,
                            int relu, const void *saved, size_t saved_bytes, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    return ia_groupnorm_bwd_reduce_dt(g, reinterpret_cast<const void *const *>(x),
                                      reinterpret_cast<const void *const *>(dy), IA_F32, channels,
                                      groups, gamma, beta, relu, saved, saved_bytes, workspace,
                                      workspace_bytes, stream);
}

int ia_groupnorm_bwd_apply_dt(const ia_wino_geom *g, const void *const *x, const void *const *dy,
                              void *const *dx, int dtype, int channels, int groups,
                              const float *gamma, const float *beta, int relu, const void *saved,
                              size_t saved_bytes, const void *workspace, size_t workspace_bytes,
                              float *dgamma, float *dbeta, void *stream)
{
    ia::GnArgs a;
    int rc = gn_bwd_args(g, x, dy, dtype, channels, groups, gamma, beta, saved, saved_bytes, relu,
                         const_cast<void *>(workspace), workspace_bytes, a);
    if (rc) return rc;
    if (dx) {                                           // NULL: parameter gradients only
        if (!ia::gn_level_ptrs(a.num_levels, dx, a.out)) return IA_E_ARG;
        for (int l = 0; l < a.num_levels; ++l)
            if (dx[l] == dy[l] || dx[l] == x[l]) return IA_E_ARG;
        rc = ia::gn_launch(dtype, ia::k_gn_bwd_apply, ia::k_gn_bwd_apply_bf16, a, stream);
        if (rc) return rc;
    }
    if (dgamma || dbeta) {
        hipLaunchKernelGGL(ia::k_gn_bwd_params, dim3((unsigned)((channels + 15) / 16)),
                           dim3(ia::kGnThreads), 0, (hipStream_t)stream, a.cpart,
                           a.blk_off[IA_MAX_LEVELS], channels, dgamma, dbeta);
        rc = ia::hip_status(hipGetLastError());
    }
    return rc;
}

int ia_groupnorm_bwd_apply(const ia_wino_geom *g, const float *const *x, const float *const *dy,
                           float *const *dx, int channels, int groups, const float *gamma,
                           const float *beta, int relu, const void *saved, size_t saved_bytes,
                           const void *workspace, size_t workspace_bytes, float *dgamma,
                           float *dbeta, void *stream)
{
    return ia_groupnorm_bwd_apply_dt(g, reinterpret_cast<const void *const *>(x),
                                     reinterpret_cast<const void *const *>(dy),
                                     reinterpret_cast<void *const *>(dx), IA_F32, channels, groups,
                                     gamma, beta, relu, saved, saved_bytes, workspace,
                                     workspace_bytes, dgamma, dbeta, stream);
}

}  // extern "C"
