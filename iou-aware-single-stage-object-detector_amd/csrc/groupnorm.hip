// GroupNorm + ReLU of the IoU-aware FCOS head towers (reference
// mmdet/models/anchor_heads/iou_aware_fcos_head.py:41-62, ConvModule(3x3, GN(32), ReLU); torch
// nn.GroupNorm semantics: biased variance, eps inside the square root): the in-place inference pair,
// and further down the out-of-place forward and the backward of the training node.
//
// Input: the activations the Winograd output transform writes, per level (B, H_l, W_l, channels)
// fp32 channels-last; all levels and images of a tower layer in one pair of launches.
//
//   k_gn_stats   one workgroup per (level, image, chunk of IA_GN_CHUNK pixels): every thread owns
//                one 16-byte column of channels (inside one group, channels / groups % 4 == 0) and
//                a strided subset of the chunk's pixels and accumulates fp64 sum and sum of
//                squares (x * x is exact in fp64); the threads of a group are added in a fixed
//                order through LDS and the workgroup writes (sum, sumsq) per group to its own slot
//                of the workspace.  No atomics: the bits do not depend on scheduling.
//   k_gn_apply   one workgroup per (level, image, chunk) again: the first `groups` threads add
//                their group's partials over the (level, image)'s chunks in index order (fp64),
//                mean = S / n, var = max(SS / n - mean^2, 0) -- fp64 keeps E[x^2] - E[x]^2 exact
//                enough for |mean| >> std (a one-pass fp32 form loses ~(mean/std)^2 * 2^-24 of
//                the variance) --, then per channel s = gamma * rstd, t = beta - mean * s (fp64,
//                rounded once), and every thread rewrites its column x = relu?(x * s + t) with
//                16-byte loads and stores.
//
// The partials of an (image, level) come from that image's pixels only and are summed in the same
// order whatever else shares the launch: an image alone gives the same bits as inside a batch.
#include "ia_internal.hpp"
#include "ia_math.hpp"

namespace ia {

constexpr int kGnThreads = 256;

struct GnArgs {
    int32_t num_levels, batch, channels, groups;
    int32_t HW[IA_MAX_LEVELS];
    int32_t nch[IA_MAX_LEVELS];                 // chunks per image of level l
    int32_t blk_off[IA_MAX_LEVELS + 1];         // prefix over levels of batch * nch[l] (= slab rows)
    float *x[IA_MAX_LEVELS];
    const float *gamma, *beta;
    float eps;
    int32_t relu;
    double2 *part;                              // (slab rows, groups) (sum, sumsq)
};

struct GnBlock { int l, b, chunk, HW, nch, row0; float *x; };

__device__ __forceinline__ GnBlock gn_block(const GnArgs &a, int blk)
{
    GnBlock k;
    int l = 0;
#pragma unroll
    for (int i = 1; i < IA_MAX_LEVELS; ++i) l += (i < a.num_levels && blk >= a.blk_off[i]) ? 1 : 0;
    k.l = l;
    k.HW = a.HW[0]; k.nch = a.nch[0]; k.x = a.x[0];
    int off = a.blk_off[0];
#pragma unroll
    for (int i = 1; i < IA_MAX_LEVELS; ++i) {
        const bool m = l == i;
        k.HW = m ? a.HW[i] : k.HW; k.nch = m ? a.nch[i] : k.nch; k.x = m ? a.x[i] : k.x;
        off = m ? a.blk_off[i] : off;
    }
    const int rem = blk - off;
    k.b = rem / k.nch;
    k.chunk = rem - k.b * k.nch;
    k.row0 = off + k.b * k.nch;                 // slab row of chunk 0 of this (level, image)
    return k;
}

__global__ void __launch_bounds__(kGnThreads) k_gn_stats(GnArgs a)
{
    __shared__ double s_sum[kGnThreads], s_sq[kGnThreads];
    const GnBlock k = gn_block(a, blockIdx.x);
    const int tid = threadIdx.x;
    const int vc = a.channels >> 2;             // 16-byte columns per pixel (divides kGnThreads)
    const int rows = kGnThreads / vc;           // pixels per pass
    const int v = tid % vc, r = tid / vc;
    const int p0 = k.chunk * IA_GN_CHUNK;
    const int p1 = min(p0 + IA_GN_CHUNK, k.HW);
    const float4 *x = reinterpret_cast<const float4 *>(k.x + (size_t)k.b * k.HW * a.channels) + v;
    double s = 0.0, ss = 0.0;
    for (int p = p0 + r; p < p1; p += rows) {
        const float4 q = x[(size_t)p * vc];
        const double d0 = q.x, d1 = q.y, d2 = q.z, d3 = q.w;
        s += ((d0 + d1) + (d2 + d3));
        ss += ((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3));
    }
    s_sum[tid] = s;
    s_sq[tid] = ss;
    __syncthreads();
    const int vpg = (a.channels / a.groups) >> 2;    // columns per group
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

__global__ void __launch_bounds__(kGnThreads) k_gn_apply(GnArgs a)
{
    __shared__ double s_mean[256], s_rstd[256];
    __shared__ float4 s_scale[256], s_shift[256];
    const GnBlock k = gn_block(a, blockIdx.x);
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
        s_mean[g] = mean;
        s_rstd[g] = 1.0 / sqrt(var + (double)a.eps);
    }
    __syncthreads();
    const int vc = a.channels >> 2;
    for (int v = tid; v < vc; v += kGnThreads) {
        const int g = (4 * v) / cpg;
        const double mean = s_mean[g], rstd = s_rstd[g];
        float sc[4], sh[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * v + j;
            sc[j] = (float)((double)a.gamma[c] * rstd);
            sh[j] = (float)((double)a.beta[c] - mean * (double)sc[j]);
        }
        s_scale[v] = make_float4(sc[0], sc[1], sc[2], sc[3]);
        s_shift[v] = make_float4(sh[0], sh[1], sh[2], sh[3]);
    }
    __syncthreads();
    const int rows = kGnThreads / vc;
    const int v = tid % vc, r = tid / vc;
    const float4 sc = s_scale[v], sh = s_shift[v];
    const int p0 = k.chunk * IA_GN_CHUNK;
    const int p1 = min(p0 + IA_GN_CHUNK, k.HW);
    float4 *x = reinterpret_cast<float4 *>(k.x + (size_t)k.b * k.HW * a.channels) + v;
    for (int p = p0 + r; p < p1; p += rows) {
        float4 q = x[(size_t)p * vc];
        q.x = q.x * sc.x + sh.x;
        q.y = q.y * sc.y + sh.y;
        q.z = q.z * sc.z + sh.z;
        q.w = q.w * sc.w + sh.w;
        if (a.relu) {
            q.x = q.x > 0.0f ? q.x : 0.0f;
            q.y = q.y > 0.0f ? q.y : 0.0f;
            q.z = q.z > 0.0f ? q.z : 0.0f;
            q.w = q.w > 0.0f ? q.w : 0.0f;
        }
        x[(size_t)p * vc] = q;
    }
}

// ------------------------------------------------------------------ bf16 (in place, inference)
// The same pair on (B, H_l, W_l, channels) bf16 channels-last activations (the towers of the bf16
// head route, conv3x3_bf16.hip in front): GnArgs::x[l] then carries the bf16 base pointers.  A
// thread's 16-byte column is 8 channels (inside one group: channels / groups % 8 == 0); the values
// convert exactly to fp32 / fp64, so the statistics are those of the stored numbers, accumulated
// and combined exactly as above.  The apply forms s and t as above, evaluates x * s + t (and the
// ReLU) in fp32 and rounds ONCE to bf16 (nearest even).
__device__ __forceinline__ const uint16_t *gn_image_bf16(const GnBlock &k, int channels)
{
    return reinterpret_cast<const uint16_t *>(k.x) + (size_t)k.b * k.HW * channels;
}

__global__ void __launch_bounds__(kGnThreads) k_gn_stats_bf16(GnArgs a)
{
    __shared__ double s_sum[kGnThreads], s_sq[kGnThreads];
    const GnBlock k = gn_block(a, blockIdx.x);
    const int tid = threadIdx.x;
    const int vc = a.channels >> 3;             // 16-byte columns per pixel (divides kGnThreads)
    const int rows = kGnThreads / vc;           // pixels per pass
    const int v = tid % vc, r = tid / vc;
    const int p0 = k.chunk * IA_GN_CHUNK;
    const int p1 = min(p0 + IA_GN_CHUNK, k.HW);
    const uint4 *x = reinterpret_cast<const uint4 *>(gn_image_bf16(k, a.channels)) + v;
    double s = 0.0, ss = 0.0;
    for (int p = p0 + r; p < p1; p += rows) {
        float f[8];
        bf16x8_to_f32(x[(size_t)p * vc], f);
        const double d0 = f[0], d1 = f[1], d2 = f[2], d3 = f[3], d4 = f[4], d5 = f[5], d6 = f[6],
                     d7 = f[7];
        s += (((d0 + d1) + (d2 + d3)) + ((d4 + d5) + (d6 + d7)));
        ss += (((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3)) +
               ((d4 * d4 + d5 * d5) + (d6 * d6 + d7 * d7)));
    }
    s_sum[tid] = s;
    s_sq[tid] = ss;
    __syncthreads();
    const int vpg = (a.channels / a.groups) >> 3;    // columns per group
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

__global__ void __launch_bounds__(kGnThreads) k_gn_apply_bf16(GnArgs a)
{
    __shared__ double s_mean[256], s_rstd[256];
    __shared__ float4 s_scale[256], s_shift[256];      // per 4 channels
    const GnBlock k = gn_block(a, blockIdx.x);
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
        s_mean[g] = mean;
        s_rstd[g] = 1.0 / sqrt(var + (double)a.eps);
    }
    __syncthreads();
    for (int q = tid; q < (a.channels >> 2); q += kGnThreads) {
        const int g = (4 * q) / cpg;
        const double mean = s_mean[g], rstd = s_rstd[g];
        float sc[4], sh[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * q + j;
            sc[j] = (float)((double)a.gamma[c] * rstd);
            sh[j] = (float)((double)a.beta[c] - mean * (double)sc[j]);
        }
        s_scale[q] = make_float4(sc[0], sc[1], sc[2], sc[3]);
        s_shift[q] = make_float4(sh[0], sh[1], sh[2], sh[3]);
    }
    __syncthreads();
    const int vc = a.channels >> 3;
    const int rows = kGnThreads / vc;
    const int v = tid % vc, r = tid / vc;
    const float4 sa = s_scale[2 * v], sb = s_scale[2 * v + 1];
    const float4 ta = s_shift[2 * v], tb = s_shift[2 * v + 1];
    const float sc[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
    const float sh[8] = {ta.x, ta.y, ta.z, ta.w, tb.x, tb.y, tb.z, tb.w};
    const int p0 = k.chunk * IA_GN_CHUNK;
    const int p1 = min(p0 + IA_GN_CHUNK, k.HW);
    uint4 *x = reinterpret_cast<uint4 *>(const_cast<uint16_t *>(gn_image_bf16(k, a.channels))) + v;
    for (int p = p0 + r; p < p1; p += rows) {
        float f[8];
        bf16x8_to_f32(x[(size_t)p * vc], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            f[j] = f[j] * sc[j] + sh[j];
            if (a.relu) f[j] = f[j] > 0.0f ? f[j] : 0.0f;
        }
        x[(size_t)p * vc] = f32_to_bf16x8(f);
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
        a.x[l] = nullptr;
    }
    a.gamma = a.beta = nullptr; a.eps = 0.0f; a.relu = 0; a.part = nullptr;
    return 0;
}

// what the bf16 pair takes on top of gn_args: whole 16-byte columns inside a group
static int gn_args_dt(const ia_wino_geom *g, int channels, int groups, int dtype, GnArgs &a)
{
    if (dtype != IA_F32 && dtype != IA_BF16) return IA_E_ARG;
    int rc = gn_args(g, channels, groups, a);
    if (rc) return rc;
    if (dtype == IA_BF16 && (channels < 8 || (channels / groups) % 8 != 0)) return IA_E_ARG;
    return 0;
}

// ------------------------------------------------------------------ training node
// Out-of-place forward and the backward of y = relu?(GroupNorm(x)) over the same level lists and the
// same (level, image, chunk) workgroups.  With xh = (x - mean) * rstd, g = dy * [x * s + t > 0]
// (the forward's fp32 expression: the same mask bit for bit) and n = channels / groups * H_l * W_l:
//     dbeta_c = sum g,  dgamma_c = sum g * xh  (all pixels, images, levels)
//     dx = rstd * (gamma * g - mean_grp(gamma * g) - xh * mean_grp(gamma * g * xh))
//   k_gn_apply_to     k_gn_apply writing y to a second tensor; chunk 0 of every (level, image) also
//                     leaves (mean, rstd) per group in fp64 for the backward.
//   k_gn_bwd_reduce   every thread owns a 16-byte column and a strided subset of the chunk's pixels
//                     and accumulates sum g and sum g * x per channel in fp64 (the product of two
//                     floats is exact there); the threads of a column are added in a fixed order
//                     through LDS, sum g * xh = rstd * (sum g * x - mean * sum g), and the workgroup
//                     writes (sum g, sum g * xh) per channel and, weighted by gamma and added over a
//                     group's channels in index order, per group to its own workspace rows.
//   k_gn_bwd_apply    the first `groups` threads add the group partials of the (level, image) over
//                     its chunks in index order; dx = s * g + (c1 + xc * c2) per element with
//                     s = gamma * rstd as in the forward, c1 = -rstd * m1, c2 = -rstd^2 * m2 and
//                     xc = (x - mean_hi) - mean_lo: the mean as two floats, so that |mean| >> std
//                     costs nothing (x - mean_hi is exact there).
//   k_gn_bwd_params   per channel the (sum g, sum g * xh) rows in a fixed order: kGnSeg contiguous
//                     runs of rows (level-major / image / chunk), each in index order by one thread,
//                     then the runs in index order.
// No atomics; dy is only read; an image's dx depends on its own pixels only.
struct GnTrainArgs {
    int32_t num_levels, batch, channels, groups;
    int32_t HW[IA_MAX_LEVELS];
    int32_t nch[IA_MAX_LEVELS];
    int32_t blk_off[IA_MAX_LEVELS + 1];
    const float *x[IA_MAX_LEVELS];
    const float *dy[IA_MAX_LEVELS];             // backward only
    float *out[IA_MAX_LEVELS];                  // y (forward) / dx (backward apply)
    const float *gamma, *beta;
    float eps;
    int32_t relu;
    const double2 *part;                        // forward: the (sum, sumsq) rows of k_gn_stats
    double2 *saved;                             // (num_levels * batch, groups) (mean, rstd)
    double2 *gpart;                             // (slab rows, groups)   (sum gamma g, sum gamma g xh)
    double2 *cpart;                             // (slab rows, channels) (sum g, sum g xh)
};

struct GnTrainBlock { int l, b, chunk, HW, nch, row0; const float *x, *dy; float *out; };

template <bool kBwd>
__device__ __forceinline__ GnTrainBlock gn_train_block(const GnTrainArgs &a, int blk)
{
    GnTrainBlock k;
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
    if (kBwd) {
        k.dy = a.dy[0];
#pragma unroll
        for (int i = 1; i < IA_MAX_LEVELS; ++i) k.dy = (l == i) ? a.dy[i] : k.dy;
    }
    k.out = a.out[0];
#pragma unroll
    for (int i = 1; i < IA_MAX_LEVELS; ++i) k.out = (l == i) ? a.out[i] : k.out;
    const int rem = blk - off;
    k.b = rem / k.nch;
    k.chunk = rem - k.b * k.nch;
    k.row0 = off + k.b * k.nch;
    return k;
}

// per channel s = gamma * rstd, t = beta - mean * s: fp64, rounded once (k_gn_apply's expression)
__device__ __forceinline__ void gn_scale_shift(const float *gamma, const float *beta, int v,
                                               double mean, double rstd, float4 &sc, float4 &sh)
{
    float s[4], t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * v + j;
        s[j] = (float)((double)gamma[c] * rstd);
        t[j] = (float)((double)beta[c] - mean * (double)s[j]);
    }
    sc = make_float4(s[0], s[1], s[2], s[3]);
    sh = make_float4(t[0], t[1], t[2], t[3]);
}

__global__ void __launch_bounds__(kGnThreads) k_gn_apply_to(GnTrainArgs a)
{
    __shared__ double s_mean[256], s_rstd[256];
    __shared__ float4 s_scale[256], s_shift[256];
    const GnTrainBlock k = gn_train_block<false>(a, blockIdx.x);
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
        if (k.chunk == 0)
            a.saved[(size_t)(k.l * a.batch + k.b) * a.groups + g] = make_double2(mean, rstd);
    }
    __syncthreads();
    const int vc = a.channels >> 2;
    for (int v = tid; v < vc; v += kGnThreads) {
        const int g = (4 * v) / cpg;
        float4 sc, sh;
        gn_scale_shift(a.gamma, a.beta, v, s_mean[g], s_rstd[g], sc, sh);
        s_scale[v] = sc;
        s_shift[v] = sh;
    }
    __syncthreads();
    const int rows = kGnThreads / vc;
    const int v = tid % vc, r = tid / vc;
    const float4 sc = s_scale[v], sh = s_shift[v];
    const int p0 = k.chunk * IA_GN_CHUNK;
    const int p1 = min(p0 + IA_GN_CHUNK, k.HW);
    const size_t img = (size_t)k.b * k.HW * a.channels;
    const float4 *x = reinterpret_cast<const float4 *>(k.x + img) + v;
    float4 *y = reinterpret_cast<float4 *>(k.out + img) + v;
    for (int p = p0 + r; p < p1; p += rows) {
        float4 q = x[(size_t)p * vc];
        q.x = q.x * sc.x + sh.x;
        q.y = q.y * sc.y + sh.y;
        q.z = q.z * sc.z + sh.z;
        q.w = q.w * sc.w + sh.w;
        if (a.relu) {
            q.x = q.x > 0.0f ? q.x : 0.0f;
            q.y = q.y > 0.0f ? q.y : 0.0f;
            q.z = q.z > 0.0f ? q.z : 0.0f;
            q.w = q.w > 0.0f ? q.w : 0.0f;
        }
        y[(size_t)p * vc] = q;
    }
}

// g = dy where the forward's pre-activation is positive (all of dy without the ReLU)
__device__ __forceinline__ float4 gn_masked(const float4 q, const float4 d, const float4 sc,
                                            const float4 sh, int relu)
{
    float4 g = d;
    if (relu) {
        g.x = (q.x * sc.x + sh.x) > 0.0f ? d.x : 0.0f;
        g.y = (q.y * sc.y + sh.y) > 0.0f ? d.y : 0.0f;
        g.z = (q.z * sc.z + sh.z) > 0.0f ? d.z : 0.0f;
        g.w = (q.w * sc.w + sh.w) > 0.0f ? d.w : 0.0f;
    }
    return g;
}

__global__ void __launch_bounds__(kGnThreads) k_gn_bwd_reduce(GnTrainArgs a)
{
    __shared__ double s_acc[8][kGnThreads];     // [2 * j + (0: g, 1: g x)][thread]
    __shared__ double2 s_ch[1024];              // per channel gamma * (sum g, sum g xh)
    const GnTrainBlock k = gn_train_block<true>(a, blockIdx.x);
    const int tid = threadIdx.x;
    const int cpg = a.channels / a.groups;
    const int vc = a.channels >> 2;
    const int rows = kGnThreads / vc;
    const int v = tid % vc, r = tid / vc;
    const double2 *saved = a.saved + (size_t)(k.l * a.batch + k.b) * a.groups;
    float4 sc, sh;
    {
        const double2 mr = saved[(4 * v) / cpg];
        gn_scale_shift(a.gamma, a.beta, v, mr.x, mr.y, sc, sh);
    }
    const int p0 = k.chunk * IA_GN_CHUNK;
    const int p1 = min(p0 + IA_GN_CHUNK, k.HW);
    const size_t img = (size_t)k.b * k.HW * a.channels;
    const float4 *x = reinterpret_cast<const float4 *>(k.x + img) + v;
    const float4 *dy = reinterpret_cast<const float4 *>(k.dy + img) + v;
    double sg[4] = {0.0, 0.0, 0.0, 0.0}, sx[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = p0 + r; p < p1; p += rows) {
        const float4 q = x[(size_t)p * vc];
        const float4 g = gn_masked(q, dy[(size_t)p * vc], sc, sh, a.relu);
        const double g0 = g.x, g1 = g.y, g2 = g.z, g3 = g.w;
        sg[0] += g0; sg[1] += g1; sg[2] += g2; sg[3] += g3;
        sx[0] += g0 * (double)q.x; sx[1] += g1 * (double)q.y;
        sx[2] += g2 * (double)q.z; sx[3] += g3 * (double)q.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s_acc[2 * j][tid] = sg[j];
        s_acc[2 * j + 1][tid] = sx[j];
    }
    __syncthreads();
    const size_t row = (size_t)(k.row0 + k.chunk);
    for (int c = tid; c < a.channels; c += kGnThreads) {
        const int cv = c >> 2, j = c & 3;
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

__global__ void __launch_bounds__(kGnThreads) k_gn_bwd_apply(GnTrainArgs a)
{
    __shared__ double2 s_mr[256];
    __shared__ float4 s_k[256];                 // per group (mean_hi, mean_lo, c1, c2)
    const GnTrainBlock k = gn_train_block<true>(a, blockIdx.x);
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
    const int vc = a.channels >> 2;
    const int rows = kGnThreads / vc;
    const int v = tid % vc, r = tid / vc;
    const int grp = (4 * v) / cpg;
    float4 sc, sh;
    gn_scale_shift(a.gamma, a.beta, v, s_mr[grp].x, s_mr[grp].y, sc, sh);
    const float4 kk = s_k[grp];
    const int p0 = k.chunk * IA_GN_CHUNK;
    const int p1 = min(p0 + IA_GN_CHUNK, k.HW);
    const size_t img = (size_t)k.b * k.HW * a.channels;
    const float4 *x = reinterpret_cast<const float4 *>(k.x + img) + v;
    const float4 *dy = reinterpret_cast<const float4 *>(k.dy + img) + v;
    float4 *dx = reinterpret_cast<float4 *>(k.out + img) + v;
    for (int p = p0 + r; p < p1; p += rows) {
        const float4 q = x[(size_t)p * vc];
        const float4 g = gn_masked(q, dy[(size_t)p * vc], sc, sh, a.relu);
        float4 o;
        o.x = sc.x * g.x + (kk.z + ((q.x - kk.x) - kk.y) * kk.w);
        o.y = sc.y * g.y + (kk.z + ((q.y - kk.x) - kk.y) * kk.w);
        o.z = sc.z * g.z + (kk.z + ((q.z - kk.x) - kk.y) * kk.w);
        o.w = sc.w * g.w + (kk.z + ((q.w - kk.x) - kk.y) * kk.w);
        dx[(size_t)p * vc] = o;
    }
}

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

// ------------------------------------------------------------------ training node, bf16
// The same three kernels on (B, H_l, W_l, channels) bf16 channels-last x, dy, y and dx (the towers of
// the bf16 training route, conv3x3_bf16.hip in front and behind): GnTrainArgs::x / dy / out then
// carry the bf16 base pointers.  A thread's 16-byte column is 8 channels (inside one group: channels
// / groups % 8 == 0).  x and dy widen exactly, so every expression is the fp32 kernel's on the stored
// values: the mask is the forward's fp32 pre-activation float(x) * s + t > 0 (y is not kept), sum g
// and sum g * x are exact products in fp64, and y and dx are rounded ONCE to bf16 (nearest even).
// The (mean, rstd) rows, the workspace rows and k_gn_bwd_params are those of the fp32 node.
__device__ __forceinline__ const uint16_t *gn_image_bf16(const float *base, int b, int HW,
                                                         int channels)
{
    return reinterpret_cast<const uint16_t *>(base) + (size_t)b * HW * channels;
}

// the column's 8 per-channel (s, t): quads 2 v and 2 v + 1 of gn_scale_shift
__device__ __forceinline__ void gn_scale_shift8(const float *gamma, const float *beta, int v,
                                                double mean, double rstd, float (&sc)[8],
                                                float (&sh)[8])
{
    float4 sa, sb, ta, tb;
    gn_scale_shift(gamma, beta, 2 * v, mean, rstd, sa, ta);
    gn_scale_shift(gamma, beta, 2 * v + 1, mean, rstd, sb, tb);
    sc[0] = sa.x; sc[1] = sa.y; sc[2] = sa.z; sc[3] = sa.w;
    sc[4] = sb.x; sc[5] = sb.y; sc[6] = sb.z; sc[7] = sb.w;
    sh[0] = ta.x; sh[1] = ta.y; sh[2] = ta.z; sh[3] = ta.w;
    sh[4] = tb.x; sh[5] = tb.y; sh[6] = tb.z; sh[7] = tb.w;
}

__global__ void __launch_bounds__(kGnThreads) k_gn_apply_to_bf16(GnTrainArgs a)
{
    __shared__ double s_mean[256], s_rstd[256];
    __shared__ float4 s_scale[256], s_shift[256];      // per 4 channels
    const GnTrainBlock k = gn_train_block<false>(a, blockIdx.x);
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
        if (k.chunk == 0)
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
    const int vc = a.channels >> 3;
    const int rows = kGnThreads / vc;
    const int v = tid % vc, r = tid / vc;
    const float4 sa = s_scale[2 * v], sb = s_scale[2 * v + 1];
    const float4 ta = s_shift[2 * v], tb = s_shift[2 * v + 1];
    const float sc[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
    const float sh[8] = {ta.x, ta.y, ta.z, ta.w, tb.x, tb.y, tb.z, tb.w};
    const int p0 = k.chunk * IA_GN_CHUNK;
    const int p1 = min(p0 + IA_GN_CHUNK, k.HW);
    const uint4 *x = reinterpret_cast<const uint4 *>(gn_image_bf16(k.x, k.b, k.HW, a.channels)) + v;
    uint4 *y = reinterpret_cast<uint4 *>(
                   const_cast<uint16_t *>(gn_image_bf16(k.out, k.b, k.HW, a.channels))) + v;
#pragma unroll 2
    for (int p = p0 + r; p < p1; p += rows) {
        float f[8];
        bf16x8_to_f32(x[(size_t)p * vc], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            f[j] = f[j] * sc[j] + sh[j];
            if (a.relu) f[j] = f[j] > 0.0f ? f[j] : 0.0f;
        }
        y[(size_t)p * vc] = f32_to_bf16x8(f);
    }
}

// g = dy where the forward's fp32 pre-activation is positive (all of dy without the ReLU)
__device__ __forceinline__ void gn_masked8(const float (&x)[8], float (&g)[8], const float (&sc)[8],
                                           const float (&sh)[8], int relu)
{
    if (relu) {
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = (x[j] * sc[j] + sh[j]) > 0.0f ? g[j] : 0.0f;
    }
}

// LDS: a column's 8 channels x 2 sums x 256 threads in doubles would be 32 KB on top of s_ch's 16 KB;
// the threads of a column are added in two halves instead (channels 0..3, then 4..7 of every column,
// through the fp32 kernel's 16 KB): the same fixed order per channel, one more barrier pair, and
// five workgroups per CU instead of three.
__global__ void __launch_bounds__(kGnThreads) k_gn_bwd_reduce_bf16(GnTrainArgs a)
{
    __shared__ double s_acc[8][kGnThreads];     // [2 * j + (0: g, 1: g x)][thread], j = channel & 3
    __shared__ double2 s_ch[1024];              // per channel gamma * (sum g, sum g xh)
    const GnTrainBlock k = gn_train_block<true>(a, blockIdx.x);
    const int tid = threadIdx.x;
    const int cpg = a.channels / a.groups;
    const int vc = a.channels >> 3;
    const int rows = kGnThreads / vc;
    const int v = tid % vc, r = tid / vc;
    const double2 *saved = a.saved + (size_t)(k.l * a.batch + k.b) * a.groups;
    float sc[8], sh[8];
    {
        const double2 mr = saved[(8 * v) / cpg];
        gn_scale_shift8(a.gamma, a.beta, v, mr.x, mr.y, sc, sh);
    }
    const int p0 = k.chunk * IA_GN_CHUNK;
    const int p1 = min(p0 + IA_GN_CHUNK, k.HW);
    const uint4 *x = reinterpret_cast<const uint4 *>(gn_image_bf16(k.x, k.b, k.HW, a.channels)) + v;
    const uint4 *dy = reinterpret_cast<const uint4 *>(gn_image_bf16(k.dy, k.b, k.HW, a.channels)) + v;
    double sg[8], sx[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sg[j] = sx[j] = 0.0;
#pragma unroll 2
    for (int p = p0 + r; p < p1; p += rows) {
        float q[8], g[8];
        bf16x8_to_f32(x[(size_t)p * vc], q);
        bf16x8_to_f32(dy[(size_t)p * vc], g);
        gn_masked8(q, g, sc, sh, a.relu);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double gj = g[j];
            sg[j] += gj;
            sx[j] += gj * (double)q[j];
        }
    }
    const size_t row = (size_t)(k.row0 + k.chunk);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h) __syncthreads();                 // the first half's sums are read
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s_acc[2 * j][tid] = sg[4 * h + j];
            s_acc[2 * j + 1][tid] = sx[4 * h + j];
        }
        __syncthreads();
        for (int i = tid; i < (a.channels >> 1); i += kGnThreads) {
            const int cv = i >> 2, j = i & 3;
            const int c = 8 * cv + 4 * h + j;
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

__global__ void __launch_bounds__(kGnThreads) k_gn_bwd_apply_bf16(GnTrainArgs a)
{
    __shared__ double2 s_mr[256];
    __shared__ float4 s_k[256];                 // per group (mean_hi, mean_lo, c1, c2)
    const GnTrainBlock k = gn_train_block<true>(a, blockIdx.x);
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
    const int vc = a.channels >> 3;
    const int rows = kGnThreads / vc;
    const int v = tid % vc, r = tid / vc;
    const int grp = (8 * v) / cpg;
    float sc[8], sh[8];
    gn_scale_shift8(a.gamma, a.beta, v, s_mr[grp].x, s_mr[grp].y, sc, sh);
    const float4 kk = s_k[grp];
    const int p0 = k.chunk * IA_GN_CHUNK;
    const int p1 = min(p0 + IA_GN_CHUNK, k.HW);
    const uint4 *x = reinterpret_cast<const uint4 *>(gn_image_bf16(k.x, k.b, k.HW, a.channels)) + v;
    const uint4 *dy = reinterpret_cast<const uint4 *>(gn_image_bf16(k.dy, k.b, k.HW, a.channels)) + v;
    uint4 *dx = reinterpret_cast<uint4 *>(
                    const_cast<uint16_t *>(gn_image_bf16(k.out, k.b, k.HW, a.channels))) + v;
#pragma unroll 2
    for (int p = p0 + r; p < p1; p += rows) {
        float q[8], g[8], o[8];
        bf16x8_to_f32(x[(size_t)p * vc], q);
        bf16x8_to_f32(dy[(size_t)p * vc], g);
        gn_masked8(q, g, sc, sh, a.relu);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = sc[j] * g[j] + (kk.z + ((q[j] - kk.x) - kk.y) * kk.w);
        dx[(size_t)p * vc] = f32_to_bf16x8(o);
    }
}

static void gn_train_args(const GnArgs &s, GnTrainArgs &a)
{
    a.num_levels = s.num_levels; a.batch = s.batch; a.channels = s.channels; a.groups = s.groups;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        a.HW[l] = s.HW[l]; a.nch[l] = s.nch[l]; a.blk_off[l] = s.blk_off[l];
        a.x[l] = nullptr; a.dy[l] = nullptr; a.out[l] = nullptr;
    }
    a.blk_off[IA_MAX_LEVELS] = s.blk_off[IA_MAX_LEVELS];
    a.gamma = a.beta = nullptr; a.eps = 0.0f; a.relu = 0;
    a.part = nullptr; a.saved = nullptr; a.gpart = nullptr; a.cpart = nullptr;
}

static bool gn_level_ptrs(int n, const float *const *p, const float **out)
{
    if (!p) return false;
    for (int l = 0; l < n; ++l) {
        if (!p[l] || ((uintptr_t)p[l] & 15u)) return false;
        out[l] = p[l];
    }
    return true;
}

// the FCOS regression epilogue bbox_pred = exp(scale_l * x) (iou_aware_fcos_head.py:105), in place
// on per-level channels-last tensors; the scales stay on the device (no host read of a parameter)
struct ScaleExpArgs {
    int32_t num_levels;
    int64_t vec_off[IA_MAX_LEVELS + 1];         // prefix of float4 counts
    float4 *x[IA_MAX_LEVELS];
    const float *scales;
};

__global__ void __launch_bounds__(256) k_scale_exp(ScaleExpArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.vec_off[a.num_levels]) return;
    int l = 0;
#pragma unroll
    for (int k = 1; k < IA_MAX_LEVELS; ++k) l += (k < a.num_levels && i >= a.vec_off[k]) ? 1 : 0;
    float4 *x = a.x[0];
    int64_t base = a.vec_off[0];
#pragma unroll
    for (int k = 1; k < IA_MAX_LEVELS; ++k) {
        x = (l == k) ? a.x[k] : x;
        base = (l == k) ? a.vec_off[k] : base;
    }
    const float s = a.scales[l];
    float4 q = x[i - base];
    q.x = expf_(q.x * s); q.y = expf_(q.y * s); q.z = expf_(q.z * s); q.w = expf_(q.w * s);
    x[i - base] = q;
}

// the same on bf16 tensors: a thread's four values are 8 bytes; bf16(expf_(scale_l * float(x))),
// the fp32 kernel's evaluation and one rounding (ScaleExpArgs::x[l] carries the bf16 pointers,
// vec_off counts groups of four values as above)
__global__ void __launch_bounds__(256) k_scale_exp_bf16(ScaleExpArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.vec_off[a.num_levels]) return;
    int l = 0;
#pragma unroll
    for (int k = 1; k < IA_MAX_LEVELS; ++k) l += (k < a.num_levels && i >= a.vec_off[k]) ? 1 : 0;
    uint2 *x = reinterpret_cast<uint2 *>(a.x[0]);
    int64_t base = a.vec_off[0];
#pragma unroll
    for (int k = 1; k < IA_MAX_LEVELS; ++k) {
        x = (l == k) ? reinterpret_cast<uint2 *>(a.x[k]) : x;
        base = (l == k) ? a.vec_off[k] : base;
    }
    const float s = a.scales[l];
    uint2 q = x[i - base];
    const float e0 = expf_(from_bits(q.x << 16) * s), e1 = expf_(from_bits(q.x & 0xffff0000u) * s);
    const float e2 = expf_(from_bits(q.y << 16) * s), e3 = expf_(from_bits(q.y & 0xffff0000u) * s);
    q.x = f32_to_bf16(e0) | (f32_to_bf16(e1) << 16);
    q.y = f32_to_bf16(e2) | (f32_to_bf16(e3) << 16);
    x[i - base] = q;
}

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
            a.x[l] = reinterpret_cast<float4 *>(x[l]);
        }
        a.vec_off[l + 1] = a.vec_off[l] + n;
    }
    const int64_t n = a.vec_off[IA_MAX_LEVELS];
    if (n > (1LL << 40)) return IA_E_ARG;
    if (dtype == IA_BF16)
        hipLaunchKernelGGL(ia::k_scale_exp_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                           (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(ia::k_scale_exp, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                           (hipStream_t)stream, a);
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
    return ((size_t)a.blk_off[IA_MAX_LEVELS] * groups * sizeof(double2) + 255) / 256 * 256;
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
    for (int l = 0; l < g->num_levels; ++l) {
        if (!x[l] || ((uintptr_t)x[l] & 15u)) return IA_E_ARG;
        a.x[l] = static_cast<float *>(const_cast<void *>(x[l]));
    }
    a.part = static_cast<double2 *>(workspace);
    const dim3 grid((unsigned)a.blk_off[IA_MAX_LEVELS]), block(ia::kGnThreads);
    if (dtype == IA_BF16)
        hipLaunchKernelGGL(ia::k_gn_stats_bf16, grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(ia::k_gn_stats, grid, block, 0, (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
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
    for (int l = 0; l < g->num_levels; ++l) {
        if (!x[l] || ((uintptr_t)x[l] & 15u)) return IA_E_ARG;
        a.x[l] = static_cast<float *>(x[l]);
    }
    a.gamma = gamma; a.beta = beta; a.eps = eps; a.relu = relu ? 1 : 0;
    a.part = const_cast<double2 *>(static_cast<const double2 *>(workspace));
    const dim3 grid((unsigned)a.blk_off[IA_MAX_LEVELS]), block(ia::kGnThreads);
    if (dtype == IA_BF16)
        hipLaunchKernelGGL(ia::k_gn_apply_bf16, grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(ia::k_gn_apply, grid, block, 0, (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
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
    return ((size_t)a.num_levels * a.batch * groups * sizeof(double2) + 255) / 256 * 256;
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
    ia::GnArgs s;
    int rc = ia::gn_args_dt(g, channels, groups, dtype, s);
    if (rc) return rc;
    if (!workspace || !saved || !gamma || !beta || !(eps >= 0.0f)) return IA_E_ARG;
    if (((uintptr_t)workspace & 15u) || ((uintptr_t)saved & 15u)) return IA_E_ARG;
    ia::GnTrainArgs a;
    ia::gn_train_args(s, a);
    if (!ia::gn_level_ptrs(a.num_levels, reinterpret_cast<const float *const *>(x), a.x) ||
        !ia::gn_level_ptrs(a.num_levels, reinterpret_cast<const float *const *>(y),
                           const_cast<const float **>(a.out)))
        return IA_E_ARG;
    for (int l = 0; l < a.num_levels; ++l)
        if (x[l] == y[l]) return IA_E_ARG;             // out of place: ia_groupnorm_apply otherwise
    if (workspace_bytes < ia_groupnorm_workspace_bytes_dt(g, channels, groups, dtype) ||
        saved_bytes < ia_groupnorm_saved_bytes_dt(g, channels, groups, dtype))
        return IA_E_WORKSPACE;
    a.gamma = gamma; a.beta = beta; a.eps = eps; a.relu = relu ? 1 : 0;
    a.part = static_cast<const double2 *>(workspace);
    a.saved = static_cast<double2 *>(saved);
    const dim3 grid((unsigned)a.blk_off[IA_MAX_LEVELS]), block(ia::kGnThreads);
    if (dtype == IA_BF16)
        hipLaunchKernelGGL(ia::k_gn_apply_to_bf16, grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(ia::k_gn_apply_to, grid, block, 0, (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
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
    return (rows * ((size_t)groups + channels) * sizeof(double2) + 255) / 256 * 256;
}

size_t ia_groupnorm_bwd_workspace_bytes(const ia_wino_geom *g, int channels, int groups)
{
    return ia_groupnorm_bwd_workspace_bytes_dt(g, channels, groups, IA_F32);
}

static int gn_bwd_args(const ia_wino_geom *g, const void *const *x, const void *const *dy, int dtype,
                       int channels, int groups, const float *gamma, const float *beta,
                       const void *saved, size_t saved_bytes, int relu, void *workspace,
                       size_t workspace_bytes, ia::GnTrainArgs &a)
{
    ia::GnArgs s;
    int rc = ia::gn_args_dt(g, channels, groups, dtype, s);
    if (rc) return rc;
    if (!workspace || !saved || !gamma || !beta) return IA_E_ARG;
    if (((uintptr_t)workspace & 15u) || ((uintptr_t)saved & 15u)) return IA_E_ARG;
    ia::gn_train_args(s, a);
    if (!ia::gn_level_ptrs(a.num_levels, reinterpret_cast<const float *const *>(x), a.x) ||
        !ia::gn_level_ptrs(a.num_levels, reinterpret_cast<const float *const *>(dy), a.dy))
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
    ia::GnTrainArgs a;
    int rc = gn_bwd_args(g, x, dy, dtype, channels, groups, gamma, beta, saved, saved_bytes, relu,
                         workspace, workspace_bytes, a);
    if (rc) return rc;
    const dim3 grid((unsigned)a.blk_off[IA_MAX_LEVELS]), block(ia::kGnThreads);
    if (dtype == IA_BF16)
        hipLaunchKernelGGL(ia::k_gn_bwd_reduce_bf16, grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(ia::k_gn_bwd_reduce, grid, block, 0, (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
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
    ia::GnTrainArgs a;
    int rc = gn_bwd_args(g, x, dy, dtype, channels, groups, gamma, beta, saved, saved_bytes, relu,
                         const_cast<void *>(workspace), workspace_bytes, a);
    if (rc) return rc;
    if (dx) {                                           // NULL: parameter gradients only
        if (!ia::gn_level_ptrs(a.num_levels, reinterpret_cast<const float *const *>(dx),
                               const_cast<const float **>(a.out)))
            return IA_E_ARG;
        for (int l = 0; l < a.num_levels; ++l)
            if (dx[l] == dy[l] || dx[l] == x[l]) return IA_E_ARG;
        const dim3 grid((unsigned)a.blk_off[IA_MAX_LEVELS]), block(ia::kGnThreads);
        if (dtype == IA_BF16)
            hipLaunchKernelGGL(ia::k_gn_bwd_apply_bf16, grid, block, 0, (hipStream_t)stream, a);
        else
            hipLaunchKernelGGL(ia::k_gn_bwd_apply, grid, block, 0, (hipStream_t)stream, a);
        rc = ia::hip_status(hipGetLastError());
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
