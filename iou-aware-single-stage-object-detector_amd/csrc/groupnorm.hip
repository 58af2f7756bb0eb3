// GroupNorm + ReLU of the IoU-aware FCOS head towers at inference (reference
// mmdet/models/anchor_heads/iou_aware_fcos_head.py:41-62, ConvModule(3x3, GN(32), ReLU); torch
// nn.GroupNorm semantics: biased variance, eps inside the square root).
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

}  // namespace ia

extern "C" {

int ia_scale_exp_levels(const ia_wino_geom *g, float *const *x, int channels, const float *scales,
                        void *stream)
{
    if (!g || g->num_levels < 1 || g->num_levels > IA_MAX_LEVELS || g->batch < 1 || !x || !scales)
        return IA_E_ARG;
    if (channels < 4 || (channels & 3)) return IA_E_ARG;
    ia::ScaleExpArgs a;
    a.num_levels = g->num_levels;
    a.scales = scales;
    a.vec_off[0] = 0;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        int64_t n = 0;
        a.x[l] = nullptr;
        if (l < g->num_levels) {
            if (g->H[l] < 1 || g->W[l] < 1 || !x[l] || ((uintptr_t)x[l] & 15u)) return IA_E_ARG;
            n = (int64_t)g->batch * g->H[l] * g->W[l] * (channels / 4);
            a.x[l] = reinterpret_cast<float4 *>(x[l]);
        }
        a.vec_off[l + 1] = a.vec_off[l] + n;
    }
    const int64_t n = a.vec_off[IA_MAX_LEVELS];
    if (n > (1LL << 40)) return IA_E_ARG;
    hipLaunchKernelGGL(ia::k_scale_exp, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
}


size_t ia_groupnorm_workspace_bytes(const ia_wino_geom *g, int channels, int groups)
{
    ia::GnArgs a;
    if (ia::gn_args(g, channels, groups, a)) return 0;
    return ((size_t)a.blk_off[IA_MAX_LEVELS] * groups * sizeof(double2) + 255) / 256 * 256;
}

int ia_groupnorm_stats(const ia_wino_geom *g, const float *const *x, int channels, int groups,
                       void *workspace, size_t workspace_bytes, void *stream)
{
    ia::GnArgs a;
    int rc = ia::gn_args(g, channels, groups, a);
    if (rc) return rc;
    if (!x || !workspace) return IA_E_ARG;
    if (workspace_bytes < ia_groupnorm_workspace_bytes(g, channels, groups)) return IA_E_WORKSPACE;
    for (int l = 0; l < g->num_levels; ++l) {
        if (!x[l] || ((uintptr_t)x[l] & 15u)) return IA_E_ARG;
        a.x[l] = const_cast<float *>(x[l]);
    }
    a.part = static_cast<double2 *>(workspace);
    hipLaunchKernelGGL(ia::k_gn_stats, dim3((unsigned)a.blk_off[IA_MAX_LEVELS]), dim3(ia::kGnThreads),
                       0, (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
}

int ia_groupnorm_apply(const ia_wino_geom *g, float *const *x, int channels, int groups,
                       const float *gamma, const float *beta, float eps, int relu,
                       const void *workspace, size_t workspace_bytes, void *stream)
{
    ia::GnArgs a;
    int rc = ia::gn_args(g, channels, groups, a);
    if (rc) return rc;
    if (!x || !workspace || !gamma || !beta || !(eps >= 0.0f)) return IA_E_ARG;
    if (workspace_bytes < ia_groupnorm_workspace_bytes(g, channels, groups)) return IA_E_WORKSPACE;
    for (int l = 0; l < g->num_levels; ++l) {
        if (!x[l] || ((uintptr_t)x[l] & 15u)) return IA_E_ARG;
        a.x[l] = x[l];
    }
    a.gamma = gamma; a.beta = beta; a.eps = eps; a.relu = relu ? 1 : 0;
    a.part = const_cast<double2 *>(static_cast<const double2 *>(workspace));
    hipLaunchKernelGGL(ia::k_gn_apply, dim3((unsigned)a.blk_off[IA_MAX_LEVELS]), dim3(ia::kGnThreads),
                       0, (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
}

}  // extern "C"
