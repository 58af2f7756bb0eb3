// Masked convolution (reference mmdet/ops/masked_conv, the inference layers of the guided-anchor
// heads): a stride-1 1x1 / 3x3 (pad 1) convolution evaluated only where a (B, H, W) mask is set and
// exactly 0 elsewhere.  fp32 on channels-last activations, as deform.hip:
//
//   compaction   mask -> idx (the kept flat pixel indices b * H * W + y * W + x, ascending), rank (per
//                pixel its row in idx, or -1) and the count, on the device.
//                  k_mask_count   one pixel per lane: a 64-bit wave ballot per wavefront, the four
//                                 popcounts of a workgroup added in a fixed order -> per-workgroup counts
//                  k_mask_scan    one workgroup: exclusive prefix over the per-workgroup counts, 256 at
//                                 a time with a running carry; the total is the count
//                  k_mask_write   the ballots again: row = workgroup prefix + the earlier wavefronts'
//                                 popcounts + popcount(ballot below the lane)
//                No atomics anywhere: the row order, and with it every bit of the output, is the same
//                in every run.  ia_logit_compact: the same on location logits, keep = sigmoid(x) >= thr
//                evaluated in the kernels with the guided decode's own expression (no mask tensor).
//   k_masked_im2col  col[r][tap * C + c] of the kept pixel idx[r] (taps outside the map: zeros), the
//                row order of ia_im2col3x3_nhwc, one 16-byte vector per lane; rows from the count up to
//                the caller's padded row count are written as zeros, so the GEMM behind it
//                (ia_linear_bias_act, k = taps * C, bias in its epilogue) reads no stale value.
//   k_masked_scatter gather-form output through the rank map: every element of the dense (B, H, W, n)
//                result is written exactly once, y[rank][c] where the mask is set and +0.0f where it
//                is not -- no memset, no atomics.
#include "ia_internal.hpp"
#include "ia_math.hpp"
#include "ia_compact_dev.hpp"      // kMaskBlock, the ballot / scan pieces (shared with ssddecode.hip)

namespace ia {

// where the keep decision comes from: a byte mask, or location logits thresholded here with the
// expression of the guided decode (guideddecode.hip, guided_keep): sigmoidf_(x) >= thr, false for NaN
struct MaskBytes {
    const uint8_t *m;
    __device__ __forceinline__ bool operator()(int64_t p) const { return m[p] != 0; }
};
struct MaskLogits {
    const float *x;
    float thr;
    __device__ __forceinline__ bool operator()(int64_t p) const { return sigmoidf_(x[p]) >= thr; }
};

template <typename Src>
__global__ void __launch_bounds__(kMaskBlock) k_mask_count(Src mask, int64_t total, int32_t *block_count)
{
    __shared__ int s_wave[kMaskBlock / 64];
    const int64_t p = (int64_t)blockIdx.x * kMaskBlock + threadIdx.x;
    const int n = block_keep_count(p < total && mask(p), s_wave);
    if (threadIdx.x == 0) block_count[blockIdx.x] = n;
}

__global__ void __launch_bounds__(256) k_mask_scan(const int32_t *block_count, int32_t *block_off, int64_t nblocks,
                                                   int32_t *count)
{
    __shared__ int s_v[256];
    __shared__ int s_carry;
    const int total = scan_block_counts(block_count, block_off, nblocks, s_v, &s_carry);
    if (threadIdx.x == 0) count[0] = total;
}

template <typename Src>
__global__ void __launch_bounds__(kMaskBlock) k_mask_write(Src mask, int64_t total, const int32_t *block_off,
                                                           int32_t *idx, int32_t *rank)
{
    __shared__ int s_wave[kMaskBlock / 64];
    const int64_t p = (int64_t)blockIdx.x * kMaskBlock + threadIdx.x;
    const bool keep = p < total && mask(p);
    const int r = block_off[blockIdx.x] + block_keep_rank(keep, s_wave);
    if (p < total) {
        rank[p] = keep ? r : -1;
        if (keep) idx[r] = (int32_t)p;       // r < count <= total: inside idx
    }
}

struct MaskedColArgs {
    const float4 *x;
    const int32_t *idx;
    float4 *col;
    int64_t count, row0, rows;
    int32_t H, W, C4, taps;
};

__global__ void __launch_bounds__(256) k_masked_im2col(MaskedColArgs a)
{
    const int64_t per_row = (int64_t)a.taps * a.C4;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.rows * per_row) return;
    const int64_t r = e / per_row;
    const int rem = (int)(e - r * per_row);
    const int tap = rem / a.C4, c = rem - tap * a.C4;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a.row0 + r < a.count) {
        const int64_t p = a.idx[a.row0 + r];
        const int64_t hw = (int64_t)a.H * a.W;
        const int64_t b = p / hw;
        const int q = (int)(p - b * hw);
        int y = q / a.W, x = q - y * a.W;
        if (a.taps == 9) {
            const int i = tap / 3, j = tap - i * 3;
            y += i - 1; x += j - 1;
        }
        if (y >= 0 && y < a.H && x >= 0 && x < a.W) v = a.x[((b * a.H + y) * a.W + x) * a.C4 + c];
    }
    a.col[e] = v;
}

__global__ void __launch_bounds__(256) k_masked_scatter(const float *y, int64_t ld, const int32_t *rank, float *out,
                                                        int64_t total, int n)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total * n) return;
    const int64_t p = e / n;
    const int c = (int)(e - p * n);
    const int r = rank[p];
    out[e] = (r >= 0 && y) ? y[(int64_t)r * ld + c] : 0.0f;
}

static int64_t mask_blocks(int64_t total) { return (total + kMaskBlock - 1) / kMaskBlock; }

}  // namespace ia

extern "C" size_t ia_mask_compact_workspace_bytes(int64_t total)
{
    if (total < 1 || total > 2147483647LL) return 0;
    return (size_t)(2 * ia::mask_blocks(total)) * sizeof(int32_t);
}

namespace ia {
template <typename Src>
static int mask_compact(Src src, int64_t total, int32_t *idx, int32_t *rank, int32_t *count, void *workspace,
                        size_t workspace_bytes, hipStream_t s)
{
    if (!idx || !rank || !count || !workspace) return IA_E_ARG;
    const size_t need = ia_mask_compact_workspace_bytes(total);
    if (need == 0) return IA_E_ARG;
    if (workspace_bytes < need) return IA_E_WORKSPACE;
    if ((uintptr_t)workspace & 3u) return IA_E_ARG;
    const int64_t nb = mask_blocks(total);
    int32_t *block_count = static_cast<int32_t *>(workspace), *block_off = block_count + nb;
    hipLaunchKernelGGL((k_mask_count<Src>), dim3((unsigned)nb), dim3(kMaskBlock), 0, s, src, total, block_count);
    hipLaunchKernelGGL(k_mask_scan, dim3(1), dim3(256), 0, s, block_count, block_off, nb, count);
    hipLaunchKernelGGL((k_mask_write<Src>), dim3((unsigned)nb), dim3(kMaskBlock), 0, s, src, total, block_off, idx,
                       rank);
    return hip_status(hipGetLastError());
}
}  // namespace ia

extern "C" int ia_mask_compact(const uint8_t *mask, int64_t total, int32_t *idx, int32_t *rank, int32_t *count,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    if (!mask) return IA_E_ARG;
    return ia::mask_compact(ia::MaskBytes{mask}, total, idx, rank, count, workspace, workspace_bytes,
                            (hipStream_t)stream);
}

extern "C" int ia_logit_compact(const float *logits, float thr, int64_t total, int32_t *idx, int32_t *rank,
                                int32_t *count, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!logits || !(thr >= 0.0f && thr <= 1.0f)) return IA_E_ARG;
    return ia::mask_compact(ia::MaskLogits{logits, thr}, total, idx, rank, count, workspace, workspace_bytes,
                            (hipStream_t)stream);
}

extern "C" int ia_masked_im2col(const float *x, const int32_t *idx, int64_t count, int64_t row0, int64_t rows,
                                float *col, int B, int H, int W, int C, int ksize, void *stream)
{
    if (!x || !idx || !col || B < 1 || H < 1 || W < 1 || C < 4 || (C & 3)) return IA_E_ARG;
    if (ksize != 1 && ksize != 3) return IA_E_ARG;
    if (((uintptr_t)x | (uintptr_t)col) & 15u) return IA_E_ARG;
    const int64_t total = (int64_t)B * H * W;
    if (total > 2147483647LL || count < 0 || count > total || row0 < 0 || rows < 1) return IA_E_ARG;
    ia::MaskedColArgs a;
    a.x = reinterpret_cast<const float4 *>(x); a.idx = idx; a.col = reinterpret_cast<float4 *>(col);
    a.count = count; a.row0 = row0; a.rows = rows;
    a.H = H; a.W = W; a.C4 = C / 4; a.taps = ksize * ksize;
    const int64_t n = rows * a.taps * a.C4;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > 2147483647LL) return IA_E_ARG;
    hipLaunchKernelGGL(ia::k_masked_im2col, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
}

extern "C" int ia_masked_scatter(const float *y, int64_t ld, const int32_t *rank, float *out, int64_t total, int n,
                                 void *stream)
{
    if (!rank || !out || total < 1 || total > 2147483647LL || n < 1 || ld < n) return IA_E_ARG;
    const int64_t blocks = (total * n + 255) / 256;
    if (blocks > 2147483647LL) return IA_E_ARG;
    // y == NULL: the caller states that nothing is kept (every rank is -1, y is never read)
    hipLaunchKernelGGL(ia::k_masked_scatter, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, y, ld, rank,
                       out, total, n);
    return ia::hip_status(hipGetLastError());
}
