// Backward of the grouped 3x3 convolution of csrc/gconv.hip (ResNeXt conv2 in training): a weight
// pack that stays on the device, the input gradient and the weight gradient, channels-last fp32,
// pad 1, stride 1 or 2, 4 / 8 / 16 / 32 channels per group, all on v_mfma_f32_16x16x4_f32 with the
// forward's supergroup idea (a wavefront owns 16 or 32 consecutive channels = 4 / 2 / 1 whole
// groups as a block-diagonal dense matrix per tap) and the forward's lane layout:
//   A operand: lane (row m = lane & 15, k = lane >> 4); B operand: lane (column n = lane & 15,
//   k = lane >> 4); D: column n = lane & 15, rows 4 * (lane >> 4) + r, r = 0..3.
//
//   pack      k_gconv_pack: one thread per element of the (SG, 9, NB, 4, NB, 64) operand layout.
//             adjoint = 0: the bits of ia_grouped_conv3x3_pack (the same single fp32 product
//             weight * scale); adjoint = 1: the weight of the input-gradient convolution -- taps
//             flipped in both directions, input and output channel swapped inside each group;
//             adjoint = 2: both in one launch, the plain pack followed by the adjoint one (the
//             training node's forward, which then has the input gradient's operand in hand).
//   dx, s = 1 the forward kernel on the adjoint pack (ia_grouped_conv3x3_nhwc, no bias, no ReLU).
//   dx, s = 2 k_gconv_dx_s2, gather form: an input pixel (y, x) sums the taps whose output pixel
//             exists, ky with (y + 1 - ky) even, kx with (x + 1 - kx) even -- 1, 2, 2 or 4 taps per
//             (row, column) parity class.  A wavefront walks one input row; a tile is 16 input
//             pixels of ONE column parity x = 2 j + px, whose taps read 16 consecutive output
//             pixels (j or j + 1) as the A operand with the forward's 16-byte loads.  Output
//             rows / columns that do not exist (oy = Ho, ox = Wo at an even H / W) are masked to
//             zero; the address alone is clamped.  Every dx element is written, no atomics.
//   dW        k_gconv_dw: the contraction index is the pixel, so the MFMA's k is the pixel: lane
//             (channel lane & 15, pixel lane >> 4) loads one float of x (A) and of dz (B), 64
//             contiguous bytes per 16 lanes, four pixels per MFMA; per tap a 16 x 16 product per
//             (input block, output block) of the supergroup, of which the groups' diagonal blocks
//             are stored.  A wavefront owns one 16-channel OUTPUT block (Cg = 32: the two halves
//             of a supergroup go to two wavefronts -- 72 instead of 144 accumulator registers) and
//             one slice of `rows_per_slice` output rows; it writes its accumulators as they lie
//             in the registers -- (slice, unit, 9, NB, 4, 64 lanes), every store 256 contiguous
//             bytes (stores in (C, Cg, 3, 3) order touch 64 cache lines each and cost more than
//             the MFMAs) -- and k_gconv_dw_reduce adds the slices in a fixed order (four
//             interleaved chains, then a fixed tree) and scatters the groups' diagonal blocks into
//             dW.  No atomics, the same bits in every run, and no fp32 chain longer than
//             rows_per_slice * Wo / 4 MFMA steps (<= 256 unless a single row is longer) or
//             slices / 4 adds.  The slice count aims at ~2048 wavefronts: more only adds
//             workspace traffic (9 * 16 * NB * C floats per slice).
#include "ia_gconv.hpp"

namespace ia {

constexpr int kDwWaves = 2048;         // wavefronts the weight gradient aims at (256 CUs x 8)
constexpr int kDwMaxPixels = 1024;     // pixels of one slice (unless one row is longer): the fp32 chain

struct GPackArgs {
    const float *weight, *scale;
    float *wpack;
    int32_t C, cg, NB, SG, adjoint;
};

__global__ void __launch_bounds__(256) k_gconv_pack(GPackArgs a)
{
    const int64_t total = (int64_t)a.SG * 9 * a.NB * 4 * a.NB * 64;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (a.adjoint == 2 ? 2 * total : total)) return;
    const bool adj = (a.adjoint == 1) || (idx >= total);     // adjoint 2: the plain pack, then the adjoint one
    a.wpack[idx] = gconv_pack_elem(a.weight, a.scale, a.cg, a.NB, (idx >= total) ? idx - total : idx, adj);
}

struct GDxArgs {
    const float *dz;           // (B, Ho, Wo, C)
    const float *wpack;        // adjoint pack
    float *dx;                 // (B, H, W, C)
    int32_t B, H, W, C, Ho, Wo, SG;
};

template <int NB>
__global__ void __launch_bounds__(256) k_gconv_dx_s2(GDxArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sg = blockIdx.y * 4 + wave;
    if (sg >= a.SG) return;
    const int i = lane & 15, kk = lane >> 4;
    const int row = blockIdx.x;                        // (b, y) of the INPUT
    const int b = row / a.H, y = row - b * a.H;
    const int cbase = sg * 16 * NB;
    float w[9][NB][4][NB];                             // adjoint pack: tap index 8 - (3 ky + kx)
    {
        const float *wp = a.wpack + (size_t)sg * 9 * NB * 4 * NB * 64 + lane;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int ci = 0; ci < NB; ++ci)
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int co = 0; co < NB; ++co)
                        w[t][ci][c][co] = wp[(size_t)(((t * NB + ci) * 4 + c) * NB + co) * 64];
    }
    const float *zb = a.dz + (size_t)b * a.Ho * a.Wo * a.C + cbase + 4 * kk;
    float *xb = a.dx + ((size_t)b * a.H + y) * a.W * a.C + cbase + i;
    // the output rows of the three vertical taps (uniform over the block)
    bool rowok[3];
    int oyc[3];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int num = y + 1 - ky;
        const int oy = num >> 1;
        rowok[ky] = (num >= 0) && !(num & 1) && (oy < a.Ho);
        oyc[ky] = (oy < 0) ? 0 : ((oy >= a.Ho) ? a.Ho - 1 : oy);
    }
#pragma unroll
    for (int px = 0; px < 2; ++px) {
        const int count = (a.W + 1 - px) >> 1;         // input pixels of this column parity
        const int tiles = (count + 15) / 16;
        for (int tile = 0; tile < tiles; ++tile) {
            const int j = tile * 16 + i;               // this lane's A-operand pixel: x = 2 j + px
            f32x4 acc[NB];
#pragma unroll
            for (int co = 0; co < NB; ++co) { acc[co].x = acc[co].y = acc[co].z = acc[co].w = 0.0f; }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                if (!rowok[ky]) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    if (((px + 1 - kx) & 1) != 0) continue;          // compile time: px 0 -> kx 1; px 1 -> kx 0, 2
                    const int ox = j + ((px + 1 - kx) >> 1);         // (2 j + px + 1 - kx) / 2
                    const bool in = (ox < a.Wo) && (j < count);      // ox = Wo at an even W: masked
                    const int oxc = (ox >= a.Wo) ? a.Wo - 1 : ox;
                    const float *p = zb + ((size_t)oyc[ky] * a.Wo + oxc) * a.C;
                    const int t = 8 - (3 * ky + kx);
#pragma unroll
                    for (int ci = 0; ci < NB; ++ci) {
                        const f32x4 q = *reinterpret_cast<const f32x4 *>(p + 16 * ci);   // unconditional
                        f32x4 z; z.x = z.y = z.z = z.w = 0.0f;
                        const f32x4 v = in ? q : z;
                        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int c = 0; c < 4; ++c)
#pragma unroll
                            for (int co = 0; co < NB; ++co)
                                acc[co] = __builtin_amdgcn_mfma_f32_16x16x4f32(e[c], w[t][ci][c][co],
                                                                               acc[co], 0, 0, 0);
                    }
                }
            }
            // D: column (lane & 15) = dx channel, row 4 * (lane >> 4) + r = pixel j of the tile
#pragma unroll
            for (int co = 0; co < NB; ++co) {
                const float o[4] = {acc[co].x, acc[co].y, acc[co].z, acc[co].w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int x = 2 * (tile * 16 + 4 * kk + r) + px;
                    if (x < a.W) xb[(size_t)x * a.C + 16 * co] = o[r];
                }
            }
        }
    }
}

struct GDwArgs {
    const float *x;            // (B, H, W, C)
    const float *dz;           // (B, Ho, Wo, C)
    float *part;               // (slices, units, 9, NB, 4, 64): the accumulators per lane
    int32_t B, H, W, C, Ho, Wo, SG, cg, rows, rows_per_slice;
};

// NB = 16-channel blocks per supergroup; a wavefront owns output block `co` of supergroup `sg`
template <int NB, int STRIDE>
__global__ void __launch_bounds__(256) k_gconv_dw(GDwArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int unit = blockIdx.y * 4 + wave;
    if (unit >= a.SG * NB) return;
    const int sg = unit / NB, co = unit - sg * NB;
    const int ch = lane & 15, kk = lane >> 4;          // channel inside a block, pixel of the step
    const int ibase = sg * 16 * NB;                    // first input channel of the supergroup
    const int o = ibase + 16 * co + ch;                // this lane's dz channel (B operand, D column)
    const int slice = blockIdx.x;
    const int r0 = slice * a.rows_per_slice;
    const int r1 = (r0 + a.rows_per_slice < a.rows) ? r0 + a.rows_per_slice : a.rows;
    f32x4 acc[9][NB];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int ci = 0; ci < NB; ++ci) { acc[t][ci].x = acc[t][ci].y = acc[t][ci].z = acc[t][ci].w = 0.0f; }
    for (int row = r0; row < r1; ++row) {
        const int b = row / a.Ho, oy = row - b * a.Ho;
        const float *zrow = a.dz + (size_t)row * a.Wo * a.C + o;
        const float *xim = a.x + (size_t)b * a.H * a.W * a.C + ibase + ch;
        for (int ox0 = 0; ox0 < a.Wo; ox0 += 4) {
            const int ox = ox0 + kk;
            const bool okp = ox < a.Wo;
            const int oxc = okp ? ox : a.Wo - 1;
            const float zq = zrow[(size_t)oxc * a.C];                  // unconditional
            const float zv = okp ? zq : 0.0f;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int yi = oy * STRIDE + ky - 1;                   // uniform
                if (yi < 0 || yi >= a.H) continue;
                const float *xrow = xim + (size_t)yi * a.W * a.C;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int xi = ox * STRIDE + kx - 1;
                    const bool in = okp && (xi >= 0) && (xi < a.W);
                    const int xc = (xi < 0) ? 0 : ((xi >= a.W) ? a.W - 1 : xi);
#pragma unroll
                    for (int ci = 0; ci < NB; ++ci) {
                        const float xq = xrow[(size_t)xc * a.C + 16 * ci];   // unconditional
                        const float xv = in ? xq : 0.0f;
                        acc[3 * ky + kx][ci] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            xv, zv, acc[3 * ky + kx][ci], 0, 0, 0);
                    }
                }
            }
        }
    }
    float *pp = a.part + ((size_t)slice * a.SG * NB + unit) * 9 * NB * 256 + lane;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int ci = 0; ci < NB; ++ci) {
            pp[((t * NB + ci) * 4 + 0) * 64] = acc[t][ci].x;
            pp[((t * NB + ci) * 4 + 1) * 64] = acc[t][ci].y;
            pp[((t * NB + ci) * 4 + 2) * 64] = acc[t][ci].z;
            pp[((t * NB + ci) * 4 + 3) * 64] = acc[t][ci].w;
        }
}

// one thread per accumulator element: the slices added in a fixed order, then
// D: column (lane & 15) = output channel o, row 4 * (lane >> 4) + r = input channel of block ci
__global__ void __launch_bounds__(256) k_gconv_dw_reduce(const float *part, float *dw, int n, int slices,
                                                         int NB, int cg)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    int s = 0;
    for (; s + 4 <= slices; s += 4) {
        s0 += part[(size_t)(s + 0) * n + e];
        s1 += part[(size_t)(s + 1) * n + e];
        s2 += part[(size_t)(s + 2) * n + e];
        s3 += part[(size_t)(s + 3) * n + e];
    }
    if (s < slices) s0 += part[(size_t)s * n + e];
    if (s + 1 < slices) s1 += part[(size_t)(s + 1) * n + e];
    if (s + 2 < slices) s2 += part[(size_t)(s + 2) * n + e];
    const float sum = (s0 + s1) + (s2 + s3);
    const int lane = e & 63, r = (e >> 6) & 3;
    int q = e >> 8;
    const int ci = q % NB; q /= NB;
    const int t = q % 9;
    const int unit = q / 9;
    const int sg = unit / NB, co = unit - sg * NB;
    const int o = sg * 16 * NB + 16 * co + (lane & 15);
    const int in = sg * 16 * NB + 16 * ci + 4 * (lane >> 4) + r;
    if (in / cg == o / cg) dw[((size_t)o * cg + (in % cg)) * 9 + t] = sum;
}

static int dw_rows_per_slice(int64_t rows, int Wo, int units)
{
    int64_t want = (kDwWaves + units - 1) / units;                 // slices
    if (want > rows) want = rows;
    int64_t rps = (rows + want - 1) / want;
    const int64_t cap = (kDwMaxPixels / Wo > 1) ? kDwMaxPixels / Wo : 1;
    return (int)(rps < cap ? rps : cap);
}

}  // namespace ia

extern "C" {

int ia_grouped_conv3x3_pack_dev(const float *weight, const float *scale, int channels, int groups,
                                int adjoint, float *wpack, void *stream)
{
    int nb = 1;
    if (!weight || !wpack || adjoint < 0 || adjoint > 2) return IA_E_ARG;
    const int cg = ia::gconv_shape(1, 1, 1, channels, groups, 1, &nb);
    if (!cg) return IA_E_ARG;
    ia::GPackArgs a;
    a.weight = weight; a.scale = (adjoint == 1) ? nullptr : scale; a.wpack = wpack;
    a.C = channels; a.cg = cg; a.NB = nb; a.SG = channels / (16 * nb); a.adjoint = adjoint;
    const int64_t total = (int64_t)a.SG * 9 * nb * 4 * nb * 64 * (adjoint == 2 ? 2 : 1);
    hipLaunchKernelGGL(ia::k_gconv_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
}

int ia_grouped_conv3x3_bwd_data_nhwc(const float *dz, const float *wpack_adjoint, float *dx, int batch,
                                     int H, int W, int channels, int groups, int stride, void *stream)
{
    int nb = 1;
    if (!dz || !wpack_adjoint || !dx) return IA_E_ARG;
    if (((uintptr_t)dz & 15u) || ((uintptr_t)dx & 15u) || ((uintptr_t)wpack_adjoint & 3u)) return IA_E_ARG;
    if (!ia::gconv_shape(batch, H, W, channels, groups, stride, &nb)) return IA_E_ARG;
    if (stride == 1)       // the forward kernel on the adjoint pack
        return ia_grouped_conv3x3_nhwc(dz, wpack_adjoint, nullptr, dx, batch, H, W, channels, groups, 1, 0,
                                       stream);
    ia::GDxArgs a;
    a.dz = dz; a.wpack = wpack_adjoint; a.dx = dx;
    a.B = batch; a.H = H; a.W = W; a.C = channels;
    a.Ho = (H - 1) / 2 + 1; a.Wo = (W - 1) / 2 + 1; a.SG = channels / (16 * nb);
    dim3 grid((unsigned)((int64_t)batch * H), (unsigned)((a.SG + 3) / 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (nb == 1) hipLaunchKernelGGL((ia::k_gconv_dx_s2<1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((ia::k_gconv_dx_s2<2>), grid, block, 0, s, a);
    return ia::hip_status(hipGetLastError());
}

size_t ia_grouped_conv3x3_bwd_weight_workspace_bytes(int batch, int H, int W, int channels, int groups,
                                                     int stride)
{
    int nb = 1;
    const int cg = ia::gconv_shape(batch, H, W, channels, groups, stride, &nb);
    if (!cg) return 0;
    const int64_t rows = (int64_t)batch * ((H - 1) / stride + 1);
    const int rps = ia::dw_rows_per_slice(rows, (W - 1) / stride + 1, channels / 16);
    const int64_t slices = (rows + rps - 1) / rps;
    return (size_t)slices * channels * 16 * nb * 9 * sizeof(float);
}

int ia_grouped_conv3x3_bwd_weight_nhwc(const float *x, const float *dz, float *dw, void *workspace,
                                       size_t workspace_bytes, int batch, int H, int W, int channels,
                                       int groups, int stride, void *stream)
{
    int nb = 1;
    if (!x || !dz || !dw || !workspace) return IA_E_ARG;
    if (((uintptr_t)x & 15u) || ((uintptr_t)dz & 15u) || ((uintptr_t)dw & 3u) || ((uintptr_t)workspace & 3u))
        return IA_E_ARG;
    const int cg = ia::gconv_shape(batch, H, W, channels, groups, stride, &nb);
    if (!cg) return IA_E_ARG;
    if (workspace_bytes < ia_grouped_conv3x3_bwd_weight_workspace_bytes(batch, H, W, channels, groups, stride))
        return IA_E_ARG;
    ia::GDwArgs a;
    a.x = x; a.dz = dz; a.part = (float *)workspace;
    a.B = batch; a.H = H; a.W = W; a.C = channels;
    a.Ho = (H - 1) / stride + 1; a.Wo = (W - 1) / stride + 1;
    a.SG = channels / (16 * nb); a.cg = cg;
    a.rows = batch * a.Ho; a.rows_per_slice = ia::dw_rows_per_slice(a.rows, a.Wo, channels / 16);
    const int slices = (a.rows + a.rows_per_slice - 1) / a.rows_per_slice;
    dim3 grid((unsigned)slices, (unsigned)((a.SG * nb + 3) / 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    GCONV_DISPATCH(nb, stride, ia::k_gconv_dw, grid, block, s, a);
    int st = ia::hip_status(hipGetLastError());
    if (st) return st;
    const int n = channels * 16 * nb * 9;              // accumulator elements of one slice
    hipLaunchKernelGGL(ia::k_gconv_dw_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       (const float *)workspace, dw, n, slices, nb, cg);
    return ia::hip_status(hipGetLastError());
}

}  // extern "C"
