// Grouped 3x3 convolution of the ResNeXt bottlenecks (BASELINE config 4: X-101-64x4d; reference
// mmdet/models/backbones/resnext.py:12-91 -- conv2 with groups = 64 / 32 and 4, 8, 16, 32
// channels per group), channels-last fp32, pad 1, stride 1 or 2, folded BatchNorm shift + ReLU
// in the epilogue.
//
// Per group the contraction is tiny (K = 9 * Cg, N = Cg): MIOpen / CK run these layers at
// 230 - 1300 us each (18.8 of the 68 ms of an X-101-64x4d step) although they move 0.14 - 1.1 GB
// -- 25 - 180 us of HBM time.  Here a wavefront owns a "supergroup" of 16 (Cg <= 16) or 32
// (Cg = 32) consecutive channels, i.e. 4 / 2 / 1 whole groups, and walks a row of output pixels
// in tiles of 16:
//   * weights of the supergroup as a dense 16 x 16 (32 x 32) matrix per tap, zero outside the
//     groups' diagonal blocks, BatchNorm scale folded in, pre-arranged per lane and kept in
//     registers for the wavefront's lifetime (36 VGPRs, 144 for Cg = 32);
//   * per tap one 16-byte load per lane -- lane (pixel i, quad kk) reads channels 4kk..4kk+3 of
//     pixel i: 16 pixels x 64 contiguous bytes -- feeds four v_mfma_f32_16x16x4_f32 (the sum
//     over input channels is order free, so component c of the quad is the k-slice of step c);
//   * exact fp32 (the f32 MFMA is a k-ordered fmaf chain), 36 MFMAs per 16 pixels x 16 channels.
// Block-diagonal zero padding wastes MFMA work for Cg = 4 / 8 (4x / 2x), which these layers can
// afford: their cost is the activation traffic.
// MI355X, batch 8 (rocprofv3, X-101-64x4d): layer1 520 us, layer2 275, layer3 153, layer4 140 per
// convolution -- CK: 1300 / 650 / 230 / 230; about half of the f32 MFMA issue rate.  Measured and
// not adopted: an XCD-contiguous row mapping (no change), 2 - 4 independent accumulator chains
// (no change: five wavefronts per SIMD already hide the 40-cycle dependent latency), several rows
// per wavefront to amortise the operand loads (no change).
#include <string.h>
#include "ia_gconv.hpp"

namespace ia {

struct GConvArgs {
    const float *x;            // (B, H, W, C) channels-last
    const float *wpack;        // (SG, 9, NB, 4, NB, 64): per-lane B operands, see pack_grouped_weights
    const float *bias;         // (C) folded BatchNorm shift, or NULL
    float *y;                  // (B, Ho, Wo, C)
    int32_t B, H, W, C, Ho, Wo, SG, relu;
};

// NB = 16-channel blocks per supergroup (1: Cg <= 16, 2: Cg = 32); STRIDE 1 or 2
template <int NB, int STRIDE>
__global__ void __launch_bounds__(256) k_gconv3x3(GConvArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sg = blockIdx.y * 4 + wave;
    if (sg >= a.SG) return;
    const int i = lane & 15, kk = lane >> 4;
    const int row = blockIdx.x;                        // (b, yo)
    const int b = row / a.Ho, yo = row - b * a.Ho;
    const int cbase = sg * 16 * NB;
    float w[9][NB][4][NB];
    gconv_load_w<NB>(a.wpack, sg, lane, w);
    float bz[NB];
#pragma unroll
    for (int co = 0; co < NB; ++co) bz[co] = a.bias ? a.bias[cbase + 16 * co + i] : 0.0f;
    const float *xb = a.x + (size_t)b * a.H * a.W * a.C + cbase + 4 * kk;
    float *yb = a.y + ((size_t)b * a.Ho + yo) * a.Wo * a.C + cbase + i;
    const int tiles = (a.Wo + 15) / 16;
    // stride 1: the three horizontal taps of a row are the same 16 pixels shifted by one lane.
    // One load per input row and tile instead of three (every load touches 16 half-used cache
    // lines; with nine loads per tile the kernel ran at 85 cycles per MFMA, with three at 75):
    // the dx = -1 / +1 operands come from the centre registers by DPP row shifts, the tile's edge
    // lanes from the previous / next tile's centre (rotated into place), which is prefetched one
    // tile ahead (loads two tiles ahead).
    f32x4 prv[3][NB], cur[3][NB], nxt[3][NB], nn[3][NB];
    auto load_rows = [&](int tile, f32x4 (&dst)[3][NB]) {
        const int xo = tile * 16 + i;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int yi = yo + r - 1;
            const bool in = (yi >= 0) && (yi < a.H) && (xo < a.W) && (tile < tiles);
            const int yc = (yi < 0) ? 0 : ((yi >= a.H) ? a.H - 1 : yi);
            const int xc = (xo >= a.W) ? a.W - 1 : xo;
            const float *p = xb + ((size_t)yc * a.W + xc) * a.C;
#pragma unroll
            for (int ci = 0; ci < NB; ++ci) dst[r][ci] = gconv_load16(p + 16 * ci, in);
        }
    };
    if (STRIDE == 1) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int ci = 0; ci < NB; ++ci) prv[r][ci].x = prv[r][ci].y = prv[r][ci].z = prv[r][ci].w = 0.0f;
        load_rows(0, cur);
        if (NB == 1) load_rows(1, nxt);
    }
    for (int tile = 0; tile < tiles; ++tile) {
        f32x4 v[9][NB];
        if (STRIDE == 1) {
            // the right edge lane of THIS tile needs the next tile's centre, so the loads run two
            // tiles ahead: what is requested here is first used in the next iteration
            // (the 32-channel variant has no registers to spare and stays one tile ahead)
            if (NB == 1) load_rows(tile + 2, nn);      // zeros beyond the last tile
            else load_rows(tile + 1, nxt);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int ci = 0; ci < NB; ++ci) {
                    v[3 * r + 1][ci] = cur[r][ci];
                    v[3 * r + 0][ci] = shift_from_left(cur[r][ci], prv[r][ci]);
                    v[3 * r + 2][ci] = shift_from_right(cur[r][ci], nxt[r][ci]);
                }
        } else {
            const int xo = tile * 16 + i;              // this lane's A-operand pixel
#pragma unroll
            for (int t = 0; t < 9; ++t) {              // all loads of the tile first
                const int yi = yo * STRIDE + t / 3 - 1;
                const int xi = xo * STRIDE + t % 3 - 1;
                const bool in = (yi >= 0) && (yi < a.H) && (xi >= 0) && (xi < a.W) && (xo < a.Wo);
                const int yc = (yi < 0) ? 0 : ((yi >= a.H) ? a.H - 1 : yi);
                const int xc = (xi < 0) ? 0 : ((xi >= a.W) ? a.W - 1 : xi);
                const float *p = xb + ((size_t)yc * a.W + xc) * a.C;
#pragma unroll
                for (int ci = 0; ci < NB; ++ci) v[t][ci] = gconv_load16(p + 16 * ci, in);
            }
        }
        f32x4 acc[NB];
#pragma unroll
        for (int co = 0; co < NB; ++co) { acc[co].x = acc[co].y = acc[co].z = acc[co].w = 0.0f; }
#pragma unroll
        for (int t = 0; t < 9; ++t) gconv_mfma_tap<NB>(v[t], w[t], acc);
#pragma unroll
        for (int co = 0; co < NB; ++co)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float val = acc[co][r] + bz[co];
                if (a.relu) val = (val > 0.0f) ? val : 0.0f;
                acc[co][r] = val;
            }
        gconv_store_tile<NB>(yb, a.C, a.Wo, kk, acc, [&](int j) { return tile * 16 + j; });
        if (STRIDE == 1) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int ci = 0; ci < NB; ++ci) {
                    prv[r][ci] = cur[r][ci]; cur[r][ci] = nxt[r][ci];
                    if (NB == 1) nxt[r][ci] = nn[r][ci];
                }
        }
    }
}

}  // namespace ia

extern "C" {

// host-side weight arrangement: (C, Cg, 3, 3) grouped weight (+ per-output-channel scale) ->
// (SG, 9, NB, 4, NB, 64) B operands.  Element [sg][t][ci][c][co][lane] = scale[o] * W[o][in][t]
// with o = sg*16*NB + 16*co + (lane & 15), in = 16*ci + 4*(lane >> 4) + c (inside the
// supergroup), zero when o and in belong to different groups: gconv_pack_elem of ia_gconv.hpp, the
// function the device pack (k_gconv_pack) calls per thread.
int ia_grouped_conv3x3_pack(const float *weight, const float *scale, int channels, int groups,
                            float *wpack)
{
    int nb = 1;
    const int cg = ia::gconv_channels(channels, groups, &nb);
    if (!weight || !wpack || !cg) return IA_E_ARG;
    const int64_t total = (int64_t)(channels / (16 * nb)) * 9 * nb * 4 * nb * 64;
    for (int64_t q = 0; q < total; ++q) wpack[q] = ia::gconv_pack_elem(weight, scale, cg, nb, q, false);
    return 0;
}

int ia_grouped_conv3x3_nhwc(const float *x, const float *wpack, const float *bias, float *y,
                            int batch, int H, int W, int channels, int groups, int stride, int relu,
                            void *stream)
{
    int nb = 1;
    if (!x || !wpack || !y || batch < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2)) return IA_E_ARG;
    if (((uintptr_t)x & 15u) || ((uintptr_t)y & 15u)) return IA_E_ARG;
    if (!ia::gconv_channels(channels, groups, &nb)) return IA_E_ARG;
    ia::GConvArgs a;
    a.x = x; a.wpack = wpack; a.bias = bias; a.y = y;
    a.B = batch; a.H = H; a.W = W; a.C = channels;
    a.Ho = (H + 2 - 3) / stride + 1; a.Wo = (W + 2 - 3) / stride + 1;
    a.SG = channels / (16 * nb); a.relu = relu ? 1 : 0;
    const int64_t rows = (int64_t)batch * a.Ho;
    if (rows > 2147483647LL) return IA_E_ARG;
    dim3 grid((unsigned)rows, (unsigned)((a.SG + 3) / 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    GCONV_DISPATCH(nb, stride, ia::k_gconv3x3, grid, block, s, a);
    return ia::hip_status(hipGetLastError());
}

}  // extern "C"
