// bf16 twin of gconv.hip: the grouped 3x3 convolution of the ResNeXt bottlenecks (conv2 with
// groups = 64 / 32 and 4, 8, 16, 32 channels per group) on bf16 channels-last tensors, pad 1,
// stride 1 or 2, fp32 accumulation on v_mfma_f32_16x16x32_bf16, folded BatchNorm shift (fp32) +
// ReLU in fp32 and ONE round-to-nearest-even to bf16 at the store.
//
// A wavefront owns a supergroup of 32 consecutive channels (8 / 4 / 2 / 1 whole groups) and walks
// a row of output pixels in tiles of 16, as the fp32 kernel does:
//   * weights of the supergroup as a dense 32 x 32 bf16 matrix per tap, zero outside the groups'
//     diagonal blocks, BatchNorm scale folded in (fp32, rounded once), pre-arranged per lane by
//     ia_grouped_conv3x3_pack_bf16 and resident in registers: 9 taps x 2 output blocks x 4 VGPRs;
//   * the weights are the A operand, the activations the B operand (D^T = W^T X^T): lane
//     (pixel i = lane & 15, octet kk = lane >> 4) reads the 8 channels 8kk .. 8kk+7 of pixel i with
//     one 16-byte load -- 16 pixels x 64 contiguous bytes per wavefront, the access pattern of the
//     fp32 kernel -- and that fragment feeds the two MFMAs (output blocks) of a tap: 18 MFMAs per
//     16 pixels x 32 channels;
//   * D has the pixel on the lane (column lane & 15) and the four consecutive output channels
//     16co + 4kk .. + 3 in the four accumulator registers: one 8-byte packed store per lane and
//     output block;
//   * stride 1: one load per input row and tile, the dx = -1 / +1 operands by DPP row shifts (a
//     32-bit register holds two channels of ONE pixel, so the shifts move whole pixels), the edge
//     lanes from the previous / next tile's centre, loads two tiles ahead; stride 2: nine loads;
//   * out-of-image taps: unconditional loads from clamped addresses, zeroed by a mask.
// No atomics, no LDS, a fixed reduction order: the same bits on every launch.
#include <string.h>
#include "ia_gconv.hpp"

namespace ia {

typedef float gb_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 gb_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 gb_bf16x2 __attribute__((ext_vector_type(2)));

constexpr int kGbSG = 32;                 // channels per supergroup

struct GConvBf16Args {
    const uint16_t *x;         // (B, H, W, C) channels-last bf16
    const uint4 *wpack;        // (SG, 9, 2, 64) x 8 bf16: per-lane A operands, see ia_grouped_conv3x3_pack_bf16
    const float *bias;         // (C) folded BatchNorm shift, or NULL
    uint16_t *y;               // (B, Ho, Wo, C) bf16
    int32_t B, H, W, C, Ho, Wo, SG, relu;
};

template <int STRIDE>
__global__ void __launch_bounds__(256) k_gconv3x3_bf16(GConvBf16Args a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sg = blockIdx.y * 4 + wave;
    if (sg >= a.SG) return;
    const int i = lane & 15, kk = lane >> 4;
    const int row = blockIdx.x;                        // (b, yo)
    const int b = row / a.Ho, yo = row - b * a.Ho;
    const int cbase = sg * kGbSG;
    // A operands: w[t][co] = W[out 16co + (lane & 15)][in 8kk .. 8kk + 7] of tap t
    gb_bf16x8 w[9][2];
    {
        const uint4 *wp = a.wpack + (size_t)sg * (9 * 2 * 64) + lane;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int co = 0; co < 2; ++co) w[t][co] = __builtin_bit_cast(gb_bf16x8, wp[(t * 2 + co) * 64]);
    }
    // this lane's four output channels of block co: 16co + 4kk .. + 3
    float bz[2][4];
#pragma unroll
    for (int co = 0; co < 2; ++co)
#pragma unroll
        for (int r = 0; r < 4; ++r) bz[co][r] = a.bias ? a.bias[cbase + 16 * co + 4 * kk + r] : 0.0f;
    const uint16_t *xb = a.x + (size_t)b * a.H * a.W * a.C + cbase + 8 * kk;
    uint16_t *yb = a.y + ((size_t)b * a.Ho + yo) * a.Wo * a.C + cbase + 4 * kk;
    const int tiles = (a.Wo + 15) / 16;
    uint4 prv[3], cur[3], nxt[3], nn[3];
    auto load_rows = [&](int tile, uint4 (&dst)[3]) {
        const int xo = tile * 16 + i;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int yi = yo + r - 1;
            const bool in = (yi >= 0) && (yi < a.H) && (xo < a.W) && (tile < tiles);
            const int yc = (yi < 0) ? 0 : ((yi >= a.H) ? a.H - 1 : yi);
            const int xc = (xo >= a.W) ? a.W - 1 : xo;
            const uint4 q = *reinterpret_cast<const uint4 *>(xb + ((size_t)yc * a.W + xc) * a.C);   // unconditional
            const uint32_t mk = in ? 0xffffffffu : 0u;
            dst[r] = make_uint4(q.x & mk, q.y & mk, q.z & mk, q.w & mk);
        }
    };
    if (STRIDE == 1) {
#pragma unroll
        for (int r = 0; r < 3; ++r) prv[r] = make_uint4(0u, 0u, 0u, 0u);
        load_rows(0, cur);
        load_rows(1, nxt);
    }
    for (int tile = 0; tile < tiles; ++tile) {
        uint4 v[9];
        if (STRIDE == 1) {
            // the right edge lane of THIS tile needs the next tile's centre, so the loads run two
            // tiles ahead: what is requested here is first used in the next iteration
            load_rows(tile + 2, nn);                   // zeros beyond the last tile
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                v[3 * r + 1] = cur[r];
                v[3 * r + 0] = shift_from_left(cur[r], prv[r]);
                v[3 * r + 2] = shift_from_right(cur[r], nxt[r]);
            }
        } else {
            const int xo = tile * 16 + i;              // this lane's output pixel
#pragma unroll
            for (int t = 0; t < 9; ++t) {              // all loads of the tile first
                const int yi = yo * STRIDE + t / 3 - 1;
                const int xi = xo * STRIDE + t % 3 - 1;
                const bool in = (yi >= 0) && (yi < a.H) && (xi >= 0) && (xi < a.W) && (xo < a.Wo);
                const int yc = (yi < 0) ? 0 : ((yi >= a.H) ? a.H - 1 : yi);
                const int xc = (xi < 0) ? 0 : ((xi >= a.W) ? a.W - 1 : xi);
                const uint4 q = *reinterpret_cast<const uint4 *>(xb + ((size_t)yc * a.W + xc) * a.C);   // unconditional
                const uint32_t mk = in ? 0xffffffffu : 0u;
                v[t] = make_uint4(q.x & mk, q.y & mk, q.z & mk, q.w & mk);
            }
        }
        f32x4 acc[2];
#pragma unroll
        for (int co = 0; co < 2; ++co) { acc[co].x = acc[co].y = acc[co].z = acc[co].w = 0.0f; }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const gb_bf16x8 xf = __builtin_bit_cast(gb_bf16x8, v[t]);
#pragma unroll
            for (int co = 0; co < 2; ++co)
                acc[co] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[t][co], xf, acc[co], 0, 0, 0);
        }
        // D: column (lane & 15) = pixel of the tile, row 4 * (lane >> 4) + r = output channel of the block
        const int px = tile * 16 + i;
#pragma unroll
        for (int co = 0; co < 2; ++co) {
            float o[4] = {acc[co].x + bz[co][0], acc[co].y + bz[co][1], acc[co].z + bz[co][2], acc[co].w + bz[co][3]};
            if (a.relu) {
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = (o[r] > 0.0f) ? o[r] : 0.0f;
            }
            const gb_f32x2 lo = {o[0], o[1]}, hi = {o[2], o[3]};
            uint2 pk;                                  // v_cvt_pk_bf16_f32: round to nearest even
            pk.x = __builtin_bit_cast(uint32_t, __builtin_convertvector(lo, gb_bf16x2));
            pk.y = __builtin_bit_cast(uint32_t, __builtin_convertvector(hi, gb_bf16x2));
            if (px < a.Wo) *reinterpret_cast<uint2 *>(yb + (size_t)px * a.C + 16 * co) = pk;
        }
        if (STRIDE == 1) {
#pragma unroll
            for (int r = 0; r < 3; ++r) { prv[r] = cur[r]; cur[r] = nxt[r]; nxt[r] = nn[r]; }
        }
    }
}

static bool gb_shape_ok(int channels, int groups)
{
    if (channels < kGbSG || channels % kGbSG) return false;
    return gconv_cg(channels, groups) != 0;
}

}  // namespace ia

extern "C" {

size_t ia_grouped_conv3x3_packed_bytes_bf16(int channels, int groups)
{
    if (!ia::gb_shape_ok(channels, groups)) return 0;
    return (size_t)(channels / ia::kGbSG) * 9 * 2 * 64 * 8 * sizeof(uint16_t);
}

// host-side weight arrangement: (C, Cg, 3, 3) grouped weight (+ per-output-channel scale) ->
// (SG, 9, 2, 64, 8) bf16 A operands.  Element [sg][t][co][lane][j] = bf16_rne(scale[o] * W[o][in][t])
// with o = 32 sg + 16 co + (lane & 15), in = 32 sg + 8 (lane >> 4) + j (W indexed by in % Cg inside
// the group), the product in fp32; zero when o and in belong to different groups.
int ia_grouped_conv3x3_pack_bf16(const float *weight, const float *scale, int channels, int groups,
                                 uint16_t *wpack)
{
    if (!weight || !wpack || !ia::gb_shape_ok(channels, groups)) return IA_E_ARG;
    const int cg = channels / groups, SG = channels / ia::kGbSG;
    for (int sg = 0; sg < SG; ++sg)
        for (int t = 0; t < 9; ++t)
            for (int co = 0; co < 2; ++co)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int o = sg * ia::kGbSG + 16 * co + (lane & 15);
                        const int in = sg * ia::kGbSG + 8 * (lane >> 4) + j;
                        uint16_t v = 0;
                        if (o / cg == in / cg) {
                            const float wv = weight[((size_t)o * cg + (in % cg)) * 9 + t];
                            v = ia::bf16_rne_host(scale ? wv * scale[o] : wv);
                        }
                        wpack[(((((size_t)sg * 9 + t) * 2 + co) * 64) + lane) * 8 + j] = v;
                    }
    return 0;
}

int ia_grouped_conv3x3_bf16_nhwc(const uint16_t *x, const uint16_t *wpack, const float *bias,
                                 uint16_t *y, int batch, int H, int W, int channels, int groups,
                                 int stride, int relu, void *stream)
{
    if (!x || !wpack || !y || batch < 1 || H < 1 || W < 1 || !ia::gb_shape_ok(channels, groups) ||
        (stride != 1 && stride != 2))
        return IA_E_ARG;
    if (((uintptr_t)x & 15u) || ((uintptr_t)y & 15u) || ((uintptr_t)wpack & 15u)) return IA_E_ARG;
    ia::GConvBf16Args a;
    a.x = x; a.wpack = reinterpret_cast<const uint4 *>(wpack); a.bias = bias; a.y = y;
    a.B = batch; a.H = H; a.W = W; a.C = channels;
    a.Ho = (H + 2 - 3) / stride + 1; a.Wo = (W + 2 - 3) / stride + 1;
    a.SG = channels / ia::kGbSG; a.relu = relu ? 1 : 0;
    const int64_t rows = (int64_t)batch * a.Ho;
    if (rows > 2147483647LL) return IA_E_ARG;
    dim3 grid((unsigned)rows, (unsigned)((a.SG + 3) / 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (stride == 1) hipLaunchKernelGGL((ia::k_gconv3x3_bf16<1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((ia::k_gconv3x3_bf16<2>), grid, block, 0, s, a);
    return ia::hip_status(hipGetLastError());
}

}  // extern "C"
