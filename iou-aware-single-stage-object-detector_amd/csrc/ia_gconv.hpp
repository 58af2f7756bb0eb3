// What the grouped 3x3 convolution family shares (gconv.hip, gconv_bwd.hip, gconv_bf16.hip): the
// shape rule, the fp32 operand layout, and the device pieces of the kernels that walk a row of
// pixels in tiles of 16 with lanes (pixel i = lane & 15, channel quad / octet kk = lane >> 4).
// The fp32 and the bf16 kernel stay two kernels: operand roles (weights as B / as A), the D tile
// (channel / pixel on the lane) and the prefetch depth differ, see DESIGN 3.11.  k_gconv_dx_s2 keeps
// its own weight load, MFMA nest and store: on the helpers below its NB = 2 instance ran slower.
#pragma once
#include "ia_internal.hpp"

namespace ia {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ shapes
// channels per group, 4 / 8 / 16 / 32 (0: not covered) -- fp32 and bf16
inline int gconv_cg(int channels, int groups)
{
    if (groups < 1 || channels % groups) return 0;
    const int cg = channels / groups;
    return (cg == 4 || cg == 8 || cg == 16 || cg == 32) ? cg : 0;
}
// the channels of the fp32 kernels: whole supergroups of 16 * nb; -> channels per group (0: not covered)
inline int gconv_channels(int channels, int groups, int *nb)
{
    const int cg = (channels < 16) ? 0 : gconv_cg(channels, groups);
    *nb = (cg == 32) ? 2 : 1;
    return (cg && channels % (16 * *nb) == 0) ? cg : 0;
}
// the shapes the fp32 entries take; -> channels per group (0: not covered)
inline int gconv_shape(int batch, int H, int W, int channels, int groups, int stride, int *nb)
{
    if (batch < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2)) return 0;
    if ((int64_t)batch * H > 2147483647LL) return 0;
    return gconv_channels(channels, groups, nb);
}

// instantiates KERNEL<nb, stride> for the four (nb, stride) the fp32 kernels come in
#define GCONV_DISPATCH(nb, stride, KERNEL, grid, block, s, a)                                        \
    do {                                                                                             \
        if ((nb) == 1 && (stride) == 1) hipLaunchKernelGGL((KERNEL<1, 1>), grid, block, 0, s, a);    \
        else if ((nb) == 1) hipLaunchKernelGGL((KERNEL<1, 2>), grid, block, 0, s, a);                \
        else if ((stride) == 1) hipLaunchKernelGGL((KERNEL<2, 1>), grid, block, 0, s, a);            \
        else hipLaunchKernelGGL((KERNEL<2, 2>), grid, block, 0, s, a);                               \
    } while (0)

// ------------------------------------------------------------------ fp32 operand layout
// Element q of the (SG, 9, NB, 4, NB, 64) per-lane B operands: [sg][t][ci][c][co][lane] =
// W[o][in % cg][t] * scale[o] with o = sg*16*NB + 16*co + (lane & 15), in = sg*16*NB + 16*ci +
// 4*(lane >> 4) + c, zero when o and in belong to different groups.  adjoint: the weight of the
// input-gradient convolution -- taps flipped in both directions, input and output channel swapped
// inside each group, no scale.  The host pack and the device pack both call it: one fp32 product.
__host__ __device__ inline float gconv_pack_elem(const float *weight, const float *scale, int cg, int NB,
                                                 int64_t q, bool adjoint)
{
    const int lane = (int)(q & 63); q >>= 6;
    const int co = (int)(q % NB); q /= NB;
    const int c = (int)(q & 3); q >>= 2;
    const int ci = (int)(q % NB); q /= NB;
    const int t = (int)(q % 9);
    const int sg = (int)(q / 9);
    const int sgc = 16 * NB;
    const int o = sg * sgc + 16 * co + (lane & 15);
    const int in = sg * sgc + 16 * ci + 4 * (lane >> 4) + c;
    if (o / cg != in / cg) return 0.0f;
    if (adjoint) return weight[((size_t)in * cg + (o % cg)) * 9 + (8 - t)];
    return weight[((size_t)o * cg + (in % cg)) * 9 + t] * (scale ? scale[o] : 1.0f);
}

// ------------------------------------------------------------------ DPP pixel shifts
// A DPP row holds the 16 pixels of one channel quad / octet.  Value of pixel i-1: row_shr:1 of the
// centre, lane 0 from the previous tile's lane 15 (row_ror:1 of it); value of pixel i+1: row_shl:1,
// lane 15 from the next tile's lane 0 (row_ror:15 of it).  Lanes without a DPP source keep `old`
// (bound_ctrl = 0).  On 32-bit words: an fp32 channel, or two bf16 channels of ONE pixel.
__device__ __forceinline__ uint32_t dpp_shr1(uint32_t old, uint32_t src)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, 0x111, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t dpp_shl1(uint32_t old, uint32_t src)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, 0x101, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_ror(uint32_t src)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)src, CTRL, 0xf, 0xf, false);
}
// a lane's 16-byte fragment of pixel i - 1 / i + 1
__device__ __forceinline__ uint4 shift_from_left(const uint4 &c, const uint4 &prev)
{
    return make_uint4(dpp_shr1(dpp_ror<0x121>(prev.x), c.x), dpp_shr1(dpp_ror<0x121>(prev.y), c.y),
                      dpp_shr1(dpp_ror<0x121>(prev.z), c.z), dpp_shr1(dpp_ror<0x121>(prev.w), c.w));
}
__device__ __forceinline__ uint4 shift_from_right(const uint4 &c, const uint4 &next)
{
    return make_uint4(dpp_shl1(dpp_ror<0x12F>(next.x), c.x), dpp_shl1(dpp_ror<0x12F>(next.y), c.y),
                      dpp_shl1(dpp_ror<0x12F>(next.z), c.z), dpp_shl1(dpp_ror<0x12F>(next.w), c.w));
}
__device__ __forceinline__ f32x4 shift_from_left(const f32x4 &c, const f32x4 &prev)
{
    return __builtin_bit_cast(f32x4, shift_from_left(__builtin_bit_cast(uint4, c), __builtin_bit_cast(uint4, prev)));
}
__device__ __forceinline__ f32x4 shift_from_right(const f32x4 &c, const f32x4 &next)
{
    return __builtin_bit_cast(f32x4, shift_from_right(__builtin_bit_cast(uint4, c), __builtin_bit_cast(uint4, next)));
}

// ------------------------------------------------------------------ loads
// out-of-image taps: the address is clamped by the caller, the 16-byte load unconditional, the
// value zeroed by `in`.  (The bf16 kernel keeps its own mask-and form inline: behind a helper the
// compiler turned the masks into selects and branched over them)
__device__ __forceinline__ f32x4 gconv_load16(const float *p, bool in)
{
    const f32x4 q = *reinterpret_cast<const f32x4 *>(p);
    f32x4 z; z.x = z.y = z.z = z.w = 0.0f;
    return in ? q : z;
}

// ------------------------------------------------------------------ fp32 MFMA pieces
// NB = 16-channel blocks per supergroup (1: Cg <= 16, 2: Cg = 32).  B operands of supergroup sg for
// this lane, w[t][ci][c][co]: resident for the wavefront's lifetime (36 VGPRs, 144 for NB = 2)
template <int NB>
__device__ __forceinline__ void gconv_load_w(const float *wpack, int sg, int lane, float (&w)[9][NB][4][NB])
{
    const float *wp = wpack + (size_t)sg * 9 * NB * 4 * NB * 64 + lane;
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
// one tap: component c of input block ci's quad is the k-slice of step c
template <int NB>
__device__ __forceinline__ void gconv_mfma_tap(const f32x4 (&v)[NB], const float (&w)[NB][4][NB], f32x4 (&acc)[NB])
{
#pragma unroll
    for (int ci = 0; ci < NB; ++ci) {
        const float e[4] = {v[ci].x, v[ci].y, v[ci].z, v[ci].w};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int co = 0; co < NB; ++co)
                acc[co] = __builtin_amdgcn_mfma_f32_16x16x4f32(e[c], w[ci][c][co], acc[co], 0, 0, 0);
    }
}
// D: column (lane & 15) = channel (the lane's, already in `out`), row 4 * kk + r = pixel j of the
// tile, stored at x = xmap(j) when x < n
template <int NB, class XMap>
__device__ __forceinline__ void gconv_store_tile(float *out, int C, int n, int kk, const f32x4 (&acc)[NB], XMap xmap)
{
#pragma unroll
    for (int co = 0; co < NB; ++co) {
        const float o[4] = {acc[co].x, acc[co].y, acc[co].z, acc[co].w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int x = xmap(4 * kk + r);
            if (x < n) out[(size_t)x * C + 16 * co] = o[r];
        }
    }
}

}  // namespace ia
