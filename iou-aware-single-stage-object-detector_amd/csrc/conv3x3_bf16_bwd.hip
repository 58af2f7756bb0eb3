// Backward of the bf16 3x3 / stride 1 / pad 1 convolution (conv3x3_bf16.hip) for mixed-precision training
// of the RetinaNet heads: bf16 activations and gradients, fp32 master weights and weight gradients.
//
//  * WEIGHT GRADIENT (k_conv3x3_bf16_wgrad + k_conv3x3_bf16_wgrad_reduce), one weight shared by a list
//    of levels and up to two groups:
//        dW[g][co][ci][ky][kx] = sum_l sum_b sum_{y,x} dy_l[b,y,x,co] * x_l[b,y+ky-1,x+kx-1,ci]
//    nine GEMMs (one per tap) on v_mfma_f32_32x32x16_bf16 with M = Cout (A operand = dy), N = Cin (B
//    operand = x) and K = every pixel of every level and image.  K is the STRIDED dimension of both
//    operands in memory (channels-last: a pixel's channels are contiguous), so a workgroup stages
//    [pixel][channel] tiles in LDS with 16-byte loads -- a 128-pixel tile of dy and its (TH + 2) x
//    (TW + 2) halo patch of x, which serves all nine taps as shifted windows -- and reads the
//    fragments K-major with ds_read_b64_tr_b16 (the transposing LDS read of gfx950).
//      - A workgroup = four wavefronts = a 64 (co) x 64 (ci) tile of dW for all nine taps: wavefront
//        (wm, wn) owns 32 x 32 of it, nine accumulator blocks = 144 registers; two workgroups share a
//        CU, one's staging runs under the other's MFMAs.
//      - LDS image: per operand two planes of 32 channels, [plane][pixel][32 channels] with 64-byte
//        rows, no padding.  A transposing read takes, per 16-lane group, 4 rows (pixels) x 16 columns
//        (channels); a 32-lane half = two groups = the same 4 pixels x 32 channels = 4 x 64 bytes.  The
//        four pixels of a block are neighbours in one tile row (TW % 4 == 0), so they are four
//        consecutive 64-byte rows of the image whatever the tap: 256 contiguous bytes = each of the 64
//        banks once.  No conflicts on either operand.
//      - The sum over K may run in any order as long as both operands agree: element j of lane half h
//        in k-step s is tile pixel 16 s + 8 h + j for dy and the same pixel shifted by the tap for x.
//      - Every lane of every wavefront supplies an in-bounds, 8-byte aligned address (the transposing
//        read gathers across lanes: EXEC must be full).  Pixels outside the map -- the halo at the image
//        border and the overhang of the last tiles -- are ZEROS in LDS, never masked lanes.  Channels
//        beyond Cout / Cin are zero rows / columns of the 64 x 64 tile that are not stored.
//      - Split K: the tiles of all levels and images form one list, cut into `slices` runs of
//        `slice_tiles` tiles; workgroup (slice, channel tile, group) accumulates its run in fp32 and
//        writes a partial dW to the caller's workspace, the reduce kernel adds the partials of an
//        element in slice order and writes the nn.Conv2d layout (groups * Cout, Cin, 3, 3).  No
//        atomics, same bits on every run, nothing read that this call did not write.
//  * ia_conv3x3_bf16_pack_f32: fp32 master weight -> rounded to bf16 (nearest even) in the forward
//    kernel's fragment order, one launch; adjoint = 1 writes the weight of the input-gradient
//    convolution, w'[ci][co][ky][kx] = w[co][ci][2-ky][2-kx], with its input channels (= Cout) padded
//    by ZERO ROWS to the next multiple of 32 -- dx = ia_conv3x3_bf16_levels(dy, w').
//  * ia_relu_bwd_bias_grad_bf16: g = dy where y > 0 (else a zero with dy's sign, what dy * (y > 0)
//    gives), db = fp32 column sums through per-strip partial rows added in a fixed order.
#include <string.h>
#include "ia_internal.hpp"
#include "ia_math.hpp"
#include "ia_conv3.hpp"

namespace ia {

typedef __attribute__((ext_vector_type(8))) __bf16 wg_bf16x8;
typedef __attribute__((ext_vector_type(4))) short wg_s16x4;
typedef __attribute__((ext_vector_type(16))) float wg_f32x16;
typedef __attribute__((address_space(3))) wg_s16x4 wg_lds_s16x4;

constexpr int kWgTilePx = 128;            // pixels of a tile: TH x TW = 32 x 4, 16 x 8, 8 x 16 or 4 x 32
constexpr int kWgPatchPx = 204;           // (TH + 2) * (TW + 2) <= this (34 x 6)
constexpr int kWgBM = 64, kWgBN = 64;     // dW tile of a workgroup: output x input channels
constexpr int kWgRow = 64;                // bytes of an LDS row: 32 channels of one pixel
constexpr int kWgDyPlane = kWgTilePx * kWgRow, kWgXPlane = kWgPatchPx * kWgRow;
constexpr int kWgXBase = 2 * kWgDyPlane;
constexpr int kWgLds = 2 * kWgDyPlane + 2 * kWgXPlane;     // 42 496 bytes
constexpr int kWgXPieces = (kWgPatchPx * 8 + 255) / 256;   // 16-byte pieces of the patch per thread: 7
// split K: about kWgTargetWgs workgroups (two per CU), at most kWgMaxSlices partial results, at least
// kWgMinSliceTiles tiles (512 pixels) per slice
constexpr int kWgTargetWgs = 512, kWgMaxSlices = 64, kWgMinSliceTiles = 4;

struct WgradArgs {
    const uint16_t *x[kCvMaxGroups][IA_MAX_LEVELS];    // (B, H_l, W_l, .) bf16, pixel stride xs, 16-byte aligned
    const uint16_t *dy[kCvMaxGroups][IA_MAX_LEVELS];   // (B, H_l, W_l, .) bf16, pixel stride dys
    float *ws;                            // [slice][group][tap][Cout][Cin] fp32 partials
    int32_t L, B, G, Cin, Cout, xs, dys;
    int32_t dy_vec;                       // every dy pointer 16-byte aligned and dys % 8 == 0: 16-byte loads
    int32_t ntiles, slice_tiles, slices, ncit;
    int32_t H[IA_MAX_LEVELS], W[IA_MAX_LEVELS], lgTW[IA_MAX_LEVELS], magic[IA_MAX_LEVELS];
    int32_t tiles_y[IA_MAX_LEVELS], tiles_x[IA_MAX_LEVELS], tile_off[IA_MAX_LEVELS + 1];
};

__device__ __forceinline__ wg_bf16x8 wg_frag(const unsigned char *s, int off0, int off1)
{
    // two transposing reads = the 8 k-values of this lane: pixels (.. + 0..3) and (.. + 4..7)
    const wg_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s16x4 *)(s + off0));
    const wg_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s16x4 *)(s + off1));
    return __builtin_bit_cast(wg_bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

__global__ void __launch_bounds__(256, 2) k_conv3x3_bf16_wgrad(WgradArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_t[kWgLds];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv >> 1, wn = wv & 1;
    const int slice = (int)blockIdx.x, grp = (int)blockIdx.z;
    const int cot = (int)blockIdx.y / a.ncit, cit = (int)blockIdx.y - cot * a.ncit;
    const int co0 = cot * kWgBM, ci0 = cit * kWgBN;

    // ---- the transposing reads of this lane (cdna4: per 16-lane group, lane 4 q + p supplies the
    // address of row q, columns 4 p .. 4 p + 3 of a 4 x 16 block and receives column (lane & 15), row q
    // in element q).  Group (lane >> 4): channels 16 * (group & 1) .., lane half h = group >> 1.
    const int fq = (lane & 15) >> 2, fp = lane & 3, fcb = (lane >> 4) & 1, fh = lane >> 5;
    const int col_off = (16 * fcb + 4 * fp) * 2;          // bytes inside a 64-byte row: 8-byte aligned
    const int m_lane = 8 * fh + fq;                       // + 16 s + 4 u: the tile pixel this lane addresses

    // ---- staging: piece c = u * 256 + tid -> pixel c >> 3, 16-byte part c & 7 (channels 8 * part ..)
    const int part = tid & 7;
    const int lds_part = (part >> 2) * 1 /* plane */, lds_col = (part & 3) * 16;
    const int ch_dy = co0 + part * 8, ch_x = ci0 + part * 8;
    const bool ch_dy_ok = ch_dy < a.Cout, ch_x_ok = ch_x < a.Cin;

    wg_f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    const int t0 = slice * a.slice_tiles;
    const int t1 = t0 + a.slice_tiles < a.ntiles ? t0 + a.slice_tiles : a.ntiles;
    int lv = 0;
    for (int t = t0; t < t1; ++t) {
        while (lv + 1 < a.L && t >= a.tile_off[lv + 1]) ++lv;     // workgroup-uniform
        int r = t - a.tile_off[lv];
        const int H = a.H[lv], W = a.W[lv], lg = a.lgTW[lv], magic = a.magic[lv];
        const int TW = 1 << lg, TH = kWgTilePx >> lg, PW = TW + 2, npatch = (TH + 2) * PW;
        const int txi = r % a.tiles_x[lv]; r /= a.tiles_x[lv];
        const int tyi = r % a.tiles_y[lv];
        const int b = r / a.tiles_y[lv];
        const int y0 = tyi * TH, x0 = txi * TW;
        const uint16_t *xb = a.x[grp][lv] + (size_t)b * H * W * a.xs;
        const uint16_t *db = a.dy[grp][lv] + (size_t)b * H * W * a.dys;

        // ---- global -> registers.  Addresses are clamped into the map, the zero padding is an AND
        // with a per-piece mask at the LDS store.
        uint4 rd[4], rx[kWgXPieces];
        uint32_t md[4], mx[kWgXPieces];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int m = (u * 256 + tid) >> 3;
            const int iy = y0 + (m >> lg), ix = x0 + (m & (TW - 1));
            const bool in = iy < H && ix < W && ch_dy_ok;
            md[u] = in ? 0xffffffffu : 0u;
            const int cy = iy < H ? iy : H - 1, cx = ix < W ? ix : W - 1;
            const uint16_t *p = db + ((size_t)cy * W + cx) * a.dys;
            if (a.dy_vec) {
                rd[u] = *reinterpret_cast<const uint4 *>(p + (ch_dy_ok ? ch_dy : 0));
            } else {
                // a dy that is not 16-byte addressable (an odd channel offset or stride): element loads
                uint32_t e[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) e[k] = ch_dy + k < a.Cout ? (uint32_t)p[ch_dy + k] : 0u;
                rd[u] = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
            }
        }
#pragma unroll
        for (int u = 0; u < kWgXPieces; ++u) {
            const int pp = (u * 256 + tid) >> 3;
            const int py = (pp * magic) >> 16, px = pp - py * PW;     // pp / PW, pp % PW (exact for pp < 224, PW <= 34)
            const int iy = y0 + py - 1, ix = x0 + px - 1;
            const bool in = pp < npatch && iy >= 0 && iy < H && ix >= 0 && ix < W && ch_x_ok;
            mx[u] = in ? 0xffffffffu : 0u;
            const int cy = iy < 0 ? 0 : (iy >= H ? H - 1 : iy), cx = ix < 0 ? 0 : (ix >= W ? W - 1 : ix);
            rx[u] = *reinterpret_cast<const uint4 *>(xb + ((size_t)cy * W + cx) * a.xs + (ch_x_ok ? ch_x : 0));
        }
        __syncthreads();                  // every wavefront is done reading the previous tile
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int m = (u * 256 + tid) >> 3;
            *reinterpret_cast<uint4 *>(s_t + lds_part * kWgDyPlane + m * kWgRow + lds_col) =
                make_uint4(rd[u].x & md[u], rd[u].y & md[u], rd[u].z & md[u], rd[u].w & md[u]);
        }
#pragma unroll
        for (int u = 0; u < kWgXPieces; ++u) {
            const int pp = (u * 256 + tid) >> 3;
            if (pp < kWgPatchPx)          // rows [npatch, 204) are written too (zeros): nothing in LDS stays undefined
                *reinterpret_cast<uint4 *>(s_t + kWgXBase + lds_part * kWgXPlane + pp * kWgRow + lds_col) =
                    make_uint4(rx[u].x & mx[u], rx[u].y & mx[u], rx[u].z & mx[u], rx[u].w & mx[u]);
        }
        __syncthreads();

        // ---- 8 k-steps of 16 pixels x 9 taps.  All 64 lanes of all four wavefronts run this loop.
        const unsigned char *sa = s_t + wm * kWgDyPlane + col_off;
        const unsigned char *sb = s_t + kWgXBase + wn * kWgXPlane + col_off;
#pragma unroll 2
        for (int s = 0; s < kWgTilePx / 16; ++s) {
            const int m0 = 16 * s + m_lane, m1 = m0 + 4;
            const wg_bf16x8 fa = wg_frag(sa, m0 * kWgRow, m1 * kWgRow);
            const int p0 = ((m0 >> lg) * PW + (m0 & (TW - 1))) * kWgRow;
            const int p1 = ((m1 >> lg) * PW + (m1 & (TW - 1))) * kWgRow;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int toff = ((tap / 3) * PW + (tap % 3)) * kWgRow;
                const wg_bf16x8 fb = wg_frag(sb, p0 + toff, p1 + toff);
                acc[tap] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[tap], 0, 0, 0);
            }
        }
    }

    // ---- partial dW of this slice: block (tap): column ci = lane & 31, row co = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int ci = ci0 + wn * 32 + (lane & 31);
    const int co_w = co0 + wm * 32 + 4 * (lane >> 5);
    if (ci < a.Cin) {
        float *wsb = a.ws + ((size_t)(slice * a.G + grp) * 9) * a.Cout * a.Cin + ci;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co_w + (r & 3) + 8 * (r >> 2);
                if (co < a.Cout) wsb[((size_t)tap * a.Cout + co) * a.Cin] = acc[tap][r];
            }
    }
}

// dW[g][co][ci][tap] = the partials [slice][g][tap][co][ci] added in slice order
__global__ void __launch_bounds__(256) k_conv3x3_bf16_wgrad_reduce(const float *ws, float *dw, int slices, int G,
                                                                    int Cout, int Cin)
{
    const int64_t total = (int64_t)G * 9 * Cout * Cin;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    float v = ws[idx];
    for (int s = 1; s < slices; ++s) v += ws[(int64_t)s * total + idx];
    int64_t r = idx;
    const int ci = (int)(r % Cin); r /= Cin;
    const int co = (int)(r % Cout); r /= Cout;
    const int tap = (int)(r % 9);
    const int g = (int)(r / 9);
    dw[(((int64_t)g * Cout + co) * Cin + ci) * 9 + tap] = v;
}

// fp32 (groups * Cout, Cin, 3, 3) -> the fragment order of k_conv3x3_pack (conv3x3_bf16.hip) for a
// convolution with Kin input and Kout output channels: (Cin, Cout), or -- adjoint -- (Cout rounded up to
// 32, Cin) with w'[ci][co][tap] = w[co][ci][8 - tap] and zero rows for the padded input channels
__global__ void __launch_bounds__(256) k_conv3x3_pack_f32(const float *w, uint16_t *wp, int Cin, int Cout, int groups,
                                                           int adjoint, int Kin, int Kout)
{
    const int ntile = (Kout + 255) / 256, nchunk = Kin / 32;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)groups * ntile * 256 * 9 * Kin;
    if (idx >= total) return;
    const int e = (int)(idx & 7);
    int64_t r = idx >> 3;
    const int lane = (int)(r & 63); r >>= 6;
    const int kk = (int)(r & 1); r >>= 1;
    const int j = (int)(r & 1); r >>= 1;
    const int wn = (int)(r & 3); r >>= 2;
    const int tap = (int)(r % 9); r /= 9;
    const int chunk = (int)(r % nchunk); r /= nchunk;
    const int nt = (int)(r % ntile);
    const int g = (int)(r / ntile);
    const int n = nt * 256 + wn * 64 + j * 32 + (lane & 31);            // output channel of the convolution
    const int k = chunk * 32 + kk * 16 + (lane >> 5) * 8 + e;            // input channel
    float v = 0.0f;
    if (adjoint) {
        if (n < Cin && k < Cout) v = w[(((int64_t)g * Cout + k) * Cin + n) * 9 + (8 - tap)];
    } else {
        if (n < Cout) v = w[(((int64_t)g * Cout + n) * Cin + k) * 9 + tap];
    }
    wp[idx] = (uint16_t)f32_to_bf16(v);
}

// ------------------------------------------------------------------ ReLU backward + bias gradient
// (rows, n) bf16 with row strides.  A workgroup of 256 threads = 16 column lanes of VEC columns x 16 row
// lanes walks one of S row strips of one column block; its column sums go to partial[cb][s][16 * VEC],
// k_colsum_finish_bf16 adds the S partial rows of a block in a fixed order.
struct ReluColsumBf16Args {
    const uint16_t *dy, *y; uint16_t *g; float *db, *partial;
    int64_t rows, dys, ys, gs, strip;
    int32_t n, S;
};

__device__ __forceinline__ uint32_t wg_mask1(uint32_t d, uint32_t y)
{
    // y > 0 as bf16: not negative, not zero, not NaN; a masked element keeps dy's sign (dy * 0)
    const bool pos = !(y & 0x8000u) && (y & 0x7fffu) != 0u && (y & 0x7fffu) <= 0x7f80u;
    return pos ? d : (d & 0x8000u);
}

template <int VEC>
__global__ void __launch_bounds__(256) k_relu_bwd_colsum_bf16(ReluColsumBf16Args a)
{
    __shared__ float red[256][VEC];
    const int t = threadIdx.x, ql = t & 15, rl = t >> 4;
    const int cb = blockIdx.y, s = blockIdx.x;
    const int c0 = (cb * 16 + ql) * VEC;
    const int64_t r0 = (int64_t)s * a.strip;
    const int64_t r1 = r0 + a.strip < a.rows ? r0 + a.strip : a.rows;
    float acc[2][VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[0][e] = acc[1][e] = 0.0f;
    if (c0 < a.n) {
        int par = 0;
        for (int64_t r = r0 + rl; r < r1; r += 16, par ^= 1) {
            uint32_t d[VEC];
            if constexpr (VEC == 8) {
                const uint4 dv = *reinterpret_cast<const uint4 *>(a.dy + r * a.dys + c0);
                uint32_t w[4] = {dv.x, dv.y, dv.z, dv.w};
                if (a.y) {
                    const uint4 yv = *reinterpret_cast<const uint4 *>(a.y + r * a.ys + c0);
                    const uint32_t yw[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        w[k] = wg_mask1(w[k] & 0xffffu, yw[k] & 0xffffu) | (wg_mask1(w[k] >> 16, yw[k] >> 16) << 16);
                }
                if (a.g) *reinterpret_cast<uint4 *>(a.g + r * a.gs + c0) = make_uint4(w[0], w[1], w[2], w[3]);
#pragma unroll
                for (int k = 0; k < 4; ++k) { d[2 * k] = w[k] & 0xffffu; d[2 * k + 1] = w[k] >> 16; }
            } else {
                d[0] = a.dy[r * a.dys + c0];
                if (a.y) d[0] = wg_mask1(d[0], a.y[r * a.ys + c0]);
                if (a.g) a.g[r * a.gs + c0] = (uint16_t)d[0];
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[par][e] += from_bits(d[e] << 16);
        }
    }
    if (!a.db) return;
#pragma unroll
    for (int e = 0; e < VEC; ++e) red[t][e] = acc[0][e] + acc[1][e];
    __syncthreads();
    if (t < 16) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = red[k * 16 + t][e];
#pragma unroll
            for (int w = 8; w > 0; w >>= 1)           // pairwise: 16 -> 8 -> 4 -> 2 -> 1
#pragma unroll
                for (int k = 0; k < w; ++k) v[k] = v[k] + v[k + w];
            a.partial[((int64_t)cb * a.S + s) * (16 * VEC) + t * VEC + e] = v[0];
        }
    }
}

template <int VEC>
__global__ void __launch_bounds__(256) k_colsum_finish_bf16(ReluColsumBf16Args a)
{
    __shared__ float red[256][VEC];
    const int t = threadIdx.x, ql = t & 15, rl = t >> 4;
    const int cb = blockIdx.x;
    float v[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = 0.0f;
    for (int k = rl; k < a.S; k += 16)
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] += a.partial[((int64_t)cb * a.S + k) * (16 * VEC) + ql * VEC + e];
#pragma unroll
    for (int e = 0; e < VEC; ++e) red[t][e] = v[e];
    __syncthreads();
    if (t < 16) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float o[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) o[k] = red[k * 16 + t][e];
#pragma unroll
            for (int w = 8; w > 0; w >>= 1)
#pragma unroll
                for (int k = 0; k < w; ++k) o[k] = o[k] + o[k + w];
            const int c = (cb * 16 + t) * VEC + e;
            if (c < a.n) a.db[c] = o[0];
        }
    }
}

// the plan of a weight-gradient call: tile shapes, the tile list, the split of K.  -> 0 or IA_E_ARG
static int wgrad_plan(const ia_conv3x3_desc *d, WgradArgs &a)
{
    if (!d || d->num_levels < 1 || d->num_levels > IA_MAX_LEVELS || d->batch < 1 || d->groups < 1 ||
        d->groups > kCvMaxGroups || d->cin < 32 || (d->cin % 32) || d->cout < 1 || d->x_stride < d->cin ||
        (d->x_stride & 7) || d->y_stride < d->cout)
        return IA_E_ARG;
    memset(&a, 0, sizeof(a));
    a.L = d->num_levels; a.B = d->batch; a.G = d->groups; a.Cin = d->cin; a.Cout = d->cout;
    a.xs = d->x_stride; a.dys = d->y_stride;
    int64_t tiles = 0;
    for (int l = 0; l < a.L; ++l) {
        const int H = d->H[l], W = d->W[l];
        if (H < 1 || W < 1) return IA_E_ARG;
        // the tile shape with the fewest tiles; 8 x 16 on a tie
        int best_lg = 4;
        int64_t best = -1;
        for (int lg : {4, 3, 5, 2}) {
            const int tw = 1 << lg, th = kWgTilePx >> lg;
            const int64_t n = (int64_t)((H + th - 1) / th) * ((W + tw - 1) / tw);
            if (best < 0 || n < best) { best = n; best_lg = lg; }
        }
        const int tw = 1 << best_lg, th = kWgTilePx >> best_lg;
        a.H[l] = H; a.W[l] = W; a.lgTW[l] = best_lg; a.magic[l] = 65536 / (tw + 2) + 1;
        a.tiles_y[l] = (H + th - 1) / th; a.tiles_x[l] = (W + tw - 1) / tw;
        a.tile_off[l] = (int32_t)tiles;
        tiles += (int64_t)a.B * a.tiles_y[l] * a.tiles_x[l];
        if (tiles > 2147483647LL / 2) return IA_E_ARG;
    }
    for (int l = a.L; l <= IA_MAX_LEVELS; ++l) a.tile_off[l] = (int32_t)tiles;
    a.ntiles = (int32_t)tiles;
    a.ncit = (a.Cin + kWgBN - 1) / kWgBN;
    const int64_t nout = (int64_t)((a.Cout + kWgBM - 1) / kWgBM) * a.ncit * a.G;
    if (nout > 65535) return IA_E_ARG;
    int64_t want = (kWgTargetWgs + nout - 1) / nout;
    if (want > kWgMaxSlices) want = kWgMaxSlices;
    int64_t st = (tiles + want - 1) / want;
    if (st < kWgMinSliceTiles) st = kWgMinSliceTiles;
    a.slice_tiles = (int32_t)st;
    a.slices = (int32_t)((tiles + st - 1) / st);
    return 0;
}

}  // namespace ia

extern "C" {

int ia_conv3x3_bf16_wgrad_plan(const ia_conv3x3_desc *d, int32_t *tiles, int32_t *slice_tiles, int32_t *slices)
{
    ia::WgradArgs a;
    const int rc = ia::wgrad_plan(d, a);
    if (rc) return rc;
    if (tiles) *tiles = a.ntiles;
    if (slice_tiles) *slice_tiles = a.slice_tiles;
    if (slices) *slices = a.slices;
    return 0;
}

size_t ia_conv3x3_bf16_wgrad_workspace_bytes(const ia_conv3x3_desc *d)
{
    ia::WgradArgs a;
    if (ia::wgrad_plan(d, a)) return 0;
    return (size_t)a.slices * a.G * 9 * a.Cout * a.Cin * sizeof(float);
}

int ia_conv3x3_bf16_wgrad_levels(const ia_conv3x3_desc *d, float *dw, void *workspace, size_t workspace_bytes,
                                 void *stream)
{
    ia::WgradArgs a;
    const int rc = ia::wgrad_plan(d, a);
    if (rc) return rc;
    if (!dw || ((uintptr_t)dw & 3u)) return IA_E_ARG;
    if (!workspace || ((uintptr_t)workspace & 15u) ||
        workspace_bytes < (size_t)a.slices * a.G * 9 * a.Cout * a.Cin * sizeof(float))
        return IA_E_WORKSPACE;
    a.dy_vec = (d->y_stride & 7) ? 0 : 1;
    for (int l = 0; l < a.L; ++l)
        for (int g = 0; g < a.G; ++g) {
            if (!d->x[g][l] || !d->y[g][l] || ((uintptr_t)d->x[g][l] & 15u) || ((uintptr_t)d->y[g][l] & 1u))
                return IA_E_ARG;
            if ((uintptr_t)d->y[g][l] & 15u) a.dy_vec = 0;
            a.x[g][l] = static_cast<const uint16_t *>(d->x[g][l]);
            a.dy[g][l] = static_cast<const uint16_t *>(d->y[g][l]);
        }
    a.ws = static_cast<float *>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)a.slices, (unsigned)(((a.Cout + ia::kWgBM - 1) / ia::kWgBM) * a.ncit), (unsigned)a.G);
    hipLaunchKernelGGL(ia::k_conv3x3_bf16_wgrad, grid, dim3(256), 0, st, a);
    const int64_t total = (int64_t)a.G * 9 * a.Cout * a.Cin;
    hipLaunchKernelGGL(ia::k_conv3x3_bf16_wgrad_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       a.ws, dw, a.slices, a.G, a.Cout, a.Cin);
    return ia::hip_status(hipGetLastError());
}

int ia_conv3x3_bf16_pack_f32(const float *w, int cin, int cout, int groups, int adjoint, void *wp, void *stream)
{
    if (!w || !wp || cin < 32 || (cin % 32) || cout < 1 || groups < 1 || groups > ia::kCvMaxGroups ||
        ((uintptr_t)w & 3u) || ((uintptr_t)wp & 15u))
        return IA_E_ARG;
    const int kin = adjoint ? (cout + 31) / 32 * 32 : cin, kout = adjoint ? cin : cout;
    const int64_t total = (int64_t)(ia_conv3x3_bf16_packed_bytes(kin, kout, groups) / 2);
    hipLaunchKernelGGL(ia::k_conv3x3_pack_f32, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, w, static_cast<uint16_t *>(wp), cin, cout, groups, adjoint ? 1 : 0,
                       kin, kout);
    return ia::hip_status(hipGetLastError());
}

size_t ia_relu_bwd_bias_grad_bf16_workspace_bytes(int64_t rows, int n)
{
    if (rows < 1 || n < 1 || n > 65536) return 0;
    return (size_t)((n + 127) / 128) * 128 * IA_COLSUM_MAX_STRIPS * sizeof(float);
}

int ia_relu_bwd_bias_grad_bf16(const void *dy, int64_t dy_stride, const void *y, int64_t y_stride, int64_t rows,
                               int n, void *g, int64_t g_stride, float *db, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    if (!dy || rows < 1 || n < 1 || n > 65536 || dy_stride < n || (y && y_stride < n) || (g && g_stride < n) ||
        (y && !g) || (!g && !db))
        return IA_E_ARG;
    if (((uintptr_t)dy | (uintptr_t)y | (uintptr_t)g) & 1u) return IA_E_ARG;
    if (db && (!workspace || ((uintptr_t)workspace & 15u) ||
               workspace_bytes < ia_relu_bwd_bias_grad_bf16_workspace_bytes(rows, n)))
        return IA_E_WORKSPACE;
    // 16-byte accesses when every row start and the channel count allow them
    const bool vec = !(n & 7) && !(dy_stride & 7) && !((uintptr_t)dy & 15u) &&
                     (!y || (!(y_stride & 7) && !((uintptr_t)y & 15u))) &&
                     (!g || (!(g_stride & 7) && !((uintptr_t)g & 15u)));
    const int cols = vec ? 128 : 16;
    const int ncb = (n + cols - 1) / cols;
    // ~2048 workgroups in all, at least 64 rows per strip
    int64_t S = 2048 / ncb;
    if (S > IA_COLSUM_MAX_STRIPS) S = IA_COLSUM_MAX_STRIPS;
    if (S > (rows + 63) / 64) S = (rows + 63) / 64;
    if (S < 1) S = 1;
    int64_t strip = (rows + S - 1) / S;
    strip = (strip + 15) / 16 * 16;
    S = (rows + strip - 1) / strip;
    ia::ReluColsumBf16Args a;
    a.dy = static_cast<const uint16_t *>(dy); a.y = static_cast<const uint16_t *>(y);
    a.g = static_cast<uint16_t *>(g); a.db = db; a.partial = static_cast<float *>(workspace);
    a.rows = rows; a.dys = dy_stride; a.ys = y_stride; a.gs = g_stride; a.strip = strip; a.n = n; a.S = (int32_t)S;
    hipStream_t st = (hipStream_t)stream;
    if (vec) {
        hipLaunchKernelGGL(ia::k_relu_bwd_colsum_bf16<8>, dim3((unsigned)S, (unsigned)ncb), dim3(256), 0, st, a);
        if (db) hipLaunchKernelGGL(ia::k_colsum_finish_bf16<8>, dim3((unsigned)ncb), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL(ia::k_relu_bwd_colsum_bf16<1>, dim3((unsigned)S, (unsigned)ncb), dim3(256), 0, st, a);
        if (db) hipLaunchKernelGGL(ia::k_colsum_finish_bf16<1>, dim3((unsigned)ncb), dim3(256), 0, st, a);
    }
    return ia::hip_status(hipGetLastError());
}

}  // extern "C"
