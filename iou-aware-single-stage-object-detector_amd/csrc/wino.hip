// Winograd F(4x4, 3x3) transforms for the 3x3 / stride-1 / pad-1 convolutions of the head
// (reference iou_aware_retina_head.py:171-219: 4+4 tower convs 256->256, retina_cls 256->720,
// retina_reg 256->36, retina_iou 256->9, weights shared by the five pyramid levels) and of the
// FPN outputs.  Those convolutions are 63 % of the network's multiply-adds at 800x1344; as direct
// / implicit-GEMM fp32 convolutions they run at ~110-125 TFLOP/s of the 157 TFLOP/s MFMA peak, so
// the only large lever left is the number of multiplications: F(4x4,3x3) needs 36 per 16 outputs
// instead of 144.
//
// Split of work:
//   k_wino_in   (this file)   d (6x6 input patch per tile, zero padded) -> V = B^T d B, scattered
//                             as 36 matrices V[k] of (tiles x Cin); ALL pyramid levels of the
//                             batch form one tile list, so the shared-weight head needs ONE
//                             batched GEMM per layer instead of five small ones;
//   batched GEMM              M[k] = V[k] (tiles x Cin) . U[k] (Cin x Cout), 36 (x groups) plain
//                             fp32 GEMMs -> rocBLAS / hipBLASLt through torch.bmm (library GEMM);
//   k_wino_out  (this file)   Y = A^T M A (4x4 outputs per tile) + bias (+ ReLU), written straight
//                             into the channels-last activation / head-output tensors;
//   k_wino_mid  (this file)   k_wino_out of a layer and k_wino_in of the next layer of the same
//                             geometry in one launch (the head's tower transitions): the
//                             activation in between stays in LDS;
//   k_wino_in_gemm (this file) k_wino_in and the 36 products of a 64 -> 64 convolution in one
//                             launch (ResNet stage 1): V stays in LDS;
//   k_wino_conv (this file)   k_wino_in_gemm and k_wino_out of that convolution in one launch: M
//                             stays in the accumulators.
// Activations are channels-last fp32: a wavefront handles one tile x 256 channels, 16 bytes per
// lane, so every load / store instruction moves one contiguous 1 KiB pixel row.  Both kernels
// are HBM-bound streams (36 x 16 B in, 36 x 16 B out per lane; 36 in, 16 out).
// Transform matrices: Lavin & Gray, "Fast Algorithms for Convolutional Neural Networks"
// (interpolation points 0, +-1, +-2, inf); weights are transformed once on the host side
// (U = G g G^T in fp64, iouaware/winograd.py).
#include <string.h>
#include "ia_internal.hpp"
#include "ia_wino.hpp"

namespace ia {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
// streaming accesses: V is written once and read by the GEMM much later, M is read exactly once
__device__ __forceinline__ float4 load_nt(const float *p)
{
    const f32x4_t q = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t *>(p));
    return make_float4(q.x, q.y, q.z, q.w);
}
__device__ __forceinline__ void store_nt(float *p, const float4 &v)
{
    f32x4_t q; q.x = v.x; q.y = v.y; q.z = v.z; q.w = v.w;
    __builtin_nontemporal_store(q, reinterpret_cast<f32x4_t *>(p));
}
__device__ __forceinline__ float4 f4(float v) { return make_float4(v, v, v, v); }
__device__ __forceinline__ float4 operator+(const float4 &a, const float4 &b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 operator-(const float4 &a, const float4 &b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 operator*(float s, const float4 &a) { return make_float4(s * a.x, s * a.y, s * a.z, s * a.w); }

// one line of B^T d (the same 6-point transform is applied to rows, then to columns)
__device__ __forceinline__ void bt6(const float4 (&d)[6], float4 (&o)[6])
{
    o[0] = (4.0f * d[0] - 5.0f * d[2]) + d[4];
    o[1] = (d[3] + d[4]) - 4.0f * (d[1] + d[2]);
    o[2] = 4.0f * (d[1] - d[2]) + (d[4] - d[3]);
    o[3] = 2.0f * (d[3] - d[1]) + (d[4] - d[2]);
    o[4] = 2.0f * (d[1] - d[3]) + (d[4] - d[2]);
    o[5] = (4.0f * d[1] - 5.0f * d[3]) + d[5];
}

// one line of A^T m
__device__ __forceinline__ void at6(const float4 (&m)[6], float4 (&o)[4])
{
    const float4 s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
    o[0] = (m[0] + s12) + s34;
    o[1] = d12 + 2.0f * d34;
    o[2] = s12 + 4.0f * s34;
    o[3] = (d12 + 8.0f * d34) + m[5];
}

struct WinoInArgs {
    WinoLevels lv;
    const float *x[IA_MAX_LEVELS];        // per level (B, H, W, Ctot) channels-last
    float *V;                             // (groups * 36, T, Cg)
    // optional pre-activation of the input: relu(x * scale[c] + shift[c]) -- the folded
    // BatchNorm + ReLU of the 1x1 convolution in front, applied on load instead of in a pass
    // of its own; padding stays zero
    const float *pre_scale, *pre_shift;
    int32_t Ctot, Cg, T, pre_relu, tpw;
};

// lane -> (tile, channel quad).  Layers with fewer than 256 channels put several tiles into one
// wavefront (64 channels: 4 tiles x 16 quads, 48 channels: 5 x 12) instead of leaving lanes idle:
// the 64- and 128-channel bottleneck layers ran at 2.5-3.8 TB/s with 16 / 32 live lanes, the
// 48-column reg|iou output transform at 0.7 TB/s with 12.
struct LaneMap { int t, c; bool on; };
// PACKED = false: one tile per wavefront -- the tile, its level and every table entry are
// wavefront-uniform (scalar registers, scalar loads)
template <bool PACKED>
__device__ __forceinline__ LaneMap lane_map(int Ctot, int T, int tpw)
{
    LaneMap m;
    const int lane = threadIdx.x;
    if (PACKED) {
        const int q = Ctot >> 2;                       // quads per tile, <= 32 here
        const int sub = lane / q;
        const int tw = xcd_tile(blockIdx.x, (T + tpw - 1) / tpw) * tpw + sub;
        m.t = tw; m.c = (lane - sub * q) * 4;
        m.on = (sub < tpw) && (tw < T);
    } else {
        m.t = __builtin_amdgcn_readfirstlane(xcd_tile(blockIdx.x, T));
        m.c = (blockIdx.y * 64 + lane) * 4;
        m.on = (m.c < Ctot) && (m.t < T);
    }
    return m;
}
static int tiles_per_wave(int channels)
{
    const int q = channels / 4;
    return (q < 64) ? (64 / q) : 1;
}

template <bool PACKED>
__global__ void __launch_bounds__(64) k_wino_in(WinoInArgs a)
{
    const LaneMap lm = lane_map<PACKED>(a.Ctot, a.T, a.tpw);
    if (!lm.on) return;
    const int t = lm.t, c = lm.c;
    int H, W;
    const TileRef r = locate_tile(a.lv, t, &H, &W);
    const float *x = level_ptr<!PACKED>(a.x, r.l) + (size_t)r.b * H * W * a.Ctot + c;
    const bool pre = a.pre_shift != nullptr;
    float4 ps = f4(1.0f), pb = f4(0.0f);
    if (pre) {
        if (a.pre_scale) ps = *reinterpret_cast<const float4 *>(a.pre_scale + c);
        pb = *reinterpret_cast<const float4 *>(a.pre_shift + c);
    }
    // All 36 loads are issued before anything consumes them.  (With the pre-activation's
    // `if (pre)` inside the load loop the compiler emitted load, branch, s_waitcnt vmcnt(0) 36
    // times over: ONE kilobyte in flight per wavefront at 3 wavefronts per SIMD.)
    float4 d[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int y = r.y0 - 1 + i;
        const int yc = (y >= 0 && y < H) ? y : 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int xx = r.x0 - 1 + j;
            const int xc = (xx >= 0 && xx < W) ? xx : 0;
            // unconditional (clamped address); padding is selected afterwards
            d[i][j] = *reinterpret_cast<const float4 *>(x + ((size_t)yc * W + xc) * a.Ctot);
        }
    }
    if (pre) {
        const bool relu = a.pre_relu != 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                float4 v = d[i][j];
                v = make_float4(v.x * ps.x + pb.x, v.y * ps.y + pb.y, v.z * ps.z + pb.z, v.w * ps.w + pb.w);
                const float4 z = make_float4(v.x > 0.f ? v.x : 0.f, v.y > 0.f ? v.y : 0.f,
                                             v.z > 0.f ? v.z : 0.f, v.w > 0.f ? v.w : 0.f);
                d[i][j] = relu ? z : v;
            }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int y = r.y0 - 1 + i;
        const bool yin = (y >= 0) && (y < H);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int xx = r.x0 - 1 + j;
            const bool in = yin && (xx >= 0) && (xx < W);
            d[i][j] = in ? d[i][j] : f4(0.0f);
        }
    }
    float4 tmp[6][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {                       // columns: tmp = B^T d
        float4 col[6], o[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) col[i] = d[i][j];
        bt6(col, o);
#pragma unroll
        for (int i = 0; i < 6; ++i) tmp[i][j] = o[i];
    }
    const int g = c / a.Cg, cc = c - g * a.Cg;
    float *v = a.V + ((size_t)g * 36 * a.T + t) * a.Cg + cc;
    const size_t kstride = (size_t)a.T * a.Cg;
#pragma unroll
    for (int i = 0; i < 6; ++i) {                       // rows: V = tmp B
        float4 o[6];
        bt6(tmp[i], o);
#pragma unroll
        for (int j = 0; j < 6; ++j)
            *reinterpret_cast<float4 *>(v + (size_t)(i * 6 + j) * kstride) = o[j];
    }
}

// ---- Input transform and the 36 Winograd-domain products in ONE launch (ResNet stage 1, the
// bottlenecks' 3x3 / 64 -> 64 convolutions): M[k] = V[k] . U[k] without V's trip through HBM (309 MB
// written by k_wino_in and read straight back by k_conv1x1_stream<64, 64> at batch 8 of 200 x 336).
// A workgroup of C / 16 wavefronts owns 16 consecutive tiles.
//   transform: the body of k_wino_in<true>, expression by expression (lane = (tile, channel quad),
//     all 36 clamped loads first, pre-activation, padding select, bt6 on columns, then bt6 row by
//     row); the 6 planes of a row go to LDS as [plane][tile 0..15][C] instead of to V;
//   products: the loop of k_conv1x1_stream<C, C> in its MFMA order: wavefront nb owns output
//     channels 16 nb .. + 15, lane (p, q) feeds its tile's channels 16 j + 4 q + c (j outer, c
//     inner) into v_mfma_f32_16x16x4_f32 against the weight fragment U[16 j + 4 q + c][16 nb + p],
//     the accumulator starts at +0 and is stored as one float4 into M[tile p][16 nb + 4 q .. + 3].
// So every element of M has the bits of the two launches.  What stays resident is the
// column-transformed tile (tmp, dying row by row) and two LDS buffers of 6 planes: row i + 1 is
// written while row i is multiplied, one barrier per row.
// U comes from global memory (L1 / L2: all workgroups read the same 36 x C x C floats) in
// FRAGMENT ORDER, packed once on the host side: [plane][nb][j][lane 16 q + p][c], so that a lane
// reads the four weights of a j step as one float4 and a wavefront 1 KiB contiguous.
// LDS image: the 16-byte slot s of tile p's row sits at slot s ^ p.  The product phase reads slot
// 4 j + q of row p; unswizzled, the 16 lanes that ds_read_b128 serves in one cycle (two lane
// quads of one q and eight lanes of another) would all hit the four banks of slot 4 j + q: 8-way.
// With the XOR every such group covers 16 different slots, and the transform's 8-lane write
// groups (one tile, 8 consecutive quads) stay on 8 different slots modulo 8.
struct WinoInGemmArgs {
    WinoLevels lv;
    const float *x[IA_MAX_LEVELS];        // per level (B, H, W, C) channels-last
    const float *U;                       // (36, C / 16, C / 16, 64, 4): fragment order
    float *M;                             // (36, T, C)
    const float *pre_scale, *pre_shift;   // as WinoInArgs
    int32_t T, pre_relu, ngroups;
};

// ---- The whole 64 -> 64 convolution in ONE launch (k_wino_conv, OUT = true below): the
// accumulator layout of the product phase IS the lane layout of k_wino_out<true> -- after plane k
// lane (p, q) of wavefront nb holds M[k][tile p][16 nb + 4 q .. + 3], the (tile, channel quad) a
// lane of the output transform owns -- so the 36 planes of a lane's tile never leave its
// registers: no M (309 MB written and read straight back at batch 8 of 200 x 336), no shuffle, no
// LDS.  The expressions are those of k_wino_out in its order (at6 down the six columns, at6 along
// the four rows, + bias, ReLU select), so y has the bits of the two launches.  The column
// transform is evaluated as its operands arrive: at6 needs rows 1, 2 of a column for s12 / d12 and
// rows 3, 4 for s34 / d34, so a column holds at most four values (st[0..3][j]) instead of six
// accumulators, the same operations in the same association: 96 registers, growing while tmp dies
// row by row, against 144 for all 36 accumulators.
struct WinoConvArgs {
    WinoInGemmArgs g;                     // g.M is not used
    const float *bias;                    // (C) or NULL
    float *y[IA_MAX_LEVELS];              // per level (B, H, W, C) channels-last
    int32_t relu;
};

template <int C, bool OUT>
__device__ __forceinline__ void wino_in_gemm_body(const WinoInGemmArgs &a, const WinoConvArgs *e)
{
    static_assert(C == 64, "lane maps and the LDS swizzle are worked out for 16 quads per tile");
    constexpr int Q = C / 4, TPW = 64 / Q, NB = C / 16, J = C / 16;
    constexpr int kPlane = 16 * C;                     // floats of one plane of the 16 tiles
    __shared__ __attribute__((aligned(16))) float s_v[2 * 6 * kPlane];
    const int grp = xcd_tile(blockIdx.x, a.ngroups);
    if (grp >= a.ngroups) return;                      // the grid is rounded up to the 8 XCDs
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // ---- transform phase: this lane's tile and channel quad
    const int sub = lane / Q, quad = lane - sub * Q, tg = wave * TPW + sub, c = 4 * quad;
    const int t0 = grp * 16 + tg;
    const int t = t0 < a.T ? t0 : a.T - 1;             // past the end: a valid tile, its products are not stored
    int H, W;
    const TileRef r = locate_tile(a.lv, t, &H, &W);
    const float *x = level_ptr<false>(a.x, r.l) + (size_t)r.b * H * W * C + c;
    const bool pre = a.pre_shift != nullptr;
    float4 ps = f4(1.0f), pb = f4(0.0f);
    if (pre) {
        if (a.pre_scale) ps = *reinterpret_cast<const float4 *>(a.pre_scale + c);
        pb = *reinterpret_cast<const float4 *>(a.pre_shift + c);
    }
    float4 d[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int y = r.y0 - 1 + i;
        const int yc = (y >= 0 && y < H) ? y : 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int xx = r.x0 - 1 + j;
            const int xc = (xx >= 0 && xx < W) ? xx : 0;
            d[i][j] = *reinterpret_cast<const float4 *>(x + ((size_t)yc * W + xc) * C);
        }
    }
    if (pre) {
        const bool relu = a.pre_relu != 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                float4 v = d[i][j];
                v = make_float4(v.x * ps.x + pb.x, v.y * ps.y + pb.y, v.z * ps.z + pb.z, v.w * ps.w + pb.w);
                const float4 z = make_float4(v.x > 0.f ? v.x : 0.f, v.y > 0.f ? v.y : 0.f,
                                             v.z > 0.f ? v.z : 0.f, v.w > 0.f ? v.w : 0.f);
                d[i][j] = relu ? z : v;
            }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int y = r.y0 - 1 + i;
        const bool yin = (y >= 0) && (y < H);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int xx = r.x0 - 1 + j;
            const bool in = yin && (xx >= 0) && (xx < W);
            d[i][j] = in ? d[i][j] : f4(0.0f);
        }
    }
    float4 tmp[6][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {                       // columns: tmp = B^T d
        float4 col[6], o[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) col[i] = d[i][j];
        bt6(col, o);
#pragma unroll
        for (int i = 0; i < 6; ++i) tmp[i][j] = o[i];
    }
    float *const sw = s_v + tg * C + 4 * (quad ^ tg);   // this lane's slot of a plane

    // ---- product phase: this lane's tile (B operand / output row) and k group
    const int p = lane & 15, q = lane >> 4;
    const int tp = grp * 16 + p;
    const bool live = tp < a.T;
    const float *const sr = s_v + p * C;
    int xo[J];                                         // float offset of slot 4 j + q in row p
#pragma unroll
    for (int j = 0; j < J; ++j) xo[j] = 4 * ((4 * j + q) ^ p);
    const float *const up = a.U + ((size_t)wave * J * 64 + lane) * 4;
    float *const mp = OUT ? nullptr : a.M + ((size_t)(live ? tp : 0) * C + 16 * wave + 4 * q);
    const size_t kstride = (size_t)a.T * C;
    // the bias is the oldest load of the store phase, for the reason given in k_wino_out
    float4 bz = f4(0.0f);
    if (OUT) {
        if (e->bias) bz = *reinterpret_cast<const float4 *>(e->bias + 16 * wave + 4 * q);
    }
    // the ReLU flag waits in a VECTOR register: as a scalar it was the one SGPR spilled over the loop
    int relu_flag = OUT ? e->relu : 0;
    if (OUT) asm volatile("" : "+v"(relu_flag));
    float4 st[4][6];                                   // OUT: the column transform s = A^T m, as it forms

    // Planes go through the MFMA pipe in pairs, their two accumulator chains interleaved (40 cycles
    // of dependent latency against 32 of issue); the weights of the next pair are requested before
    // this pair's MFMAs, also across the barrier.
    constexpr int PG = 2;
    f32x4_t wn[PG][J];
#pragma unroll
    for (int g = 0; g < PG; ++g)
#pragma unroll
        for (int j = 0; j < J; ++j) wn[g][j] = *reinterpret_cast<const f32x4_t *>(up + g * (C * C) + j * 256);

    {                                                   // row 0 of V = tmp B -> buffer 0
        float4 o[6];
        bt6(tmp[0], o);
#pragma unroll
        for (int j = 0; j < 6; ++j) *reinterpret_cast<float4 *>(sw + j * kPlane) = o[j];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        if (i + 1 < 6) {                                // row i + 1 -> the other buffer
            float4 o[6];
            bt6(tmp[i + 1], o);
            float *const s = sw + ((i + 1) & 1) * 6 * kPlane;
#pragma unroll
            for (int j = 0; j < 6; ++j) *reinterpret_cast<float4 *>(s + j * kPlane) = o[j];
        }
#pragma unroll
        for (int j6 = 0; j6 < 6; j6 += PG) {
            const int k = i * 6 + j6;
            const float *const s = sr + ((i & 1) * 6 + j6) * kPlane;
            f32x4_t xv[PG][J], wv[PG][J], acc[PG];
#pragma unroll
            for (int g = 0; g < PG; ++g) {
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    xv[g][j] = *reinterpret_cast<const f32x4_t *>(s + g * kPlane + xo[j]);
                    wv[g][j] = wn[g][j];
                }
                acc[g] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
            }
            if (k + PG < 36) {
                const float *const un = up + (size_t)(k + PG) * (C * C);
#pragma unroll
                for (int g = 0; g < PG; ++g)
#pragma unroll
                    for (int j = 0; j < J; ++j) wn[g][j] = *reinterpret_cast<const f32x4_t *>(un + g * (C * C) + j * 256);
            }
            // (without it the scheduler sinks these loads to the end of the pair's MFMAs, right in
            // front of the wait of the next pair: one L2 round trip exposed per pair)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < J; ++j)
#pragma unroll
                for (int cc = 0; cc < 4; ++cc)
#pragma unroll
                    for (int g = 0; g < PG; ++g)
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[g][j][cc], xv[g][j][cc], acc[g], 0, 0, 0);
            if (!OUT) {
                if (live) {
#pragma unroll
                    for (int g = 0; g < PG; ++g) *reinterpret_cast<f32x4_t *>(mp + (size_t)(k + g) * kstride) = acc[g];
                }
            } else {
                // at6 down column j = j6 + g, row i of it: o[0] = (m0 + s12) + s34, o[1] = d12 + 2 d34,
                // o[2] = s12 + 4 s34, o[3] = (d12 + 8 d34) + m5
#pragma unroll
                for (int g = 0; g < PG; ++g) {
                    const int j = j6 + g;
                    const float4 m = make_float4(acc[g].x, acc[g].y, acc[g].z, acc[g].w);
                    if (i == 0) st[0][j] = m;
                    if (i == 1) st[1][j] = m;
                    if (i == 2) {
                        const float4 s12 = st[1][j] + m, d12 = st[1][j] - m;
                        st[0][j] = st[0][j] + s12; st[1][j] = d12; st[2][j] = s12;
                    }
                    if (i == 3) st[3][j] = m;
                    if (i == 4) {
                        const float4 s34 = st[3][j] + m, d34 = st[3][j] - m;
                        const float4 o0 = st[0][j] + s34, o1 = st[1][j] + 2.0f * d34, o2 = st[2][j] + 4.0f * s34,
                                     o3 = st[1][j] + 8.0f * d34;
                        st[0][j] = o0; st[1][j] = o1; st[2][j] = o2; st[3][j] = o3;
                    }
                    if (i == 5) st[3][j] = st[3][j] + m;
                }
            }
        }
        if (i + 1 < 6) __syncthreads();
    }
    if (OUT) {
        // rows: Y = s A, + bias, ReLU, one float4 per pixel straight from the accumulator layout
        // (16 tiles x 64 B per wavefront instruction).  A row past T (the last group) stores nothing.
        // (L and T pass through `opaque`: the compiler otherwise shares the `i < L` masks, T - 1 and the
        // `live` mask with the code in front of the loop and keeps them through it, 18 SGPRs spilled to
        // VGPR lanes)
        WinoLevels lv = a.lv;
        lv.L = opaque(a.lv.L);
        const int T = opaque(a.T);
        const bool on = tp < T;
        const int tq = on ? tp : T - 1;
        int H, W;
        const TileRef r = locate_tile(lv, tq, &H, &W);
        float *const y0 = level_ptr<false>(e->y, r.l) + 16 * wave + 4 * q;
        const bool relu = relu_flag != 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float4 o[4];
            at6(st[i], o);
            const int y = r.y0 + i;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int xx = r.x0 + j;
                if (!on || y >= H || xx >= W) continue;
                float4 v = o[j] + bz;
                if (relu) v = make_float4(v.x > 0.f ? v.x : 0.f, v.y > 0.f ? v.y : 0.f,
                                          v.z > 0.f ? v.z : 0.f, v.w > 0.f ? v.w : 0.f);
                const size_t pix = ((size_t)r.b * H + y) * W + xx;
                *reinterpret_cast<float4 *>(y0 + pix * C) = v;
            }
        }
    }
}

template <int C>
__global__ void __launch_bounds__(4 * C) k_wino_in_gemm(WinoInGemmArgs a)
{
    wino_in_gemm_body<C, false>(a, nullptr);
}

template <int C>
__global__ void __launch_bounds__(4 * C) k_wino_conv(WinoConvArgs a)
{
    wino_in_gemm_body<C, true>(a.g, &a);
}

// one line of A dy: the adjoint of at6 (4 values -> 6), A = (A^T)^T
__device__ __forceinline__ void a6(const float4 (&y)[4], float4 (&o)[6])
{
    const float4 s02 = y[0] + y[2], s13 = y[1] + y[3];
    const float4 t02 = y[0] + 4.0f * y[2], t13 = 2.0f * y[1] + 8.0f * y[3];
    o[0] = y[0];
    o[1] = s02 + s13;
    o[2] = s02 - s13;
    o[3] = t02 + t13;
    o[4] = t02 - t13;
    o[5] = y[3];
}

// Gradient of the output transform (training, weight gradient in the Winograd domain):
// dM = A dY A^T per tile, dY = the 4x4 output pixels of the tile (zero outside the feature map,
// where the forward output transform wrote nothing), scattered as 36 matrices like V.
template <bool PACKED>
__global__ void __launch_bounds__(64) k_wino_dy(WinoInArgs a)
{
    const LaneMap lm = lane_map<PACKED>(a.Ctot, a.T, a.tpw);
    if (!lm.on) return;
    const int t = lm.t, c = lm.c;
    int H, W;
    const TileRef r = locate_tile(a.lv, t, &H, &W);
    const float *x = level_ptr<!PACKED>(a.x, r.l) + (size_t)r.b * H * W * a.Ctot + c;
    float4 d[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = r.y0 + i;
        const int yc = (y < H) ? y : (H - 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xx = r.x0 + j;
            const int xc = (xx < W) ? xx : (W - 1);
            const float4 v = *reinterpret_cast<const float4 *>(x + ((size_t)yc * W + xc) * a.Ctot);
            d[i][j] = (y < H && xx < W) ? v : f4(0.0f);
        }
    }
    float4 tmp[6][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {                       // columns: tmp = A d
        float4 col[4], o[6];
#pragma unroll
        for (int i = 0; i < 4; ++i) col[i] = d[i][j];
        a6(col, o);
#pragma unroll
        for (int i = 0; i < 6; ++i) tmp[i][j] = o[i];
    }
    const int g = c / a.Cg, cc = c - g * a.Cg;
    float *v = a.V + ((size_t)g * 36 * a.T + t) * a.Cg + cc;
    const size_t kstride = (size_t)a.T * a.Cg;
#pragma unroll
    for (int i = 0; i < 6; ++i) {                       // rows: dM = tmp A^T
        float4 o[6];
        a6(tmp[i], o);
#pragma unroll
        for (int j = 0; j < 6; ++j)
            *reinterpret_cast<float4 *>(v + (size_t)(i * 6 + j) * kstride) = o[j];
    }
}

struct WinoOutArgs {
    WinoLevels lv;
    const float *M;                       // (groups * 36, T, Cg)
    const float *bias;                    // (groups * Cg) or NULL
    WinoSeg seg[kMaxSeg];
    int32_t nseg, Ctot, Cg, T, relu, tpw;
};

template <bool PACKED>
__global__ void __launch_bounds__(64) k_wino_out(WinoOutArgs a)
{
    const LaneMap lm = lane_map<PACKED>(a.Ctot, a.T, a.tpw);
    if (!lm.on) return;
    const int t = lm.t, c = lm.c;
    int H, W;
    const TileRef r = locate_tile(a.lv, t, &H, &W);
    const int g = c / a.Cg, cc = c - g * a.Cg;
    const float *m = a.M + ((size_t)g * 36 * a.T + t) * a.Cg + cc;
    const size_t kstride = (size_t)a.T * a.Cg;
    // the bias is the OLDEST load: were it issued after the 36 loads of M, its s_waitcnt vmcnt(0)
    // would sit in the store phase, where (behind the per-pixel branches) it is repeated in front
    // of every pixel and waits for all the stores issued so far
    float4 bz = f4(0.0f);
    if (a.bias) bz = *reinterpret_cast<const float4 *>(a.bias + c);
    float4 s[4][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {                       // columns: s = A^T m
        float4 col[6], o[4];
#pragma unroll
        for (int i = 0; i < 6; ++i) col[i] = load_nt(m + (size_t)(i * 6 + j) * kstride);
        at6(col, o);
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i][j] = o[i];
    }
    // Destination of this lane's four channels: the last segment that starts at or before c
    // (segments ascend).  Its parameters are selected ONCE into registers from scalar loads;
    // `a.seg[si]` with a per-lane si was a vector load from the kernarg segment that the compiler
    // re-issued in front of every one of the 16 stores (load, s_waitcnt vmcnt(0), store).
    int sc0 = opaque(a.seg[0].c0), sn = opaque(a.seg[0].n), sC = opaque(a.seg[0].Cdst), soff = opaque(a.seg[0].coff);
    float *sdst = level_ptr<!PACKED>(a.seg[0].dst, r.l);
#pragma unroll
    for (int k = 1; k < kMaxSeg; ++k) {
        const int kc0 = opaque(a.seg[k].c0), kn = opaque(a.seg[k].n), kC = opaque(a.seg[k].Cdst),
                  koff = opaque(a.seg[k].coff);
        float *kdst = level_ptr<!PACKED>(a.seg[k].dst, r.l);
        const bool m = (k < a.nseg) && (c >= kc0);
        sc0 = m ? kc0 : sc0; sn = m ? kn : sn; sC = m ? kC : sC; soff = m ? koff : soff;
        sdst = m ? kdst : sdst;
    }
    const bool whole = (c >= sc0) && (c + 4 <= sc0 + sn) && (((soff + c - sc0) & 3) == 0) && ((sC & 3) == 0);
    float *const dst0 = sdst + soff + (c - sc0);
    // a lane that straddles segments / padding, or whose destination is not 16-byte aligned
    // (the 9-channel IoU output): destination of each of its four channels, resolved once
    float *qdst[4] = {nullptr, nullptr, nullptr, nullptr};
    int qC[4] = {0, 0, 0, 0}, qoff[4] = {0, 0, 0, 0};
    if (!whole) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ch = c + q;
            for (int k = 0; k < a.nseg; ++k) {
                const WinoSeg &z = a.seg[k];
                if (ch >= z.c0 && ch < z.c0 + z.n) {
                    qdst[q] = level_ptr<!PACKED>(z.dst, r.l); qC[q] = z.Cdst; qoff[q] = z.coff + (ch - z.c0);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {                       // rows: Y = s A
        float4 o[4];
        at6(s[i], o);
        const int y = r.y0 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xx = r.x0 + j;
            if (y >= H || xx >= W) continue;
            float4 v = o[j] + bz;
            if (a.relu) v = make_float4(v.x > 0.f ? v.x : 0.f, v.y > 0.f ? v.y : 0.f,
                                        v.z > 0.f ? v.z : 0.f, v.w > 0.f ? v.w : 0.f);
            const size_t pix = ((size_t)r.b * H + y) * W + xx;
            if (whole) {
                *reinterpret_cast<float4 *>(dst0 + pix * sC) = v;
            } else {
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (qdst[q]) qdst[q][pix * qC[q] + qoff[q]] = e[q];
            }
        }
    }
}

// ---- Output transform of one tower layer and input transform of the next in ONE launch: the
// bias + ReLU activation between two 3x3 convolutions of the same geometry never goes to HBM.
// k_wino_out writes 16 pixels per tile and channel and k_wino_in reads them back as overlapping
// 6x6 patches (36 issued loads per tile): 36 + 36 load and 16 + 36 store units per tile for the
// pair.  Here a workgroup owns a block of 8 x 8 tiles of one (level, image) and a slice of 32
// channels (128-byte pieces of M and V):
//   phase 1  M of the block and of a one-tile ring around it (clipped to the tile grid) ->
//            Y = A^T M A + bias, ReLU -> the 34 x 34 pixel window of the activation in LDS; pixels
//            outside the feature map are the ZERO PADDING of the input transform, not what
//            A^T M A gives there (partial tiles);
//   phase 2  every tile of the block takes its 6x6 patch from LDS -> V = B^T d B.
// 36 * (10/8)^2 = 56 load and 36 store units per tile.  The arithmetic is that of k_wino_out
// followed by k_wino_in, expression by expression: V has the same bits.
constexpr int kMidB = 8;                              // tiles per side of a block
constexpr int kMidR = kMidB + 2;                      // ... with the ring
constexpr int kMidP = 4 * kMidB + 2;                  // pixels per side of the activation window
constexpr int kMidCh = 32;                            // channels per workgroup
constexpr int kMidQ = kMidCh / 4;                     // lanes (channel quads) per tile
constexpr int kMidThreads = kMidB * kMidB * kMidQ;    // 512: one lane per (tile, quad) of phase 2
constexpr int kMidPasses = (kMidR * kMidR * kMidQ + kMidThreads - 1) / kMidThreads;

struct WinoMidArgs {
    WinoLevels lv;
    const float *M;                       // (groups_m * 36, T, Cm)
    const float *bias;                    // (Ctot) or NULL
    float *V;                             // (groups_v * 36, T, Cv)
    int32_t bx[IA_MAX_LEVELS], bpi[IA_MAX_LEVELS];        // blocks per row of blocks / per image
    int32_t blk_off[IA_MAX_LEVELS + 1];                   // prefix of B * blocks_per_image
    int32_t nblk, Ctot, Cm, Cv, T, relu;
};

__global__ void __launch_bounds__(kMidThreads) k_wino_mid(WinoMidArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_y[kMidP * kMidP * kMidCh];     // 144.5 KiB
    const int tid = threadIdx.x;
    const int blk = __builtin_amdgcn_readfirstlane(xcd_tile(blockIdx.x, a.nblk));
    if (blk >= a.nblk) return;                            // the whole workgroup
    // block -> level, image, block row / column (workgroup-uniform: scalar compares and selects)
    int l = 0;
#pragma unroll
    for (int i = 1; i < IA_MAX_LEVELS; ++i) l += (i < a.lv.L && blk >= a.blk_off[i]) ? 1 : 0;
    int off = a.blk_off[0], bpi = a.bpi[0], bx = a.bx[0], tx = a.lv.tx[0], tpi = a.lv.tpi[0],
        toff = a.lv.tile_off[0], H = a.lv.H[0], W = a.lv.W[0];
#pragma unroll
    for (int i = 1; i < IA_MAX_LEVELS; ++i) {
        const bool m = l == i;
        off = m ? a.blk_off[i] : off; bpi = m ? a.bpi[i] : bpi; bx = m ? a.bx[i] : bx;
        tx = m ? a.lv.tx[i] : tx; tpi = m ? a.lv.tpi[i] : tpi; toff = m ? a.lv.tile_off[i] : toff;
        H = m ? a.lv.H[i] : H; W = m ? a.lv.W[i] : W;
    }
    const int qb = blk - off;
    const int b = qb / bpi, rb = qb - b * bpi;
    const int byi = rb / bx, bxi = rb - byi * bx;
    const int ty_n = tpi / tx;
    const int tbase = toff + b * tpi;                     // first tile of this image
    const int cq = (tid & (kMidQ - 1)) * 4;
    const int c = blockIdx.y * kMidCh + cq;
    // the channel -> group mapping of M (the layer behind) and of V (the layer in front) may differ:
    // the first tower layer is one GEMM with 2F columns, the second 2 x 36 GEMMs of F
    const int gm = c / a.Cm, gv = c / a.Cv;
    const size_t mstride = (size_t)a.T * a.Cm, vstride = (size_t)a.T * a.Cv;
    float4 bz = f4(0.0f);
    if (a.bias) bz = *reinterpret_cast<const float4 *>(a.bias + c);

    // ---- phase 1: lane = (tile of the ringed block, channel quad)
#pragma unroll 1
    for (int p = 0; p < kMidPasses; ++p) {
        const int ti = tid / kMidQ + p * (kMidThreads / kMidQ);
        if (ti >= kMidR * kMidR) break;
        const int ry = ti / kMidR, rx = ti - ry * kMidR;
        const int tyi = kMidB * byi - 1 + ry, txi = kMidB * bxi - 1 + rx;
        const int ly0 = 4 * ry - 3, lx0 = 4 * rx - 3;     // window coordinates of the tile's first pixel
        float *sy = s_y + cq;
        if (tyi >= 0 && tyi < ty_n && txi >= 0 && txi < tx) {
            const float *m = a.M + (size_t)gm * 36 * mstride + (size_t)(tbase + tyi * tx + txi) * a.Cm + (c - gm * a.Cm);
            float4 s[4][6];
#pragma unroll
            for (int j = 0; j < 6; ++j) {                 // columns: s = A^T m
                float4 col[6], o[4];
#pragma unroll
                for (int i = 0; i < 6; ++i) col[i] = *reinterpret_cast<const float4 *>(m + (size_t)(i * 6 + j) * mstride);
                at6(col, o);
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i][j] = o[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {                 // rows: Y = s A
                float4 o[4];
                at6(s[i], o);
                const int y = 4 * tyi + i, ly = ly0 + i;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int xx = 4 * txi + j, lx = lx0 + j;
                    float4 v = o[j] + bz;
                    if (a.relu) v = make_float4(v.x > 0.f ? v.x : 0.f, v.y > 0.f ? v.y : 0.f,
                                                v.z > 0.f ? v.z : 0.f, v.w > 0.f ? v.w : 0.f);
                    v = (y < H && xx < W) ? v : f4(0.0f); // a partial tile: padding of the next layer
                    if (ly >= 0 && ly < kMidP && lx >= 0 && lx < kMidP)
                        *reinterpret_cast<float4 *>(sy + (ly * kMidP + lx) * kMidCh) = v;
                }
            }
        } else {                                          // no such tile: padding
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ly = ly0 + i, lx = lx0 + j;
                    if (ly >= 0 && ly < kMidP && lx >= 0 && lx < kMidP)
                        *reinterpret_cast<float4 *>(sy + (ly * kMidP + lx) * kMidCh) = f4(0.0f);
                }
        }
    }
    __syncthreads();

    // ---- phase 2: lane = (tile of the block, channel quad)
    const int tl = tid / kMidQ, tyl = tl / kMidB, txl = tl - tyl * kMidB;
    const int tyi = kMidB * byi + tyl, txi = kMidB * bxi + txl;
    if (tyi >= ty_n || txi >= tx) return;                 // a partial block: no tile here
    const float *sp = s_y + ((4 * tyl) * kMidP + 4 * txl) * kMidCh + cq;
    float4 tmp[6][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {                         // columns: tmp = B^T d
        float4 col[6], o[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) col[i] = *reinterpret_cast<const float4 *>(sp + (i * kMidP + j) * kMidCh);
        bt6(col, o);
#pragma unroll
        for (int i = 0; i < 6; ++i) tmp[i][j] = o[i];
        // (left alone the scheduler hoists all 36 LDS reads next to tmp: 288 registers)
        __builtin_amdgcn_sched_barrier(0);
    }
    float *v = a.V + (size_t)gv * 36 * vstride + (size_t)(tbase + tyi * tx + txi) * a.Cv + (c - gv * a.Cv);
#pragma unroll
    for (int i = 0; i < 6; ++i) {                         // rows: V = tmp B
        float4 o[6];
        bt6(tmp[i], o);
#pragma unroll
        for (int j = 0; j < 6; ++j)
            *reinterpret_cast<float4 *>(v + (size_t)(i * 6 + j) * vstride) = o[j];
    }
}

}  // namespace ia

extern "C" {

int ia_wino_tiles(const ia_wino_geom *g, int32_t *tiles)
{
    ia::WinoLevels w;
    int rc = ia::make_wino_levels(g, w);
    if (rc) return rc;
    if (tiles) *tiles = w.tile_off[w.L];
    return 0;
}

int ia_wino_input_transform(const ia_wino_geom *g, const float *const *x, int channels, int groups,
                            const float *pre_scale, const float *pre_shift, int pre_relu, float *V,
                            void *stream)
{
    ia::WinoInArgs a;
    int rc = ia::make_wino_levels(g, a.lv);
    if (rc) return rc;
    if (!x || !V || channels < 4 || (channels & 3) || groups < 1 || channels % groups) return IA_E_ARG;
    a.Ctot = channels; a.Cg = channels / groups; a.T = a.lv.tile_off[a.lv.L];
    if (a.Cg & 3) return IA_E_ARG;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        a.x[l] = (l < a.lv.L) ? x[l] : nullptr;
        if (l < a.lv.L && (!x[l] || ((uintptr_t)x[l] & 15u))) return IA_E_ARG;
    }
    a.V = V;
    if (pre_scale && !pre_shift) return IA_E_ARG;
    a.pre_scale = pre_scale; a.pre_shift = pre_shift; a.pre_relu = pre_relu ? 1 : 0;
    a.tpw = ia::tiles_per_wave(channels);
    const int waves = (a.T + a.tpw - 1) / a.tpw;
    dim3 grid((unsigned)((waves + 7) / 8 * 8), (unsigned)((channels / 4 + 63) / 64));
    if (a.tpw > 1) hipLaunchKernelGGL(ia::k_wino_in<true>, grid, dim3(64), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(ia::k_wino_in<false>, grid, dim3(64), 0, (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
}

int ia_wino_in_gemm(const ia_wino_geom *g, const float *const *x, int channels, const float *pre_scale,
                    const float *pre_shift, int pre_relu, const float *u_packed, float *M, void *stream)
{
    ia::WinoInGemmArgs a;
    int rc = ia::make_wino_levels(g, a.lv);
    if (rc) return rc;
    if (!x || !u_packed || !M || channels != 64) return IA_E_ARG;
    if (((uintptr_t)u_packed & 15u) || ((uintptr_t)M & 15u) || ((uintptr_t)pre_scale & 15u) ||
        ((uintptr_t)pre_shift & 15u))
        return IA_E_ARG;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        a.x[l] = (l < a.lv.L) ? x[l] : nullptr;
        if (l < a.lv.L && (!x[l] || ((uintptr_t)x[l] & 15u))) return IA_E_ARG;
    }
    if (pre_scale && !pre_shift) return IA_E_ARG;
    a.U = u_packed; a.M = M;
    a.pre_scale = pre_scale; a.pre_shift = pre_shift; a.pre_relu = pre_relu ? 1 : 0;
    a.T = a.lv.tile_off[a.lv.L];
    a.ngroups = (int32_t)(((int64_t)a.T + 15) / 16);
    dim3 grid((unsigned)((a.ngroups + 7) / 8 * 8));
    hipLaunchKernelGGL(ia::k_wino_in_gemm<64>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
}

int ia_wino_conv3x3_c64(const ia_wino_geom *g, const float *const *x, int channels, const float *pre_scale,
                        const float *pre_shift, int pre_relu, const float *u_packed, const float *bias,
                        int relu, float *const *y, void *stream)
{
    ia::WinoConvArgs a;
    int rc = ia::make_wino_levels(g, a.g.lv);
    if (rc) return rc;
    if (!x || !y || !u_packed || channels != 64) return IA_E_ARG;
    if (((uintptr_t)u_packed & 15u) || ((uintptr_t)bias & 15u) || ((uintptr_t)pre_scale & 15u) ||
        ((uintptr_t)pre_shift & 15u))
        return IA_E_ARG;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        const bool on = l < a.g.lv.L;
        a.g.x[l] = on ? x[l] : nullptr;
        a.y[l] = on ? y[l] : nullptr;
        if (on && (!x[l] || ((uintptr_t)x[l] & 15u) || !y[l] || ((uintptr_t)y[l] & 15u))) return IA_E_ARG;
    }
    if (pre_scale && !pre_shift) return IA_E_ARG;
    a.g.U = u_packed; a.g.M = nullptr;
    a.g.pre_scale = pre_scale; a.g.pre_shift = pre_shift; a.g.pre_relu = pre_relu ? 1 : 0;
    a.g.T = a.g.lv.tile_off[a.g.lv.L];
    a.g.ngroups = (int32_t)(((int64_t)a.g.T + 15) / 16);
    a.bias = bias; a.relu = relu ? 1 : 0;
    dim3 grid((unsigned)((a.g.ngroups + 7) / 8 * 8));
    hipLaunchKernelGGL(ia::k_wino_conv<64>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
}

int ia_wino_grad_output_transform(const ia_wino_geom *g, const float *const *dy, int channels,
                                   float *dM, void *stream)
{
    ia::WinoInArgs a;
    int rc = ia::make_wino_levels(g, a.lv);
    if (rc) return rc;
    if (!dy || !dM || channels < 4 || (channels & 3)) return IA_E_ARG;
    a.Ctot = channels; a.Cg = channels; a.T = a.lv.tile_off[a.lv.L];
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        a.x[l] = (l < a.lv.L) ? dy[l] : nullptr;
        if (l < a.lv.L && (!dy[l] || ((uintptr_t)dy[l] & 15u))) return IA_E_ARG;
    }
    a.V = dM;
    a.pre_scale = a.pre_shift = nullptr; a.pre_relu = 0;
    a.tpw = ia::tiles_per_wave(channels);
    const int waves = (a.T + a.tpw - 1) / a.tpw;
    dim3 grid((unsigned)((waves + 7) / 8 * 8), (unsigned)((channels / 4 + 63) / 64));
    if (a.tpw > 1) hipLaunchKernelGGL(ia::k_wino_dy<true>, grid, dim3(64), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(ia::k_wino_dy<false>, grid, dim3(64), 0, (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
}

int ia_wino_output_transform(const ia_wino_geom *g, const float *M, int channels, int groups,
                             const float *bias, int relu, int nseg, const ia_wino_seg *segs,
                             void *stream)
{
    ia::WinoOutArgs a;
    int rc = ia::make_wino_levels(g, a.lv);
    if (rc) return rc;
    if (!M || channels < 4 || (channels & 3) || groups < 1 || channels % groups || !segs ||
        nseg < 1 || nseg > ia::kMaxSeg)
        return IA_E_ARG;
    a.M = M; a.bias = bias; a.Ctot = channels; a.Cg = channels / groups;
    if (a.Cg & 3) return IA_E_ARG;
    a.T = a.lv.tile_off[a.lv.L]; a.relu = relu ? 1 : 0; a.nseg = nseg;
    memset(a.seg, 0, sizeof(a.seg));
    for (int k = 0; k < nseg; ++k) {
        const ia_wino_seg &s = segs[k];
        if (s.c0 < 0 || s.n < 1 || s.c0 + s.n > channels || s.dst_channels < s.n + s.dst_offset ||
            s.dst_offset < 0)
            return IA_E_ARG;
        if (k > 0 && s.c0 < segs[k - 1].c0 + segs[k - 1].n) return IA_E_ARG;       // ascending
        a.seg[k].c0 = s.c0; a.seg[k].n = s.n; a.seg[k].Cdst = s.dst_channels; a.seg[k].coff = s.dst_offset;
        for (int l = 0; l < a.lv.L; ++l) {
            if (!s.dst[l]) return IA_E_ARG;
            a.seg[k].dst[l] = s.dst[l];
        }
    }
    a.tpw = ia::tiles_per_wave(channels);
    const int waves = (a.T + a.tpw - 1) / a.tpw;
    dim3 grid((unsigned)((waves + 7) / 8 * 8), (unsigned)((channels / 4 + 63) / 64));
    if (a.tpw > 1) hipLaunchKernelGGL(ia::k_wino_out<true>, grid, dim3(64), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(ia::k_wino_out<false>, grid, dim3(64), 0, (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
}

int ia_wino_mid_transform(const ia_wino_geom *g, const float *M, int channels, int groups_m,
                          const float *bias, int relu, float *V, int groups_v, void *stream)
{
    ia::WinoMidArgs a;
    int rc = ia::make_wino_levels(g, a.lv);
    if (rc) return rc;
    if (!M || !V || channels < ia::kMidCh || groups_m < 1 || channels % groups_m || groups_v < 1 ||
        channels % groups_v)
        return IA_E_ARG;
    a.M = M; a.bias = bias; a.V = V; a.Ctot = channels;
    a.Cm = channels / groups_m; a.Cv = channels / groups_v;
    // a workgroup's 32 channels lie inside one group on both sides; 128-byte pieces of M and V
    if (a.Cm % ia::kMidCh || a.Cv % ia::kMidCh || ((uintptr_t)M & 15u) || ((uintptr_t)V & 15u) ||
        ((uintptr_t)bias & 15u))
        return IA_E_ARG;
    a.T = a.lv.tile_off[a.lv.L]; a.relu = relu ? 1 : 0;
    int64_t n = 0;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        const bool on = l < a.lv.L;
        const int ty = on ? a.lv.tpi[l] / a.lv.tx[l] : 0;
        a.bx[l] = on ? (a.lv.tx[l] + ia::kMidB - 1) / ia::kMidB : 0;
        a.bpi[l] = on ? ((ty + ia::kMidB - 1) / ia::kMidB) * a.bx[l] : 0;
        a.blk_off[l] = (int32_t)n;
        n += (int64_t)a.lv.B * a.bpi[l];
    }
    a.blk_off[IA_MAX_LEVELS] = (int32_t)n;
    a.nblk = (int32_t)n;
    dim3 grid((unsigned)((n + 7) / 8 * 8), (unsigned)(channels / ia::kMidCh));
    hipLaunchKernelGGL(ia::k_wino_mid, grid, dim3(ia::kMidThreads), 0, (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
}

}  // extern "C"
