// The large Winograd-domain products of the RetinaNet head, D[b] (rows, N) = V[b] (rows, K) . U[b] (K, N),
// fp32 in and out, on bf16 MFMA through an exact three-way split of every fp32 operand.
//
//  * gfx950 has no xf32, and its fp32 MFMA runs at 1/16 of the bf16 rate.  Every fp32 value splits
//    exactly into three bf16 pieces, x = h + m + l, with round-to-nearest casts: h = bf16(x),
//    m = bf16(x - h), l = bf16(x - h - m).  Both differences are exact in fp32 (|x - h| <= 2^-9 |x| on the
//    grid of x, so it has at most 16 significant bits, and x - h - m at most 8), so l takes the rest.
//  * Six of the nine product terms are kept: hh, hm, mh, hl, lh, mm.  The dropped ml, lm, ll are below
//    2^-26 of |v| |u|: under the fp32 rounding of the sum.  That is 6/16 of the fp32 MFMA cycles.
//  * Two accumulator sets: hh alone, and hm + mh + hl + lh + mm.  The main chain rounds the way an fp32
//    GEMM's does, the corrections are ~2^-8 smaller; the two are added once, in the epilogue.
//  * V is split in the kernel, once per element, on its way from global memory into LDS: no byte is
//    added to V.  U is split once when the head is built (iouaware/winograd.py split3_pack_u) and comes
//    in fragment order.
//  * A workgroup = four wavefronts as 2 x 2, each 64 rows x 64 columns (2 x 2 blocks of
//    v_mfma_f32_32x32x16_bf16, two sets: 128 accumulators); it owns 128 rows x 128 columns of one matrix.
//    K in chunks of 32: the chunk's V (128 x 32 fp32) and U (32 x 128, three pieces) are staged in
//    registers one chunk ahead and stored to LDS as fragment images (one 1-KiB image per (k-step,
//    32-block, piece): every ds_read_b128 / ds_write_b128 of a wavefront is 1 KiB contiguous).
//  * No split-K, no atomics: every run gives the same bits.  Rows beyond the matrix read its last row
//    and are not stored; columns beyond N multiply the zero columns of the packed U and are not stored.
#include "ia_internal.hpp"

namespace ia {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int kSgBM = 128;                // rows per workgroup
constexpr int kSgBN = 128;                // columns per workgroup (the packed U is padded to a multiple)
constexpr int kSgBK = 32;                 // K per chunk: two k-steps of 16
constexpr int kSgThreads = 256;
constexpr int kSgImg = 64 * 16;           // one fragment image: 64 lanes x 8 bf16
constexpr int kSgStage = 2 * 4 * 3 * kSgImg;   // [k-step 2][32-block 4][piece 3] images: 24 KiB

struct SplitGemmArgs {
    const float *v;           // (batch, rows, K)
    const uint4 *up;          // [batch][K / 16][Np / 32][piece 3][lane 64] x 8 bf16
    float *d;                 // (batch, rows, N)
    int64_t rows;
    int K, N, np32;
    int ntiles, mtiles;       // column tiles, row blocks: the grid is ntiles * mtiles * batch workgroups
};

// 8 consecutive fp32 -> their h, m, l pieces as three bf16x8 fragments
__device__ __forceinline__ void split3(const float4 &x0, const float4 &x1, bf16x8 &h, bf16x8 &m, bf16x8 &l)
{
    const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 hb = (__bf16)x[e];
        const float r = x[e] - (float)hb;
        const __bf16 mb = (__bf16)r;
        h[e] = hb;
        m[e] = mb;
        l[e] = (__bf16)(r - (float)mb);
    }
}

__global__ void __launch_bounds__(kSgThreads, 2) k_gemm_split3(SplitGemmArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_a[kSgStage];   // V pieces: [s][row block][piece][lane]
    __shared__ __attribute__((aligned(16))) unsigned char s_b[kSgStage];   // U pieces: [s][col block][piece][lane]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv >> 1, wn = wv & 1;
    // Workgroups are dealt to the eight XCDs in turn, and each XCD has its own L2.  Renumbered so that an
    // XCD runs a contiguous range of (column tile fastest, row block, matrix): the column tiles of one row
    // block then share their V rows in one L2 instead of reading them from memory once per tile.
    int nt, b;
    int64_t row0;
    {
        const int total = (int)gridDim.x, q = total >> 3, r = total & 7;
        const int xcd = (int)blockIdx.x & 7, idx = (int)blockIdx.x >> 3;
        int t = xcd < r ? xcd * (q + 1) + idx : r * (q + 1) + (xcd - r) * q + idx;
        nt = t % a.ntiles;
        t /= a.ntiles;
        row0 = (int64_t)(t % a.mtiles) * kSgBM;
        b = t / a.mtiles;
    }
    const int nchunk = a.K / kSgBK;

    // staging of V: wavefront wv loads row block wv (32 rows), lane = (row lane & 31, k-half lane >> 5):
    // exactly the slot of the A fragment image it stores (lane l of the MFMA reads row l & 31,
    // k = 8 (l >> 5) .. + 7), both k-steps of the chunk
    int64_t r = row0 + wv * 32 + (lane & 31);
    if (r >= a.rows) r = a.rows - 1;
    const float *vp = a.v + ((int64_t)b * a.rows + r) * a.K + 8 * (lane >> 5);
    // staging of U: the chunk's two k-steps are two contiguous runs of 4 x 3 images (12 KiB) in the
    // packed U; 16-byte piece q = tid + 256 i goes to LDS byte 16 q
    const uint4 *up = a.up + ((int64_t)b * (a.K / 16) * a.np32 + nt * 4) * (3 * 64);
    const int64_t ks_stride = (int64_t)a.np32 * 3 * 64;          // uint4 per k-step in the packed U

    float4 x0, x1, x2, x3;
    uint4 u0, u1, u2, u3, u4, u5;
#define SG_LOAD(c)                                                                                  \
    {                                                                                               \
        const float *src = vp + (c) * kSgBK;                                                        \
        x0 = *reinterpret_cast<const float4 *>(src);                                                \
        x1 = *reinterpret_cast<const float4 *>(src + 4);                                            \
        x2 = *reinterpret_cast<const float4 *>(src + 16);                                           \
        x3 = *reinterpret_cast<const float4 *>(src + 20);                                           \
        const uint4 *us = up + (int64_t)(2 * (c)) * ks_stride;                                      \
        u0 = us[tid];                                                                               \
        u1 = us[tid + 256];                                                                         \
        u2 = us[tid + 512];                                                                         \
        u3 = us[ks_stride + tid];                                                                   \
        u4 = us[ks_stride + tid + 256];                                                             \
        u5 = us[ks_stride + tid + 512];                                                             \
    }
#define SG_STORE()                                                                                  \
    {                                                                                               \
        bf16x8 h, m, l;                                                                             \
        split3(x0, x1, h, m, l);                                                                    \
        unsigned char *da = s_a + ((0 * 4 + wv) * 3 * 64 + lane) * 16;                              \
        *reinterpret_cast<bf16x8 *>(da) = h;                                                        \
        *reinterpret_cast<bf16x8 *>(da + kSgImg) = m;                                               \
        *reinterpret_cast<bf16x8 *>(da + 2 * kSgImg) = l;                                           \
        split3(x2, x3, h, m, l);                                                                    \
        da += 4 * 3 * kSgImg;                                                                       \
        *reinterpret_cast<bf16x8 *>(da) = h;                                                        \
        *reinterpret_cast<bf16x8 *>(da + kSgImg) = m;                                               \
        *reinterpret_cast<bf16x8 *>(da + 2 * kSgImg) = l;                                           \
        uint4 *db = reinterpret_cast<uint4 *>(s_b);                                                 \
        db[tid] = u0;                                                                               \
        db[tid + 256] = u1;                                                                         \
        db[tid + 512] = u2;                                                                         \
        db[tid + 768] = u3;                                                                         \
        db[tid + 1024] = u4;                                                                        \
        db[tid + 1280] = u5;                                                                        \
    }

    f32x16 hi[2][2], lo[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                hi[i][j][e] = 0.0f;
                lo[i][j][e] = 0.0f;
            }

    SG_LOAD(0)
    for (int c = 0; c < nchunk; ++c) {
        if (c > 0) __syncthreads();          // every wavefront is done with the previous chunk's images
        SG_STORE()
        __syncthreads();
        if (c + 1 < nchunk) SG_LOAD(c + 1)
        // the next chunk's loads stay HERE, in flight under this chunk's MFMAs
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 fa[2][3], fb[2][3];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    fa[i][p] = *reinterpret_cast<const bf16x8 *>(s_a + (((s * 4 + wm * 2 + i) * 3 + p) * 64 + lane) * 16);
                    fb[i][p] = *reinterpret_cast<const bf16x8 *>(s_b + (((s * 4 + wn * 2 + i) * 3 + p) * 64 + lane) * 16);
                }
            // term-major: four independent accumulators between two MFMAs on the same one
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    hi[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[j][0], hi[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    lo[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][1], fb[j][1], lo[i][j], 0, 0, 0);   // mm
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    lo[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[j][2], lo[i][j], 0, 0, 0);   // hl
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    lo[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][2], fb[j][0], lo[i][j], 0, 0, 0);   // lh
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    lo[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[j][1], lo[i][j], 0, 0, 0);   // hm
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    lo[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][1], fb[j][0], lo[i][j], 0, 0, 0);   // mh
        }
    }
#undef SG_LOAD
#undef SG_STORE

    // ---- epilogue: D = hh + (the five correction terms), one fp32 addition.  Accumulator register e of
    // a 32 x 32 block holds row (e & 3) + 8 (e >> 2) + 4 (lane >> 5), column lane & 31.
    float *dst = a.d + (int64_t)b * a.rows * a.N;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = nt * kSgBN + wn * 64 + j * 32 + (lane & 31);
        if (col >= a.N) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t rb = row0 + wm * 64 + i * 32 + 4 * (lane >> 5);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int64_t row = rb + (e & 3) + 8 * (e >> 2);
                if (row < a.rows) dst[row * a.N + col] = hi[i][j][e] + lo[i][j][e];
            }
        }
    }
}

}  // namespace ia

/* D[b] (rows, n) = V[b] (rows, k) . U[b] (k, n) through the exact three-way bf16 split (k_gemm_split3
 * above).  U3 = U split and packed by iouaware/winograd.py split3_pack_u: (batch, k / 16, ceil(n / 128) * 4,
 * 3, 64, 8) bf16.  k a multiple of 32; V and U3 16-byte aligned.  Same bits in every run.  */
extern "C" int ia_batched_gemm_split3(const float *V, const void *U3, float *D, int batch, int64_t rows, int k,
                                      int n, void *stream)
{
    if (!V || !U3 || !D || rows < 1 || batch < 1 || batch > 65535 || k < ia::kSgBK || k % ia::kSgBK || n < 1)
        return IA_E_ARG;
    if (((uintptr_t)V & 15u) || ((uintptr_t)U3 & 15u) || ((uintptr_t)D & 3u)) return IA_E_ARG;
    const int64_t mt = (rows + ia::kSgBM - 1) / ia::kSgBM, ntiles = (n + ia::kSgBN - 1) / ia::kSgBN;
    if (mt * ntiles * batch > 2147483647LL) return IA_E_ARG;      // the workgroup number is an int
    ia::SplitGemmArgs a;
    a.v = V; a.up = (const uint4 *)U3; a.d = D; a.rows = rows; a.K = k; a.N = n;
    a.np32 = (int)(ntiles * (ia::kSgBN / 32));
    a.ntiles = (int)ntiles; a.mtiles = (int)mt;
    const dim3 grid((unsigned)(mt * ntiles * batch)), block(ia::kSgThreads);
    hipLaunchKernelGGL(ia::k_gemm_split3, grid, block, 0, (hipStream_t)stream, a);
    return ia::hip_status(hipGetLastError());
}
