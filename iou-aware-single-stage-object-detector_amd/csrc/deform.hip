// Deformable 3x3 convolution (DCN v1 / v2; reference mmdet/ops/dcn, models/backbones/resnet.py) in
// fp32 on channels-last activations: the deformable im2col (this file) -> one library GEMM with the
// bias / folded BatchNorm / ReLU in its epilogue (gemm.hip), and the adjoint of the gather.
//
//   col[(b, ho, wo)][(i * 3 + j) * C + c] = mask * bilinear(x[b][.][.][c]; h, w)
//   h = ho * s - p + i * d + offset[b][ho][wo][g * 18 + 2 (i * 3 + j)]        g = c / (C / dg)
//   w = wo * s - p + j * d + offset[b][ho][wo][g * 18 + 2 (i * 3 + j) + 1]
// the row order of ia_im2col3x3_nhwc, so the (9 * C, Cout) weight of that route is the operand here
// too.  The sample is 0 unless -1 < h < H and -1 < w < W; otherwise the four floor / floor + 1
// corners, a corner outside [0, H - 1] x [0, W - 1] contributing 0.  Offsets and masks are read as
// channels-last rows with a pixel stride, so both may be channel slices of one tensor (the fused
// inference route hands over conv2_offset's output as it is, the mask as raw logits).
//
// One RUN = one (pixel, tap, deformable group): C / dg contiguous channels of col, whose start is
// run * (C / dg).  The sampling position, the corner weights, validity and addresses are computed
// once per run, in front of the channel loop.
//   k_deform_im2col   lanes along the run's channels, 16 bytes per lane (4 corner loads, 1 store)
//   k_deform_col2im   lanes along the run's channels, one float per lane: every wave instruction of
//     the dx scatter (fp32 atomicAdd to the four corners) adds a contiguous run of bytes;
//     d_offset / d_mask are sums over the run's channels -- per lane in ascending channel order,
//     then an in-wave butterfly over the run's lanes: a fixed order, the same bits in every run.
//     dx is NOT bit-reproducible: the order in which the atomics of different runs arrive is not fixed.
#include "ia_internal.hpp"
#include "ia_math.hpp"

namespace ia {

struct DeformArgs {
    const float *x;
    const float *offset;
    const float *mask;       // NULL: no modulation
    int64_t off_ps, mask_ps; // pixel strides of offset / mask in floats
    int32_t mask_logits;     // the mask holds logits: sigmoid here
    int32_t H, W, C, Ho, Wo, stride, pad, dil, dg;
    int32_t cg;              // channels per deformable group
    int32_t shift;           // log2 of the lanes per run
    int64_t runs;            // B * Ho * Wo * 9 * dg
};

// what a run needs: corner element offsets into x (channel 0 of the group; 0 where the corner is
// outside), corner validity, the bilinear fractions and the mask value
struct DeformRun {
    int64_t o1, o2, o3, o4;
    bool ok1, ok2, ok3, ok4;
    float lh, lw, hh, hw, m;
    int64_t pix;
    int32_t g, tap;
};

__device__ __forceinline__ DeformRun deform_run(const DeformArgs &a, int64_t run)
{
    DeformRun r;
    const int64_t t = run / a.dg;
    r.g = (int)(run - t * a.dg);
    r.pix = t / 9;
    r.tap = (int)(t - r.pix * 9);
    const int i = r.tap / 3, j = r.tap - i * 3;
    const int wo = (int)(r.pix % a.Wo);
    const int64_t t2 = r.pix / a.Wo;
    const int ho = (int)(t2 % a.Ho);
    const int64_t b = t2 / a.Ho;
    const float *op = a.offset + r.pix * a.off_ps + (r.g * 18 + 2 * r.tap);
    const float h = (float)(ho * a.stride - a.pad + i * a.dil) + op[0];
    const float w = (float)(wo * a.stride - a.pad + j * a.dil) + op[1];
    const bool in = h > -1.0f && w > -1.0f && h < (float)a.H && w < (float)a.W;   // false for NaN
    const float hl = in ? floorf(h) : 0.0f, wl = in ? floorf(w) : 0.0f;
    const int h0 = (int)hl, w0 = (int)wl, h1 = h0 + 1, w1 = w0 + 1;
    r.lh = in ? h - hl : 0.0f; r.lw = in ? w - wl : 0.0f;
    r.hh = 1.0f - r.lh; r.hw = 1.0f - r.lw;
    r.ok1 = in && h0 >= 0 && w0 >= 0;
    r.ok2 = in && h0 >= 0 && w1 <= a.W - 1;
    r.ok3 = in && h1 <= a.H - 1 && w0 >= 0;
    r.ok4 = in && h1 <= a.H - 1 && w1 <= a.W - 1;
    const int64_t img = b * a.H;
    const int64_t gc = (int64_t)r.g * a.cg;
    r.o1 = r.ok1 ? ((img + h0) * a.W + w0) * a.C + gc : 0;
    r.o2 = r.ok2 ? ((img + h0) * a.W + w1) * a.C + gc : 0;
    r.o3 = r.ok3 ? ((img + h1) * a.W + w0) * a.C + gc : 0;
    r.o4 = r.ok4 ? ((img + h1) * a.W + w1) * a.C + gc : 0;
    r.m = 1.0f;
    if (a.mask) {
        const float v = a.mask[r.pix * a.mask_ps + (r.g * 9 + r.tap)];
        r.m = a.mask_logits ? sigmoidf_(v) : v;
    }
    return r;
}

__device__ __forceinline__ float bilinear(const DeformRun &r, float v1, float v2, float v3, float v4)
{
    return r.hh * r.hw * v1 + r.hh * r.lw * v2 + r.lh * r.hw * v3 + r.lh * r.lw * v4;
}

__global__ __launch_bounds__(256) void k_deform_im2col(DeformArgs a, float4 *col)
{
    const int lane = threadIdx.x & 63;
    const int lanes = 1 << a.shift, sub = lane >> a.shift, l = lane & (lanes - 1);
    const int per_wave = 64 >> a.shift;
    const int cgv = a.cg >> 2;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // every wavefront takes 4 rounds of `per_wave` consecutive runs
    for (int k = 0; k < 4; ++k) {
        const int64_t run = (wave * 4 + k) * per_wave + sub;
        if (run >= a.runs) return;
        const DeformRun r = deform_run(a, run);
        const float4 *p1 = (const float4 *)(a.x + r.o1), *p2 = (const float4 *)(a.x + r.o2);
        const float4 *p3 = (const float4 *)(a.x + r.o3), *p4 = (const float4 *)(a.x + r.o4);
        float4 *dst = col + run * cgv;
        for (int c = l; c < cgv; c += lanes) {
            float4 v1 = p1[c], v2 = p2[c], v3 = p3[c], v4 = p4[c];
            if (!r.ok1) v1 = zero;
            if (!r.ok2) v2 = zero;
            if (!r.ok3) v3 = zero;
            if (!r.ok4) v4 = zero;
            float4 o;
            o.x = r.m * bilinear(r, v1.x, v2.x, v3.x, v4.x);
            o.y = r.m * bilinear(r, v1.y, v2.y, v3.y, v4.y);
            o.z = r.m * bilinear(r, v1.z, v2.z, v3.z, v4.z);
            o.w = r.m * bilinear(r, v1.w, v2.w, v3.w, v4.w);
            dst[c] = o;
        }
    }
}

// the adjoint: dx (atomics, zero-filled by the entry), d_offset (pix, dg * 18), d_mask (pix, dg * 9)
__global__ __launch_bounds__(256) void k_deform_col2im(DeformArgs a, const float *dcol, float *dx,
                                                        float *d_offset, float *d_mask)
{
    const int lane = threadIdx.x & 63;
    const int lanes = 1 << a.shift, sub = lane >> a.shift, l = lane & (lanes - 1);
    const int per_wave = 64 >> a.shift;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool need_v = d_offset != nullptr || d_mask != nullptr;
    for (int k = 0; k < 4; ++k) {
        const int64_t first = (wave * 4 + k) * per_wave;
        if (first >= a.runs) return;                       // wave-uniform
        const int64_t run = first + sub;
        const bool live = run < a.runs;                    // the shuffles below need every lane
        float gh = 0.0f, gw = 0.0f, gm = 0.0f;
        DeformRun r = deform_run(a, live ? run : first);
        if (live) {
            const float *dc = dcol + run * a.cg;
            const float w1 = r.hh * r.hw, w2 = r.hh * r.lw, w3 = r.lh * r.hw, w4 = r.lh * r.lw;
            for (int c = l; c < a.cg; c += lanes) {
                const float d = dc[c];
                const float dm = d * r.m;
                if (dx) {
                    if (r.ok1) atomicAdd(dx + r.o1 + c, dm * w1);
                    if (r.ok2) atomicAdd(dx + r.o2 + c, dm * w2);
                    if (r.ok3) atomicAdd(dx + r.o3 + c, dm * w3);
                    if (r.ok4) atomicAdd(dx + r.o4 + c, dm * w4);
                }
                if (need_v) {
                    float v1 = a.x[r.o1 + c], v2 = a.x[r.o2 + c], v3 = a.x[r.o3 + c], v4 = a.x[r.o4 + c];
                    if (!r.ok1) v1 = 0.0f;
                    if (!r.ok2) v2 = 0.0f;
                    if (!r.ok3) v3 = 0.0f;
                    if (!r.ok4) v4 = 0.0f;
                    gm += d * bilinear(r, v1, v2, v3, v4);
                    gh += dm * (r.hw * (v3 - v1) + r.lw * (v4 - v2));
                    gw += dm * (r.hh * (v2 - v1) + r.lh * (v4 - v3));
                }
            }
        }
        if (need_v) {
            for (int o = lanes >> 1; o > 0; o >>= 1) {
                gh += __shfl_xor(gh, o);
                gw += __shfl_xor(gw, o);
                gm += __shfl_xor(gm, o);
            }
            if (live && l == 0) {
                if (d_offset) {
                    float *p = d_offset + r.pix * ((int64_t)a.dg * 18) + (r.g * 18 + 2 * r.tap);
                    p[0] = gh; p[1] = gw;
                }
                if (d_mask) d_mask[r.pix * ((int64_t)a.dg * 9) + (r.g * 9 + r.tap)] = gm;
            }
        }
    }
}

// shared argument check of the two entries; fills everything of `a` but shift
static int deform_args(DeformArgs &a, const float *x, const float *offset, int64_t off_ps, const float *mask,
                       int64_t mask_ps, int mask_logits, int B, int H, int W, int C, int stride, int pad,
                       int dil, int dg)
{
    if (!x || !offset || B < 1 || H < 1 || W < 1 || C < 1 || stride < 1 || pad < 0 || dil < 1 || dg < 1)
        return IA_E_ARG;
    if (C % (4 * dg)) return IA_E_ARG;
    if (stride > 65536 || pad > 65536 || dil > 65536 || H > (1 << 24) || W > (1 << 24)) return IA_E_ARG;
    const int64_t eh = (int64_t)H + 2 * pad - (2 * dil + 1), ew = (int64_t)W + 2 * pad - (2 * dil + 1);
    if (eh < 0 || ew < 0) return IA_E_ARG;
    if (off_ps < (int64_t)dg * 18 || (mask && mask_ps < (int64_t)dg * 9)) return IA_E_ARG;
    if (((uintptr_t)x) & 15) return IA_E_ARG;
    a.x = x; a.offset = offset; a.mask = mask;
    a.off_ps = off_ps; a.mask_ps = mask ? mask_ps : 0; a.mask_logits = mask && mask_logits ? 1 : 0;
    a.H = H; a.W = W; a.C = C; a.stride = stride; a.pad = pad; a.dil = dil; a.dg = dg;
    a.Ho = (int)(eh / stride + 1); a.Wo = (int)(ew / stride + 1);
    a.cg = C / dg;
    a.runs = (int64_t)B * a.Ho * a.Wo * 9 * dg;
    return 0;
}

static int deform_blocks(const DeformArgs &a, unsigned &blocks)
{
    const int64_t per_block = 16LL * (64 >> a.shift);
    const int64_t n = (a.runs + per_block - 1) / per_block;
    if (n > 2147483647LL) return IA_E_ARG;
    blocks = (unsigned)n;
    return 0;
}

}  // namespace ia

extern "C" size_t ia_deform_im2col3x3_bytes(int B, int H, int W, int C, int stride, int pad, int dil)
{
    if (B < 1 || H < 1 || W < 1 || C < 1 || stride < 1 || pad < 0 || dil < 1) return 0;
    const int64_t eh = (int64_t)H + 2 * pad - (2 * dil + 1), ew = (int64_t)W + 2 * pad - (2 * dil + 1);
    if (eh < 0 || ew < 0) return 0;
    return (size_t)((int64_t)B * (eh / stride + 1) * (ew / stride + 1) * 9 * C * 4);
}

extern "C" int ia_deform_im2col3x3_nhwc(const float *x, const float *offset, int64_t offset_pix_stride,
                                        const float *mask, int64_t mask_pix_stride, int mask_logits,
                                        float *col, int B, int H, int W, int C, int stride, int pad,
                                        int dil, int deformable_groups, void *stream)
{
    ia::DeformArgs a;
    const int rc = ia::deform_args(a, x, offset, offset_pix_stride, mask, mask_pix_stride, mask_logits, B, H, W,
                                   C, stride, pad, dil, deformable_groups);
    if (rc) return rc;
    if (!col || ((uintptr_t)col & 15)) return IA_E_ARG;
    const int cgv = a.cg / 4;
    a.shift = 0;
    while (a.shift < 6 && (2 << a.shift) <= cgv) ++a.shift;
    unsigned blocks;
    if (ia::deform_blocks(a, blocks)) return IA_E_ARG;
    hipLaunchKernelGGL(ia::k_deform_im2col, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, (float4 *)col);
    return ia::hip_status(hipGetLastError());
}

extern "C" int ia_deform_col2im3x3_nhwc(const float *dcol, const float *x, const float *offset,
                                        int64_t offset_pix_stride, const float *mask,
                                        int64_t mask_pix_stride, float *dx, float *d_offset, float *d_mask,
                                        int B, int H, int W, int C, int stride, int pad, int dil,
                                        int deformable_groups, void *stream)
{
    ia::DeformArgs a;
    const int rc = ia::deform_args(a, x, offset, offset_pix_stride, mask, mask_pix_stride, 0, B, H, W, C, stride,
                                   pad, dil, deformable_groups);
    if (rc) return rc;
    if (!dcol || (d_mask && !mask) || (!dx && !d_offset && !d_mask)) return IA_E_ARG;
    a.shift = 0;
    while (a.shift < 6 && (2 << a.shift) <= a.cg) ++a.shift;
    unsigned blocks;
    if (ia::deform_blocks(a, blocks)) return IA_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (dx) {
        const hipError_t e = hipMemsetAsync(dx, 0, (size_t)B * H * W * C * sizeof(float), s);
        if (e != hipSuccess) return ia::hip_status(e);
    }
    hipLaunchKernelGGL(ia::k_deform_col2im, dim3(blocks), dim3(256), 0, s, a, dcol, dx, d_offset, d_mask);
    return ia::hip_status(hipGetLastError());
}
