// L2Norm of the SSD backbone (reference mmdet/models/backbones/ssd_vgg.py, class L2Norm): every
// pixel's channel vector scaled to unit length and multiplied by a per-channel weight,
//
//     norm = sqrt(sum_c x[b, c, p]^2) + eps;     y[b, c, p] = (w[c] * x[b, c, p]) / norm
//
// in the reference's operation order.  fp32 NCHW.  One lane per pixel, lanes consecutive along
// H * W, so every channel plane is read and written in coalesced rows; a grid-stride loop over
// B * H * W.  The sum of squares runs over the channels in ascending order in fp64 (the products
// are exact there) and is rounded to fp32 once, like the GroupNorm statistics: the result does not
// depend on the launch shape and lies well inside any fp32 summation order.  The second pass over
// the pixel's channels (conv4_3: 512 x 38 x 38, 3 MB per image) is served by L2; nothing is staged
// in LDS.  A lane has no neighbour to share its work with, so the loops are unrolled 32 times: a
// wavefront keeps 32 rows of 256 bytes in flight, which is what hides the memory latency here (at
// 8 in flight the kernel ran at a few hundred GB/s).  No atomics: the same bits in every run.  A
// pixel whose channels are all zero gives 0 / eps = 0.
#include "ia_internal.hpp"

namespace ia {

__global__ void __launch_bounds__(64) k_l2norm_nchw(const float *__restrict__ x, const float *__restrict__ w,
                                                     float eps, int64_t total, int C, int64_t HW,
                                                     float *__restrict__ y)
{
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += step) {
        const int64_t b = p / HW, q = p - b * HW;
        const float *xp = x + b * C * HW + q;
        float *yp = y + b * C * HW + q;
        double s = 0.0;
#pragma unroll 32
        for (int c = 0; c < C; ++c) {
            const double v = (double)xp[(int64_t)c * HW];
            s = s + v * v;
        }
        const float norm = __builtin_sqrtf((float)s) + eps;
#pragma unroll 32
        for (int c = 0; c < C; ++c) yp[(int64_t)c * HW] = (w[c] * xp[(int64_t)c * HW]) / norm;
    }
}

}  // namespace ia

extern "C" int ia_l2norm_nchw(const float *x, const float *weight, float eps, int B, int C, int H, int W,
                              float *y, void *stream)
{
    if (!x || !weight || !y || B < 1 || C < 1 || H < 1 || W < 1) return IA_E_ARG;
    const int64_t HW = (int64_t)H * W, total = (int64_t)B * HW;
    if (total > 2147483647LL || total * C > (1LL << 40)) return IA_E_ARG;
    // in place, or any overlap of the two buffers, is not supported: the second pass reads x again
    const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y;
    const uint64_t bytes = (uint64_t)total * C * sizeof(float);
    if (xa < ya + bytes && ya < xa + bytes) return IA_E_ARG;
    // single-wavefront workgroups: conv4_3 of SSD300 has 1 444 pixels per image, 23 wavefronts
    int64_t blocks = (total + 63) / 64;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(ia::k_l2norm_nchw, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, x, weight, eps,
                       total, C, HW, y);
    return ia::hip_status(hipGetLastError());
}
