// Softmax statistics of one anchor row, shared by the softmax kernels of decode.hip
// (k_rowscore_softmax, k_gather_softmax) and the SSD decode (ssddecode.hip): every softmax score of
// this build comes from this one sequence of operations, so the paths agree to the bit.
#pragma once
#include "ia_math.hpp"

namespace ia {

// x: the row's first logit, cs: channel stride, Cin = C + 1 logits (channel 0 = background).
// m = max over the Cin logits; s = sum of exp(x_c - m), added in class order; e_fg = the largest
// exp(x_c - m) over the FOREGROUND columns c >= 1.
template <typename T>
__device__ __forceinline__ void softmax_row_stats(const T *x, size_t cs, int Cin, float &m, float &s, float &e_fg)
{
    m = -__builtin_inff();
    for (int c = 0; c < Cin; ++c) {
        const float v = load_f32<T>(x + (size_t)c * cs);
        m = (m < v) ? v : m;
    }
    s = 0.0f; e_fg = 0.0f;
    for (int c = 0; c < Cin; ++c) {
        const float e = expf_(load_f32<T>(x + (size_t)c * cs) - m);
        s = s + e;
        if (c >= 1) e_fg = (e_fg < e) ? e : e_fg;
    }
}

}  // namespace ia
