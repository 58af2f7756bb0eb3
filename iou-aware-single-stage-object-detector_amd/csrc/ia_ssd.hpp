// The per-level table of an SSD head (ia_ssd_geom: a different number of anchors per level), shared
// by the decode (ssddecode.hip) and the training loss (ssdloss.hip).
#pragma once
#include "ia_internal.hpp"

namespace ia {

struct SsdTable {
    int32_t num_levels, C;
    int32_t H[IA_MAX_LEVELS], W[IA_MAX_LEVELS], stride[IA_MAX_LEVELS], A[IA_MAX_LEVELS];
    int32_t row_off[IA_MAX_LEVELS + 1];      // prefix of H_l * W_l * A_l (rows per image)
    const float *cls[IA_MAX_LEVELS], *reg[IA_MAX_LEVELS];
};

inline int make_ssd_table(const ia_ssd_geom *g, const ia_ssd_level_ptrs *p, SsdTable &t)
{
    if (!g) return IA_E_ARG;
    if (g->num_levels < 1 || g->num_levels > IA_MAX_LEVELS) return IA_E_ARG;
    if (g->num_classes < 1 || g->num_classes > 4096) return IA_E_ARG;
    t.num_levels = g->num_levels; t.C = g->num_classes;
    t.row_off[0] = 0;
    for (int l = 0; l < IA_MAX_LEVELS; ++l) {
        const bool on = l < g->num_levels;
        if (on && (g->H[l] < 1 || g->W[l] < 1 || g->stride[l] < 1)) return IA_E_ARG;
        if (on && (g->num_anchors[l] < 1 || g->num_anchors[l] > IA_MAX_ANCHORS)) return IA_E_ARG;
        t.H[l] = on ? g->H[l] : 0; t.W[l] = on ? g->W[l] : 0; t.stride[l] = on ? g->stride[l] : 0;
        t.A[l] = on ? g->num_anchors[l] : 1;
        const int64_t n = (int64_t)t.H[l] * t.W[l] * t.A[l];
        if (n > (1 << 30) || t.row_off[l] + n > 2147483647LL) return IA_E_ARG;
        t.row_off[l + 1] = t.row_off[l] + (int32_t)n;
        t.cls[l] = (on && p) ? static_cast<const float *>(p->cls[l]) : nullptr;
        t.reg[l] = (on && p) ? static_cast<const float *>(p->reg[l]) : nullptr;
        if (on && p && (!t.cls[l] || !t.reg[l])) return IA_E_ARG;
    }
    return 0;
}

// workgroups along x of the kernels that put one lane on every (anchor, pixel) of a level
// (k_ssd_rowscore, the loss kernels): enough for the largest level
inline int64_t ssd_row_grid_x(const SsdTable &t)
{
    int64_t nmax = 1;
    for (int l = 0; l < t.num_levels; ++l) {
        const int64_t n = t.row_off[l + 1] - t.row_off[l];
        nmax = n > nmax ? n : nmax;
    }
    return (nmax + 255) / 256;
}

}  // namespace ia
