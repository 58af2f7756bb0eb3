// What the all-levels head-loss kernels of headloss.hip share with the point-head loss
// (pointloss.hip): the level / launch-order table, the focal kernel's arguments with their scalar
// tail (FocalTail, filled by focal_tail() for every caller) and the focal launcher.
// The kernels themselves stay in headloss.hip (one translation unit owns their device code);
// pointloss.hip runs the focal kernels through launch_focal_ml_f32 / launch_focal_nhwc_unit with A = 1.
#pragma once
#include "ia_internal.hpp"

namespace ia {

struct HLLevels {
    int32_t L, B, A, C;
    int32_t H[IA_MAX_LEVELS], W[IA_MAX_LEVELS], stride[IA_MAX_LEVELS];
    int32_t blk_off[IA_MAX_LEVELS + 1];   // prefix over launch order o (level = L-1-o) of B*A*tiles
    // focal kernel: the class range of the small levels is cut into csplit chunks of cchunk classes
    // (a lone wavefront per (image, anchor, tile) would run 80 dependent class steps while the
    // big level streams: the small levels' chains, not HBM, would set the kernel's duration)
    int32_t csplit[IA_MAX_LEVELS], cchunk[IA_MAX_LEVELS];
    int32_t fblk_off[IA_MAX_LEVELS + 1];  // prefix of B*A*csplit*tiles
    int32_t pack_off[IA_MAX_LEVELS + 1];  // prefix of B*A*HW: element offset of a level in the packed targets
};

// the scalar tail of every focal kernel's arguments (k_focal_ml, k_focal_nhwc)
struct FocalTail {
    double *sums;                         // fwd: [3][L][IA_LOSS_SLOTS] (+ [2][L][..]: S1, S2 of BAL_CLS)
    const float *gin, *res;               // bwd
    float alpha_pos, alpha_neg, loss_weight;
    int32_t big_logits;                   // evaluate the exact tail for logits > kXMax (fwd)
};

struct FocalMLArgs {
    HLLevels lv;
    const void *cls[IA_MAX_LEVELS];
    const int32_t *lab_am;                // packed targets: anchor-major labels / weights,
    const float *w_am;                    // level l at pack_off[l], then (B, A, HW)
    float *grad[IA_MAX_LEVELS];
    FocalTail tail;
};

// the channels-last kernels' level table (k_focal_nhwc, k_box_nhwc) and the focal kernel's arguments
struct NhwcLevels {
    int32_t L, B, A, C;
    int32_t H[IA_MAX_LEVELS], W[IA_MAX_LEVELS], stride[IA_MAX_LEVELS];
    int32_t fblk_off[IA_MAX_LEVELS + 1];      // focal: blocks of kFocalChunks float4 chunks, launch order
    int32_t bblk_off[IA_MAX_LEVELS + 1];      // box: blocks of 256 anchors, launch order
};
constexpr int kFocalU = 4;                    // float4 chunks per thread
constexpr int kFocalChunks = 256 * kFocalU;   // per block

struct FocalNhwcArgs {
    NhwcLevels lv;
    const void *cls[IA_MAX_LEVELS];           // fp32 or bf16 (the kernel's storage type)
    int64_t ps_cls[IA_MAX_LEVELS], ps_grad[IA_MAX_LEVELS];   // pixel strides (elements)
    const int64_t *labels[IA_MAX_LEVELS];
    const float *lw[IA_MAX_LEVELS];           // not read by the unit-weight instances
    void *grad[IA_MAX_LEVELS];
    FocalTail tail;
};

// IoU-balanced focal loss (BAL_CLS instances only): what the rare positive correction needs to
// recompute its anchor's IoU with the code the box kernel runs -- four deltas, one float4 target,
// the regenerated anchor.  It rides BEHIND the plain argument block, so the plain instances (and
// the point heads' launches) keep their kernel arguments as they are.
struct FocalBal {
    BaseAnchors ba;
    const void *reg[IA_MAX_LEVELS];           // NCHW: the kernel's storage type; channels-last: fp32 rows
    const float *bt[IA_MAX_LEVELS];           // (B, N_l, 4)
    int64_t ps_reg[IA_MAX_LEVELS];            // channels-last: pixel stride of reg (elements)
    float means[4], stds[4];
    float eta;
};
struct FocalMLBalArgs : FocalMLArgs { FocalBal bal; };
struct FocalNhwcBalArgs : FocalNhwcArgs { FocalBal bal; };
template <bool BAL_CLS> struct FocalSel { typedef FocalMLArgs ML; typedef FocalNhwcArgs Nhwc; };
template <> struct FocalSel<true> { typedef FocalMLBalArgs ML; typedef FocalNhwcBalArgs Nhwc; };

// forward: sums and the exact_large_logits switch, gin = res = NULL; backward: sums = NULL;
// headloss.hip
FocalTail focal_tail(float alpha, float loss_weight, bool exact_large_logits, double *sums,
                     const float *gin, const float *res);
// geometry -> table (IA_E_ARG for what the kernels do not cover); headloss.hip
int fill_levels(const ia_head_geom *g, int B, HLLevels &lv);
// k_focal_ml<float, bwd> over fa.lv.fblk_off[L] wavefronts; headloss.hip
int launch_focal_ml_f32(const FocalMLArgs &fa, bool bwd, hipStream_t s);

// geometry -> channels-last table (C % 4 == 0); headloss.hip
int fill_levels_nhwc(const ia_head_geom *g, int B, NhwcLevels &lv);
// k_focal_nhwc<bwd, float | bf16, unit label weights> (fa.lw is not read); headloss.hip
int launch_focal_nhwc_unit(const FocalNhwcArgs &fa, int dtype, bool bwd, hipStream_t s);

}  // namespace ia
