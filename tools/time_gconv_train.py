"""Scratch: the grouped 3x3 conv2 shapes of X-101-32x4d / 64x4d in training (800 x 1344 input, stages
2-4, both strides) -- the three backward launches of csrc/gconv_bwd.hip (adjoint pack, input
gradient, weight gradient) against the library's grouped-convolution backward on the same tensors
(what the module route runs), and the forward kernel on the shape (the floor one expects for the
stride-1 input gradient, which IS that kernel).

    python tools/time_gconv_train.py [B]        B images (default 2, the configs' own)
    GROUPS=32|64   REPS=n (default 30)

Device events around REPS back-to-back calls after 5 warm-up calls, per shape; one line per shape."""
import os
import sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.join(ROOT, 'iou-aware-single-stage-object-detector_amd'))
import torch
from iouaware import ops

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
GROUPS = int(os.environ.get('GROUPS', '32'))
REPS = int(os.environ.get('REPS', '30'))
torch.backends.cudnn.benchmark = True


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS * 1e3          # us


def main():
    cl = torch.channels_last
    print('X-101-%dx4d conv2, batch %d, 800 x 1344, fp32, us per call (mean of %d)' % (GROUPS, B, REPS))
    print('%-26s %9s %9s %9s %9s | %9s %9s' % ('stage stride C cg HxW(in)', 'pack', 'dx', 'dW', 'sum', 'library', 'forward'))
    # (stage, stride, input map of conv2): the first block of a stage strides, the others do not
    shapes = [(2, 2, 200, 336), (2, 1, 100, 168), (3, 2, 100, 168), (3, 1, 50, 84), (4, 2, 50, 84), (4, 1, 25, 42)]
    for stage, stride, H, W in shapes:
        cg = 4 * 2 ** (stage - 1)
        C = cg * GROUPS
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        g = torch.Generator(device='cuda').manual_seed(stage * 10 + stride)
        x = torch.randn(B, C, H, W, device='cuda', generator=g).contiguous(memory_format=cl)
        dz = torch.randn(B, C, Ho, Wo, device='cuda', generator=g).contiguous(memory_format=cl)
        w = torch.randn(C, cg, 3, 3, device='cuda', generator=g) * (1.0 / (9 * cg)) ** 0.5
        wcl = w.contiguous(memory_format=cl)
        wp = ops.pack_grouped_weight_dev(w)
        wadj = ops.pack_grouped_weight_dev(w, adjoint=True)
        t_pack = timed(lambda: ops.pack_grouped_weight_dev(w, adjoint=True))
        t_dx = timed(lambda: ops.grouped_conv3x3_bwd_data(dz, wadj, GROUPS, stride, (H, W)))
        t_dw = timed(lambda: ops.grouped_conv3x3_bwd_weight(x, dz, GROUPS, stride))
        t_fwd = timed(lambda: ops.grouped_conv3x3(x, wp, None, GROUPS, stride, False))
        t_lib = timed(lambda: torch.ops.aten.convolution_backward(
            dz, x, wcl, None, (stride, stride), (1, 1), (1, 1), False, (0, 0), GROUPS, (True, True, False)))
        # same results, to the order of the sums
        dx_l, dw_l, _ = torch.ops.aten.convolution_backward(
            dz, x, wcl, None, (stride, stride), (1, 1), (1, 1), False, (0, 0), GROUPS, (True, True, False))
        dx_o = ops.grouped_conv3x3_bwd_data(dz, wadj, GROUPS, stride, (H, W))
        dw_o = ops.grouped_conv3x3_bwd_weight(x, dz, GROUPS, stride)
        ex = float((dx_o - dx_l).abs().max() / dx_l.abs().max())
        ew = float((dw_o - dw_l).abs().max() / dw_l.abs().max())
        print('%d %d %5d %2d %3dx%-4d       %9.1f %9.1f %9.1f %9.1f | %9.1f %9.1f   (dx %.1e dW %.1e vs library)'
              % (stage, stride, C, cg, H, W, t_pack, t_dx, t_dw, t_pack + t_dx + t_dw, t_lib, t_fwd, ex, ew))


if __name__ == '__main__':
    main()
