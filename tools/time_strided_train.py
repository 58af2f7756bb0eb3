#!/usr/bin/env python
"""the five strided 3x3 convolutions of the R-50 RetinaNet training iteration (conv2 of the first
block of stages 2-4, P6, P7; 800 x 1344, B images, default 4), forward + backward, piece by piece:
the node train_fuse.conv3x3_strided (im2col + GEMM | dcol GEMM | k_col2im3x3 | im2col again |
sliced weight-gradient product) against the framework's convolution, by device events.

    python tools/time_strided_train.py [B]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'iou-aware-single-stage-object-detector_amd'))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from iouaware import ops, train_fuse  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
HBM_PEAK = 8.0e12


def timeit(fn, n=10):
    fn(); fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


print('batch %d; us per call' % B)
tot_own = tot_lib = 0.0
for name, C, H, W, n in (('stage 2', 128, 200, 336, 128), ('stage 3', 256, 100, 168, 256), ('stage 4', 512, 50, 84, 512),
                         ('P6', 2048, 25, 42, 256), ('P7', 256, 13, 21, 256)):
    x = torch.randn(B, C, H, W, device='cuda').contiguous(memory_format=torch.channels_last)
    w = (torch.randn(n, C, 3, 3, device='cuda') * 0.01).contiguous(memory_format=torch.channels_last)
    b = torch.randn(n, device='cuda')
    wk = ops.conv3x3_weight_kn(w)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    P = B * Ho * Wo
    g = torch.randn(B, n, Ho, Wo, device='cuda').contiguous(memory_format=torch.channels_last)
    g2 = train_fuse._rows(g)
    t_fwd = timeit(lambda: ops.conv3x3_im2col(x, wk, b, 2, True))
    t_dcol = timeit(lambda: ops.conv3x3_dcol(g, wk))
    dcol = ops.conv3x3_dcol(g, wk)
    t_c2i = timeit(lambda: ops.col2im3x3(dcol, B, H, W, C, 2))
    t_i2c = timeit(lambda: ops.im2col3x3(x, 2))
    col = ops.im2col3x3(x, 2)
    t_dw = timeit(lambda: train_fuse.weight_grad_1x1(g2, col))
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)

    def node():
        torch.autograd.grad(train_fuse.conv3x3_strided(xr, wr, br, 2, True), (xr, wr, br), g)
    t_node = timeit(node)

    def lib():
        torch.autograd.grad(F.relu(F.conv2d(xr, wr, br, 2, 1)), (xr, wr, br), g)
    t_lib = timeit(lib)
    nbytes = (9 * C * P + B * H * W * C) * 4
    gf = 2.0 * P * 9 * C * n / 1e9
    tot_own += t_node
    tot_lib += t_lib
    print('%-7s %4d -> %4d @ %3dx%3d: fwd %6.1f | dcol GEMM %6.1f (%3.0f TFLOP/s) | col2im %6.1f (%5.1f MB, %.2f TB/s, %.0f %% of 8 TB/s) | '
          'im2col %6.1f | dW %6.1f (%3.0f TFLOP/s) | node fwd+bwd %7.1f | framework conv + relu fwd+bwd %7.1f'
          % (name, C, n, H, W, t_fwd, t_dcol, gf / t_dcol * 1e3, t_c2i, nbytes / 1e6, nbytes / t_c2i / 1e6,
             100 * nbytes / (t_c2i * 1e-6) / HBM_PEAK, t_i2c, t_dw, gf / t_dw * 1e3, t_node, t_lib), flush=True)
print('five layers, fwd + bwd: node %.1f us, framework %.1f us' % (tot_own, tot_lib))
print(ops.gemm_table_stats())
