#!/usr/bin/env python
"""the conv2 shapes of an R-50 with DCN at 800 x 1344 (C = 128 / 256 / 512 on 100 x 168 / 50 x 84 /
25 x 42; the stride-1 blocks and the strided first block of each stage; B images, default 4) as a
deformable convolution (csrc/deform.hip + the library GEMMs) beside the SAME layer as a plain
convolution on the route it has today -- Winograd at stride 1, im2col + GEMM with a stride -- which
is what the layer costs without `dcn=`: the difference is what deformation costs.

Per layer, by device events, in alternating rounds (deformable, plain, deformable, ...; the median
round is printed with the spread): the forward, the three backward launches of the deformable op
(dcol GEMM | adjoint gather with the dx atomics | column matrix again + weight-gradient GEMM) and
forward + backward of both autograd nodes.  The adjoint's time stands beside the estimate from the
chip-wide float-atomic rate (4 corner adds of 4 bytes per column element at ~1.3 TB/s of added
bytes): DESIGN 3.20.  conv2_offset, an ordinary convolution, is not in these figures.

    python tools/time_dcn.py [B] [--modulated] [--rounds N]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'iou-aware-single-stage-object-detector_amd'))
import torch  # noqa: E402
from iouaware import ops, train_fuse, winograd_train as WT  # noqa: E402
from iouaware.deform_conv import deform_conv, modulated_deform_conv  # noqa: E402
from iouaware.winograd import WinogradConv3x3  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
B = int(args[0]) if args else 4
MOD = '--modulated' in sys.argv
ROUNDS = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 5
ATOMIC_RATE = 1.3e12          # bytes of fp32 atomic adds per second, chip-wide


def once(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def alternate(fns, n=10):
    """{name: fn} -> {name: (median us, min, max)}: every round times each fn once, in turn"""
    for fn in fns.values():
        fn(); fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(once(fn, n))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def show(r, k):
    m, lo, hi = r[k]
    return '%8.1f [%7.1f..%7.1f]' % (m, lo, hi)


print('batch %d, %s, %d alternating rounds; us per call: median [min..max]' % (B, 'modulated' if MOD else 'v1', ROUNDS))
for name, C, H, W, s in (('stage 2 first', 128, 200, 336, 2), ('stage 2', 128, 100, 168, 1),
                         ('stage 3 first', 256, 100, 168, 2), ('stage 3', 256, 50, 84, 1),
                         ('stage 4 first', 512, 50, 84, 2), ('stage 4', 512, 25, 42, 1)):
    cl = torch.channels_last
    g = torch.Generator(device='cuda').manual_seed(C + s)
    x = torch.randn(B, C, H, W, device='cuda', generator=g).contiguous(memory_format=cl)
    w = (torch.randn(C, C, 3, 3, device='cuda', generator=g) * 0.01)
    b = torch.randn(C, device='cuda', generator=g)
    Ho, Wo = ops.deform_out_hw(H, W, s, 1, 1)
    off = (torch.rand(B, 18, Ho, Wo, device='cuda', generator=g) * 2 - 1).contiguous(memory_format=cl)
    mask = torch.rand(B, 9, Ho, Wo, device='cuda', generator=g).contiguous(memory_format=cl) if MOD else None
    dy = torch.randn(B, C, Ho, Wo, device='cuda', generator=g).contiguous(memory_format=cl)
    wk = ops.conv3x3_weight_kn(w)
    # --- forward, inference routes
    if s == 1:
        wino = WinogradConv3x3(w, b, relu=True)
        plain_fwd = lambda: wino(x)                                              # noqa: E731
    else:
        plain_fwd = lambda: ops.conv3x3_im2col(x, wk, b, stride=s, relu=True)    # noqa: E731
    with torch.no_grad():
        r = alternate({'dcn': lambda: ops.deform_conv3x3(x, off, mask, wk, b, s, 1, 1, 1, relu=True),
                       'plain': plain_fwd})
        # --- the three backward launches of the deformable op (one chunk's buffers are reused as in the node)
        r.update(alternate({
            'adjoint+dcol': lambda: ops.deform_conv3x3_backward(dy, x, off, mask, wk, s, 1, 1, 1, need=(True, True, True, False)),
            'dW': lambda: ops.deform_conv3x3_backward(dy, x, off, mask, wk, s, 1, 1, 1, need=(False, False, False, True))}))
        step = ops._deform_chunk(x, s, 1, 1, None)
        xs, os_, ms, gs = x[:step], off[:step], None if mask is None else mask[:step], dy[:step]
        dcol = ops.conv3x3_dcol(gs, wk).clone()
        r.update(alternate({
            'dcol GEMM': lambda: ops.conv3x3_dcol(gs, wk),
            'adjoint': lambda: ops.deform_col2im3x3(dcol, xs, os_, ms, s, 1, 1, 1),
            'adjoint, dx only': lambda: ops.deform_col2im3x3(dcol, xs, os_, ms, s, 1, 1, 1, need=(True, False, False)),
            'im2col': lambda: ops.deform_im2col3x3(xs, os_, ms, s, 1, 1, 1)}))
    # --- forward + backward of the autograd nodes
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    offr = off.clone().requires_grad_(True)
    mr = None if mask is None else mask.clone().requires_grad_(True)

    def dcn_node():
        if MOD:
            y = modulated_deform_conv(xr, offr, mr, wr, br, s, 1, 1, 1, 1)
            torch.autograd.grad(y, (xr, offr, mr, wr, br), dy)
        else:
            torch.autograd.grad(deform_conv(xr, offr, wr, s, 1, 1, 1, 1), (xr, offr, wr), dy)

    def plain_node():
        if s == 1:
            y = WT.wino_conv_levels([xr], wr, br, relu=True)[0]
        else:
            y = train_fuse.conv3x3_strided(xr, wr, br, s, True)
        torch.autograd.grad(y, (xr, wr, br), dy)
    r.update(alternate({'dcn node': dcn_node, 'plain node': plain_node}, n=5))
    rows = step * Ho * Wo
    est = rows * 9 * C * 4 * 4 / ATOMIC_RATE * 1e6          # 4 corners x 4 bytes per column element
    print('%-14s %3d ch %3dx%3d s%d, %d of %d images per chunk' % (name, C, Ho, Wo, s, step, B))
    print('    forward          deformable %s | plain (%s) %s' % (show(r, 'dcn'), 'Winograd' if s == 1 else 'im2col', show(r, 'plain')))
    print('    backward, whole batch:  dcol GEMM + adjoint %s | col again + dW %s' % (
        show(r, 'adjoint+dcol'), show(r, 'dW')))
    print('    one chunk:  dcol GEMM %s | adjoint %s | adjoint dx only %s | im2col %s' % (
        show(r, 'dcol GEMM'), show(r, 'adjoint'), show(r, 'adjoint, dx only'), show(r, 'im2col')))
    print('    adjoint, one chunk: %.1f MB of atomic adds -> estimate %.1f us at 1.3 TB/s, measured %.1f us (dx only %.1f)' % (
        rows * 9 * C * 16 / 1e6, est, r['adjoint'][0], r['adjoint, dx only'][0]))
    print('    forward + backward nodes   deformable %s | plain %s' % (show(r, 'dcn node'), show(r, 'plain node')), flush=True)
print(ops.gemm_table_stats())
