"""One stage-1 3x3 / 64 -> 64 convolution at batch 8 (200 x 336, T = 33 600 tiles): k_wino_in_gemm<64> into M
followed by k_wino_out<true> (two launches) against the one-launch k_wino_conv<64> (csrc/wino.hip, the output
transform on the accumulators), HIP events around single launches; cold = a 384 MB fill in between.

    python tools/time_wino_conv64.py
"""
import os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.join(ROOT, 'iou-aware-single-stage-object-detector_amd'))
import torch
from iouaware import winograd as wg
dev = 'cuda'
torch.manual_seed(0)
B, H, W = 8, 200, 336
x = torch.randn(B, 64, H, W, device=dev).contiguous(memory_format=torch.channels_last)
u = torch.randn(36, 64, 64, device=dev) * 0.1
up = wg.pack_u_fragments(u)
ps, pb = torch.rand(64, device=dev) + 0.5, torch.randn(64, device=dev)
bias = torch.randn(64, device=dev)
pre = (ps, pb, True)
plan = wg._Plan([(H, W)], B, torch.device(dev))
T = plan.T
m = plan.buf('m', (36, T, 64))
y1 = torch.empty_like(x); y2 = torch.empty_like(x)
big = torch.empty(96 << 20, device=dev)     # 384 MB: evicts L2 / MALL between repetitions
def timeit(fn, n=10, flush=True):
    ts = []
    for i in range(n + 2):
        if flush: big.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        if i >= 2: ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts
def t_in_gemm(): wg.input_transform_gemm(plan, [x], up, m, pre)
def t_out(): wg.output_transform(plan, m, 64, 1, bias, True, [(0, 64, [y1], 0)])
def t_pair(): t_in_gemm(); t_out()
def t_one(): wg.input_transform_gemm(plan, [x], up, None, pre, epilogue=(bias, True, [y2]))
t_pair(); t_one(); torch.cuda.synchronize()
print('T', T, 'equal', torch.equal(y1, y2))
res = {}
for name, fn in (('k_wino_in_gemm', t_in_gemm), ('k_wino_out', t_out), ('pair', t_pair), ('one launch', t_one)):
    for flush in (True, False):
        ts = res[(name, flush)] = timeit(fn, flush=flush)
        print('%-14s %s  median %.1f us  (min %.1f max %.1f)' % (name, 'cold' if flush else 'warm', ts[len(ts) // 2], ts[0], ts[-1]),
              flush=True)
for flush in (True, False):
    print('%s: every one-launch repetition below every repetition of the pair: %s'
          % ('cold' if flush else 'warm', res[('one launch', flush)][-1] < res[('pair', flush)][0]))
