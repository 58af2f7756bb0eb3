"""One stage-1 3x3 / 64 -> 64 convolution at batch 8 (200 x 336, T = 33 600 tiles): the input transform and the
batched streaming products as two launches (k_wino_in<true> + k_conv1x1_stream<64, 64>) against the one-launch
k_wino_in_gemm<64> (csrc/wino.hip), HIP events around single launches; cold = a 384 MB fill in between.

    python tools/time_wino_in_gemm.py
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
pre = (ps, pb, True)
plan = wg._Plan([(H, W)], B, torch.device(dev))
T = plan.T
v = plan.buf('v', (36, T, 64)); m = plan.buf('m', (36, T, 64)); m2 = torch.empty(36, T, 64, device=dev)
big = torch.empty(96 << 20, device=dev)     # 384 MB: evicts L2 / MALL between repetitions
def timeit(fn, n=10, flush=True):
    ts = []
    for i in range(n + 2):
        if flush: big.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        if i >= 2: ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]
def t_in(): wg.input_transform(plan, [x], 1, v, pre)
def t_bmm(): wg.batched_gemm(v, u, m)
def t_pair(): t_in(); t_bmm()
def t_fused(): wg.input_transform_gemm(plan, [x], up, m2, pre)
t_pair(); t_fused(); torch.cuda.synchronize()
print('T', T, 'equal', torch.equal(m, m2))
for name, fn in (('k_wino_in', t_in), ('stream bmm', t_bmm), ('pair', t_pair), ('fused', t_fused)):
    for flush in (True, False):
        print('%-12s %s  median %.1f us  (min %.1f max %.1f)' % ((name, 'cold' if flush else 'warm') + timeit(fn, flush=flush)), flush=True)
