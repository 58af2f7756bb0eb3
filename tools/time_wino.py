"""Scratch: the head's Winograd layer (input transform, batched GEMM, output transform) at the
benchmark size, timed with events; then a tower transition as GEMM -> output transform -> input
transform against GEMM -> the fused k_wino_mid launch."""
import sys, os
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.join(ROOT, 'iou-aware-single-stage-object-detector_amd'))
import torch
from iouaware import winograd as wg
B, F = 8, 256
sizes = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
plan = wg._Plan(sizes, B, torch.device('cuda'))
T = plan.T
acts = [torch.randn(B, 2 * F, h, w, device='cuda').contiguous(memory_format=torch.channels_last) for h, w in sizes]
outs = [torch.empty_like(a) for a in acts]
u = torch.randn(72, F, F, device='cuda') * 0.05
bias = torch.randn(2 * F, device='cuda')
v = torch.empty(72, T, F, device='cuda'); m = torch.empty(72, T, F, device='cuda')
def run():
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record(); wg.input_transform(plan, acts, 2, v)
    ev[1].record(); torch.bmm(v, u, out=m)
    ev[2].record(); wg.output_transform(plan, m, 2 * F, 2, bias, True, [(0, 2 * F, outs, 0)])
    ev[3].record(); torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(3)]
for _ in range(3): run()
import numpy as np
t = np.mean([run() for _ in range(20)], 0)
act_b = sum(a.numel() for a in acts) * 4; vm_b = v.numel() * 4
print('T=%d  in %.3f ms (%.0f GB/s)  gemm %.3f ms (%.0f TF)  out %.3f ms (%.0f GB/s)' % (
    T, t[0], (act_b + vm_b) / t[0] / 1e6, t[1], 2 * 72 * T * F * F / t[1] / 1e9, t[2], (act_b + vm_b) / t[2] / 1e6))


v2 = torch.empty(72, T, F, device='cuda')
def pair(fused):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.bmm(v, u, out=m)                    # M as the step leaves it: fresh from the GEMM
    ev[0].record()
    if fused:
        wg.mid_transform(plan, m, 2 * F, 2, bias, True, v2, 2)
    else:
        wg.output_transform(plan, m, 2 * F, 2, bias, True, [(0, 2 * F, outs, 0)])
        wg.input_transform(plan, outs, 2, v2)
    ev[1].record(); torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])
for f in (False, True): pair(f)
ts = {False: [], True: []}
for _ in range(20):
    for f in (False, True): ts[f].append(pair(f))
for f, name in ((False, 'out + in'), (True, 'mid     ')):
    print('%s  median %.3f ms  min %.3f  max %.3f' % (name, np.median(ts[f]), min(ts[f]), max(ts[f])))
