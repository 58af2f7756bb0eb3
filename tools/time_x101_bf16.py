"""The whole bf16 inference step of X-101-64x4d (or X-101-32x4d) at batch 8, 800 x 1344, random init: the
model construction of `bench.py --config x101-64x4d`, converted to bf16, the benchmark's step (network +
post-conv path + host results) and its timing contract -- with the grouped 3x3 convolutions on the bf16 MFMA
kernel of csrc/gconv_bf16.hip (backbone switch `gconv_bf16` on) and on the library's grouped convolution +
affine pass (switch off: what the tree computed before the kernel existed), in alternating pairs.

    python tools/time_x101_bf16.py [--pairs 3] [--steps 10] [--warmup 3] [--groups 64]
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'iou-aware-single-stage-object-detector_amd'))
import torch

import bench
from iouaware import ops
from iouaware.backbones import ResNet


def stepper_for(on, groups, batch):
    default = ResNet.gconv_bf16
    ResNet.gconv_bf16 = on                       # read by fuse_inference
    try:
        model = bench.build_model(torch.device('cuda', 0), fuse=True, channels_last=True, winograd=True,
                                  backbone=dict(type='ResNeXt', depth=101, groups=groups, base_width=4))
    finally:
        ResNet.gconv_bf16 = default
    g = torch.Generator(device='cuda').manual_seed(1234)
    imgs = torch.randn(batch, 3, bench.PAD_H, bench.PAD_W, device='cuda', generator=g)
    model, imgs = model.to(torch.bfloat16), imgs.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    return bench.Stepper(model, imgs, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--groups', type=int, default=64, choices=[32, 64])
    ap.add_argument('--batch', type=int, default=8)
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = False       # as bench.py: immediate mode, nothing picked by timing
    ops.gemm_tuning('frozen')
    steppers = {on: stepper_for(on, args.groups, args.batch) for on in (True, False)}
    calls = []
    real = ops.grouped_conv3x3_bf16
    ops.grouped_conv3x3_bf16 = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    for on in (True, False):
        del calls[:]
        steppers[on].step(timed=True)
        steppers[on].drain()
        assert len(calls) == (33 if on else 0), (on, len(calls))      # the route under test did / did not run
    ops.grouped_conv3x3_bf16 = real
    device = torch.device('cuda', 0)
    pairs = []
    for p in range(args.pairs):
        ms = {}
        for on in ((True, False) if p % 2 == 0 else (False, True)):
            s = steppers[on]
            el = bench.timed_region(lambda: s.step(timed=True), args.steps, args.warmup, 1, torch.cuda.synchronize,
                                    None, device, drain=s.drain)
            ms[on] = el / args.steps * 1e3
        pairs.append(dict(own_kernel_ms=round(ms[True], 3), library_ms=round(ms[False], 3)))
        print('pair %d: own kernel %.2f ms/step, library %.2f ms/step' % (p, ms[True], ms[False]), flush=True)
    print(json.dumps(dict(what='X-101-%dx4d bf16 inference step, batch %d, 800 x 1344' % (args.groups, args.batch),
                          steps=args.steps, warmup=args.warmup, pairs=pairs,
                          own_kernel_faster_in_all_pairs=all(q['own_kernel_ms'] < q['library_ms'] for q in pairs))))


if __name__ == '__main__':
    main()
