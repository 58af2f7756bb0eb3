"""The head's large Winograd-domain products (bench config 2: R-50, batch 8, 800 x 1344, T = 11 440 tiles) on
ia_batched_gemm_split3 (bf16 MFMA, exact three-way split) against the library's fp32 batched GEMM (frozen
table kernels), on two kinds of data: random-normal operands, and V / U captured from a bench forward (the
library gains ~15 % on the step's low-entropy data, so the captured data decide).  A shape belongs in
winograd._SPLIT_SHAPES only if every repetition of the split kernel beats every library repetition on the
captured data.

    python tools/time_split_gemm.py [--reps 5] [--iters 10]
"""
import argparse
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
from iouaware import winograd as wg  # noqa: E402

NAMES = ['layer 0', 'tower layer 1', 'tower layer 2', 'tower layer 3', 'retina_cls']


def timed(fn, iters):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3       # us


def race(v, u, u3, reps, iters):
    out = torch.empty(v.shape[0], v.shape[1], u.shape[2], device=v.device)
    lib, own = [], []
    for _ in range(reps):                          # alternating: the same clock state for both
        wg.SPLIT_GEMM = False
        lib.append(timed(lambda: wg.batched_gemm(v, u, out, u3), iters))
        wg.SPLIT_GEMM = True
        own.append(timed(lambda: wg.batched_gemm(v, u, out, u3), iters))
    a = wg.batched_gemm(v, u, torch.empty_like(out), u3)
    wg.SPLIT_GEMM = False
    b = wg.batched_gemm(v, u, torch.empty_like(out), u3)
    wg.SPLIT_GEMM = True
    diff = float((a - b).abs().max() / b.abs().max())
    return lib, own, diff


def report(name, v, u, lib, own, diff):
    b, rows, k = v.shape
    n = u.shape[2]
    fl = 2.0 * b * rows * k * n
    ml, mo = sum(lib) / len(lib), sum(own) / len(own)
    print('%-14s (%d, %d, %d, %d)  library %7.1f us [%s] %5.1f TF   split3 %7.1f us [%s] %5.1f TF   '
          'x%.3f  every split rep faster: %s   max |split - library| / max %.1e'
          % (name, b, rows, k, n, ml, ' '.join('%.1f' % t for t in lib), fl / ml / 1e6, mo,
             ' '.join('%.1f' % t for t in own), fl / mo / 1e6, ml / mo, 'YES' if max(own) < min(lib) else 'no', diff),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    keep = list(wg._SPLIT_SHAPES)
    wg._SPLIT_SHAPES = ((256, 512), (256, 256), (256, 720))   # pack every candidate, whatever the table says
    model = bench.build_model(dev, fuse=True, channels_last=True)
    head = model.bbox_head._ia_wino
    captured = []
    real = wg.batched_gemm

    def capture(v, u, out, u3=None):
        r = real(v, u, out, u3)
        if u3 is not None:
            captured.append((v.clone(), u, u3))
        return r
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(8, 3, bench.PAD_H, bench.PAD_W, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        wg.batched_gemm = capture
        try:
            model.forward_head(x)
        finally:
            wg.batched_gemm = real
    torch.cuda.synchronize()
    assert len(captured) == len(NAMES), len(captured)
    del model
    print('# captured from a bench forward (R-50, batch 8, 800 x 1344), %d reps x %d launches each, alternating'
          % (args.reps, args.iters))
    with torch.no_grad():
        for name, (v, u, u3) in zip(NAMES, captured):
            report(name, v, u, *race(v, u, u3, args.reps, args.iters))
        print('# random-normal operands of the same shapes (V ~ N(0, 1), U ~ N(0, 0.05^2))')
        seen = set()
        for name, (v, u, _) in zip(NAMES, captured):
            key = (tuple(v.shape), tuple(u.shape))
            if key in seen:
                continue
            seen.add(key)
            gr = torch.Generator(device=dev).manual_seed(len(seen))
            vr = torch.randn(v.shape, device=dev, generator=gr)
            ur = torch.randn(u.shape, device=dev, generator=gr) * 0.05
            report(name, vr, ur, *race(vr, ur, wg.split3_pack_u(ur), args.reps, args.iters))
            del vr
    print('# _SPLIT_SHAPES of this tree: %s; head built with %s' % (keep, [s is not None for s in [head.u0_3] + head.u_3 + [head.u_cls3]]))


if __name__ == '__main__':
    main()
