#!/usr/bin/env python
"""the masked convolution of the guided-anchor head (csrc/masked_conv.hip + the library GEMM) and
the whole IoUawareGARetinaHead at the five level sizes of an 800 x 1344 input, batch 1.

Per level (100 x 168 .. 7 x 11) one masked layer -- retina_cls: 3x3, 256 -> 80 -- at keep fractions
1 %, 10 %, 50 % and 100 % beside the DENSE convolution of the same layer on the route it has with
mask=None (the module route: the framework's channels-last convolution):
    masked      compaction + gather + GEMM + scatter, the kept count read back from the device
                (the operator as masked_conv2d runs it)
    no copy     the same with the count already on the host (what a layer costs when the head has
                read all counts back in one copy): masked - no copy = the cost of the D2H copy
    dense       the plain convolution
and the keep fraction at which masked = dense, interpolated between the two measured fractions
that bracket it.  Then the head: eval forward (masked layers, one count copy per forward) and
training-mode forward (dense layers) on random-init weights, and get_bboxes.

Wall-clock time around a synchronised batch of calls (the operator contains a host
synchronisation, so device events alone would not see its cost), in alternating rounds; the median
round is printed with the spread.

    python tools/time_ga.py [--rounds N]"""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'iou-aware-single-stage-object-detector_amd'))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from iouaware import masked_conv  # noqa: E402
from iouaware.config import ConfigDict  # noqa: E402
from iouaware.ga_head import IoUawareGARetinaHead  # noqa: E402

ROUNDS = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 7
SIZES = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
FRACS = [0.01, 0.10, 0.50, 1.00]


def once(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def alternate(fns, n=10):
    """{name: fn} -> {name: (median us, min, max)}: every round times each fn once, in turn"""
    for fn in fns.values():
        fn(); fn()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(once(fn, n))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def show(r, k):
    m, lo, hi = r[k]
    return '%8.1f [%7.1f..%7.1f]' % (m, lo, hi)


def main():
    dev = 'cuda'
    cl = torch.channels_last
    print('batch 1, %d alternating rounds; us per call: median [min..max]' % ROUNDS)
    g = torch.Generator(device=dev).manual_seed(1)
    w = torch.randn(80, 256, 3, 3, device=dev, generator=g) * 0.01
    b = torch.randn(80, device=dev, generator=g)
    packed = masked_conv.pack_weight(w, b)
    for (H, W) in SIZES:
        x = torch.randn(1, 256, H, W, device=dev, generator=g).contiguous(memory_format=cl)
        rnd = torch.rand(1, H, W, device=dev, generator=g)
        res = {}
        with torch.no_grad():
            for f in FRACS:
                mask = rnd < f

                def masked():
                    return masked_conv.masked_conv_packed(x, masked_conv.compact_mask(mask), packed, 3)

                kept = int(mask.sum())

                def no_copy():
                    return masked_conv.masked_conv_packed(x, masked_conv.compact_mask(mask).set_n(kept), packed, 3)

                res[f] = alternate({'masked': masked, 'no copy': no_copy,
                                    'dense': lambda: F.conv2d(x, w, b, padding=1)})
                print('%3d x %3d  keep %5.1f %% (%5d rows)  masked %s  no copy %s  dense %s'
                      % (H, W, 100 * f, kept, show(res[f], 'masked'), show(res[f], 'no copy'), show(res[f], 'dense')))
        cross = None
        for f0, f1 in zip(FRACS[:-1], FRACS[1:]):
            d0 = res[f0]['masked'][0] - res[f0]['dense'][0]
            d1 = res[f1]['masked'][0] - res[f1]['dense'][0]
            if d0 < 0 <= d1:
                cross = f0 + (f1 - f0) * (-d0) / (d1 - d0)
        if cross is None:
            cross = 'above 100 %' if res[FRACS[-1]]['masked'][0] < res[FRACS[-1]]['dense'][0] else 'below 1 %'
        else:
            cross = 'about %.0f %%' % (100 * cross)
        print('%3d x %3d  the masked route stops paying at a keep fraction %s' % (H, W, cross))
    # ---- the whole head
    torch.manual_seed(0)
    head = IoUawareGARetinaHead(81, 256, stacked_convs=4, feat_channels=256, octave_base_scale=4,
                                anchor_strides=[8, 16, 32, 64, 128],
                                loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25,
                                              loss_weight=1.0),
                                loss_bbox=dict(type='SmoothL1Loss', beta=0.04, loss_weight=1.0))
    head.init_weights()
    head = head.to(dev).to(memory_format=cl)
    feats = [torch.randn(1, 256, H, W, device=dev, generator=g).contiguous(memory_format=cl) for (H, W) in SIZES]
    cfg = ConfigDict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_thr=0.5),
                     max_per_img=100)
    meta = [dict(img_shape=(800, 1333, 3), scale_factor=1.0, pad_shape=(800, 1344, 3))]
    with torch.no_grad():
        head.eval()
        outs = head(feats)
        fr = [float(head.loc_mask(lo).float().mean()) for lo in outs[4]]
        print('head, random init: keep fraction per level ' + ' '.join('%.0f %%' % (100 * f) for f in fr))

        def fwd_eval():
            head.eval()
            return head(feats)

        def fwd_dense():
            head.train()
            return head(feats)

        def decode():
            head.eval()
            return head.get_bboxes_batched(*outs, meta, cfg, False)

        r = alternate({'eval': fwd_eval, 'dense': fwd_dense, 'get_bboxes': decode}, n=5)
        head.eval()
    print('head forward, masked layers (eval) %s   dense layers (training mode) %s   get_bboxes %s'
          % (show(r, 'eval'), show(r, 'dense'), show(r, 'get_bboxes')))


if __name__ == '__main__':
    main()
