"""Time the FCOS whole path (backbone -> FPN -> head -> ia_point_get_bboxes, or for the plain
FCOSHead with --head plain ia_point_ctr_get_bboxes) at batch 8,
1333 x 800 (800 x 1344 padded), fp32: the module route (torch GroupNorm towers, MIOpen
convolutions) against the fused route (fuse_inference(winograd=True), channels-last: Winograd
towers + the HIP GroupNorm + ReLU), and the GroupNorm kernels alone on one tower layer's
activations (both towers, 512 channels, all five levels) with their share of the HBM bound.

    python tools/time_fcos.py [--head {iou_aware,plain}] [--batch 8] [--iters 20] [--warmup 5]
                              [--dtype {fp32,bf16}] [--out results.json]

--dtype bf16 times three variants in alternation, three runs each (medians and their range): the
fused fp32 route; the bf16 network (fuse_inference(winograd=True), channels-last, .to(bfloat16))
with the head on the module forward (eager bf16 convolutions, torch GroupNorm / ReLU); and the same
network with the bf16 head route (conv3x3_bf16.Bf16ConvFCOSHead).  Both bf16 variants decode their
bf16 maps with the bf16 point entries.  Then the bf16 GroupNorm pair alone.

Device events around the timed window, after warm-up of every shape; the detections of the two
routes are compared on the same input (name-seeded weights, tests/synth_fcos.py)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
for p in (os.path.join(ROOT, 'iou-aware-single-stage-object-detector_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

HBM_PEAK = 8.0e12            # MI355X HBM3E, spec (bytes / s)


HEADS = dict(iou_aware='IoUawareFCOSHead', plain='FCOSHead')


def build(seed=5, head='iou_aware'):
    import iouaware
    from iouaware.config import ConfigDict
    import synth_fcos
    model = dict(
        type='FCOS', pretrained=None,
        backbone=dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3),
                      frozen_stages=1, norm_cfg=dict(type='BN', requires_grad=False), style='caffe'),
        neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1,
                  add_extra_convs=True, extra_convs_on_inputs=False, num_outs=5,
                  relu_before_extra_convs=True),
        bbox_head=dict(type=HEADS[head], num_classes=81, in_channels=256, stacked_convs=4,
                       feat_channels=256, strides=[8, 16, 32, 64, 128]))
    test_cfg = dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_thr=0.5),
                    max_per_img=100)
    m = iouaware.build_detector(ConfigDict(model), test_cfg=ConfigDict(test_cfg))
    state = m.state_dict()
    synth_fcos.fill_state(state, seed)
    m.load_state_dict(state)
    return m.cuda().eval()


def time_fn(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main_bf16(a):
    """the three variants of --dtype bf16, alternating"""
    import synth_fcos
    from iouaware import fcos_ops
    from iouaware.fuse import fuse_inference
    B, pad_h, pad_w = a.batch, 800, 1344
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.standard_normal((B, 3, pad_h, pad_w)).astype(np.float32)).cuda()
    x = x.contiguous(memory_format=torch.channels_last)
    xb = x.to(torch.bfloat16)
    meta = [dict(ori_shape=(800, 1333, 3), img_shape=(800, 1333, 3), pad_shape=(pad_h, pad_w, 3),
                 scale_factor=1.0, flip=False)] * B
    res = dict(batch=B, pad=[pad_h, pad_w], dtype='bf16', head=a.head)
    m32, mb = build(head=a.head), build(head=a.head)
    with torch.no_grad():
        fuse_inference(m32, winograd=True)
        fuse_inference(mb, winograd=True)
        mb = mb.to(memory_format=torch.channels_last).to(torch.bfloat16)
        head = mb.bbox_head
        mb.simple_test_device(xb, meta, rescale=True)            # folds and packs the bf16 runner
        runner = head._ia_c3
        assert runner and runner.calls == 1, 'the bf16 head route was not taken'

        def bf16_run(route):
            head._ia_c3 = runner if route else False             # False: the module forward
            return mb.simple_test_device(xb, meta, rescale=True)
        variants = [('fused_fp32_ms', lambda: m32.simple_test_device(x, meta, rescale=True)),
                    ('bf16_module_head_ms', lambda: bf16_run(False)),
                    ('bf16_head_route_ms', lambda: bf16_run(True))]
        for name, _ in variants:
            res[name] = []
        for _ in range(3):
            for name, fn in variants:
                res[name].append(time_fn(fn, a.iters, a.warmup)[0])
        calls = runner.calls
        _, _, _, n_mod = bf16_run(False)
        assert runner.calls == calls
        _, _, _, n_new = bf16_run(True)
        assert runner.calls == calls + 1
        _, _, _, n32 = m32.simple_test_device(x, meta, rescale=True)
        res['num_dets'] = dict(fp32=n32.tolist(), bf16_module_head=n_mod.tolist(),
                               bf16_head_route=n_new.tolist())
        sizes = synth_fcos.level_shapes(pad_h, pad_w)
        acts = [torch.randn((B, 512, h, w), device='cuda').to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last) for (h, w) in sizes]
        gamma, beta = torch.ones(512, device='cuda'), torch.zeros(512, device='cuda')
        act_bytes = sum(t.numel() for t in acts) * 2
        med, lo, hi = time_fn(lambda: fcos_ops.groupnorm_relu_(acts, gamma, beta, 64), a.iters * 5,
                              a.warmup)
        res['gn_layer_us'] = [med * 1e3, lo * 1e3, hi * 1e3]
        res['gn_activation_mb'] = act_bytes / 1e6
        res['gn_hbm_fraction'] = 3 * act_bytes / HBM_PEAK / (med * 1e-3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--head', choices=sorted(HEADS), default='iou_aware')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--dtype', choices=('fp32', 'bf16'), default='fp32')
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_fcos.py needs the MI355X')
    if a.dtype == 'bf16':
        res = main_bf16(a)
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as fh:
                json.dump(res, fh, indent=1)
        return
    import synth_fcos
    from iouaware import fcos_ops
    from iouaware.fuse import fuse_inference
    B, pad_h, pad_w = a.batch, 800, 1344
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.standard_normal((B, 3, pad_h, pad_w)).astype(np.float32)).cuda()
    meta = [dict(ori_shape=(800, 1333, 3), img_shape=(800, 1333, 3), pad_shape=(pad_h, pad_w, 3),
                 scale_factor=1.0, flip=False)] * B
    res = dict(batch=B, pad=[pad_h, pad_w])
    if a.head != 'iou_aware':
        res['head'] = a.head
    m = build(head=a.head)
    with torch.no_grad():
        run = lambda xx: m.simple_test_device(xx, meta, rescale=True)    # noqa: E731
        res['module_ms'] = time_fn(lambda: run(x), a.iters, a.warmup)
        d0, l0, _, n0 = run(x)
        fuse_inference(m, winograd=True)
        xc = x.contiguous(memory_format=torch.channels_last)
        res['fused_ms'] = time_fn(lambda: run(xc), a.iters, a.warmup)
        d1, l1, _, n1 = run(xc)
        assert m.bbox_head._ia_wino.calls > 0
        torch.cuda.synchronize()
        res['num_dets'] = [n0.tolist(), n1.tolist()]
        same = [int(min(p, q)) for p, q in zip(n0.tolist(), n1.tolist())]
        res['max_det_diff'] = max(float((d0[b, :k] - d1[b, :k]).abs().max()) if k else 0.0
                                  for b, k in enumerate(same))
        if a.head != 'iou_aware':
            # rank-wise score difference: insensitive to the order of near-equal scores (the plain
            # head's products are close together, neighbours can swap between the routes)
            res['max_sorted_score_diff'] = max(
                float((d0[b, :k, 4].sort()[0] - d1[b, :k, 4].sort()[0]).abs().max()) if k else 0.0
                for b, k in enumerate(same))
        # GroupNorm + ReLU alone: one tower layer (both towers, 512 channels, five levels)
        sizes = synth_fcos.level_shapes(pad_h, pad_w)
        acts = [torch.randn((B, 512, h, w), device='cuda').contiguous(memory_format=torch.channels_last)
                for (h, w) in sizes]
        gamma, beta = torch.ones(512, device='cuda'), torch.zeros(512, device='cuda')
        act_bytes = sum(t.numel() for t in acts) * 4
        med, lo, hi = time_fn(lambda: fcos_ops.groupnorm_relu_(acts, gamma, beta, 64), a.iters * 5,
                              a.warmup)
        res['gn_layer_us'] = [med * 1e3, lo * 1e3, hi * 1e3]
        res['gn_activation_mb'] = act_bytes / 1e6
        # three passes (stats read, apply read + write) over the activation
        res['gn_hbm_fraction'] = 3 * act_bytes / HBM_PEAK / (med * 1e-3)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
