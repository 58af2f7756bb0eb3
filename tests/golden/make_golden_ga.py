"""Generate the guided-anchor fixtures tests/golden/ga_*.{npz,json} by running the REFERENCE
IoUawareGARetinaHead (imported read-only through ref_shim.py) on seeded synthetic inputs.  Runs only
in the build container:

    python tests/golden/make_golden_ga.py [config get_bboxes forward]

ref_shim.py's DeformConv and MaskedConv2d are empty dummies; after the import this generator binds
CPU stand-ins of its own to those names in the two reference head modules: DeformConv on
tests/dcn_ref.py, MaskedConv2d as a convolution whose output is zeroed where the mask is false.
Fixtures hold seeds, settings and recorded outputs -- never reference source.  Inputs are regenerated
from the seeds by tests/ga_ref.py.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))
import ref_shim  # noqa: E402

ref_shim.install()
import dcn_ref  # noqa: E402
import ga_ref  # noqa: E402

import mmdet.models.anchor_heads.guided_anchor_head as ref_ga  # noqa: E402
import mmdet.models.anchor_heads.iou_aware_ga_retina_head as ref_iga  # noqa: E402
from mmdet.models import build_detector  # noqa: E402

MARGIN = 1e-5          # relative, for every decision of the get_bboxes fixture (make_golden_retina_plain.py)
CONFIG = ref_shim.REF + '/configs/guided_anchoring/ga_retinanet_r50_caffe_fpn_1x.py'


class DeformConvCPU(nn.Module):
    """DCN v1 layer without bias on tests/dcn_ref.py"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 deformable_groups=1, bias=False):
        super().__init__()
        assert not bias and groups == 1
        self.stride, self.padding, self.dilation, self.dg = stride, padding, dilation, deformable_groups
        self.weight = nn.Parameter(torch.zeros(out_channels, in_channels, kernel_size, kernel_size))

    def forward(self, x, offset):
        return dcn_ref.deform_conv(x, offset, self.weight, self.stride, self.padding, self.dilation, self.dg)


class MaskedConv2dCPU(nn.Conv2d):
    """a convolution whose output is zeroed where the (1, H, W) mask is false"""

    def forward(self, input, mask=None):
        y = super().forward(input)
        return y if mask is None else torch.where(mask[:, None], y, torch.zeros((), dtype=y.dtype))


for mod in (ref_ga, ref_iga):
    mod.MaskedConv2d = MaskedConv2dCPU
ref_ga.DeformConv = DeformConvCPU


def plain(v):
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple, range)):
        return [plain(x) for x in v]
    return v


def gen_config():
    """the GA-RetinaNet config with the head type swapped, and the detector's parameter names / shapes"""
    cfg = ref_shim.load_config(CONFIG)
    cfg.model['pretrained'] = None
    cfg.model['bbox_head']['type'] = 'IoUawareGARetinaHead'
    torch.manual_seed(0)
    m = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    assert type(m.bbox_head).__name__ == 'IoUawareGARetinaHead'
    out = dict(model=plain(cfg.model), test_cfg=plain(cfg.test_cfg),
               state_dict=[[k, list(v.shape)] for k, v in m.state_dict().items()])
    path = os.path.join(HERE, 'ga_ref.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, sort_keys=True, separators=(',', ':'))
    print('wrote %s (%d state-dict entries, %.1f KB)' % (path, len(out['state_dict']), os.path.getsize(path) / 1024))


def _head(**kw):
    args = dict(ga_ref.FWD_HEAD, in_channels=256, feat_channels=256, anchor_strides=[8, 16, 32, 64, 128])
    args.update(kw)
    return ref_iga.IoUawareGARetinaHead(**args).eval()


def _iou(b):
    x1, y1, x2, y2 = [b[:, k].astype(np.float64) for k in range(4)]
    ar = (x2 - x1 + 1) * (y2 - y1 + 1)
    ww = np.maximum(0, np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]) + 1)
    hh = np.maximum(0, np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]) + 1)
    return ww * hh / (ar[:, None] + ar[None] - ww * hh)


def _run_ref(head, maps, b, meta, cfg, rescale):
    """reference get_bboxes for image b -> (dets, labels, candidate boxes, candidate scores)"""
    seen = []
    orig = ref_iga.multiclass_nms

    def capture(multi_bboxes, multi_scores, *a, **k):
        seen.append((multi_bboxes.numpy().copy(), multi_scores.numpy().copy()))
        return orig(multi_bboxes, multi_scores, *a, **k)
    ref_iga.multiclass_nms = capture
    try:
        with torch.no_grad():
            per = [[torch.from_numpy(m[b:b + 1]) for m in kind] for kind in maps]
            dets, labels = head.get_bboxes(*per, [torch.zeros(0, 4)], [torch.zeros(0, dtype=torch.long)],
                                           [meta], cfg, rescale)[0]
    finally:
        ref_iga.multiclass_nms = orig
    assert len(seen) == 1
    return dets.numpy(), labels.numpy(), seen[0][0], seen[0][1]


def _margins(maps, b, meta, nms_pre, score_thr, boxes, scores, kept_dets, kept_labels, max_per_img):
    """relative margins of every decision: the keep threshold, each level's top-k cut (row maxima of
    the kept locations), every candidate score against score_thr, the IoU of every NMS survivor
    against every lower-scored box of its class, the max_per_img cut"""
    out = [np.inf]
    thr = ga_ref.LOC_FILTER_THR
    for lo in maps[4]:
        s = torch.from_numpy(lo[b]).sigmoid().double().numpy()
        out.append((np.abs(s - thr) / thr).min())
    per = [[torch.from_numpy(m[b]) for m in kind] for kind in maps]
    rowmax = ga_ref.candidates_single(*per, meta['img_shape'], nms_pre)[3]
    for m in rowmax:
        m = np.sort(m.double().numpy())[::-1]
        if 0 < nms_pre < m.size:
            out.append((m[nms_pre - 1] - m[nms_pre]) / m[nms_pre - 1])
    sc = scores[:, 1:].astype(np.float64)
    out.append((np.abs(sc - score_thr) / score_thr).min())
    for c in np.unique(kept_labels):
        rows = np.nonzero(sc[:, c] > score_thr)[0]
        kept = kept_dets[kept_labels == c]
        for k in range(kept.shape[0]):
            lower = rows[sc[rows, c] < kept[k, 4]]
            if lower.size:
                ov = _iou(np.concatenate([kept[k:k + 1, :4], boxes[lower]]))[0, 1:]
                out.append(np.abs(ov - 0.5).min() / 0.5)
    srt = np.sort(kept_dets[:, 4].astype(np.float64))[::-1]
    if srt.size > max_per_img:
        out.append((srt[max_per_img - 1] - srt[max_per_img]) / srt[max_per_img - 1])
    return float(min(out))


def gen_get_bboxes():
    head = _head()
    arrs = {}
    cover = dict(over=False, under=False, none=False, masks_differ=False, clip=False, below_max=False, cut=False)
    for k, case in enumerate(ga_ref.GA_CASES):
        seed, B, ph, pw, nms_pre, max_per_img, rescale, sf = case[:8]
        maps = ga_ref.ga_head_outputs(k)
        metas = ga_ref.case_metas(k)
        cfg = ref_shim.to_cfg(dict(nms_pre=nms_pre, min_bbox_size=0, score_thr=0.05,
                                   nms=dict(type='nms', iou_thr=0.5), max_per_img=max_per_img))
        mine = ga_ref.get_bboxes(maps, metas, rescale, nms_pre, 0.05, 0.5, max_per_img)
        kept = [[int(ga_ref.keep_mask(torch.from_numpy(lo[b])).sum()) for lo in maps[4]] for b in range(B)]
        print('case %d: kept per image and level %s' % (k, kept))
        for b in range(B):
            for n in kept[b]:
                cover['over'] |= n > nms_pre
                cover['under'] |= 0 < n < nms_pre
                cover['none'] |= n == 0
            if b > 0:
                cover['masks_differ'] |= any(
                    not np.array_equal(ga_ref.keep_mask(torch.from_numpy(lo[0])).numpy(),
                                       ga_ref.keep_mask(torch.from_numpy(lo[b])).numpy()) for lo in maps[4])
            dets, labels, boxes, scores = _run_ref(head, maps, b, metas[b], cfg, rescale)
            every, every_l = _run_ref(head, maps, b, metas[b], ref_shim.to_cfg(dict(cfg, max_per_img=100000)),
                                      rescale)[:2]
            m = _margins(maps, b, metas[b], nms_pre, 0.05, boxes, scores, every, every_l, max_per_img)
            print('case %d image %d: %d detections (%d before the cut), decision margin %.1e'
                  % (k, b, len(dets), len(every), m))
            assert len(dets) > 0 and m >= MARGIN
            cover['below_max'] |= len(every) < max_per_img
            cover['cut'] |= len(every) > max_per_img
            # the plain-torch definition of tests/ga_ref.py gives the reference's bits
            d2, l2, i2 = mine[b]
            assert np.array_equal(d2, dets) and np.array_equal(l2, labels), 'ga_ref != reference'
            # a detection from a location whose |shape_pred| lies between the two clips
            off = 0
            for l, sh in enumerate(maps[3]):
                n = sh.shape[2] * sh.shape[3]
                big = np.nonzero(np.abs(sh[b]).reshape(2, -1).max(0) > ga_ref.CLIP_BOX)[0] + off
                cover['clip'] |= bool(np.isin(i2, big).any())
                off += n
            arrs['dets_%d_%d' % (k, b)] = dets.astype(np.float32)
            arrs['labels_%d_%d' % (k, b)] = labels.astype(np.int64)
            arrs['ids_%d_%d' % (k, b)] = i2.astype(np.int64)
        arrs['case_%d' % k] = np.array([seed, B, ph, pw, nms_pre, max_per_img, int(rescale)], np.int64)
        arrs['sf_%d' % k] = np.array(sf, np.float32)
    print('coverage', cover)
    assert all(cover.values()), cover
    path = os.path.join(HERE, 'ga_get_bboxes.npz')
    np.savez_compressed(path, **arrs)
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


def gen_forward():
    """the reference head's eval forward at batch 1 on small seeded features, name-seeded weights:
    in fp32 (the recorded reference) and, the same head and tensors converted, in fp64 (the
    yardstick of the GPU test's gates: <name>_<level>_f64)"""
    head = ref_iga.IoUawareGARetinaHead(**ga_ref.FWD_HEAD).eval()
    head.load_state_dict(ga_ref.fill_head_state(head.state_dict(), ga_ref.FWD['seed']))
    feats = ga_ref.forward_features()
    with torch.no_grad():
        outs = head([torch.from_numpy(f) for f in feats])
        outs64 = head.double()([torch.from_numpy(f).double() for f in feats])
    arrs = {}
    thr = ga_ref.LOC_FILTER_THR
    for l in range(len(feats)):
        assert torch.equal(outs64[4][l].sigmoid() >= thr, outs[4][l].sigmoid() >= thr)      # the same mask
        for name, o in zip(ga_ref.FWD_MAPS, outs64):
            arrs['%s_%d_f64' % (name, l)] = o[l].numpy().astype(np.float64)
        s = outs[4][l].sigmoid().double().numpy()
        frac = float((s >= thr).mean())
        m = float((np.abs(s - thr) / thr).min())
        print('level %d: %.0f %% of the locations kept, mask margin %.1e' % (l, 100 * frac, m))
        assert 0.05 <= frac <= 0.95 and m >= MARGIN
        for name, o in zip(ga_ref.FWD_MAPS, outs):
            arrs['%s_%d' % (name, l)] = o[l].numpy().astype(np.float32)
    path = os.path.join(HERE, 'ga_forward.npz')
    np.savez_compressed(path, **arrs)
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    which = sys.argv[1:] or ['config', 'get_bboxes', 'forward']
    for w in which:
        dict(config=gen_config, get_bboxes=gen_get_bboxes, forward=gen_forward)[w]()
