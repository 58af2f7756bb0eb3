"""Generate the SSD fixtures tests/golden/ssd_ref.json and ssd_get_bboxes.npz by running the REFERENCE
SSDVGG / SSDHead (imported read-only through ref_shim.py) on seeded synthetic inputs.  Needs the
reference tree at ref_shim.REF:

    python tests/golden/make_golden_ssd.py [config get_bboxes]

mmcv is not installed; ref_shim.py stubs mmcv.cnn.VGG with an empty class.  Before the reference's
ssd_vgg.py is imported this generator puts a VGG-16 stand-in of its own in that place (the 2-2-3-3-3
body as an nn.Sequential `features`: 30 entries without the last pool), so that the reference's own
SSDVGG.__init__ and _make_extra_layers run on it.  The stand-in's layout follows from the indices the
reference uses (features[21] must be conv4_3; its five appended modules land at 30-34); it is not
checked against mmcv itself.
Fixtures hold settings, names, shapes and recorded outputs -- never reference source.  dets_* and labels_*
are the reference's output; ids_* (anchor row ids, which the reference does not return) are those of
tests/ssd_ref.py, written after its dets and labels were found equal to the reference's.  Inputs are
regenerated from the seeds by tests/ssd_ref.py.
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
import ssd_ref  # noqa: E402


class VGGStandIn(nn.Module):
    """what SSDVGG needs of mmcv.cnn.VGG: `features`, depth 16, no batch norm"""

    def __init__(self, depth, with_last_pool=True, ceil_mode=False, out_indices=(0, 1, 2, 3, 4)):
        super().__init__()
        assert depth == 16
        layers, inplanes = [], 3
        for i, n in enumerate((2, 2, 3, 3, 3)):
            planes = 64 * 2 ** i if i < 4 else 512
            for _ in range(n):
                layers += [nn.Conv2d(inplanes, planes, 3, padding=1), nn.ReLU(inplace=True)]
                inplanes = planes
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2, ceil_mode=ceil_mode))
        if not with_last_pool:
            layers.pop(-1)
        self.features = nn.Sequential(*layers)
        self.out_indices = out_indices


assert 'mmdet.models.backbones.ssd_vgg' not in sys.modules
sys.modules['mmcv.cnn'].VGG = VGGStandIn
sys.modules['mmcv'].cnn.VGG = VGGStandIn

import mmdet.models.backbones.ssd_vgg as ref_vgg  # noqa: E402
import mmdet.models.anchor_heads.ssd_head as ref_head  # noqa: E402

assert ref_vgg.VGG is VGGStandIn

CONFIGS = ['ssd300_coco', 'ssd300_coco_2gpu', 'ssd512_coco', 'ssd512_coco_2gpu', 'pascal_voc/ssd300_voc',
           'pascal_voc/ssd300_voc_2gpu', 'pascal_voc/ssd512_voc', 'pascal_voc/ssd512_voc_2gpu']
MARGIN = 1e-5


def plain(v):
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple, range)):
        return [plain(x) for x in v]
    return v


def shapes(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def gen_config():
    out = dict(configs={}, vgg_state={}, head={})
    for name in CONFIGS:
        cfg = ref_shim.load_config('%s/configs/%s.py' % (ref_shim.REF, name))
        out['configs'][name] = dict(model=plain(cfg.model), test_cfg=plain(cfg.test_cfg))
    for size in (300, 512):
        vgg = ref_vgg.SSDVGG(size, 16)
        assert isinstance(vgg.features[21], nn.Conv2d) and vgg.features[21].out_channels == 512
        assert len(vgg.features) == 35
        out['vgg_state'][str(size)] = shapes(vgg)
    for name, s in ssd_ref.ANCHOR_SETTINGS.items():
        head = ref_head.SSDHead(num_classes=81, **s)
        base = [g.base_anchors.numpy() for g in head.anchor_generators]
        mine = ssd_ref.base_anchors(**s)
        assert all(np.array_equal(a, b.numpy()) for a, b in zip(base, mine)), 'ssd_ref anchors != reference'
        out['head'][name] = dict(state=shapes(head), base_anchors=[b.tolist() for b in base])
    path = os.path.join(HERE, 'ssd_ref.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, sort_keys=True, separators=(',', ':'))
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


def _iou64(b):
    x1, y1, x2, y2 = [b[:, k] for k in range(4)]
    ar = (x2 - x1 + 1) * (y2 - y1 + 1)
    ww = np.maximum(0, np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]) + 1)
    hh = np.maximum(0, np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]) + 1)
    return ww * hh / (ar[:, None] + ar[None] - ww * hh)


def _margins(cls, reg, b, meta, rescale, nc):
    """in fp64: the distance of every foreground score from score_thr, and of every IoU between two
    candidates of one class from iou_thr"""
    head = ssd_ref.CASE_HEAD
    base = ssd_ref.base_anchors(**head)
    boxes, scores = ssd_ref.candidates_single([torch.from_numpy(c[b]).double() for c in cls],
                                              [torch.from_numpy(r[b]).double() for r in reg], base,
                                              head['anchor_strides'], nc, head['target_means'],
                                              head['target_stds'], meta['img_shape'])
    if rescale:
        boxes = boxes / boxes.new_tensor(np.asarray(meta['scale_factor'], np.float64).reshape(-1))
    boxes, scores = boxes.numpy(), scores.numpy()[:, 1:]
    m_score = float(np.abs(scores - ssd_ref.SCORE_THR).min())
    m_iou, kept = np.inf, int((scores.max(1) > ssd_ref.SCORE_THR).sum())
    for c in range(scores.shape[1]):
        rows = np.nonzero(scores[:, c] > ssd_ref.SCORE_THR)[0]
        if rows.size > 1:
            ov = _iou64(boxes[rows])
            m_iou = min(m_iou, float(np.abs(ov[np.triu_indices(rows.size, 1)] - ssd_ref.IOU_THR).min()))
    return m_score, m_iou, kept


def gen_get_bboxes():
    arrs = {}
    cfg = ref_shim.to_cfg(dict(nms=dict(type='nms', iou_thr=ssd_ref.IOU_THR), min_bbox_size=0,
                               score_thr=ssd_ref.SCORE_THR, max_per_img=ssd_ref.MAX_PER_IMG))
    for name, case in ssd_ref.CASES.items():
        nc = case['num_classes']
        head = ref_head.SSDHead(num_classes=nc, **ssd_ref.CASE_HEAD).eval()
        cls, reg = ssd_ref.head_outputs(name)
        tc, tr = [torch.from_numpy(c) for c in cls], [torch.from_numpy(r) for r in reg]
        B = len(case['metas'])
        for rescale in case['rescale']:
            with torch.no_grad():
                ref = head.get_bboxes(tc, tr, [torch.zeros(0, 4)] * B, [torch.zeros(0, dtype=torch.long)] * B,
                                      case['metas'], cfg, rescale)
            mine = ssd_ref.get_bboxes(tc, tr, case['metas'], rescale, num_classes=nc)
            for b in range(B):
                dets, labels = ref[b][0].numpy(), ref[b][1].numpy()
                m_score, m_iou, kept = _margins(cls, reg, b, case['metas'][b], rescale, nc)
                print('%s image %d rescale %d: %d rows above score_thr, %d detections, margins score %.1e iou %.1e'
                      % (name, b, rescale, kept, len(dets), m_score, m_iou))
                assert len(dets) > 0 and m_score >= MARGIN and m_iou >= MARGIN
                d2, l2, i2 = mine[b]
                assert np.array_equal(l2, labels) and np.abs(d2 - dets).max() <= 1e-6, 'ssd_ref != reference'
                tag = '%s_%d_%d' % (name, b, int(rescale))
                arrs['dets_' + tag] = dets.astype(np.float32)
                arrs['labels_' + tag] = labels.astype(np.int64)
                arrs['ids_' + tag] = i2.astype(np.int64)
    path = os.path.join(HERE, 'ssd_get_bboxes.npz')
    np.savez_compressed(path, **arrs)
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    which = sys.argv[1:] or ['config', 'get_bboxes']
    for w in which:
        dict(config=gen_config, get_bboxes=gen_get_bboxes)[w]()
