"""Generate the plain RetinaNet fixtures tests/golden/retina_plain_*.{npz,json} by running the
REFERENCE RetinaHead (imported read-only through ref_shim.py, as make_golden_fcos_plain.py does)
on seeded synthetic inputs.  Runs only in the build container:

    python tests/golden/make_golden_retina_plain.py [config get_bboxes]

Fixtures hold seeds, settings and recorded outputs -- never reference source.  Inputs are
regenerated from the seeds by tests/synth.py.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))
import make_golden_fcos as mgf  # noqa: E402  (installs ref_shim; its plain helper)
import ref_shim  # noqa: E402
import synth  # noqa: E402

from mmdet.models import build_detector  # noqa: E402
from mmdet.models.anchor_heads.retina_head import RetinaHead  # noqa: E402
import mmdet.models.anchor_heads.anchor_head as ref_anchor_head  # noqa: E402

CONFIGS = ['retinanet_r18_fpn_1x', 'retinanet_r50_fpn_1x', 'retinanet_r50_fpn_1x_2gpu',
           'retinanet_r50_fpn_1x_4gpu', 'retinanet_r101_fpn_1x', 'retinanet_r101_fpn_1x_2gpu',
           'retinanet_x101_32x4d_fpn_1x', 'retinanet_x101_32x4d_fpn_1x_2gpu',
           'retinanet_x101_64x4d_fpn_1x']
MARGIN = 1e-5          # relative, for every decision of the get_bboxes fixture
# (seed, batch, pad h, pad w, nms_pre, rescale, scale factors): nms_pre below the small level
# sizes (top-k cut on every level but the last one or two)
CASES = [(1301, 2, 128, 192, 150, True, [0.75, 1.5]), (1302, 1, 64, 96, 60, False, [1.0])]


def ref_model(name):
    cfg = ref_shim.load_config(ref_shim.REF + '/configs/%s.py' % name)
    cfg.model['pretrained'] = None
    torch.manual_seed(0)
    return cfg, build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)


def gen_config():
    """per config: the model / train / test settings and the detector's parameter names / shapes"""
    out = {}
    for name in CONFIGS:
        cfg, m = ref_model(name)
        assert type(m.bbox_head).__name__ == 'RetinaHead'
        out[name] = dict(model=mgf.plain(cfg.model), train_cfg=mgf.plain(cfg.train_cfg),
                         test_cfg=mgf.plain(cfg.test_cfg),
                         state_dict=[[k, list(v.shape)] for k, v in m.state_dict().items()])
        print('%s: %d state-dict entries' % (name, len(out[name]['state_dict'])))
    path = os.path.join(HERE, 'retina_plain_ref.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, sort_keys=True, separators=(',', ':'))
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


def _iou(b):
    x1, y1, x2, y2 = [b[:, k].astype(np.float64) for k in range(4)]
    ar = (x2 - x1 + 1) * (y2 - y1 + 1)
    ww = np.maximum(0, np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]) + 1)
    hh = np.maximum(0, np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]) + 1)
    return ww * hh / (ar[:, None] + ar[None] - ww * hh)


def _margins(cls, b, nms_pre, score_thr, boxes, scores, kept_dets, kept_labels, all_scores,
             max_per_img):
    """relative margins of the decisions the result depends on, from the reference's own fp32
    intermediates (boxes (R,4), scores (R,C+1) of the candidates, what get_bboxes_single hands to
    multiclass_nms): the per-level top-k cut (scores sigmoid(cls).max over classes), every
    candidate score against score_thr, the IoU of every box the NMS keeps (kept_dets / kept_labels:
    all survivors, before the max_per_img cut) against every lower-scored box of its class (the
    suppression decisions), and the max_per_img cut between the scores of the survivors ranked
    max_per_img and max_per_img + 1 (all_scores)"""
    out = [np.inf]
    for c in cls:
        s = torch.from_numpy(c[b]).permute(1, 2, 0).reshape(-1, synth.C).sigmoid()
        m = s.max(1)[0].double().sort(descending=True)[0].numpy()
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
    srt = np.sort(all_scores.astype(np.float64))[::-1]
    if srt.size > max_per_img:
        out.append((srt[max_per_img - 1] - srt[max_per_img]) / srt[max_per_img - 1])
    return float(min(out))


def _run_ref(head, cls, reg, b, meta, cfg, rescale):
    """reference get_bboxes for image b -> (dets, labels, candidate boxes, candidate scores)"""
    seen = []
    orig = ref_anchor_head.multiclass_nms

    def capture(multi_bboxes, multi_scores, *a, **k):
        seen.append((multi_bboxes.numpy().copy(), multi_scores.numpy().copy()))
        return orig(multi_bboxes, multi_scores, *a, **k)
    ref_anchor_head.multiclass_nms = capture
    try:
        with torch.no_grad():
            dets, labels = head.get_bboxes([torch.from_numpy(c[b:b + 1]) for c in cls],
                                           [torch.from_numpy(r[b:b + 1]) for r in reg],
                                           [torch.zeros(0, 4)], [torch.zeros(0, dtype=torch.long)],
                                           [meta], cfg, rescale)[0]
    finally:
        ref_anchor_head.multiclass_nms = orig
    assert len(seen) == 1
    return dets.numpy(), labels.numpy(), seen[0][0], seen[0][1]


def gen_get_bboxes():
    kw = dict(num_classes=81, in_channels=256, stacked_convs=4, feat_channels=256,
              octave_base_scale=4, scales_per_octave=3, anchor_ratios=[0.5, 1.0, 2.0],
              anchor_strides=[8, 16, 32, 64, 128], target_means=[.0] * 4, target_stds=[1.0] * 4,
              loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25,
                            loss_weight=1.0),
              loss_bbox=dict(type='SmoothL1Loss', beta=0.11, loss_weight=1.0))
    head = RetinaHead(**kw).eval()
    arrs = {}
    for k, (seed, B, ph, pw, nms_pre, rescale, sf) in enumerate(CASES):
        cls, reg, _ = synth.head_outputs(seed, B, ph, pw, 'A')
        cfg = ref_shim.to_cfg(dict(nms_pre=nms_pre, min_bbox_size=0, score_thr=0.05,
                                   nms=dict(type='nms', iou_thr=0.5), max_per_img=100))
        metas = [dict(img_shape=(ph - 9 * b, pw - 13 * b, 3), scale_factor=sf[b],
                      pad_shape=(ph, pw, 3)) for b in range(B)]
        for b in range(B):
            dets, labels, boxes, scores = _run_ref(head, cls, reg, b, metas[b], cfg, rescale)
            # the same call without the max_per_img cut: every survivor of the NMS
            every, every_l = _run_ref(head, cls, reg, b, metas[b],
                                      ref_shim.to_cfg(dict(cfg, max_per_img=100000)), rescale)[:2]
            m = _margins(cls, b, nms_pre, 0.05, boxes, scores, every, every_l, every[:, 4], 100)
            print('case %d image %d: %d detections (%d before the cut), decision margin %.1e'
                  % (k, b, len(dets), len(every), m))
            assert len(dets) > 0 and m >= MARGIN
            arrs['dets_%d_%d' % (k, b)] = dets.astype(np.float32)
            arrs['labels_%d_%d' % (k, b)] = labels.astype(np.int64)
        arrs['case_%d' % k] = np.array([seed, B, ph, pw, nms_pre, int(rescale)], np.int64)
        arrs['sf_%d' % k] = np.array(sf, np.float32)
    path = os.path.join(HERE, 'retina_plain_get_bboxes.npz')
    np.savez_compressed(path, **arrs)
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    which = sys.argv[1:] or ['config', 'get_bboxes']
    for w in which:
        dict(config=gen_config, get_bboxes=gen_get_bboxes)[w]()
