"""Generate the plain FCOS fixtures tests/golden/fcos_plain_*.{npz,json} by running the REFERENCE
FCOSHead (imported read-only through ref_shim.py, as make_golden_fcos.py does) on seeded
synthetic inputs.  Runs only in the build container:

    python tests/golden/make_golden_fcos_plain.py [config get_bboxes e2e train]

Fixtures hold seeds, settings and recorded outputs -- never reference source.  Inputs are
regenerated from the seeds by tests/synth_fcos.py (and tests/synth_fcos_plain.py).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))
import make_golden_fcos as mgf  # noqa: E402  (installs ref_shim; its plain / save / focal helpers)
import ref_shim  # noqa: E402
import synth_fcos  # noqa: E402
import synth_fcos_plain  # noqa: E402

from mmdet.core import bbox2result  # noqa: E402
from mmdet.models import build_detector  # noqa: E402
import mmdet.models.anchor_heads.fcos_head as ref_plain_mod  # noqa: E402

CONFIGS = ['fcos_r50_caffe_fpn_gn_1x_4gpu', 'fcos_mstrain_640_800_r101_caffe_fpn_gn_2x_4gpu',
           'fcos_mstrain_640_800_x101_64x4d_fpn_gn_2x']
MARGIN = 1e-5          # relative, for every decision of the get_bboxes fixture (as make_golden.py)


def ref_model(name=CONFIGS[0], seed=None):
    cfg = ref_shim.load_config(ref_shim.REF + '/configs/fcos/%s.py' % name)
    cfg.model['pretrained'] = None
    torch.manual_seed(0)
    m = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    if seed is not None:
        state = m.state_dict()
        synth_fcos.fill_state(state, seed)
        m.load_state_dict(state)
    return cfg, m


def gen_config():
    """per config: the model / train / test settings and the detector's parameter names / shapes"""
    out = {}
    for name in CONFIGS:
        cfg, m = ref_model(name)
        out[name] = dict(model=mgf.plain(cfg.model), train_cfg=mgf.plain(cfg.train_cfg),
                         test_cfg=mgf.plain(cfg.test_cfg),
                         state_dict=[[k, list(v.shape)] for k, v in m.state_dict().items()])
        print('%s: %d state-dict entries' % (name, len(out[name]['state_dict'])))
    path = os.path.join(HERE, 'fcos_plain_ref.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, sort_keys=True, separators=(',', ':'))
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


def _iou(b):
    x1, y1, x2, y2 = [b[:, k].astype(np.float64) for k in range(4)]
    ar = (x2 - x1 + 1) * (y2 - y1 + 1)
    ww = np.maximum(0, np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]) + 1)
    hh = np.maximum(0, np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]) + 1)
    return ww * hh / (ar[:, None] + ar[None] - ww * hh)


def _margins(head, cls, reg, ctr, b, meta, cfg, rescale):
    """every decision of get_bboxes_single for image b, recomputed from the reference's own fp32
    intermediates: top-k cut, raw score against score_thr, product order between pairs of a class
    whose boxes overlap above iou_thr (the only pairs whose order NMS reads), IoU against iou_thr,
    the final max_per_img cut.  -> dict of relative margins"""
    sizes = [c.shape[-2:] for c in cls]
    pts = head.get_points(sizes, torch.float32, 'cpu')
    cut, boxes, raw, prod = [], [], [], []
    for l in range(len(cls)):
        s = torch.from_numpy(cls[l][b]).permute(1, 2, 0).reshape(-1, head.cls_out_channels).sigmoid()
        f = torch.from_numpy(ctr[l][b]).permute(1, 2, 0).reshape(-1).sigmoid()
        d = torch.from_numpy(reg[l][b]).permute(1, 2, 0).reshape(-1, 4)
        p = pts[l]
        if 0 < cfg.nms_pre < s.shape[0]:
            ms = (s * f[:, None]).max(dim=1)[0].numpy().astype(np.float64)
            srt = np.sort(ms)[::-1]
            cut.append((srt[cfg.nms_pre - 1] - srt[cfg.nms_pre]) / srt[cfg.nms_pre - 1])
            idx = torch.from_numpy(np.argsort(-ms, kind='stable')[:cfg.nms_pre].copy())
            s, f, d, p = s[idx], f[idx], d[idx], p[idx]
        bb = mgf.distance2bbox(p, d, max_shape=meta['img_shape'])
        if rescale:
            bb = bb / bb.new_tensor(meta['scale_factor'])
        boxes.append(bb.numpy())
        raw.append(s.numpy())
        prod.append((s * f[:, None]).numpy())
    boxes, raw, prod = np.concatenate(boxes), np.concatenate(raw), np.concatenate(prod)
    thr, iou_thr = cfg.score_thr, cfg.nms['iou_thr']
    thr_m = float((np.abs(raw.astype(np.float64) - thr) / thr).min())
    passing = raw > np.float32(thr)
    ov = _iou(boxes)
    np.fill_diagonal(ov, 0.0)
    active = passing.any(1)
    iou_m = float((np.abs(ov[np.ix_(active, active)] - iou_thr) / iou_thr).min())
    order_m = np.inf
    for c in range(raw.shape[1]):
        rows = np.nonzero(passing[:, c])[0]
        if rows.size < 2:
            continue
        pc = prod[rows, c].astype(np.float64)
        near = ov[np.ix_(rows, rows)] > iou_thr
        i, j = np.nonzero(np.triu(near, 1))
        if i.size:
            gap = np.abs(pc[i] - pc[j]) / np.maximum(np.maximum(pc[i], pc[j]), 1e-30)
            order_m = min(order_m, float(gap.min()))
    return dict(topk=min(cut) if cut else np.inf, thr=thr_m, iou=iou_m, order=order_m)


def gen_get_bboxes():
    """FCOSHead.get_bboxes on synthetic head outputs for nms_pre below / above the level sizes and
    rescale on / off, plus a sparse case (class logits shifted down) whose kept detections include
    pairs with raw score > score_thr > product.  The first seed whose every decision margin is
    >= MARGIN (relative) in every case is taken (asserted)."""
    _, m = ref_model()
    head = m.bbox_head
    T = lambda xs: [torch.from_numpy(x) for x in xs]   # noqa: E731
    for seed in range(41, 241):
        out = dict(seed=np.int64(seed))
        ok, below = True, 0
        for tag, pad_h, pad_w, nms_pre, rescale, shift in synth_fcos_plain.GET_BBOXES_CASES:
            sizes = synth_fcos.level_shapes(pad_h, pad_w)
            metas = synth_fcos_plain.get_bboxes_metas(pad_h, pad_w)
            cls, reg, ctr = synth_fcos_plain.head_outputs(seed, 2, sizes, shift)
            cfg = ref_shim.to_cfg(dict(nms_pre=nms_pre, min_bbox_size=0, score_thr=0.05,
                                       nms=dict(type='nms', iou_thr=0.5), max_per_img=100))
            res = head.get_bboxes(T(cls), T(reg), T(ctr), metas, cfg, rescale)
            cfg_all = ref_shim.to_cfg(dict(cfg, max_per_img=1024))
            res_all = head.get_bboxes(T(cls), T(reg), T(ctr), metas, cfg_all, rescale)
            for b, (dets, labels) in enumerate(res):
                out['dets_%s_%d' % (tag, b)] = dets.numpy()
                out['labels_%s_%d' % (tag, b)] = labels.numpy()
                mg = _margins(head, cls, reg, ctr, b, metas[b], cfg, rescale)
                alls = np.sort(res_all[b][0][:, 4].numpy().astype(np.float64))[::-1]
                if alls.size > 100:            # the final max_per_img cut
                    mg['final_cut'] = (alls[99] - alls[100]) / alls[99]
                ok = ok and all(v >= MARGIN for v in mg.values()) and dets.shape[0] > 0
                # kept detections whose product is below score_thr (raw score above it)
                below += int((dets[:, 4] < 0.05).sum())
                print('seed %d %s img %d: %d dets (%d below score_thr), margins %s'
                      % (seed, tag, b, dets.shape[0], int((dets[:, 4] < 0.05).sum()),
                         ', '.join('%s %.1e' % kv for kv in sorted(mg.items()))))
        if ok and below > 0:
            break
    assert ok and below > 0, 'no seed with every decision margin >= %g' % MARGIN
    mgf.save('fcos_plain_get_bboxes', **out)


def gen_e2e():
    """the whole R-50 caffe FCOS + FCOSHead detector on a small image, name-seeded weights.  The
    fork's single_stage.simple_test hands gt_bboxes / gt_labels to get_bboxes, which the plain
    head does not take, so the reference is called the way the upstream simple_test calls it:
    extract_feat -> bbox_head -> get_bboxes(img_meta, test_cfg, rescale=True) -> bbox2result."""
    cfg, m = ref_model(seed=5)
    m.eval()
    img_h, img_w, pad_h, pad_w = 120, 150, 128, 160
    x = synth_fcos.image(6, 1, pad_h, pad_w, img_h, img_w)
    meta = dict(ori_shape=(96, 120, 3), img_shape=(img_h, img_w, 3), pad_shape=(pad_h, pad_w, 3),
                scale_factor=1.25, flip=False)
    with torch.no_grad():
        outs = m.bbox_head(m.extract_feat(torch.from_numpy(x)))
        dets, labels = m.bbox_head.get_bboxes(*(outs + ([meta], m.test_cfg, True)))[0]
        res = bbox2result(dets, labels, m.bbox_head.num_classes)
    dets = np.concatenate([r for r in res], 0).astype(np.float32)
    labels = np.concatenate([np.full(len(r), c, np.int64) for c, r in enumerate(res)])
    out = dict(weight_seed=np.int64(5), image_seed=np.int64(6),
               shape=np.array([img_h, img_w, pad_h, pad_w], np.int32), scale_factor=np.float32(1.25),
               dets=dets, labels=labels)
    for kind, ts in zip(('cls', 'bbox', 'ctr'), outs):
        for l, t in enumerate(ts):
            out['%s_%d' % (kind, l)] = t.numpy()
    print('e2e: %d detections' % len(dets))
    mgf.save('fcos_plain_e2e', **out)


def gen_train():
    """one training forward + backward of the plain detector: the three loss terms and the
    gradient norms of the head and FPN parameters; a case with positives and one without"""
    ref_plain_mod.sigmoid_focal_loss = mgf._focal_op_cpu
    out = {}
    img_h, img_w, pad_h, pad_w = 120, 150, 128, 160
    for tag, gseed in (('pos', 8), ('nopos', None)):
        cfg, m = ref_model(seed=9)
        m.train()
        x = torch.from_numpy(synth_fcos.image(10, 2, pad_h, pad_w, img_h, img_w))
        metas = [dict(ori_shape=(img_h, img_w, 3), img_shape=(img_h, img_w, 3),
                      pad_shape=(pad_h, pad_w, 3), scale_factor=1.0, flip=False)] * 2
        if gseed is not None:
            gb, gl = synth_fcos.gts(gseed, 2, img_h, img_w)
        else:        # boxes between the points of every level: no positives
            gb = [np.array([[0.5, 0.5, 3.0, 3.0]], np.float32)] * 2
            gl = [np.array([3], np.int64)] * 2
        losses = m(img=x, img_meta=metas, gt_bboxes=[torch.from_numpy(b) for b in gb],
                   gt_labels=[torch.from_numpy(b) for b in gl])
        total = sum(v.sum() for v in losses.values())
        total.backward()
        for k, v in losses.items():
            out['%s_%s' % (tag, k)] = v.detach().numpy()
        names, norms = [], []
        for n, p in m.named_parameters():
            if (n.startswith('bbox_head.') or n.startswith('neck.')) and p.grad is not None:
                names.append(n)
                norms.append(float(p.grad.norm()))
        out['%s_grad_names' % tag] = np.array(names)
        out['%s_grad_norms' % tag] = np.array(norms, np.float64)
        if gseed is not None:
            for i, b in enumerate(gb):
                out['%s_gt_bboxes_%d' % (tag, i)], out['%s_gt_labels_%d' % (tag, i)] = b, gl[i]
        print(tag, {k: float(v) for k, v in losses.items()})
    out.update(weight_seed=np.int64(9), image_seed=np.int64(10),
               shape=np.array([img_h, img_w, pad_h, pad_w], np.int32))
    mgf.save('fcos_plain_train', **out)


if __name__ == '__main__':
    only = sys.argv[1:]
    for name, fn in (('config', gen_config), ('get_bboxes', gen_get_bboxes), ('e2e', gen_e2e),
                     ('train', gen_train)):
        if not only or name in only:
            fn()
