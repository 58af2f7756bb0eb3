"""Generate the IoU-aware FCOS fixtures tests/golden/fcos_*.{npz,json} by running the REFERENCE
(imported read-only through ref_shim.py, as make_golden.py does) on seeded synthetic inputs.
Runs only in the build container:

    python tests/golden/make_golden_fcos.py

Fixtures hold seeds, settings and recorded outputs -- never reference source.  Inputs are
regenerated from the seeds by tests/synth_fcos.py.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))
import ref_shim  # noqa: E402
import synth_fcos  # noqa: E402

ref_shim.install()
from mmdet.core import distance2bbox  # noqa: E402
from mmdet.models import build_detector  # noqa: E402
import mmdet.core.loss.losses as ref_losses  # noqa: E402
import mmdet.models.anchor_heads.iou_aware_fcos_head as ref_fcos_mod  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)
CONFIG = ref_shim.REF + '/configs/fcos/iou_aware_fcos_r50_caffe_fpn_gn_1x_4gpu.py'


def save(name, **arrs):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **arrs)
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


def plain(v):
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple, range)):
        return [plain(x) for x in v]
    return v


def ref_model(seed=None):
    cfg = ref_shim.load_config(CONFIG)
    cfg.model['pretrained'] = None
    torch.manual_seed(0)
    m = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    if seed is not None:
        state = m.state_dict()
        synth_fcos.fill_state(state, seed)
        m.load_state_dict(state)
    return cfg, m


def gen_config():
    """the config's settings (JSON) and the detector's parameter names / shapes"""
    cfg, m = ref_model()
    out = dict(config=plain(cfg), state_dict=[[k, list(v.shape)] for k, v in m.state_dict().items()])
    with open(os.path.join(HERE, 'fcos_ref.json'), 'w') as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
    print('wrote fcos_ref.json (%d parameters)' % len(out['state_dict']))


def gen_helpers():
    """get_points, distance2bbox (with / without max_shape), fcos_target, centerness_target"""
    _, m = ref_model()
    head = m.bbox_head
    out = {}
    sizes = synth_fcos.level_shapes(200, 264)
    pts = head.get_points(sizes, torch.float32, 'cpu')
    for l, p in enumerate(pts):
        out['points_%d' % l] = p.numpy()
    rs = np.random.RandomState(11)
    n = 512
    p = np.stack([rs.uniform(0, 300, n), rs.uniform(0, 220, n)], 1).astype(np.float32)
    d = np.exp(rs.standard_normal((n, 4)) * 1.0 + 2.5).astype(np.float32)
    out.update(d2b_points=p, d2b_dist=d,
               d2b_free=distance2bbox(torch.from_numpy(p), torch.from_numpy(d)).numpy(),
               d2b_clamped=distance2bbox(torch.from_numpy(p), torch.from_numpy(d),
                                         max_shape=(200, 264, 3)).numpy())
    # gts: nested boxes (points in several gts), a box whose largest distance hits a range edge
    # exactly (64 from a point at 36: x2 = 36 + 64), a box that contains no point
    gb, gl = synth_fcos.gts(13, 2, 200, 264)
    gb[0] = np.concatenate([gb[0], np.array([[20, 28, 100, 44], [1, 1, 2, 2]], np.float32)])
    gl[0] = np.concatenate([gl[0], np.array([7, 9], np.int64)])
    labels, targets = head.fcos_target(pts, [torch.from_numpy(b) for b in gb],
                                       [torch.from_numpy(x) for x in gl])
    for i, b in enumerate(gb):
        out['gt_bboxes_%d' % i], out['gt_labels_%d' % i] = b, gl[i]
    for l in range(len(sizes)):
        out['labels_%d' % l] = labels[l].numpy()
        out['bbox_targets_%d' % l] = targets[l].numpy()
    flat_l, flat_t = torch.cat(labels), torch.cat(targets)
    pos = flat_l.nonzero().reshape(-1)
    out['centerness'] = head.centerness_target(flat_t[pos]).numpy()
    out['sizes'] = np.array(sizes, np.int32)
    save('fcos_helpers', **out)


def gen_forward():
    """the head's forward on seeded features with name-seeded weights (CPU)"""
    _, m = ref_model(seed=3)
    head = m.bbox_head.eval()
    sizes = synth_fcos.level_shapes(96, 128)
    rs = np.random.RandomState(4)
    feats = [rs.standard_normal((2, 256, h, w)).astype(np.float32) for (h, w) in sizes]
    with torch.no_grad():
        outs = head([torch.from_numpy(f) for f in feats])
    res = dict(seed=np.int64(3), feat_seed=np.int64(4), sizes=np.array(sizes, np.int32))
    for kind, ts in zip(('cls', 'bbox', 'ctr', 'iou'), outs):
        for l, t in enumerate(ts):
            res['%s_%d' % (kind, l)] = t.numpy()
    save('fcos_forward', **res)


def gen_get_bboxes():
    """get_bboxes on synthetic head outputs (wide spread, min fused-score gap recorded) for
    nms_pre below / above the level sizes, rescale on / off"""
    _, m = ref_model()
    head = m.bbox_head
    pad_h, pad_w = 160, 224
    sizes = synth_fcos.level_shapes(pad_h, pad_w)
    seed = 21
    cls, reg, ctr, iou = synth_fcos.head_outputs(seed, 2, sizes)
    out = dict(seed=np.int64(seed), pad=np.array([pad_h, pad_w], np.int32),
               min_gap=np.float64(synth_fcos.min_score_gap(cls, iou)))
    metas = [dict(img_shape=(150, 213, 3), scale_factor=0.75, pad_shape=(pad_h, pad_w, 3)),
             dict(img_shape=(160, 200, 3), scale_factor=1.25, pad_shape=(pad_h, pad_w, 3))]
    T = lambda xs: [torch.from_numpy(x) for x in xs]   # noqa: E731
    for tag, nms_pre, rescale in (('pre100_r', 100, True), ('pre100', 100, False),
                                  ('pre1000_r', 1000, True)):
        cfg = ref_shim.to_cfg(dict(nms_pre=nms_pre, min_bbox_size=0, score_thr=0.05,
                                   nms=dict(type='nms', iou_thr=0.5), max_per_img=100))
        res = head.get_bboxes(T(cls), T(reg), T(ctr), T(iou), None, None, metas, cfg, rescale)
        for b, (dets, labels) in enumerate(res):
            out['dets_%s_%d' % (tag, b)] = dets.numpy()
            out['labels_%s_%d' % (tag, b)] = labels.numpy()
    save('fcos_get_bboxes', **out)


def gen_e2e():
    """the detector called the way tools/test.py calls it (return_loss=False, rescale=True, the
    fork's gt arguments) on a small image, name-seeded weights; also its head outputs"""
    cfg, m = ref_model(seed=5)
    m.eval()
    img_h, img_w, pad_h, pad_w = 120, 150, 128, 160
    x = synth_fcos.image(6, 1, pad_h, pad_w, img_h, img_w)
    meta = dict(ori_shape=(96, 120, 3), img_shape=(img_h, img_w, 3), pad_shape=(pad_h, pad_w, 3),
                scale_factor=1.25, flip=False)
    gb, gl = synth_fcos.gts(7, 1, img_h, img_w)
    with torch.no_grad():
        res = m(img=[torch.from_numpy(x)], img_meta=[[meta]], return_loss=False, rescale=True,
                gt_bboxes=[[torch.from_numpy(gb[0])]], gt_labels=[[torch.from_numpy(gl[0])]])
        outs = m.bbox_head(m.extract_feat(torch.from_numpy(x)))
    dets = np.concatenate([r for r in res], 0).astype(np.float32)
    labels = np.concatenate([np.full(len(r), c, np.int64) for c, r in enumerate(res)])
    out = dict(weight_seed=np.int64(5), image_seed=np.int64(6), gt_seed=np.int64(7),
               shape=np.array([img_h, img_w, pad_h, pad_w], np.int32), scale_factor=np.float32(1.25),
               dets=dets, labels=labels)
    for kind, ts in zip(('cls', 'bbox', 'ctr', 'iou'), outs):
        for l, t in enumerate(ts):
            out['%s_%d' % (kind, l)] = t.numpy()
    print('e2e: %d detections' % len(dets))
    save('fcos_e2e', **out)


def _focal_op_cpu(pred, target, gamma, alpha, reduction='none'):
    """the CUDA op's quantity on the CPU: py_sigmoid_focal_loss on the one-hot of the integer
    targets (see make_golden.gen_focal_op)"""
    onehot = torch.zeros_like(pred)
    pos = torch.nonzero(target >= 1).squeeze(1)
    onehot[pos, target[pos] - 1] = 1
    return ref_losses.py_sigmoid_focal_loss(pred, onehot, torch.ones_like(pred), gamma=gamma,
                                            alpha=alpha, reduction=reduction)


def gen_train():
    """one training forward + backward of the detector (return_loss=True): the four loss terms and
    the gradient norms of the head and FPN parameters; a case with positives and one without"""
    ref_fcos_mod.sigmoid_focal_loss = _focal_op_cpu
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
    save('fcos_train', **out)


if __name__ == '__main__':
    only = sys.argv[1:]
    for name, fn in (('config', gen_config), ('helpers', gen_helpers), ('forward', gen_forward),
                     ('get_bboxes', gen_get_bboxes), ('e2e', gen_e2e), ('train', gen_train)):
        if not only or name in only:
            fn()
