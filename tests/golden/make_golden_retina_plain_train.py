"""Generate tests/golden/retina_plain_train.npz by running the REFERENCE RetinaHead.loss
(anchor_head.py:234-299, imported read-only through ref_shim.py as make_golden_retina_plain.py
does) on the CPU, on seeded synthetic head outputs.  Runs only in the build container:

    python tests/golden/make_golden_retina_plain_train.py

The fixture holds seeds, settings and recorded numbers -- never reference source.  The head outputs
are regenerated from the seed by tests/synth.py (`head_outputs(seed, B, ph, pw, 'A')`; its IoU maps
are ignored).  Keys, per case k:
    case_k             int64 [seed, B, pad h, pad w, img h, img w]
    gt_bboxes_k_b, gt_labels_k_b      ground truth of image b
    loss_cls_k, loss_bbox_k           (5,) fp64, the reference's per-level losses
    num_total_pos_k                   the reference's normaliser
    g_cls_k_l_idx / g_cls_k_l, g_reg_k_l_idx / g_reg_k_l
                       a fixed index subset (<= 3000 entries of the flattened NCHW gradient, every
                       non-zero box gradient first) and the reference's autograd gradient of the
                       sum of all losses there (as losses_small.npz stores them)
and once: gamma, alpha, beta, pos_iou_thr, neg_iou_thr (the train_cfg of
tests/test_gpu_retina_plain.py::test_training_step_on_the_hip_losses).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))
import make_golden_fcos as mgf  # noqa: E402,F401  (installs ref_shim)
import ref_shim  # noqa: E402
import synth  # noqa: E402

from mmdet.models.anchor_heads.retina_head import RetinaHead  # noqa: E402
import mmdet.models.anchor_heads.anchor_head as ref_anchor_head  # noqa: E402

# (seed, batch, pad h, pad w, img h, img w, boxes per image, labels per image)
CASES = [
    # box loss on the three finest levels
    (1401, 2, 128, 192, 120, 180,
     [[[20, 20, 52, 52], [50, 40, 150, 120]], [[5, 5, 185, 125], [100, 30, 164, 94]]],
     [[3, 17], [45, 80]]),
    # one small box: a handful of positives, a small normaliser, another per-image count
    (1402, 1, 64, 96, 64, 96, [[[30, 22, 58, 50]]], [[9]]),
]
N_IDX = 3000


def gen():
    kw = dict(num_classes=81, in_channels=256, stacked_convs=4, feat_channels=256,
              octave_base_scale=4, scales_per_octave=3, anchor_ratios=[0.5, 1.0, 2.0],
              anchor_strides=[8, 16, 32, 64, 128], target_means=[.0] * 4, target_stds=[1.0] * 4,
              loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25,
                            loss_weight=1.0),
              loss_bbox=dict(type='SmoothL1Loss', beta=0.11, loss_weight=1.0))
    head = RetinaHead(**kw)
    train_cfg = ref_shim.to_cfg(dict(
        assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0,
                      ignore_iof_thr=-1),
        allowed_border=-1, pos_weight=-1, debug=False))
    out = dict(gamma=np.float32(2.0), alpha=np.float32(0.25), beta=np.float32(0.11),
               pos_iou_thr=np.float32(0.5), neg_iou_thr=np.float32(0.4))
    rs = np.random.RandomState(77)
    for k, (seed, B, ph, pw, ih, iw, boxes, labs) in enumerate(CASES):
        cls, reg, _ = synth.head_outputs(seed, B, ph, pw, 'A')
        gts = [np.asarray(b, np.float32) for b in boxes]
        gls = [np.asarray(l, np.int64) for l in labs]
        metas = [dict(img_shape=(ih, iw, 3), pad_shape=(ph, pw, 3), scale_factor=1.0, flip=False)
                 for _ in range(B)]
        tc = [torch.from_numpy(x).requires_grad_(True) for x in cls]
        tr = [torch.from_numpy(x).requires_grad_(True) for x in reg]
        seen = []
        orig = ref_anchor_head.anchor_target

        def capture(*a, **kw_):
            seen.append(orig(*a, **kw_))
            return seen[-1]
        ref_anchor_head.anchor_target = capture
        try:
            losses = head.loss(tc, tr, [torch.from_numpy(g) for g in gts],
                               [torch.from_numpy(g) for g in gls], metas, train_cfg)
        finally:
            ref_anchor_head.anchor_target = orig
        n_pos = int(seen[0][4])                     # num_total_pos, the normaliser (:262-263)
        assert sorted(losses) == ['loss_bbox', 'loss_cls']
        sum(sum(v) for v in losses.values()).backward()
        out['case_%d' % k] = np.array([seed, B, ph, pw, ih, iw], np.int64)
        for b in range(B):
            out['gt_bboxes_%d_%d' % (k, b)] = gts[b]
            out['gt_labels_%d_%d' % (k, b)] = gls[b]
        for name, v in losses.items():
            out['%s_%d' % (name, k)] = np.array([float(x) for x in v], np.float64)
        lb, lc = out['loss_bbox_%d' % k], out['loss_cls_%d' % k]
        assert (lc > 0).all()
        if k == 0:
            assert int((lb > 0).sum()) >= 3, lb
        else:
            assert (lb > 0).any()
        for l in range(5):
            for nm, tl in (('cls', tc), ('reg', tr)):
                g = tl[l].grad.numpy().reshape(-1)
                nz = np.nonzero(g)[0] if nm == 'reg' else np.zeros(0, np.int64)
                rest = np.setdiff1d(np.arange(g.size), nz)
                take = max(0, min(g.size, N_IDX) - nz.size)
                idx = np.sort(np.concatenate([nz[:N_IDX], rs.choice(rest, min(take, rest.size),
                                                                    replace=False)]))
                out['g_%s_%d_%d_idx' % (nm, k, l)] = idx.astype(np.int64)
                out['g_%s_%d_%d' % (nm, k, l)] = g[idx]
        out['num_total_pos_%d' % k] = np.int64(n_pos)
        print('case %d: loss_cls %s loss_bbox %s, %d positive anchors'
              % (k, np.round(lc, 4), np.round(lb, 4), n_pos))
    path = os.path.join(HERE, 'retina_plain_train.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('wrote %s (%.1f KB)' % (path, size / 1024))
    assert size < 1000000


if __name__ == '__main__':
    gen()
