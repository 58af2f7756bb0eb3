"""Generate tests/golden/targets_edge.npz: the REFERENCE's own anchor_target (imported read-only
through ref_shim.py, on the CPU, where `max` returns the first index on ties) on the adversarial
assigner inputs of tests/synth_targets.py.  Runs only in the build container:

    python tests/golden/make_golden_targets_edge.py

The fixture holds inputs (gt boxes / labels, settings, an input checksum) and outputs (the
per-level targets and the counts) -- never reference source.  Keys are '<case>/<name>'.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))
import ref_shim  # noqa: E402
import synth_targets  # noqa: E402

ref_shim.install()
from mmdet.core import anchor_target  # noqa: E402
from mmdet.models.anchor_heads.iou_aware_retina_head import IoUawareRetinaHead  # noqa: E402

HEAD_KW = dict(num_classes=81, in_channels=256, stacked_convs=4, feat_channels=256,
               octave_base_scale=4, scales_per_octave=3, anchor_ratios=[0.5, 1.0, 2.0],
               anchor_strides=[8, 16, 32, 64, 128], target_means=[.0] * 4,
               target_stds=[1.0] * 4,
               loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25,
                             loss_weight=1.0),
               loss_bbox=dict(type='SmoothL1Loss', beta=0.11, loss_weight=1.0))


def gen_targets_edge():
    out = dict(cases=np.array(synth_targets.CASES))
    for name in synth_targets.CASES:
        c = synth_targets.case(name)
        head = IoUawareRetinaHead(**synth_targets.head_kw(c, HEAD_KW))
        metas = synth_targets.metas(c)
        cfg = ref_shim.to_cfg(synth_targets.train_cfg(c))
        anchors, flags = head.get_anchors(c['featmap_sizes'], metas)
        assert np.array_equal(torch.cat(anchors[0]).numpy(), c['anchors'])
        gts = [torch.from_numpy(g) for g in c['gts']]
        gls = None if c['labels'] is None else [torch.from_numpy(l) for l in c['labels']]
        r = anchor_target(anchors, flags, gts, metas, head.target_means, head.target_stds, cfg,
                          gt_labels_list=gls, label_channels=80, sampling=False)
        labels, lw, bt, bw, npos, nneg, _ = r
        B = len(gts)
        p = name + '/'
        out[p + 'checksum'] = c['checksum']
        out[p + 'tensor'] = np.array(c['tensor'])
        out[p + 'pads'] = np.array(c['pads'])
        out[p + 'settings'] = np.array([c['pos_iou_thr'], c['neg_iou_thr'], c['min_pos_iou'],
                                        c['pos_weight']], np.float64)
        out[p + 'means_stds'] = np.array([c['means'], c['stds']], np.float64)
        out[p + 'scales_per_octave'] = c['scales_per_octave']
        for b in range(B):
            out[p + 'gt_bboxes_%d' % b] = c['gts'][b]
            if c['labels'] is not None:
                out[p + 'gt_labels_%d' % b] = c['labels'][b]
        out[p + 'num_total_pos'] = npos
        out[p + 'num_total_neg'] = nneg
        for l, n in enumerate(c['level_anchors']):
            # images_to_levels squeezes a batch of one: store (B, N_l[, 4]) always
            out[p + 'labels_%d' % l] = labels[l].numpy().reshape(B, n)
            out[p + 'label_weights_%d' % l] = lw[l].numpy().reshape(B, n)
            out[p + 'bbox_targets_%d' % l] = bt[l].numpy().reshape(B, n, 4)
            out[p + 'bbox_weights_%d' % l] = bw[l].numpy().reshape(B, n, 4)
        print('%-15s G %s  num_total_pos %d  num_total_neg %d' %
              (name, [g.shape[0] for g in c['gts']], npos, nneg))
    path = os.path.join(HERE, 'targets_edge.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    gen_targets_edge()
