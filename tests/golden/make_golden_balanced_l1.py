"""Generate tests/golden/balanced_l1.npz by running the REFERENCE on the CPU (imported read-only
through ref_shim.py, as make_golden_retina_plain_train.py does): weighted_balanced_l1_loss
(core/loss/losses.py:482-520) on a planted element list, and RetinaHead.loss / IoUawareRetinaHead.loss
with loss_bbox = BalancedL1Loss(alpha=0.5, gamma=1.5, beta=0.11) on the two seeded cases of
make_golden_retina_plain_train.py.  Runs only in the build container:

    python tests/golden/make_golden_balanced_l1.py

The fixture holds seeds, settings and recorded numbers -- never reference source.  Head outputs are
regenerated from the seed by tests/synth.py (`head_outputs(seed, B, ph, pw, 'A')`; the plain head
ignores the IoU maps).  Keys:
    alpha, gamma, beta, betas         settings; betas = the knees of the element list
    el_pred_i, el_weight_i            (n,) fp32: the planted list for betas[i] (target 0) -- |d| in
                                      {0, beta, both fp32 neighbours of beta, 1e-4, 3, 1e4}, both signs,
                                      weights cycling through (1, 0.5, 0, 2)
    el_sum_i, el_grad_i               weighted_balanced_l1_loss(..., avg_factor=1) in fp32 and its autograd
                                      gradient
    el_unit_grad, el_unit_sum         the eight elements of the table in the issue (beta 0.11, weight 1)
  per case k (both heads see the same ground truth):
    case_k, gt_bboxes_k_b, gt_labels_k_b, num_total_pos_k      as retina_plain_train.npz
    plain_loss_cls_k, plain_loss_bbox_k                        (5,) fp64, RetinaHead.loss
    iou_loss_cls_k, iou_loss_bbox_k, iou_losses_iou_k          (5,) fp64, IoUawareRetinaHead.loss
    {plain,iou}_g_{cls,reg,iou}_k_l_idx / {plain,iou}_g_{cls,reg,iou}_k_l
                       a fixed index subset (<= 3000 entries of the flattened NCHW gradient, every non-zero box
                       gradient first) and the reference's autograd gradient of the sum of all losses there
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
from make_golden_retina_plain_train import CASES, N_IDX  # noqa: E402

from mmdet.core.loss.losses import weighted_balanced_l1_loss  # noqa: E402
from mmdet.models.anchor_heads.retina_head import RetinaHead  # noqa: E402
from mmdet.models.anchor_heads.iou_aware_retina_head import IoUawareRetinaHead  # noqa: E402
import mmdet.models.anchor_heads.anchor_head as ref_anchor_head  # noqa: E402
import mmdet.models.anchor_heads.iou_aware_retina_head as ref_iou_head  # noqa: E402

ALPHA, GAMMA, BETA = 0.5, 1.5, 0.11
BETAS = (0.11, 1.0)
UNIT_PRED = (0.0, 0.11, 0.10999999, -0.11, 3.0, -1e4, 1e-4, 0.0)


def planted(beta):
    b = np.float32(beta)
    up, down = np.nextafter(b, np.float32(np.inf)), np.nextafter(b, np.float32(-np.inf))
    mags = np.array([0.0, b, up, down, 1e-4, 3.0, 1e4], np.float32)
    pred = np.concatenate([mags, -mags, mags, -mags]).astype(np.float32)
    weight = np.array([(1.0, 0.5, 0.0, 2.0)[(k + k // 7) % 4] for k in range(pred.size)], np.float32)
    return pred, weight


def elements(out):
    out['betas'] = np.array(BETAS, np.float32)
    for i, beta in enumerate(BETAS):
        pred, weight = planted(beta)
        p = torch.from_numpy(pred).reshape(-1, 1).requires_grad_(True)
        s = weighted_balanced_l1_loss(p, torch.zeros_like(p), torch.from_numpy(weight).reshape(-1, 1),
                                      beta=beta, alpha=ALPHA, gamma=GAMMA, avg_factor=1.0)
        s.sum().backward()
        out['el_pred_%d' % i], out['el_weight_%d' % i] = pred, weight
        out['el_sum_%d' % i] = np.float32(float(s))
        out['el_grad_%d' % i] = p.grad.numpy().reshape(-1).copy()
    p = torch.tensor(UNIT_PRED, dtype=torch.float32).reshape(-1, 1).requires_grad_(True)
    s = weighted_balanced_l1_loss(p, torch.zeros_like(p), torch.ones_like(p), beta=BETA, alpha=ALPHA,
                                  gamma=GAMMA, avg_factor=1.0)
    s.sum().backward()
    out['el_unit_pred'] = np.array(UNIT_PRED, np.float32)
    out['el_unit_sum'] = np.float32(float(s))
    out['el_unit_grad'] = p.grad.numpy().reshape(-1).copy()
    print('unit elements: gradient %s, loss %.7g' % (out['el_unit_grad'], float(s)))


def gen():
    kw = dict(num_classes=81, in_channels=256, stacked_convs=4, feat_channels=256,
              octave_base_scale=4, scales_per_octave=3, anchor_ratios=[0.5, 1.0, 2.0],
              anchor_strides=[8, 16, 32, 64, 128], target_means=[.0] * 4, target_stds=[1.0] * 4,
              loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25,
                            loss_weight=1.0),
              loss_bbox=dict(type='BalancedL1Loss', alpha=ALPHA, gamma=GAMMA, beta=BETA, loss_weight=1.0))
    heads = (('plain', RetinaHead(**kw), ref_anchor_head, ('cls', 'reg')),
             ('iou', IoUawareRetinaHead(**kw), ref_iou_head, ('cls', 'reg', 'iou')))
    train_cfg = ref_shim.to_cfg(dict(
        assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0,
                      ignore_iof_thr=-1),
        allowed_border=-1, pos_weight=-1, debug=False))
    out = dict(alpha=np.float32(ALPHA), gamma=np.float32(GAMMA), beta=np.float32(BETA),
               focal_gamma=np.float32(2.0), focal_alpha=np.float32(0.25),
               pos_iou_thr=np.float32(0.5), neg_iou_thr=np.float32(0.4))
    elements(out)
    rs = np.random.RandomState(78)
    for k, (seed, B, ph, pw, ih, iw, boxes, labs) in enumerate(CASES):
        cls, reg, iou = synth.head_outputs(seed, B, ph, pw, 'A')
        gts = [np.asarray(b, np.float32) for b in boxes]
        gls = [np.asarray(l, np.int64) for l in labs]
        metas = [dict(img_shape=(ih, iw, 3), pad_shape=(ph, pw, 3), scale_factor=1.0, flip=False)
                 for _ in range(B)]
        out['case_%d' % k] = np.array([seed, B, ph, pw, ih, iw], np.int64)
        for b in range(B):
            out['gt_bboxes_%d_%d' % (k, b)] = gts[b]
            out['gt_labels_%d_%d' % (k, b)] = gls[b]
        for tag, head, mod, names in heads:
            leaves = dict(cls=[torch.from_numpy(x).requires_grad_(True) for x in cls],
                          reg=[torch.from_numpy(x).requires_grad_(True) for x in reg],
                          iou=[torch.from_numpy(x).requires_grad_(True) for x in iou])
            seen = []
            orig = mod.anchor_target

            def capture(*a, **kw_):
                seen.append(orig(*a, **kw_))
                return seen[-1]
            mod.anchor_target = capture
            try:
                losses = head.loss(*[leaves[n] for n in names], [torch.from_numpy(g) for g in gts],
                                   [torch.from_numpy(g) for g in gls], metas, train_cfg)
            finally:
                mod.anchor_target = orig
            out['num_total_pos_%d' % k] = np.int64(int(seen[0][4]))
            sum(sum(v) for v in losses.values()).backward()
            for name, v in losses.items():
                out['%s_%s_%d' % (tag, name, k)] = np.array([float(x) for x in v], np.float64)
            lb = out['%s_loss_bbox_%d' % (tag, k)]
            if k == 0:
                assert int((lb > 0).sum()) >= 3, lb
            else:
                assert (lb > 0).any()
            for l in range(5):
                for nm in names:
                    g = leaves[nm][l].grad.numpy().reshape(-1)
                    nz = np.nonzero(g)[0] if nm == 'reg' else np.zeros(0, np.int64)
                    rest = np.setdiff1d(np.arange(g.size), nz)
                    take = max(0, min(g.size, N_IDX) - nz.size)
                    idx = np.sort(np.concatenate([nz[:N_IDX], rs.choice(rest, min(take, rest.size),
                                                                        replace=False)]))
                    out['%s_g_%s_%d_%d_idx' % (tag, nm, k, l)] = idx.astype(np.int64)
                    out['%s_g_%s_%d_%d' % (tag, nm, k, l)] = g[idx]
            print('case %d %s: loss_bbox %s, %d positive anchors'
                  % (k, tag, np.round(lb, 4), int(out['num_total_pos_%d' % k])))
    path = os.path.join(HERE, 'balanced_l1.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('wrote %s (%.1f KB)' % (path, size / 1024))
    assert size < 1000000


if __name__ == '__main__':
    gen()
