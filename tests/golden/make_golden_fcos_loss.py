"""Generate tests/golden/fcos_loss.npz by running the REFERENCE FCOSHead / IoUawareFCOSHead
`fcos_target` and `loss` (imported read-only through ref_shim.py, as make_golden_fcos.py does, with
its `_focal_op_cpu` in place of the CUDA focal op) on the CPU, on the seeded inputs of
tests/synth_fcos_loss.py.  Runs only in the build container:

    python tests/golden/make_golden_fcos_loss.py

The fixture holds seeds, settings and recorded numbers -- never reference source.  Keys, per case k
(0: synth_fcos_loss.SMALL, 1: synth_fcos_loss.MAIN1):
    case_k                           int64 [pad h, pad w, img h, img w, batch, gt seed, gts from, to, output seed]
    labels_k_l, bbox_targets_k_l     the reference's fcos_target, level l: (B * N_l) int64, (B * N_l, 4) fp32
    loss_<head>_k                    fp64 [loss_cls, loss_reg, loss_centerness(, loss_iou)], head = iou / plain
    g_<head>_k_<kind>_l_idx / g_<head>_k_<kind>_l
                                     a fixed index subset (<= N_IDX entries of the flattened NCHW gradient,
                                     non-zero entries of reg / ctr / iou first) and the reference's autograd
                                     gradient of the sum of all losses there; kind = cls / reg / ctr / iou
and once: gamma, alpha.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))
import make_golden_fcos as mgf  # noqa: E402  (installs ref_shim)
import ref_shim  # noqa: E402
import synth_fcos_loss as S  # noqa: E402

import mmdet.models.anchor_heads.fcos_head as ref_plain  # noqa: E402
import mmdet.models.anchor_heads.iou_aware_fcos_head as ref_iou  # noqa: E402

N_IDX = 500
GAMMA, ALPHA = 2.0, 0.25


def gen():
    ref_plain.sigmoid_focal_loss = mgf._focal_op_cpu
    ref_iou.sigmoid_focal_loss = mgf._focal_op_cpu
    cfg = ref_shim.to_cfg(dict(gamma=GAMMA, alpha=ALPHA))
    out = dict(gamma=np.float32(GAMMA), alpha=np.float32(ALPHA))
    rs = np.random.RandomState(78)
    kw = dict(num_classes=S.C + 1, in_channels=32, feat_channels=32, stacked_convs=1,
              strides=S.STRIDES, regress_ranges=S.RANGES)
    for k, case in enumerate((S.SMALL, S.MAIN1)):
        sizes, gb, gl, outs = S.case_inputs(case)
        S.check_conditions(sizes, gb, gl)
        out['case_%d' % k] = np.array(case[1:], np.int64)
        tb = [torch.from_numpy(b) for b in gb]
        tl = [torch.from_numpy(x) for x in gl]
        for tag, cls_, nmaps in (('iou', ref_iou.IoUawareFCOSHead, 4), ('plain', ref_plain.FCOSHead, 3)):
            head = cls_(**kw)
            if tag == 'iou':
                pts = head.get_points(sizes, torch.float32, 'cpu')
                labels, targets = head.fcos_target(pts, tb, tl)
                for l in range(len(sizes)):
                    out['labels_%d_%d' % (k, l)] = labels[l].numpy()
                    out['bbox_targets_%d_%d' % (k, l)] = targets[l].numpy()
                print('case %d: positives per level %s' % (k, [int((x > 0).sum()) for x in labels]))
            maps = [[torch.from_numpy(x).requires_grad_(True) for x in m] for m in outs[:nmaps]]
            losses = head.loss(*(maps + [tb, tl, None, cfg]))
            keys = ['loss_cls', 'loss_reg', 'loss_centerness'] + (['loss_iou'] if tag == 'iou' else [])
            assert list(losses) == keys, list(losses)
            sum(v.sum() for v in losses.values()).backward()
            out['loss_%s_%d' % (tag, k)] = np.array([float(losses[n].sum()) for n in keys], np.float64)
            print(tag, k, out['loss_%s_%d' % (tag, k)])
            for kind, m in zip(('cls', 'reg', 'ctr', 'iou'), maps):
                for l, t in enumerate(m):
                    g = t.grad.numpy().reshape(-1)
                    nz = np.nonzero(g)[0] if kind != 'cls' else np.zeros(0, np.int64)
                    if nz.size > N_IDX:
                        nz = np.sort(rs.choice(nz, N_IDX, replace=False))
                    rest = np.setdiff1d(np.arange(g.size), nz)
                    take = max(0, min(g.size, N_IDX) - nz.size)
                    idx = np.sort(np.concatenate([nz, rs.choice(rest, min(take, rest.size),
                                                                replace=False)]))
                    out['g_%s_%d_%s_%d_idx' % (tag, k, kind, l)] = idx.astype(np.int32)
                    out['g_%s_%d_%s_%d' % (tag, k, kind, l)] = g[idx]
    path = os.path.join(HERE, 'fcos_loss.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('wrote %s (%.1f KB)' % (path, size / 1024))
    assert size < 1000000


if __name__ == '__main__':
    gen()
