"""Generate tests/golden/ssd_loss.npz by running the REFERENCE SSDHead.loss and its backward (imported
read-only through ref_shim.py) on the seeded inputs of tests/ssd_loss_ref.py.  Needs the reference tree
at ref_shim.REF:

    python tests/golden/make_golden_ssd_loss.py

The fixture holds recorded results and settings only -- never reference source.  Case `small`: the
reference's targets, anchors, valid flags, losses and all gradients.  Case `mid`: the losses, the
selected negative row ids (the negatives with a non-zero class gradient) and the box gradients; its
inputs are regenerated from the seed.  `train_cfg` is the ssd300_coco config's, as JSON.

Asserted here in fp64 (and again by tests/test_host_ssd_loss.py): every gt's best anchor is unique and
no IoU lies within 1e-5 of 0.5; outside the tie images the k-th and (k + 1)-th largest negative loss
differ by >= 1e-4; the fp32 evaluation of ssd_loss_ref selects the same set as its fp64 evaluation.
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

ref_shim.install()
import ssd_loss_ref as R  # noqa: E402
import mmdet.models.anchor_heads.ssd_head as ref_head  # noqa: E402


def plain(v):
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v


def check_margins(name, inp):
    for b, kind in enumerate(R.CASES[name]['kinds']):
        m = R.margins(inp, b)
        print('%s image %d (%s): num_pos %d, num_neg %d, k %d, margins iou %.1e best %.1e gap %s'
              % (name, b, kind, m['num_pos'], m['num_neg'], m['k'], m['iou'], m['best'], m['gap']))
        assert m['iou'] >= 1e-5 and m['best'] >= 1e-5
        if kind == 'few':
            assert 0 < m['k'] < m['num_neg'] and m['gap'] >= 1e-4
        if kind == 'many':
            assert m['k'] == m['num_neg'] and R.NEG_POS_RATIO * m['num_pos'] > m['num_neg']
        if kind == 'tie':
            assert m['gap'] == 0.0


def main():
    cfg = ref_shim.load_config('%s/configs/ssd300_coco.py' % ref_shim.REF)
    train_cfg = plain(cfg.train_cfg)
    assert train_cfg['neg_pos_ratio'] == R.NEG_POS_RATIO and train_cfg['smoothl1_beta'] == R.BETA
    arrs = dict(train_cfg=np.asarray(json.dumps(train_cfg, sort_keys=True)))
    for name in ('small', 'mid'):
        case = R.CASES[name]
        inp = R.inputs(name)
        check_margins(name, inp)
        nc, B = case['num_classes'], inp['B']
        head = ref_head.SSDHead(num_classes=nc, **case['head'])
        cls = [c.clone().requires_grad_(True) for c in inp['cls']]
        reg = [r.clone().requires_grad_(True) for r in inp['reg']]
        tcfg = ref_shim.to_cfg(train_cfg)
        out = head.loss(cls, reg, inp['gt_bboxes'], inp['gt_labels'], inp['metas'], tcfg)
        total = sum(l.sum() for l in out['loss_cls']) + sum(l.sum() for l in out['loss_bbox'])
        total.backward()
        g_cls = R.rows([c.grad for c in cls], nc).numpy()
        g_reg = R.rows([r.grad for r in reg], 4).numpy()
        labels = inp['targets'][0].numpy()
        sel_neg = [np.nonzero((labels[b] == 0) & (np.abs(g_cls[b]).max(1) > 0))[0] for b in range(B)]
        # ssd_loss_ref against the reference, fp32 and fp64
        ones = np.ones((B, 2))
        tg = inp['targets']
        mine32 = R.loss(inp['cls'], inp['reg'], *tg, grad_out=ones)
        mine64 = R.loss([c.double() for c in inp['cls']], [r.double() for r in inp['reg']], *tg, grad_out=ones)
        assert torch.equal(mine32['sel'], mine64['sel']), 'fp32 and fp64 select different sets'
        for b, kind in enumerate(case['kinds']):
            ids = np.nonzero(mine32['sel'][b].numpy() & (labels[b] == 0))[0]
            assert len(ids) == len(sel_neg[b]) == mine32['counts'][b, 1]
            if kind != 'tie':
                assert np.array_equal(ids, sel_neg[b]), 'ssd_loss_ref selects another set than the reference'
        lc = torch.cat(out['loss_cls']).detach().numpy()
        lb = torch.cat(out['loss_bbox']).detach().numpy()
        assert np.abs(mine32['loss_cls'].numpy() - lc).max() <= 1e-6 * np.abs(lc).max()
        assert np.abs(mine32['loss_bbox'].numpy() - lb).max() <= 1e-6 * np.abs(lb).max()
        arrs[name + '_loss_cls'], arrs[name + '_loss_bbox'] = lc.astype(np.float32), lb.astype(np.float32)
        for b in range(B):
            arrs['%s_sel_neg_%d' % (name, b)] = sel_neg[b].astype(np.int32)
        arrs[name + '_grad_reg'] = g_reg.astype(np.float32)
        if name == 'small':
            anchor_list, flag_list = head.get_anchors([tuple(c.shape[-2:]) for c in cls], inp['metas'])
            # recorded first: the reference's anchor_target concatenates the lists in place
            arrs['small_anchors'] = torch.cat(anchor_list[0]).numpy().astype(np.float32)
            arrs['small_flags'] = torch.stack([torch.cat(f) for f in flag_list]).numpy().astype(np.uint8)
            rt = ref_head.anchor_target(anchor_list, flag_list, inp['gt_bboxes'], inp['metas'], head.target_means,
                                        head.target_stds, tcfg, gt_labels_list=inp['gt_labels'], label_channels=1,
                                        sampling=False, unmap_outputs=False)
            arrs['small_labels'] = torch.cat(rt[0], -1).view(B, -1).numpy().astype(np.int8)
            arrs['small_label_weights'] = torch.cat(rt[1], -1).view(B, -1).numpy().astype(np.float32)
            arrs['small_bbox_targets'] = torch.cat(rt[2], -2).view(B, -1, 4).numpy().astype(np.float32)
            arrs['small_bbox_weights'] = torch.cat(rt[3], -2).view(B, -1, 4).numpy().astype(np.float32)
            arrs['small_num_total_pos'] = np.asarray(rt[4], np.int64)
            arrs['small_grad_cls'] = g_cls.astype(np.float32)
    path = os.path.join(HERE, 'ssd_loss.npz')
    np.savez_compressed(path, **arrs)
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
