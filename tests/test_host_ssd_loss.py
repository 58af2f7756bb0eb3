"""CPU: SSD's training loss -- tests/ssd_loss_ref.py against the reference's recorded targets, losses,
selections and gradients (tests/golden/ssd_loss.npz, written by tests/golden/make_golden_ssd_loss.py),
SSDHead.loss on its torch route (fuse_loss = False) and SSDHead.get_anchors against the same record, the
C-ABI declarations and the refusal of CPU tensors on the fused route."""
import json
import os
import re

import numpy as np
import pytest
import torch

import ssd_loss_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REL = 1e-6          # ssd_ref's figure against the reference: the same ops in fp32 on both sides

LOSS_SYMBOLS = ('ia_ssd_mine_lds_rows', 'ia_ssd_loss_partials', 'ia_ssd_loss_rows', 'ia_ssd_mine', 'ia_ssd_loss_bwd',
                'ia_ssd_head_loss_workspace_bytes', 'ia_ssd_head_loss_workspace_layout', 'ia_ssd_head_loss_fwd',
                'ia_ssd_head_loss_bwd')


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(HERE, 'golden', 'ssd_loss.npz'))


@pytest.fixture(scope='module')
def cases():
    """{name: (inputs, ssd_loss_ref in fp32 with unit upstream gradients)}, computed once"""
    out = {}
    for name in ('small', 'mid'):
        inp = R.inputs(name)
        out[name] = (inp, R.loss(inp['cls'], inp['reg'], *inp['targets'], grad_out=np.ones((inp['B'], 2))))
    return out


def _train_cfg(gold):
    from iouaware.config import ConfigDict
    return ConfigDict(json.loads(str(gold['train_cfg'])))


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert err <= REL * scale, '%s: error %.3e against %.3e' % (what, err, scale)


def _neg_ids(sel, labels):
    return np.nonzero(np.asarray(sel) & (np.asarray(labels) == 0))[0]


def test_fixture_margins_hold_in_fp64(cases):
    for name, (inp, res) in cases.items():
        res64 = R.loss([c.double() for c in inp['cls']], [r.double() for r in inp['reg']], *inp['targets'])
        assert torch.equal(res['sel'], res64['sel']), name          # fp32 selects what fp64 selects
        for b, kind in enumerate(R.CASES[name]['kinds']):
            m = R.margins(inp, b)
            assert m['iou'] >= 1e-5 and m['best'] >= 1e-5, (name, b, m)
            if kind == 'few':
                assert m['gap'] >= 1e-4, (name, b, m)


def test_recorded_cases_cover_what_they_are_for(cases):
    inp, res = cases['small']
    kinds = R.CASES['small']['kinds']
    m = [R.margins(inp, b) for b in range(3)]
    few, many, tie = kinds.index('few'), kinds.index('many'), kinds.index('tie')
    assert 0 < m[few]['k'] < m[few]['num_neg']
    assert m[many]['k'] == m[many]['num_neg'] and R.NEG_POS_RATIO * m[many]['num_pos'] > m[many]['num_neg']
    # the threshold of the tie image lies in a run of bit-identical losses, part of it taken
    assert m[tie]['gap'] == 0.0 and len(inp['tie_rows'][tie]) == R.TIE_BELOW + R.TIE_ABOVE
    taken = res['sel'][tie].numpy()[inp['tie_rows'][tie]]
    assert taken.tolist() == [True] * R.TIE_BELOW + [False] * R.TIE_ABOVE      # the lowest row ids
    assert inp['R'] == 192 and cases['mid'][0]['R'] == 2268
    assert res['counts'][:, 1].tolist() == [x['k'] for x in m]


def test_ssd_loss_ref_targets_equal_the_recorded_reference(gold, cases):
    inp, _ = cases['small']
    labels, lw, bt, bw, num_total_pos = inp['targets']
    assert np.array_equal(labels.numpy(), gold['small_labels'].astype(np.int64))
    assert np.array_equal(lw.numpy(), gold['small_label_weights'])
    assert np.array_equal(bw.numpy(), gold['small_bbox_weights'])
    assert num_total_pos == int(gold['small_num_total_pos'])
    assert float(np.abs(bt.numpy() - gold['small_bbox_targets']).max()) <= 1e-6
    assert np.array_equal(inp['anchors'].numpy(), gold['small_anchors'])


def test_ssd_loss_ref_reproduces_the_recorded_reference(gold, cases):
    for name, (inp, res) in cases.items():
        _close(res['loss_cls'], gold[name + '_loss_cls'], name + ' loss_cls')
        _close(res['loss_bbox'], gold[name + '_loss_bbox'], name + ' loss_bbox')
        _close(res['grad_reg'], gold[name + '_grad_reg'], name + ' grad_reg')
        labels = inp['targets'][0].numpy()
        for b, kind in enumerate(R.CASES[name]['kinds']):
            ids, want = _neg_ids(res['sel'][b].numpy(), labels[b]), gold['%s_sel_neg_%d' % (name, b)]
            assert len(ids) == len(want) == res['counts'][b, 1]
            if kind != 'tie':                # torch's topk leaves the choice among ties open
                assert np.array_equal(ids, want), (name, b)
    inp, res = cases['small']
    g, want = res['grad_cls'].numpy().copy(), gold['small_grad_cls'].copy()
    for b, tie in enumerate(inp['tie_rows']):
        # the tie rows carry equal gradients; which of them carry one is the tie rule's business
        assert int((np.abs(want[b, tie]).max(1) > 0).sum()) == int((np.abs(g[b, tie]).max(1) > 0).sum())
        g[b, tie], want[b, tie] = 0, 0
    _close(g, want, 'small grad_cls')


def _head(name):
    from iouaware.ssd_head import SSDHead
    case = R.CASES[name]
    return SSDHead(num_classes=case['num_classes'], **case['head'])


def test_get_anchors_equals_the_recorded_reference(gold, cases):
    inp, _ = cases['small']
    head = _head('small')
    anchors, flags = head.get_anchors(R.CASES['small']['sizes'], inp['metas'])
    assert len(anchors) == len(flags) == 3 and len(anchors[0]) == 6
    assert np.array_equal(torch.cat(anchors[1]).numpy(), gold['small_anchors'])
    assert np.array_equal(torch.stack([torch.cat(f) for f in flags]).numpy(), gold['small_flags'])
    # a pad_shape that covers only part of the map: flags from ceil(pad / stride)
    _, f2 = head.get_anchors([(5, 5)], [dict(pad_shape=(17, 33, 3))])
    assert f2[0][0].view(5, 5, 4)[:, :, 0].tolist() == [[1] * 5] * 3 + [[0] * 5] * 2


@pytest.mark.parametrize('name', ['small', 'mid'])
def test_head_loss_torch_route_equals_the_recorded_reference(gold, cases, name):
    """SSDHead.loss with fuse_loss = False on the CPU: the reference's structure and values"""
    from iouaware.train import parse_losses
    inp, res = cases[name]
    head = _head(name)
    head.fuse_loss = False
    cls = [c.clone().requires_grad_(True) for c in inp['cls']]
    reg = [r.clone().requires_grad_(True) for r in inp['reg']]
    out = head.loss(cls, reg, inp['gt_bboxes'], inp['gt_labels'], inp['metas'], _train_cfg(gold))
    assert sorted(out) == ['loss_bbox', 'loss_cls']
    assert all(isinstance(v, list) and len(v) == inp['B'] and all(tuple(t.shape) == (1,) for t in v)
               for v in out.values())
    _close(torch.cat(out['loss_cls']).detach(), gold[name + '_loss_cls'], 'loss_cls')
    _close(torch.cat(out['loss_bbox']).detach(), gold[name + '_loss_bbox'], 'loss_bbox')
    total, log_vars = parse_losses(out)
    _close(float(total.detach()), float(gold[name + '_loss_cls'].sum() + gold[name + '_loss_bbox'].sum()), 'total')
    assert list(log_vars) == ['loss_cls', 'loss_bbox', 'loss']
    total.backward()
    _close(R.rows([r.grad for r in reg], 4), gold[name + '_grad_reg'], 'grad_reg')
    g = R.rows([c.grad for c in cls], inp['num_classes']).numpy()
    labels = inp['targets'][0].numpy()
    for b, kind in enumerate(R.CASES[name]['kinds']):
        ids = _neg_ids(np.abs(g[b]).max(1) > 0, labels[b])
        assert len(ids) == len(gold['%s_sel_neg_%d' % (name, b)])
        if kind != 'tie':
            assert np.array_equal(ids, gold['%s_sel_neg_%d' % (name, b)])
    if name == 'small':
        want = gold['small_grad_cls'].copy()
        for b, tie in enumerate(inp['tie_rows']):
            g[b, tie], want[b, tie] = 0, 0
        _close(g, want, 'grad_cls')


def test_new_symbols_are_declared_in_the_header_and_in_lib():
    from iouaware import _lib
    with open(os.path.join(ROOT, 'include', 'iouaware.h')) as fh:
        header = fh.read()
    for sym in LOSS_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % sym, header), sym
        assert sym in _lib.SIGNATURES, sym
    build = open(os.path.join(ROOT, 'iou-aware-single-stage-object-detector_amd', 'csrc', 'build.py')).read()
    assert "'ssdloss.hip'" in build and "'ia_ssd.hpp'" in build


def test_cpu_tensors_and_bad_settings_are_refused_by_name(gold, cases):
    from iouaware import _lib, ssd_ops
    inp, _ = cases['small']
    head = _head('small')
    head.fuse_loss = True
    with pytest.raises(_lib.IouAwareLibraryError, match='no CPU'):
        head.loss(inp['cls'], inp['reg'], inp['gt_bboxes'], inp['gt_labels'], inp['metas'], _train_cfg(gold))
    geom = head.geometry(R.CASES['small']['sizes'])
    args = (geom, inp['cls'], inp['reg']) + tuple(inp['targets'][:4])
    with pytest.raises(_lib.IouAwareLibraryError, match='head output is on cpu'):
        ssd_ops.ssd_head_loss(*args, 4.0)
    with pytest.raises(ValueError, match='neg_pos_ratio'):
        ssd_ops.ssd_head_loss(*args, 4.0, neg_pos_ratio=-1)
    with pytest.raises(ValueError, match='beta'):
        ssd_ops.ssd_head_loss(*args, 4.0, beta=0.0)
    with pytest.raises(_lib.IouAwareLibraryError, match='ce is on cpu'):
        ssd_ops.ssd_mine(torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.int64), 3)
