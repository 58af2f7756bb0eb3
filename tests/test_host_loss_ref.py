"""CPU: the float64 yardstick of the anchor-head losses (tests/loss_ref.py)

  * pinned to the reference's own loss values and autograd gradients
    (tests/golden/losses_small.npz, losses_balanced.npz; the bars of test_oracle_losses.py), and
  * the CPU oracle (oracle/iouaware_oracle_loss.c) held to it on the whole edge set of
    tests/test_gpu_loss_edges.py -- every output, every element -- so that what the GPU tests ask
    of the kernels is known to be sound before anything runs on a GPU.  The worst
    oracle-against-yardstick error per output is printed (`pytest -s`); the GPU tests' bars for the
    exact-math kernels are four times these figures (test_gpu_loss_edges.BOX_MEASURED).

Bars here.  The exact-math outputs: 2e-6 (of the tensor's maximum; sums relative; IoU targets
absolute).  That is the fp32 rounding of the box corners: at the 17 x 19 level (stride 8) they
reach 200 px, where one rounding is 200 * 2^-24 = 1.2e-5 px; the narrowest base anchor is 23 px
wide, so one corner moves an IoU by 5e-7, four corners by 2e-6.  Focal: 2.5e-5, a quarter of the
1e-4 parity limit of the losses (csrc/ia_loss.hpp).  Each figure is also held below the one
recorded in test_gpu_loss_edges.BOX_MEASURED, from which the GPU bars are formed."""
import os

import numpy as np
import pytest
import torch

import loss_ref as R
import synth
import test_gpu_loss_edges as E

GS = 0.375
WORST = {}


def note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), float(err))


@pytest.fixture(scope='module', autouse=True)
def table():
    yield
    print('\noracle against yardstick, worst per output')
    for k in sorted(WORST):
        print('    %-34s %.3g' % (k, WORST[k]))


# ------------------------------------------------------------------ yardstick against the reference
@pytest.fixture(scope='module')
def fx(golden_dir):
    f = np.load(os.path.join(golden_dir, 'losses_small.npz'))
    ih, iw, ph, pw = [int(v) for v in f['img']]
    B = int(f['batch'])
    cls, reg, iou = synth.head_outputs(int(f['seed']), B, ph, pw, str(f['kind']))
    assert synth.checksum(cls + reg + iou) == int(f['checksum'])
    return f, cls, reg, iou, B, synth.level_shapes(ph, pw)


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-12)


def sampled_close(g, f, key, tol):
    want = f[key].astype(np.float64)
    idx = f[key.rsplit('_', 1)[0] + '_idx'] if key.endswith('tached') else f[key + '_idx']
    got = np.asarray(g, np.float64).reshape(-1)[idx]
    scale = max(np.abs(want).max(), 1e-30)
    assert np.abs(got - want).max() <= tol * scale, (key, np.abs(got - want).max(), scale)


def test_yardstick_matches_reference(oracle_lib, fx):
    f, cls, reg, iou, B, shapes = fx
    base = oracle_lib.head_base_anchors(synth.STRIDES)
    avg = float(f['num_total_pos'])
    for l, (h, w) in enumerate(shapes):
        labels, lw = f['labels_%d' % l].reshape(B, -1), f['label_weights_%d' % l].reshape(B, -1)
        bt, bw = f['bbox_targets_%d' % l].reshape(B, -1, 4), f['bbox_weights_%d' % l].reshape(B, -1, 4)
        c = R.focal(cls[l], labels, lw, synth.A, 2.0, 0.25, 1.0 / avg)
        assert rel(c['sum'] / avg, f['loss_cls'][l]) < 1e-4
        sampled_close(c['grad'], f, 'g_cls_%d_attached' % l, 1e-4)
        s = R.smooth_l1(reg[l], bt, bw, synth.A, 0.11, 1.0 / avg)
        assert abs(s['sum'] / avg - f['loss_bbox'][l]) <= 1e-4 * max(f['loss_bbox'][l], 1e-6)
        for attach in (True, False):
            i = R.iou_bce(reg[l], iou[l], bt, bw, base[l], synth.STRIDES[l], gscale=1.0 / avg,
                          attach=attach)
            assert abs(i['sum'] / avg - f['losses_iou'][l]) <= 1e-4 * max(f['losses_iou'][l], 1e-6)
            sampled_close(i['g_iou'], f, 'g_iou_%d_attached' % l, 1e-4)   # the same either way
            if attach:
                sampled_close(s['grad'] + i['g_box'], f, 'g_reg_%d_attached' % l, 2e-4)
            else:
                assert i['g_box'] is None
                sampled_close(s['grad'], f, 'g_reg_%d_detached' % l, 2e-4)


def test_balanced_yardstick_matches_reference(oracle_lib, fx, golden_dir):
    f, cls, reg, iou, B, shapes = fx
    fb = np.load(os.path.join(golden_dir, 'losses_balanced.npz'))
    base = oracle_lib.head_base_anchors(synth.STRIDES)
    avg = float(f['num_total_pos'])
    eta, delta, lwt = float(fb['eta']), float(fb['delta']), float(fb['bbox_loss_weight'])
    for l, (h, w) in enumerate(shapes):
        labels, lw = f['labels_%d' % l].reshape(B, -1), f['label_weights_%d' % l].reshape(B, -1)
        bt, bw = f['bbox_targets_%d' % l].reshape(B, -1, 4), f['bbox_weights_%d' % l].reshape(B, -1, 4)
        i = R.iou_bce(reg[l], iou[l], bt, bw, base[l], synth.STRIDES[l], gscale=1.0 / avg)
        c = R.focal(cls[l], labels, lw, synth.A, 2.0, 0.25, 1.0 / avg, i['iou'], eta)
        s = R.smooth_l1(reg[l], bt, bw, synth.A, 0.11, lwt / avg, i['iou'], delta)
        assert rel(c['sum'] / avg, fb['loss_cls'][l]) < 1e-4
        assert abs(s['sum'] * lwt / avg - fb['loss_bbox'][l]) <= 1e-4 * max(fb['loss_bbox'][l], 1e-6)
        sampled_close(c['grad'], fb, 'g_cls_%d' % l, 2e-4)
        sampled_close(s['grad'] + i['g_box'], fb, 'g_reg_%d' % l, 2e-4)
        sampled_close(i['g_iou'], fb, 'g_iou_%d' % l, 2e-4)


# ------------------------------------------------------------------ autograd's conventions
def test_yardstick_conventions_are_the_documented_ones():
    """what csrc/ia_loss.hpp documents at the non-differentiable points is what this torch does"""
    a = torch.tensor([1.0, 2.0], dtype=torch.float64, requires_grad=True)
    b = torch.tensor([1.0, 3.0], dtype=torch.float64, requires_grad=True)
    (torch.max(a, b).sum() + 2 * torch.min(a, b).sum()).backward()
    assert a.grad.tolist() == [1.5, 2.0] and b.grad.tolist() == [1.5, 1.0]
    x = torch.tensor([-R.MAX_RATIO, R.MAX_RATIO, 5.0, 0.0], dtype=torch.float64, requires_grad=True)
    x.clamp(min=-R.MAX_RATIO, max=R.MAX_RATIO).sum().backward()
    assert x.grad.tolist() == [1.0, 1.0, 0.0, 1.0]
    z = torch.tensor([0.0], dtype=torch.float64, requires_grad=True)
    z.clamp(min=0).sum().backward()
    assert z.grad.tolist() == [1.0]


# ------------------------------------------------------------------ oracle against yardstick
BOX_BAR = 2e-6
FOCAL_BAR = 2.5e-5


def _oracle_box_level(oracle_lib, d, set_name, base, stride, fp32):
    """every box / IoU / smooth-L1 output of the oracle on one level against the yardstick"""
    means, stds = E.SETS[set_name]
    ref = R.iou_bce(d['reg'], d['iou'], d['bt'], d['bw'], base, stride, means, stds, GS, True)
    assert E.finite(ref['iou'], ref['g_iou'], ref['g_box'], ref['sum'])
    so, tgt, gi, gb = oracle_lib.iou_bce(d['reg'], d['iou'], d['bt'], d['bw'], base, stride, means,
                                         stds, gscale=GS)
    assert E.finite(tgt, gi, gb, so)
    errs = dict(iou=np.abs(tgt.astype(np.float64).reshape(E.B, -1) - ref['iou'].numpy()).max(),
                iou_sum=rel(so, ref['sum']), g_iou=E.share_of_max(gi, ref['g_iou']),
                g_box=E.share_of_max(gb, ref['g_box']))
    rs = R.smooth_l1(d['reg'], d['bt'], d['bw'], E.A, E.BETA, GS)
    ss, gsl = oracle_lib.smooth_l1(d['reg'], d['bt'], d['bw'], E.A, E.BETA, gscale=GS)
    assert E.finite(rs['grad'], rs['sum'], gsl, ss)
    errs.update(sl1_sum=rel(ss, rs['sum']), sl1_grad=E.share_of_max(gsl, rs['grad']),
                g_reg=E.share_of_max(gsl + gb, rs['grad'] + ref['g_box']))
    errs['sl1b_sum'] = errs['sl1b_grad'] = 0.0
    for delta in (1.5, 0.5, 1.0):
        rb = R.smooth_l1(d['reg'], d['bt'], d['bw'], E.A, E.BETA, GS, d['anchor_iou'], delta)
        sb, gbal = oracle_lib.smooth_l1_balanced(d['reg'], d['bt'], d['bw'], d['anchor_iou'], E.A,
                                                 E.BETA, delta, gscale=GS)
        assert E.finite(rb['grad'], rb['sum'], gbal, sb)
        errs['sl1b_sum'] = max(errs['sl1b_sum'], rel(sb, rb['sum']))
        errs['sl1b_grad'] = max(errs['sl1b_grad'], E.share_of_max(gbal, rb['grad']))
    for k, v in errs.items():
        note(k, v)
        assert v <= BOX_BAR, (k, v)
        assert v <= E.BOX_MEASURED[k], (k, v)     # the recorded table bounds what is measured
    # the == statements hold for the oracle, and (to float64 rounding) for the yardstick
    E.check_box_exact(d, set_name, tgt, gb, gi, fp32)
    E.check_box_exact(d, set_name, ref['iou'].numpy(), ref['g_box'].numpy(), ref['g_iou'].numpy(),
                      fp32, zero_tol=1e-13)
    # detached: the same IoU-logit gradient, none for the boxes
    refd = R.iou_bce(d['reg'], d['iou'], d['bt'], d['bw'], base, stride, means, stds, GS, False)
    assert refd['g_box'] is None and torch.equal(refd['g_iou'], ref['g_iou'])


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('level', sorted(E.BOX_LEVELS))
@pytest.mark.parametrize('set_name', sorted(E.SETS))
def test_oracle_box_losses_on_the_edge_set(oracle_lib, set_name, level, bf16):
    h, w, li = E.BOX_LEVELS[level]
    d = E.box_level(h, w, set_name, 11, bf16=bf16)
    assert set(d['slots']) == set(n for n, *_ in E.box_specs(*E.SETS[set_name]))
    base = oracle_lib.head_base_anchors(synth.STRIDES)[li]
    _oracle_box_level(oracle_lib, d, set_name, base, synth.STRIDES[li], not bf16)


@pytest.mark.parametrize('set_name', E.NODE_SETS)
def test_oracle_box_losses_on_the_node_levels(oracle_lib, set_name):
    """the five levels the all-levels node is given (96, 24, 6, 2, 1 positions)"""
    sizes, levels, cls, labels, lw = E.node_data(set_name)
    base = oracle_lib.head_base_anchors(synth.STRIDES)
    seen = set()
    for l, d in enumerate(levels):
        _oracle_box_level(oracle_lib, d, set_name, base[l], synth.STRIDES[l], True)
        seen |= set(d['slots'])
        rf = R.focal(cls[l], labels[l], lw[l], E.A, 2.0, E.ALPHA, GS)
        s, g = oracle_lib.focal_loss(cls[l], labels[l], lw[l], E.A, 2.0, E.ALPHA, gscale=GS)
        assert E.finite(rf['grad'], rf['sum'], g, s)
        assert rel(s, rf['sum']) <= FOCAL_BAR and E.share_of_max(g, rf['grad']) <= FOCAL_BAR
    assert seen == set(n for n, *_ in E.box_specs(*E.SETS[set_name]))


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('gamma', E.GAMMAS)
def test_oracle_focal_on_the_edge_set(oracle_lib, gamma, bf16):
    wg = ws = 0.0
    for C in E.FOCAL_C:
        for HW in sorted(E.FOCAL_HW):
            f = E.focal_level(HW, C, bf16)
            for eta in (None,) + E.ETAS:
                ref = R.focal(f['cls'], f['labels'], f['lw'], E.A, gamma, E.ALPHA, GS,
                              None if eta is None else f['anchor_iou'], eta)
                assert E.finite(ref['grad'], ref['sum']), (gamma, C, HW, eta)
                if eta is None:
                    s, g = oracle_lib.focal_loss(f['cls'], f['labels'], f['lw'], E.A, gamma, E.ALPHA,
                                                 gscale=GS)
                else:
                    s, g, _ = oracle_lib.focal_loss_balanced(f['cls'], f['labels'], f['lw'],
                                                             f['anchor_iou'], E.A, gamma, E.ALPHA, eta,
                                                             gscale=GS)
                assert E.finite(g, s), (gamma, C, HW, eta)
                wg, ws = max(wg, E.share_of_max(g, ref['grad'])), max(ws, rel(s, ref['sum']))
    note('focal gamma %g grad' % gamma, wg)
    note('focal gamma %g sum' % gamma, ws)
    assert wg <= FOCAL_BAR and ws <= FOCAL_BAR, (gamma, wg, ws)
