"""CPU: plain RetinaNet (RetinaHead) -- the nine reference configs build with the reference's
parameter names, shapes and order, the mmdet.* aliases, the argument checks, and the new score
kinds of the C-ABI (fixtures: tests/golden/retina_plain_*, written by
tests/golden/make_golden_retina_plain.py)."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
REF = '/root/reference'


def _ref():
    with open(os.path.join(GOLD, 'retina_plain_ref.json')) as fh:
        return json.load(fh)


def _build_rec(tmp_path, name, rec):
    import iouaware
    from iouaware.config import Config
    path = tmp_path / (name + '.py')
    path.write_text('\n'.join('%s = %r' % (k, rec[k]) for k in ('model', 'train_cfg', 'test_cfg')) + '\n')
    cfg = Config.fromfile(str(path))
    cfg.model['pretrained'] = None
    return cfg, iouaware.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)


@pytest.mark.parametrize('name', sorted(json.load(open(os.path.join(GOLD, 'retina_plain_ref.json')))))
def test_plain_configs_build_with_reference_state_dict(tmp_path, name):
    from iouaware.detectors import RetinaNet
    from iouaware.head import IoUawareRetinaHead, RetinaHead
    cfg, m = _build_rec(tmp_path, name, _ref()[name])
    assert isinstance(m, RetinaNet) and type(m.bbox_head) is RetinaHead
    assert not isinstance(m.bbox_head, IoUawareRetinaHead)
    ours = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert ours == _ref()[name]['state_dict']
    assert not hasattr(m.bbox_head, 'retina_iou')


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'configs')), reason='reference tree absent')
def test_every_reference_retinanet_config_builds():
    """every configs/retinanet_*.py of the reference, read as it is"""
    import glob
    import iouaware
    from iouaware.config import Config
    from iouaware.head import RetinaHead
    paths = sorted(glob.glob(os.path.join(REF, 'configs', 'retinanet_*.py')))
    assert len(paths) == 9
    for p in paths:
        cfg = Config.fromfile(p)
        cfg.model['pretrained'] = None
        m = iouaware.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
        assert type(m.bbox_head) is RetinaHead, p


def test_plain_head_forward_and_signatures():
    from iouaware.head import RetinaHead
    head = RetinaHead(81, 256).eval()
    head.init_weights()
    feats = [torch.randn(1, 256, h, w) for (h, w) in synth.level_shapes(64, 96)]
    with torch.no_grad():
        outs = head(feats)
    assert len(outs) == 2 and all(len(o) == 5 for o in outs)
    assert outs[0][0].shape[1] == 9 * 80 and outs[1][0].shape[1] == 9 * 4
    assert list(inspect.signature(RetinaHead.get_bboxes).parameters) == [
        'self', 'cls_scores', 'bbox_preds', 'gt_bboxes', 'gt_labels', 'img_metas', 'cfg', 'rescale']
    assert list(inspect.signature(RetinaHead.loss).parameters) == [
        'self', 'cls_scores', 'bbox_preds', 'gt_bboxes', 'gt_labels', 'img_metas', 'cfg',
        'gt_bboxes_ignore']
    assert [k for k, _ in head.named_parameters()][-4:] == [
        'retina_cls.weight', 'retina_cls.bias', 'retina_reg.weight', 'retina_reg.bias']


def test_iou_aware_head_keeps_its_branch():
    from iouaware.head import IoUawareRetinaHead
    head = IoUawareRetinaHead(81, 256)
    assert head.iou_branch and hasattr(head, 'retina_iou')
    g = head.geometry([(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)], 100)
    assert g.iou_branch and g.struct.cls_activation == 0


def test_plain_geometry_uses_the_noiou_kinds():
    from iouaware import _lib
    from iouaware.head import RetinaHead
    sizes = [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
    g = RetinaHead(81, 256).geometry(sizes, 100)
    assert not g.iou_branch and g.struct.cls_activation == _lib.IA_CLS_SIGMOID_NOIOU
    soft = RetinaHead(81, 256, loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False,
                                             loss_weight=1.0)).geometry(sizes, 100)
    assert soft.softmax and soft.struct.cls_activation == _lib.IA_CLS_SOFTMAX_NOIOU
    from iouaware.head import IoUawareRetinaHead
    assert g.key != IoUawareRetinaHead(81, 256).geometry(sizes, 100).key


def test_plain_retina_compat_aliases():
    from iouaware import compat, head
    compat.install()
    import mmdet.models
    import mmdet.models.anchor_heads
    assert mmdet.models.RetinaHead is head.RetinaHead
    assert mmdet.models.anchor_heads.RetinaHead is head.RetinaHead
    assert mmdet.models.anchor_heads.IoUawareRetinaHead is head.IoUawareRetinaHead


@pytest.mark.parametrize('kw', ['loss_iou', 'attach_iou_target'])
def test_iou_kwargs_are_rejected(kw):
    from iouaware.head import RetinaHead
    with pytest.raises(TypeError, match=kw):
        RetinaHead(81, 256, **{kw: dict(type='CrossEntropyLoss') if kw == 'loss_iou' else True})


@pytest.mark.parametrize('which', ['cls', 'bbox'])
def test_iou_balanced_losses_raise_named_error_at_loss_time(which):
    from iouaware.config import ConfigDict
    from iouaware.head import RetinaHead
    kw = dict(loss_cls=dict(type='IOUbalancedSigmoidFocalLoss', use_sigmoid=True, gamma=2.0,
                            alpha=0.25, eta=1.5, loss_weight=1.0)) if which == 'cls' else \
        dict(loss_bbox=dict(type='IoUbalancedSmoothL1Loss', beta=0.11, delta=1.5, loss_weight=1.0))
    head = RetinaHead(81, 256, **kw)
    name = 'IOUbalancedSigmoidFocalLoss' if which == 'cls' else 'IoUbalancedSmoothL1Loss'
    sizes = synth.level_shapes(64, 96)
    cls = [torch.zeros(1, 720, h, w) for h, w in sizes]
    reg = [torch.zeros(1, 36, h, w) for h, w in sizes]
    with pytest.raises(NotImplementedError, match=name):
        head.loss(cls, reg, [torch.zeros(1, 4)], [torch.ones(1, dtype=torch.long)],
                  [dict(pad_shape=(64, 96, 3), img_shape=(64, 96, 3))], ConfigDict())


@pytest.mark.parametrize('component,missing', [('neck', 'BFP'), ('bbox_head', 'GARetinaHead')])
def test_out_of_scope_components_fail_at_their_registry(tmp_path, component, missing):
    """GHM / Libra / GA-RetinaNet get past the head now and fail naming the missing component"""
    import copy
    rec = copy.deepcopy(_ref()['retinanet_r50_fpn_1x'])
    rec['model'][component] = dict(rec['model'][component], type=missing)
    with pytest.raises(KeyError, match=missing):
        _build_rec(tmp_path, 'x', rec)
    rec = copy.deepcopy(_ref()['retinanet_r50_fpn_1x'])
    rec['model']['bbox_head']['loss_cls'] = dict(type='GHMC', bins=30, momentum=0.75,
                                                 use_sigmoid=True, loss_weight=1.0)
    with pytest.raises(KeyError, match='GHMC'):
        _build_rec(tmp_path, 'y', rec)


def test_plain_ops_refuse_cpu_tensors():
    from iouaware import ops
    from iouaware._lib import IouAwareLibraryError
    from iouaware.config import ConfigDict
    from iouaware.head import RetinaHead
    head = RetinaHead(81, 256)
    sizes = synth.level_shapes(64, 96)
    cls = [torch.zeros(1, 720, h, w) for h, w in sizes]
    reg = [torch.zeros(1, 36, h, w) for h, w in sizes]
    cfg = ConfigDict(nms_pre=100, score_thr=0.05, nms=dict(type='nms', iou_thr=0.5), max_per_img=100)
    meta = [dict(img_shape=(64, 96, 3), scale_factor=1.0, pad_shape=(64, 96, 3))]
    with pytest.raises(IouAwareLibraryError, match='cls_score'):
        head.get_bboxes(cls, reg, None, None, meta, cfg, True)
    with pytest.raises(IouAwareLibraryError):
        head.loss(cls, reg, [torch.zeros(1, 4)], [torch.ones(1, dtype=torch.long)], meta,
                  ConfigDict())
    geom = head.geometry(sizes, 100)
    with pytest.raises(ValueError, match='without the IoU branch'):      # no IoU map for this kind
        ops.level_ptrs(geom, cls, reg, [torch.zeros(1, 9, h, w) for h, w in sizes])


def test_noiou_constants_declared_and_rejected_values():
    """IA_CLS_SIGMOID_NOIOU / IA_CLS_SOFTMAX_NOIOU in the header and _lib; the geometry helper takes
    them, and values past them are still an argument error"""
    from iouaware import _lib
    text = open(os.path.join(HERE, '..', 'include', 'iouaware.h')).read()
    assert '#define IA_CLS_SIGMOID_NOIOU 2' in text and '#define IA_CLS_SOFTMAX_NOIOU 3' in text
    assert (_lib.IA_CLS_SIGMOID_NOIOU, _lib.IA_CLS_SOFTMAX_NOIOU) == (2, 3)
    so = ctypes.CDLL(_lib.SO_PATH)
    g = _lib.HeadGeom()
    g.num_levels, g.num_anchors, g.num_classes, g.nms_pre = 1, 1, 80, 10
    g.H[0], g.W[0], g.stride[0] = 4, 4, 8
    for k in range(4):
        g.stds[k] = 1.0
    n, r, rs = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    for act, rc in ((0, 0), (1, 0), (2, 0), (3, 0), (4, -1), (-1, -1)):
        g.cls_activation = act
        assert so.ia_geom_sizes(ctypes.byref(g), ctypes.byref(n), ctypes.byref(r),
                                ctypes.byref(rs)) == rc, act
    assert n.value == 16 and r.value == 10


def test_plain_get_bboxes_fixture_is_small_and_consistent():
    f = np.load(os.path.join(GOLD, 'retina_plain_get_bboxes.npz'))
    assert os.path.getsize(os.path.join(GOLD, 'retina_plain_get_bboxes.npz')) < 1 << 20
    for k in range(2):
        seed, B, ph, pw, nms_pre, rescale = [int(v) for v in f['case_%d' % k]]
        for b in range(B):
            d, l = f['dets_%d_%d' % (k, b)], f['labels_%d_%d' % (k, b)]
            assert d.shape == (l.shape[0], 5) and 0 < d.shape[0] <= 100
            assert (l >= 0).all() and (l < 80).all() and (d[:, 4] > 0.05).all()
