"""CPU: plain FCOS (FCOSHead) -- the three reference configs build with the reference's parameter
names and shapes, the mmdet.* aliases, the ia_point_ctr_* C-ABI entries, and the argument checks
of the new device ops (fixtures: tests/golden/fcos_plain_*, written by
tests/golden/make_golden_fcos_plain.py)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import synth_fcos

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
CONFIGS = ['fcos_r50_caffe_fpn_gn_1x_4gpu', 'fcos_mstrain_640_800_r101_caffe_fpn_gn_2x_4gpu',
           'fcos_mstrain_640_800_x101_64x4d_fpn_gn_2x']


def _ref():
    with open(os.path.join(GOLD, 'fcos_plain_ref.json')) as fh:
        return json.load(fh)


def _build(tmp_path, name):
    import iouaware
    from iouaware.config import Config
    rec = _ref()[name]
    path = tmp_path / (name + '.py')
    path.write_text('\n'.join('%s = %r' % (k, rec[k]) for k in ('model', 'train_cfg', 'test_cfg')) + '\n')
    cfg = Config.fromfile(str(path))
    cfg.model['pretrained'] = None
    return cfg, iouaware.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)


@pytest.mark.parametrize('name', CONFIGS)
def test_plain_configs_build_with_reference_state_dict(tmp_path, name):
    from iouaware.detectors import FCOS
    from iouaware.fcos_head import FCOSHead, IoUawareFCOSHead
    cfg, m = _build(tmp_path, name)
    assert isinstance(m, FCOS) and type(m.bbox_head) is FCOSHead
    assert not isinstance(m.bbox_head, IoUawareFCOSHead)
    ours = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert ours == _ref()[name]['state_dict']
    assert not hasattr(m.bbox_head, 'fcos_iou')


def test_plain_head_forward_and_signatures():
    import inspect
    from iouaware.fcos_head import FCOSHead
    head = FCOSHead(81, 256, strides=[8, 16, 32, 64, 128]).eval()
    feats = [torch.randn(1, 256, h, w) for (h, w) in synth_fcos.level_shapes(64, 96)]
    with torch.no_grad():
        outs = head(feats)
    assert len(outs) == 3 and all(len(o) == 5 for o in outs)
    assert outs[0][0].shape[1] == 80 and outs[1][0].shape[1] == 4 and outs[2][0].shape[1] == 1
    assert list(inspect.signature(FCOSHead.get_bboxes).parameters) == [
        'self', 'cls_scores', 'bbox_preds', 'centernesses', 'img_metas', 'cfg', 'rescale']
    assert list(inspect.signature(FCOSHead.loss).parameters) == [
        'self', 'cls_scores', 'bbox_preds', 'centernesses', 'gt_bboxes', 'gt_labels', 'img_metas',
        'cfg', 'gt_bboxes_ignore']


def test_plain_fcos_compat_aliases():
    from iouaware import compat, fcos_head
    compat.install()
    import mmdet.models
    import mmdet.models.anchor_heads
    assert mmdet.models.FCOSHead is fcos_head.FCOSHead
    assert mmdet.models.anchor_heads.FCOSHead is fcos_head.FCOSHead
    assert mmdet.models.anchor_heads.IoUawareFCOSHead is fcos_head.IoUawareFCOSHead


def test_point_ctr_entries_declared_and_exported():
    from iouaware import _lib
    text = open(os.path.join(HERE, '..', 'include', 'iouaware.h')).read()
    so = ctypes.CDLL(_lib.SO_PATH)
    for name in ('ia_point_ctr_decode_stage', 'ia_point_ctr_get_bboxes'):
        assert name in text and name in _lib.SIGNATURES
        assert hasattr(so, name)
    # same arguments as ia_point_get_bboxes; the decode stage additionally takes score_thr
    assert _lib.SIGNATURES['ia_point_ctr_get_bboxes'] == _lib.SIGNATURES['ia_point_get_bboxes']
    args = _lib.SIGNATURES['ia_point_decode_stage'][1]
    assert _lib.SIGNATURES['ia_point_ctr_decode_stage'][1] == args[:6] + [ctypes.c_float] + args[6:]


def test_point_ctr_ops_refuse_cpu_tensors():
    from iouaware import fcos_ops
    sizes = synth_fcos.level_shapes(64, 96)
    geom = fcos_ops.PointGeometry(sizes, synth_fcos.STRIDES, 80, 100)
    cls = [torch.zeros((1, 80, h, w)) for (h, w) in sizes]
    reg = [torch.ones((1, 4, h, w)) for (h, w) in sizes]
    ctr = [torch.zeros((1, 1, h, w)) for (h, w) in sizes]
    meta = [(64, 96, 3)], [1.0]
    from iouaware._lib import IouAwareLibraryError
    with pytest.raises(IouAwareLibraryError, match='centerness|cls_score'):
        fcos_ops.point_ctr_get_bboxes(geom, cls, reg, ctr, *meta, True, 0.05, 0.5, 100)
    with pytest.raises(IouAwareLibraryError, match='centerness|cls_score'):
        fcos_ops.point_ctr_decode_stage(geom, cls, reg, ctr, *meta, True, 0.05)


@pytest.mark.parametrize('bad', [-0.25, float('nan'), float('inf')])
def test_multiclass_nms_rejects_bad_score_factors(bad):
    from iouaware.nms_op import multiclass_nms
    rs = np.random.RandomState(0)
    xy = rs.uniform(0, 50, (6, 2))
    boxes = torch.from_numpy(np.concatenate([xy, xy + 10], 1).astype(np.float32))
    scores = torch.from_numpy(rs.uniform(0, 1, (6, 4)).astype(np.float32))
    f = torch.full((6,), 0.5)
    f[3] = bad
    with pytest.raises(ValueError):
        multiclass_nms(boxes, scores, 0.05, dict(type='nms', iou_thr=0.5), 100, score_factors=f)
    with pytest.raises(ValueError):             # one factor per box
        multiclass_nms(boxes, scores, 0.05, dict(type='nms', iou_thr=0.5), 100,
                       score_factors=torch.ones(5))


def test_per_image_fallback_passes_gt_arguments_only_to_heads_that_take_them(tmp_path):
    """SingleStageDetector.simple_test_batch without the batched device route: the IoU-aware
    heads' get_bboxes takes gt_bboxes / gt_labels (the fork's signature), FCOSHead's does not"""
    _, m = _build(tmp_path, CONFIGS[0])
    seen = {}

    def plain_get_bboxes(cls_scores, bbox_preds, centernesses, img_metas, cfg, rescale=None):
        seen['plain'] = (img_metas, rescale)
        return [(torch.zeros((0, 5)), torch.zeros((0,), dtype=torch.long))]

    def iou_get_bboxes(cls_scores, bbox_preds, centernesses, ious, gt_bboxes, gt_labels, img_metas,
                       cfg, rescale=None):
        seen['iou'] = (gt_bboxes, img_metas, rescale)
        return [(torch.zeros((0, 5)), torch.zeros((0,), dtype=torch.long))]

    meta = [dict(img_shape=(32, 32, 3), scale_factor=1.0)]
    m.forward_head = lambda img: ([1], [2], [3])
    m.bbox_head.get_bboxes = plain_get_bboxes
    res = m.simple_test_batch(torch.zeros(1, 3, 32, 32), meta, 'gtb', 'gtl', rescale=True)
    assert seen['plain'] == (meta, True) and len(res) == 1 and len(res[0]) == 80
    m.forward_head = lambda img: ([1], [2], [3], [4])
    m.bbox_head.get_bboxes = iou_get_bboxes
    m.simple_test_batch(torch.zeros(1, 3, 32, 32), meta, 'gtb', 'gtl', rescale=True)
    assert seen['iou'] == ('gtb', meta, True)
