"""CPU: the training side of plain RetinaNet -- the fused head-loss entries accept the score kind
without the IoU term (host part: the workspace size), `ops.head_loss` checks the IoU maps against
the geometry before anything touches the device, the Winograd training route declines CPU
tensors for a head without `retina_iou`, and the reference fixture
(tests/golden/retina_plain_train.npz, written by tests/golden/make_golden_retina_plain_train.py)
holds what it documents."""
import ctypes
import os

import numpy as np
import pytest
import torch

import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')


def test_head_loss_workspace_bytes_takes_the_noiou_sigmoid_kind():
    """pure host code: non-zero for IA_CLS_SIGMOID_NOIOU and no larger than for IA_CLS_SIGMOID;
    0 (unsupported) for both softmax kinds"""
    from iouaware import _lib
    so = ctypes.CDLL(_lib.SO_PATH)
    so.ia_head_loss_workspace_bytes.restype = ctypes.c_size_t
    so.ia_head_loss_workspace_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int]
    g = _lib.HeadGeom()
    g.num_levels, g.num_anchors, g.num_classes, g.nms_pre = 2, 9, 80, -1
    for l, (h, w, s) in enumerate(((8, 12, 8), (4, 6, 16))):
        g.H[l], g.W[l], g.stride[l] = h, w, s
    for k in range(4):
        g.stds[k] = 1.0
    size = {}
    for act in (_lib.IA_CLS_SIGMOID, _lib.IA_CLS_SOFTMAX, _lib.IA_CLS_SIGMOID_NOIOU,
                _lib.IA_CLS_SOFTMAX_NOIOU):
        g.cls_activation = act
        size[act] = so.ia_head_loss_workspace_bytes(ctypes.byref(g), 2)
    assert size[_lib.IA_CLS_SIGMOID] > 0
    assert 0 < size[_lib.IA_CLS_SIGMOID_NOIOU] <= size[_lib.IA_CLS_SIGMOID]
    assert size[_lib.IA_CLS_SOFTMAX] == 0 and size[_lib.IA_CLS_SOFTMAX_NOIOU] == 0


def test_head_loss_checks_iou_maps_against_the_geometry_before_the_device():
    from iouaware import ops
    from iouaware.head import IoUawareRetinaHead, RetinaHead
    sizes = synth.level_shapes(64, 96)
    cls = [torch.zeros(1, 720, h, w) for h, w in sizes]
    reg = [torch.zeros(1, 36, h, w) for h, w in sizes]
    iou = [torch.zeros(1, 9, h, w) for h, w in sizes]
    tg = ([torch.zeros(1, h * w * 9, dtype=torch.long) for h, w in sizes],
          [torch.ones(1, h * w * 9) for h, w in sizes],
          [torch.zeros(1, h * w * 9, 4) for h, w in sizes],
          [torch.zeros(1, h * w * 9, 4) for h, w in sizes])
    with pytest.raises(ValueError, match='with the IoU branch'):
        ops.head_loss(IoUawareRetinaHead(81, 256).geometry(sizes, -1), cls, reg, None, *tg,
                      avg_factor=1.0)
    with pytest.raises(ValueError, match='without the IoU branch'):
        ops.head_loss(RetinaHead(81, 256).geometry(sizes, -1), cls, reg, iou, *tg, avg_factor=1.0)


def test_winograd_training_route_declines_cpu_tensors_for_the_plain_head():
    from iouaware import winograd_train
    from iouaware.head import RetinaHead
    feats = [torch.zeros(1, 256, h, w) for h, w in synth.level_shapes(64, 96)]
    assert winograd_train.usable(feats, RetinaHead(81, 256)) is False


def test_plain_head_shares_the_fused_training_switches():
    from iouaware.head import IoUawareRetinaHead, RetinaHead
    for cls in (RetinaHead, IoUawareRetinaHead):
        head = cls(81, 256)
        assert head.fuse_levels is True and head.train_winograd is True
        assert callable(head._fused_loss_ok)


def test_plain_train_fixture_is_small_and_holds_the_documented_keys():
    path = os.path.join(GOLD, 'retina_plain_train.npz')
    assert os.path.getsize(path) < 1000000
    f = np.load(path)
    want = {'gamma', 'alpha', 'beta', 'pos_iou_thr', 'neg_iou_thr'}
    for k in range(2):
        seed, B, ph, pw, ih, iw = [int(v) for v in f['case_%d' % k]]
        want |= {'case_%d' % k, 'loss_cls_%d' % k, 'loss_bbox_%d' % k, 'num_total_pos_%d' % k}
        for b in range(B):
            want |= {'gt_bboxes_%d_%d' % (k, b), 'gt_labels_%d_%d' % (k, b)}
            assert f['gt_bboxes_%d_%d' % (k, b)].shape == (f['gt_labels_%d_%d' % (k, b)].shape[0], 4)
        for l, (h, w) in enumerate(synth.level_shapes(ph, pw)):
            for nm, ch in (('cls', 720), ('reg', 36)):
                key = 'g_%s_%d_%d' % (nm, k, l)
                want |= {key, key + '_idx'}
                idx = f[key + '_idx']
                assert f[key].shape == idx.shape and idx.size <= 3000
                assert idx.min() >= 0 and idx.max() < B * ch * h * w
        assert f['loss_cls_%d' % k].shape == (5,) and (f['loss_cls_%d' % k] > 0).all()
        assert int(f['num_total_pos_%d' % k]) >= 1
    assert set(f.files) == want
    assert int((f['loss_bbox_0'] > 0).sum()) >= 3          # the box loss on several levels
    assert int((f['loss_bbox_1'] > 0).sum()) >= 1
    assert int(f['num_total_pos_1']) < int(f['num_total_pos_0'])
