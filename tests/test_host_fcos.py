"""CPU: the IoU-aware FCOS detector builds from the reference config and matches the reference's
parameter names, pure helpers and head forward (fixtures: tests/golden/fcos_*, written by
tests/golden/make_golden_fcos.py)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import synth_fcos

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')


def _ref():
    with open(os.path.join(GOLD, 'fcos_ref.json')) as fh:
        return json.load(fh)


def _config_file(tmp_path):
    """the reference config's settings written back as a config file"""
    path = tmp_path / 'iou_aware_fcos_r50_caffe_fpn_gn_1x_4gpu.py'
    cfg = _ref()['config']
    path.write_text('\n'.join('%s = %r' % (k, v) for k, v in sorted(cfg.items())) + '\n')
    return str(path)


def _model(tmp_path, seed=None):
    import iouaware
    from iouaware.config import Config
    cfg = Config.fromfile(_config_file(tmp_path))
    cfg.model['pretrained'] = None
    m = iouaware.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    if seed is not None:
        state = m.state_dict()
        synth_fcos.fill_state(state, seed)
        m.load_state_dict(state)
    return cfg, m


def test_fcos_config_builds_with_reference_state_dict(tmp_path):
    from iouaware.detectors import FCOS
    from iouaware.fcos_head import IoUawareFCOSHead
    _, m = _model(tmp_path)
    assert isinstance(m, FCOS) and isinstance(m.bbox_head, IoUawareFCOSHead)
    ours = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert ours == _ref()['state_dict']
    assert m.bbox_head.score_alpha == 0.3
    assert m.backbone.style == 'caffe'


def test_fcos_compat_aliases():
    from iouaware import bbox, compat, detectors, fcos_head, layers, losses
    compat.install()
    import mmdet.core
    import mmdet.models.anchor_heads
    import mmdet.models.detectors
    import mmdet.models.utils
    assert mmdet.models.detectors.FCOS is detectors.FCOS
    assert mmdet.models.anchor_heads.IoUawareFCOSHead is fcos_head.IoUawareFCOSHead
    assert mmdet.core.distance2bbox is bbox.distance2bbox
    assert mmdet.core.iou_loss is losses.iou_loss
    assert mmdet.models.utils.Scale is layers.Scale


def test_get_points_and_targets_match_reference():
    from iouaware.fcos_head import IoUawareFCOSHead
    g = np.load(os.path.join(GOLD, 'fcos_helpers.npz'))
    head = IoUawareFCOSHead(81, 256, strides=[8, 16, 32, 64, 128])
    sizes = [tuple(s) for s in g['sizes']]
    pts = head.get_points(sizes, torch.float32, 'cpu')
    for l, p in enumerate(pts):
        assert np.array_equal(p.numpy(), g['points_%d' % l])
    gb = [torch.from_numpy(g['gt_bboxes_%d' % i]) for i in range(2)]
    gl = [torch.from_numpy(g['gt_labels_%d' % i]) for i in range(2)]
    labels, targets = head.fcos_target(pts, gb, gl)
    for l in range(len(sizes)):
        assert np.array_equal(labels[l].numpy(), g['labels_%d' % l])
        assert np.array_equal(targets[l].numpy(), g['bbox_targets_%d' % l])
    flat_l, flat_t = torch.cat(labels), torch.cat(targets)
    pos = flat_l.nonzero().reshape(-1)
    assert len(pos) > 0
    assert np.array_equal(head.centerness_target(flat_t[pos]).numpy(), g['centerness'])


def test_distance2bbox_matches_reference():
    from iouaware.bbox import distance2bbox
    g = np.load(os.path.join(GOLD, 'fcos_helpers.npz'))
    p, d = torch.from_numpy(g['d2b_points']), torch.from_numpy(g['d2b_dist'])
    assert np.array_equal(distance2bbox(p, d).numpy(), g['d2b_free'])
    assert np.array_equal(distance2bbox(p, d, max_shape=(200, 264, 3)).numpy(), g['d2b_clamped'])


def test_head_forward_matches_reference(tmp_path):
    g = np.load(os.path.join(GOLD, 'fcos_forward.npz'))
    _, m = _model(tmp_path, seed=int(g['seed']))
    head = m.bbox_head.eval()
    rs = np.random.RandomState(int(g['feat_seed']))
    feats = [torch.from_numpy(rs.standard_normal((2, 256, h, w)).astype(np.float32))
             for (h, w) in g['sizes']]
    with torch.no_grad():
        outs = head(feats)
    for kind, ts in zip(('cls', 'bbox', 'ctr', 'iou'), outs):
        for l, t in enumerate(ts):
            ref = g['%s_%d' % (kind, l)]
            scale = max(1.0, float(np.abs(ref).max()))
            assert np.abs(t.numpy() - ref).max() <= 1e-5 * scale, (kind, l)


def test_point_geometry_struct_mirrors_header():
    from iouaware import _lib
    # num_levels, num_classes, nms_pre + H, W, stride (8 each) + layout + score_alpha
    assert ctypes.sizeof(_lib.PointHeadGeom) == 3 * 4 + 3 * 8 * 4 + 4 + 4
    assert _lib.PointHeadGeom.score_alpha.offset == ctypes.sizeof(_lib.PointHeadGeom) - 4
    text = open(os.path.join(HERE, '..', 'include', 'iouaware.h')).read()
    for name in ('ia_point_get_bboxes', 'ia_point_decode_stage', 'ia_point_workspace_bytes',
                 'ia_groupnorm_stats', 'ia_groupnorm_apply', 'ia_groupnorm_workspace_bytes',
                 'ia_scale_exp_levels'):
        assert name in text and name in _lib.SIGNATURES
        assert hasattr(ctypes.CDLL(_lib.SO_PATH), name)


def test_point_workspace_is_the_anchor_workspace_of_one_anchor():
    """the point head shares the anchor head's workspace carve-up (A = 1); sizes on the host"""
    from iouaware import _lib, fcos_ops, ops
    sizes = synth_fcos.level_shapes(800, 1344)
    pg = fcos_ops.PointGeometry(sizes, synth_fcos.STRIDES, 80, nms_pre=1000)
    hg = ops.HeadGeometry(sizes, synth_fcos.STRIDES, np.zeros((5, 1, 4), np.float32), 80, nms_pre=1000)
    L = _lib.lib()
    assert (pg.N, pg.R, pg.Rs) == (hg.N, hg.R, hg.Rs) == (22400, 3350, 3392)
    assert L.ia_point_workspace_bytes(pg.ref(), 8) == L.ia_get_bboxes_workspace_bytes(hg.ref(), 8) > 0
    bad = fcos_ops.PointGeometry(sizes, synth_fcos.STRIDES, 80, nms_pre=1000, score_alpha=1.5)
    assert L.ia_point_workspace_bytes(bad.ref(), 8) == 0


def test_groupnorm_workspace_sizes():
    from iouaware import _lib, fcos_ops
    xs = [torch.empty((8, 512, h, w)) for (h, w) in synth_fcos.level_shapes(800, 1344)]
    g = fcos_ops._wino_geom(xs)
    L = _lib.lib()
    chunks = sum((h * w + 255) // 256 for (h, w) in synth_fcos.level_shapes(800, 1344))
    assert L.ia_groupnorm_workspace_bytes(ctypes.byref(g), 512, 64) == 8 * chunks * 64 * 16
    assert L.ia_groupnorm_workspace_bytes(ctypes.byref(g), 512, 48) == 0      # 512 % 48
    assert L.ia_groupnorm_workspace_bytes(ctypes.byref(g), 384, 32) == 0      # not a power of 2


def test_fcos_ops_refuse_cpu_tensors():
    from iouaware import fcos_ops
    x = torch.zeros((1, 512, 4, 4)).contiguous(memory_format=torch.channels_last)
    with pytest.raises(Exception):
        fcos_ops.groupnorm_relu_([x], torch.ones(512), torch.zeros(512), 64)
