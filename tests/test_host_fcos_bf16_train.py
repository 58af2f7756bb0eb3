"""CPU: the opt-in bf16 training route of the FCOS heads (conv3x3_bf16_train.fcos_head_forward,
fcos_ops.groupnorm_relu_bf16) -- off by default, its C entry points declared and bound, the module
side of the route's coverage answered without a device, and the node's argument contract."""
import json
import os

import pytest
import torch

import synth
from test_capi_symbols import declared_functions

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
ENTRIES = ('ia_groupnorm_saved_bytes_dt', 'ia_groupnorm_apply_to_dt', 'ia_groupnorm_bwd_workspace_bytes_dt',
           'ia_groupnorm_bwd_reduce_dt', 'ia_groupnorm_bwd_apply_dt')


def _heads(**kw):
    from iouaware.fcos_head import FCOSHead, IoUawareFCOSHead
    kw = dict(dict(num_classes=81, in_channels=256), **kw)
    return [cls(**kw) for cls in (FCOSHead, IoUawareFCOSHead)]


def _built(name):
    import iouaware
    from iouaware.config import ConfigDict
    if name == 'iou':
        with open(os.path.join(GOLD, 'fcos_ref.json')) as fh:
            rec = json.load(fh)['config']
    else:
        with open(os.path.join(GOLD, 'fcos_plain_ref.json')) as fh:
            rec = json.load(fh)['fcos_r50_caffe_fpn_gn_1x_4gpu']
    model = dict(rec['model'], pretrained=None)
    return iouaware.build_detector(ConfigDict(model), train_cfg=ConfigDict(rec['train_cfg']),
                                   test_cfg=ConfigDict(rec['test_cfg']))


def test_the_route_is_off_by_default():
    from iouaware.fcos_head import FCOSHead, IoUawareFCOSHead
    assert FCOSHead.train_bf16 is False and IoUawareFCOSHead.train_bf16 is False
    for head in _heads():
        assert head.train_bf16 is False and 'train_bf16' not in head.__dict__
    for name in ('iou', 'plain'):
        assert _built(name).bbox_head.train_bf16 is False


def test_entry_points_are_declared_and_exported():
    import ctypes
    from iouaware import _lib
    names = declared_functions()
    _lib.lib()
    h = ctypes.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert name in names and name in _lib.SIGNATURES and hasattr(h, name), name


def test_head_supported_answers_without_a_device():
    from iouaware import conv3x3_bf16_train as T, fcos_ops
    sizes = synth.level_shapes(800, 1344)
    assert len(sizes) == 5
    for head in _heads():
        assert T.fcos_head_supported(head, sizes, 4) is True
        assert T.fcos_head_supported(head, sizes[:1], 1) is True
        assert T.fcos_head_supported(head, sizes + sizes[:1], 4) is False          # more levels than scales
    gn = lambda n: dict(type='GN', num_groups=n, requires_grad=True)
    for kw in (dict(norm_cfg=gn(64)),                                               # 4 channels per group
               dict(feat_channels=48, norm_cfg=gn(6)),                              # no multiple of 32
               dict(in_channels=48),
               dict(norm_cfg=None),                                                 # bias + ReLU, no GroupNorm
               dict(feat_channels=96, norm_cfg=gn(12))):                            # 2F is no power of two
        for head in _heads(**kw):
            assert T.fcos_head_supported(head, sizes, 4) is False, kw
    for head in _heads():
        head.cls_convs[1].gn = torch.nn.GroupNorm(16, 256)                          # towers that differ
        assert T.fcos_head_supported(head, sizes, 4) is False
    # the library's own answer
    assert fcos_ops.groupnorm_bf16_supported(sizes, 4, 512, 64) is True
    assert fcos_ops.groupnorm_bf16_supported(sizes, 4, 512, 128) is False           # fp32 takes it:
    assert fcos_ops.groupnorm_supported(sizes, 4, 512, 128) is True
    assert fcos_ops.groupnorm_bf16_supported(sizes, 4, 96, 12) is False
    assert fcos_ops.groupnorm_bf16_supported([(0, 4)], 1, 64, 8) is False


def test_cpu_features_fall_through_to_the_module_forward():
    from iouaware import conv3x3_bf16_train as T
    sizes = synth.level_shapes(64, 96)
    gn = dict(type='GN', num_groups=8, requires_grad=True)
    for head in _heads(num_classes=5, in_channels=64, feat_channels=64, stacked_convs=2, norm_cfg=gn):
        head.train()
        g = torch.Generator().manual_seed(2)
        feats = [torch.randn(2, 64, h, w, generator=g) for (h, w) in sizes]
        assert T.fcos_head_supported(head, sizes, 2) is True
        assert T.fcos_usable(feats, head) is False                                  # CPU features
        ref = head(feats)
        head.train_bf16 = True
        got = head(feats)
        assert len(got) == len(ref)
        for a, b in zip(got, ref):
            for x, y in zip(a, b):
                assert x.dtype == torch.float32 and torch.equal(x, y)


def test_node_rejects_cpu_and_fp32_input():
    from iouaware import fcos_ops
    g, b = torch.ones(64), torch.zeros(64)
    cl = torch.channels_last
    for x in (torch.zeros(1, 64, 4, 4, dtype=torch.bfloat16).contiguous(memory_format=cl),     # CPU
              torch.zeros(1, 64, 4, 4).contiguous(memory_format=cl)):                          # CPU, fp32
        with pytest.raises(ValueError):
            fcos_ops.groupnorm_relu_bf16([x], g, b, 8)
    with pytest.raises(ValueError):
        fcos_ops.groupnorm_relu_bf16([], g, b, 8)
