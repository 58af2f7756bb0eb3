"""CPU side of the FCOS loss node on channels-last rows (ia_point_head_loss_*_nhwc,
fcos_ops.point_head_loss_packed, _FCOSHeadBase.forward_loss): the entries are exported with the
header's prototypes declared in _lib, the size query refuses what the kernels do not cover, the op
refuses CPU tensors and malformed rows before the device is touched, and the head's switch is off by
default and falls back on a CPU model."""
import ctypes
import os
import re

import pytest
import torch

import synth_fcos_loss as S

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
ENTRIES = ('ia_point_head_loss_nhwc_workspace_bytes', 'ia_point_head_loss_fwd_nhwc',
           'ia_point_head_loss_bwd_nhwc')
SIZES = S.synth_fcos.level_shapes(128, 160)


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'iouaware.h')).read(), flags=re.S)


def test_entries_are_declared_bound_and_exported():
    from iouaware import _lib
    text = _header()
    h = ctypes.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        m = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % name, text)
        assert m, '%s not declared' % name
        assert name in _lib.SIGNATURES, '%s not bound' % name
        assert hasattr(h, name), '%s not exported' % name
        # one ctypes argument per parameter of the header's prototype
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(',')), name
    assert re.search(r'\}\s*ia_point_pix_strides\s*;', text)
    assert ctypes.sizeof(_lib.PointPixStrides) == 4 * 8 * 8 and _lib.PointPixStrides.iou.offset == 3 * 8 * 8
    # the structs the NCHW entries take are as they were
    assert ctypes.sizeof(_lib.PointLossCfg) == 16 and ctypes.sizeof(_lib.PointTargets) == 2 * 8 * 8 + 2 * 8
    lib = _lib.lib()
    assert lib.ia_point_head_loss_fwd_nhwc.argtypes[3] is ctypes.c_int            # dtype
    assert lib.ia_point_head_loss_bwd_nhwc.argtypes[14] is ctypes.c_int           # grad_rows_packed


def test_workspace_query_and_argument_checks_need_no_device():
    from iouaware import _lib, fcos_ops
    L = _lib.lib()
    g = fcos_ops.PointGeometry(SIZES, S.STRIDES, S.C)
    assert L.ia_point_head_loss_nhwc_workspace_bytes(g.ref(), 2) > 0
    assert L.ia_point_head_loss_nhwc_workspace_bytes(g.ref(), 0) == 0
    assert L.ia_point_head_loss_nhwc_workspace_bytes(None, 2) == 0
    bad = fcos_ops.PointGeometry(SIZES, S.STRIDES, S.C)
    bad.struct.num_levels = 9
    assert L.ia_point_head_loss_nhwc_workspace_bytes(bad.ref(), 2) == 0
    odd = fcos_ops.PointGeometry(SIZES, S.STRIDES, 81)                   # class quads: C % 4 == 0
    assert L.ia_point_head_loss_nhwc_workspace_bytes(odd.ref(), 2) == 0
    assert not fcos_ops.point_loss_packed_supported(odd, 2) and fcos_ops.point_loss_packed_supported(g, 2)
    assert L.ia_point_head_loss_fwd_nhwc(g.ref(), None, None, 0, 2, None, None, None, None, 0, None, None) == -1
    assert L.ia_point_head_loss_bwd_nhwc(g.ref(), None, None, 0, 2, None, None, None, None, 0, None, None,
                                         None, None, 1, None, None) == -1


def _rows(wc=84, wr=8, dtype=torch.float32, levels=SIZES):
    cl = lambda w, h, ww: torch.zeros(2, h, ww, w, dtype=dtype).permute(0, 3, 1, 2)   # noqa: E731
    return [cl(wc, h, w) for (h, w) in levels], [cl(wr, h, w) for (h, w) in levels]


def test_packed_op_refuses_misuse_before_the_device():
    from iouaware import _lib, fcos_ops
    g = fcos_ops.PointGeometry(SIZES, S.STRIDES, S.C)
    scales = [torch.ones(1) for _ in SIZES]
    tail = (None, None, None, 2.0, 0.25)
    cc, ri = _rows()
    with pytest.raises(_lib.IouAwareLibraryError, match='no CPU'):
        fcos_ops.point_head_loss_packed(g, cc, ri, scales, *tail)
    with pytest.raises(ValueError, match='levels'):
        fcos_ops.point_head_loss_packed(g, cc[:-1], ri[:-1], scales, *tail)
    with pytest.raises(ValueError, match='scales'):
        fcos_ops.point_head_loss_packed(g, cc, ri, scales[:-1], *tail)
    # (CPU tensors throughout: the shape and dtype checks come before the device check)
    cc16 = _rows(dtype=torch.bfloat16)[0]
    with pytest.raises(TypeError, match='one dtype'):
        fcos_ops.point_head_loss_packed(g, cc16, ri, scales, *tail)
    narrow_c, narrow_r = _rows(wc=80, wr=4)
    with pytest.raises(ValueError, match='too narrow'):
        fcos_ops.point_head_loss_packed(g, narrow_c, ri, scales, *tail)
    with pytest.raises(ValueError, match='too narrow'):
        fcos_ops.point_head_loss_packed(g, cc, narrow_r, scales, *tail, with_iou=True)
    nchw = [t.contiguous() for t in cc]
    with pytest.raises(ValueError, match='channels-last'):
        fcos_ops.point_head_loss_packed(g, nchw, ri, scales, *tail)
    with pytest.raises(ValueError, match='shape'):
        fcos_ops.point_head_loss_packed(g, cc[::-1], ri, scales, *tail)


def _detector(fuse):
    import iouaware
    from iouaware.config import ConfigDict
    torch.manual_seed(0)
    model = dict(type='FCOS', pretrained=None,
                 backbone=dict(type='ResNet', depth=18, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=-1,
                               style='pytorch'),
                 neck=dict(type='FPN', in_channels=[64, 128, 256, 512], out_channels=32, start_level=1,
                           add_extra_convs=True, extra_convs_on_inputs=False, num_outs=5,
                           relu_before_extra_convs=True),
                 bbox_head=dict(type='IoUawareFCOSHead', num_classes=5, in_channels=32, stacked_convs=1,
                                feat_channels=32, strides=[8, 16, 32, 64, 128],
                                norm_cfg=dict(type='GN', num_groups=8, requires_grad=True)))
    m = iouaware.build_detector(ConfigDict(model), train_cfg=ConfigDict(dict(gamma=2.0, alpha=0.25)),
                                test_cfg=None).train()
    m.bbox_head.fuse_head_loss = fuse
    return m


def test_switch_is_off_by_default_and_falls_back_on_the_cpu(monkeypatch):
    from iouaware import fcos_head
    from iouaware.fcos_head import FCOSHead, IoUawareFCOSHead, _FCOSHeadBase
    assert _FCOSHeadBase.fuse_head_loss is False
    assert FCOSHead.fuse_head_loss is False and IoUawareFCOSHead.fuse_head_loss is False
    img = torch.randn(2, 3, 64, 96)
    gb = [torch.tensor([[4.5, 6.5, 50.0, 40.0], [30.5, 20.5, 90.0, 60.0]]), torch.tensor([[10.5, 8.5, 80.0, 55.0]])]
    gl = [torch.tensor([1, 3]), torch.tensor([2])]
    res, called = {}, []
    real = _FCOSHeadBase.forward_loss
    monkeypatch.setattr(_FCOSHeadBase, 'forward_loss',
                        lambda self, *a, **k: (called.append(1), real(self, *a, **k))[1])
    with S.torch_route(cpu_focal=True):            # (the HIP focal op has no CPU form)
        for fuse in (False, True):
            m = _detector(fuse)
            m.bbox_head.train_winograd = m.bbox_head.train_bf16 = fuse
            res[fuse] = m.forward_train(img, [None, None], gb, gl)
            assert len(called) == int(fuse)
    assert list(res[True]) == list(res[False]) == ['loss_cls', 'loss_reg', 'loss_centerness', 'loss_iou']
    for k in res[False]:
        assert torch.equal(res[True][k], res[False][k]), k
