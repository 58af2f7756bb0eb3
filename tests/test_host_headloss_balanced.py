"""CPU side of the IoU-balanced all-levels head-loss node: ia_head_loss_cfg grew at its end and the ctypes
twin with it, the sizing entry is declared, bound and exported, and the head's switch (`_fused_loss_ok`)
admits the balanced losses only on a head with the IoU branch and only with `fuse_balanced` set."""
import ctypes
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'iouaware.h')

OLD_FIELDS = ['gamma', 'alpha', 'loss_weight_cls', 'beta', 'loss_weight_bbox', 'attach_iou_target',
              'exact_large_logits', 'grad_rows_start_at_reg']
NEW_FIELDS = [('eta', ctypes.c_float), ('delta', ctypes.c_float), ('balanced_cls', ctypes.c_int32),
              ('balanced_loc', ctypes.c_int32)]


def test_cfg_struct_grew_at_its_end():
    from iouaware._lib import HeadLossCfg
    names = [f[0] for f in HeadLossCfg._fields_]
    assert names == OLD_FIELDS + [n for n, _ in NEW_FIELDS]
    assert ctypes.sizeof(HeadLossCfg) == 48
    for k, name in enumerate(OLD_FIELDS):                    # the old layout is unmoved
        assert getattr(HeadLossCfg, name).offset == 4 * k
    for k, (name, typ) in enumerate(NEW_FIELDS):
        assert getattr(HeadLossCfg, name).offset == 32 + 4 * k and dict(HeadLossCfg._fields_)[name] is typ


def test_header_declares_the_fields_in_the_same_order():
    txt = open(HEADER).read()
    body = re.search(r'typedef struct ia_head_loss_cfg \{(.*?)\} ia_head_loss_cfg;', txt, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    got = []
    for typ, names in re.findall(r'\b(float|int32_t)\s+([^;]+);', body):
        got += [(n.strip(), typ) for n in names.split(',')]
    from iouaware._lib import HeadLossCfg
    want = [(n, 'float' if t is ctypes.c_float else 'int32_t') for n, t in HeadLossCfg._fields_]
    assert got == want
    assert re.search(r'size_t ia_head_loss_workspace_bytes_cfg\(const ia_head_geom \*g, int batch,\s*'
                     r'const ia_head_loss_cfg \*cfg\);', txt)


def test_eight_positional_arguments_leave_the_new_fields_zero():
    from iouaware._lib import HeadLossCfg
    hc = HeadLossCfg(2.0, 0.25, 1.0, 0.11, 1.0, 1, 0, 1)
    assert (hc.eta, hc.delta, hc.balanced_cls, hc.balanced_loc) == (0.0, 0.0, 0, 0)
    assert hc.grad_rows_start_at_reg == 1 and hc.attach_iou_target == 1
    assert bytes(hc)[32:] == b'\0' * 16
    hc = HeadLossCfg(2.0, 0.25, 1.0, 0.11, 1.0, 1, 0, 0, 1.5, 2.5, 1, 0)
    assert (hc.eta, hc.delta, hc.balanced_cls, hc.balanced_loc) == (1.5, 2.5, 1, 0)


def test_sizing_entry_is_declared_bound_and_exported_and_sizes_the_two_extra_rows():
    """host code alone: no device is touched"""
    import synth
    import gpu_util as G
    from iouaware import _lib, ops
    assert 'ia_head_loss_workspace_bytes_cfg' in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), 'ia_head_loss_workspace_bytes_cfg')
    L = _lib.lib()
    sizes = synth.level_shapes(64, 96)
    g = ops.HeadGeometry(sizes, synth.STRIDES, G.product_base_anchors(), synth.C)
    plain = L.ia_head_loss_workspace_bytes(g.ref(), 2)
    cfg = lambda bc, bl: _lib.HeadLossCfg(2.0, 0.25, 1.0, 0.11, 1.0, 1, 0, 0, 1.5, 1.5, bc, bl)   # noqa: E731
    assert plain > 0
    assert L.ia_head_loss_workspace_bytes_cfg(g.ref(), 2, ctypes.byref(cfg(0, 0))) == plain
    assert L.ia_head_loss_workspace_bytes_cfg(g.ref(), 2, ctypes.byref(cfg(0, 1))) == plain
    assert L.ia_head_loss_workspace_bytes_cfg(g.ref(), 2, ctypes.byref(cfg(1, 0))) == \
        plain + 8 * 2 * len(sizes) * _lib.IA_LOSS_SLOTS
    assert L.ia_head_loss_workspace_bytes_cfg(g.ref(), 2, None) == 0
    assert L.ia_head_loss_workspace_bytes_cfg(g.ref(), 0, ctypes.byref(cfg(1, 1))) == 0


class _FakeMap(object):
    """what _fused_loss_ok looks at, claiming to live on the device"""
    is_cuda = True
    dtype = torch.float32


FOCAL = dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0)
BAL_FOCAL = dict(type='IOUbalancedSigmoidFocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, eta=1.5,
                 loss_weight=1.0)
SMOOTH = dict(type='SmoothL1Loss', beta=0.11, loss_weight=1.0)
BAL_SMOOTH = dict(type='IoUbalancedSmoothL1Loss', beta=0.11, delta=1.5, loss_weight=1.0)


@pytest.mark.parametrize('loss_cls,loss_bbox', list(itertools.product((FOCAL, BAL_FOCAL), (SMOOTH, BAL_SMOOTH))))
def test_fused_loss_switch_truth_table(loss_cls, loss_bbox):
    from iouaware.head import IoUawareRetinaHead
    head = IoUawareRetinaHead(81, 256, loss_cls=dict(loss_cls), loss_bbox=dict(loss_bbox))
    assert type(head).fuse_balanced is False and head.fuse_levels is True
    balanced = loss_cls is BAL_FOCAL or loss_bbox is BAL_SMOOTH
    maps = [_FakeMap() for _ in range(5)]
    for fuse_balanced, iou_branch, fuse_levels in itertools.product((False, True), repeat=3):
        head.fuse_balanced, head.iou_branch, head.fuse_levels = fuse_balanced, iou_branch, fuse_levels
        want = fuse_levels and (not balanced or (fuse_balanced and iou_branch))
        assert bool(head._fused_loss_ok(maps)) == want, (fuse_balanced, iou_branch, fuse_levels)
    head.fuse_balanced, head.iou_branch, head.fuse_levels = True, True, True
    assert not head._fused_loss_ok([torch.zeros(1, 1, 1, 1)])          # CPU maps: the per-level route
    if loss_cls is BAL_FOCAL:
        head.loss_cls.gamma = 1.5                                       # the node is specialised for gamma = 2
        assert not head._fused_loss_ok(maps)
