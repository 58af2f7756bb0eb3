"""CPU side of the FCOS training kernels (csrc/pointloss.hip): the entries are declared, bound and
exported, the structs have the header's layout, the ops refuse CPU tensors, the head's switch
(`_fused_loss_ok`) turns away what the node does not cover, and the synthetic inputs of
tests/synth_fcos_loss.py meet the conditions the GPU comparisons rest on."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import synth_fcos_loss as S

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
ENTRIES = ('ia_point_packed_labels_elems', 'ia_point_targets_ptrs',
           'ia_point_head_loss_workspace_bytes', 'ia_point_head_loss_fwd', 'ia_point_head_loss_bwd')


def test_entries_are_declared_bound_and_exported():
    from iouaware import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'iouaware.h')).read(), flags=re.S)
    h = ctypes.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, text), '%s not declared' % name
        assert name in _lib.SIGNATURES, '%s not bound' % name
        assert hasattr(h, name), '%s not exported' % name
    for struct in ('ia_point_level_ptrs', 'ia_point_targets', 'ia_point_loss_cfg'):
        assert re.search(r'\}\s*%s\s*;' % struct, text), struct


def test_struct_layout_matches_header():
    from iouaware import _lib
    assert ctypes.sizeof(_lib.PointLevelPtrs) == 4 * 8 * 8
    assert _lib.PointLevelPtrs.iou.offset == 3 * 8 * 8
    assert ctypes.sizeof(_lib.PointTargets) == 2 * 8 * 8 + 2 * 8
    assert _lib.PointTargets.packed.offset == 2 * 8 * 8
    assert ctypes.sizeof(_lib.PointLossCfg) == 16
    # the structs the decode entries share are as they were
    assert ctypes.sizeof(_lib.LevelPtrs) == 3 * 8 * 8
    assert ctypes.sizeof(_lib.PointHeadGeom) == 3 * 4 + 3 * 8 * 4 + 4 + 4


def test_argument_checks_need_no_device():
    """IA_E_ARG / 0 come back before anything is launched"""
    from iouaware import _lib, fcos_ops
    L = _lib.lib()
    sizes = S.synth_fcos.level_shapes(128, 160)
    g = fcos_ops.PointGeometry(sizes, S.STRIDES, S.C)
    assert L.ia_point_head_loss_workspace_bytes(g.ref(), 2) > 0
    assert L.ia_point_head_loss_workspace_bytes(g.ref(), 0) == 0
    assert L.ia_point_packed_labels_elems(g.ref(), 2) >= 2 * 2 * g.N
    assert L.ia_point_packed_labels_elems(None, 2) == 0
    bad = fcos_ops.PointGeometry(sizes, S.STRIDES, S.C)
    bad.struct.num_levels = 9
    assert L.ia_point_head_loss_workspace_bytes(bad.ref(), 2) == 0
    assert L.ia_point_head_loss_fwd(g.ref(), None, 2, None, None, None, 0, None, None) == -1
    assert L.ia_point_head_loss_bwd(g.ref(), None, 2, None, None, None, None, None, None, None) == -1
    assert L.ia_point_targets_ptrs(g.ref(), None, None, None, 2, None, None, None, None, None, None) == -1


def test_ops_refuse_cpu_tensors():
    from iouaware import _lib, fcos_ops
    sizes, gb, gl, outs = S.case_inputs(S.SMALL)
    g = fcos_ops.PointGeometry(sizes, S.STRIDES, S.C)
    tb, tl = [torch.from_numpy(b) for b in gb], [torch.from_numpy(x) for x in gl]
    with pytest.raises(_lib.IouAwareLibraryError):
        fcos_ops.point_targets(g, tb, tl, S.RANGES)
    lab, tgt = S.np_targets(sizes, gb, gl)
    T = lambda xs: [torch.from_numpy(x) for x in xs]   # noqa: E731
    with pytest.raises(_lib.IouAwareLibraryError):
        fcos_ops.point_head_loss(g, T(outs[0]), T(outs[1]), T(outs[2]), T(outs[3]), T(lab), T(tgt),
                                 None)


class _FakeMap(object):
    """what _fused_loss_ok looks at, claiming to live on the device"""
    is_cuda = True

    def __init__(self, dtype=torch.float32, contiguous=True, batch=2):
        self.dtype, self._c, self._b = dtype, contiguous, batch

    def dim(self):
        return 4

    def is_contiguous(self):
        return self._c

    def size(self, i):
        return self._b if i == 0 else 1


def test_fused_loss_switch():
    head = S.make_head(True, True)
    assert head.fuse_loss is True and type(head).fuse_loss is True
    gt = lambda n: SimpleNamespace(is_cuda=True, size=lambda i: n)   # noqa: E731
    maps = lambda **kw: tuple([_FakeMap(**kw) for _ in range(5)] for _ in range(4))   # noqa: E731
    cfg = SimpleNamespace(gamma=2.0, alpha=0.25)
    assert head._fused_loss_ok(maps(), [gt(3), gt(1)], [gt(3), gt(1)], cfg)
    assert not head._fused_loss_ok(maps(), [gt(3), gt(1)], [gt(3), gt(1)], SimpleNamespace(gamma=1.5, alpha=0.25))
    assert not head._fused_loss_ok(maps(), [gt(3), gt(0)], [gt(3), gt(0)], cfg)      # an image without gts
    assert not head._fused_loss_ok(maps(), [gt(3), gt(513)], [gt(3), gt(513)], cfg)
    assert not head._fused_loss_ok(maps(dtype=torch.bfloat16), [gt(3), gt(1)], [gt(3), gt(1)], cfg)
    assert not head._fused_loss_ok(maps(contiguous=False), [gt(3), gt(1)], [gt(3), gt(1)], cfg)   # channels-last
    assert not head._fused_loss_ok(maps(batch=17), [gt(1)] * 17, [gt(1)] * 17, cfg)
    cpu = tuple([torch.zeros(2, 1, 1, 1) for _ in range(5)] for _ in range(4))
    assert not head._fused_loss_ok(cpu, [gt(3), gt(1)], [gt(3), gt(1)], cfg)


@pytest.mark.parametrize('case,min_pos', [(S.MAIN, 50), (S.SMALL, 0), (S.MAIN1, 1)])
def test_generator_conditions(case, min_pos):
    sizes, gb, gl, outs = S.case_inputs(case)
    for b in gb:
        assert (b != np.round(b)).any() and (b[:, 2] > b[:, 0]).all() and (b[:, 3] > b[:, 1]).all()
    pos = S.check_conditions(sizes, gb, gl, min_pos)
    print(case[0], 'positives per level', pos)
    lab, tgt = S.np_targets(sizes, gb, gl)
    assert S.edge_ties(sizes, lab, tgt, outs[1]) == 0


def test_numpy_targets_are_the_torch_targets_bit_for_bit():
    """the numpy evaluation the tie case is checked against is the head's torch fcos_target"""
    sizes, gb, gl, _ = S.case_inputs(S.SMALL)
    head = S.make_head(False, False)
    pts = head.get_points(sizes, torch.float32, 'cpu')
    lab, tgt = head.fcos_target(pts, [torch.from_numpy(b) for b in gb], [torch.from_numpy(x) for x in gl])
    l32, t32 = S.np_targets(sizes, gb, gl)
    for l in range(len(sizes)):
        assert np.array_equal(lab[l].numpy().reshape(len(gb), -1), l32[l])
        assert np.array_equal(tgt[l].numpy().reshape(len(gb), -1, 4).view(np.uint32), t32[l].view(np.uint32))


def test_fixture_matches_the_generator():
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'fcos_loss.npz'))
    for k, case in enumerate((S.SMALL, S.MAIN1)):
        assert list(g['case_%d' % k]) == list(case[1:])
        sizes, gb, gl, _ = S.case_inputs(case)
        lab, tgt = S.np_targets(sizes, gb, gl)
        for l in range(len(sizes)):
            assert np.array_equal(g['labels_%d_%d' % (k, l)], lab[l].reshape(-1))
            assert np.array_equal(g['bbox_targets_%d_%d' % (k, l)].view(np.uint32),
                                  tgt[l].reshape(-1, 4).view(np.uint32))
