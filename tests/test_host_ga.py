"""CPU: the IoU-aware guided-anchor RetinaNet head -- the plain-torch definition tests/ga_ref.py
against the reference's recorded get_bboxes (tests/golden/ga_get_bboxes.npz, written by
tests/golden/make_golden_ga.py), the wrong variants the fixture tells apart, the reference's
parameter names, the config, the refusals and the mmdet.* aliases."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import ga_ref
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')


def _ref():
    with open(os.path.join(GOLD, 'ga_ref.json')) as fh:
        return json.load(fh)


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(GOLD, 'ga_get_bboxes.npz'))


@pytest.fixture(scope='module')
def ref_results():
    """ga_ref's get_bboxes of both cases, computed once: {variant: [case][image] -> (dets, labels, ids)}"""
    out = {}
    for variant in (None, 'sqrt', 'clip', 'mask0', 'topk_all'):
        res = []
        for k, case in enumerate(ga_ref.GA_CASES):
            nms_pre, max_per_img, rescale = case[4], case[5], case[6]
            res.append(ga_ref.get_bboxes(ga_ref.ga_head_outputs(k), ga_ref.case_metas(k), rescale, nms_pre, 0.05,
                                         0.5, max_per_img, variant=variant))
        out[variant] = res
    return out


def test_fixture_matches_the_case_table(fixture):
    for k, case in enumerate(ga_ref.GA_CASES):
        assert fixture['case_%d' % k].tolist() == [case[0], case[1], case[2], case[3], case[4], case[5],
                                                   int(case[6])]
        assert fixture['sf_%d' % k].tolist() == [np.float32(v) for v in case[7]]
    assert [(c[2], c[3], c[1]) for c in ga_ref.GA_CASES] == [(64, 96, 1), (128, 192, 2)]


def test_ga_ref_reproduces_the_reference_to_the_bit(fixture, ref_results):
    """the same kept locations and labels in the reference's order, floats to the bit (the same torch
    CPU operations in the same order as the reference; the NMS decisions carry the generator's margin)"""
    for k, case in enumerate(ga_ref.GA_CASES):
        for b in range(case[1]):
            d, l, i = ref_results[None][k][b]
            assert np.array_equal(l, fixture['labels_%d_%d' % (k, b)])
            assert np.array_equal(i, fixture['ids_%d_%d' % (k, b)])
            assert np.array_equal(d.view(np.uint32), fixture['dets_%d_%d' % (k, b)].view(np.uint32))


@pytest.mark.parametrize('variant', ['sqrt', 'clip', 'mask0', 'topk_all'])
def test_fixture_tells_wrong_variants_apart(fixture, ref_results, variant):
    """each wrong reading of the reference changes the result of at least one image: other
    detections, or the same ones with boxes / scores that differ by more than the GPU tolerance"""
    changed = []
    for k, case in enumerate(ga_ref.GA_CASES):
        for b in range(case[1]):
            d, l, i = ga_ref.canonical(*ref_results[variant][k][b])
            rd, rl, ri = ga_ref.canonical(fixture['dets_%d_%d' % (k, b)], fixture['labels_%d_%d' % (k, b)],
                                          fixture['ids_%d_%d' % (k, b)])
            same = d.shape == rd.shape and np.array_equal(l, rl) and np.array_equal(i, ri) \
                and bool(np.all(np.abs(d - rd) <= 1e-4 * np.maximum(1.0, np.abs(rd))))
            changed.append(not same)
    assert any(changed), variant
    if variant == 'mask0':                      # image 0 itself is untouched by it
        assert not changed[0] and not changed[1] and changed[2]


def test_coverage_of_the_cases():
    """what the generator asserted, restated on the regenerated inputs: a level with more kept
    locations than nms_pre, one with fewer, one with none, different masks in the batch-2 case"""
    kept = []
    for k, case in enumerate(ga_ref.GA_CASES):
        loc = ga_ref.ga_head_outputs(k)[4]
        for b in range(case[1]):
            kept.append((case[4], [int(ga_ref.keep_mask(torch.from_numpy(lo[b])).sum()) for lo in loc]))
    assert any(n > pre for pre, ns in kept for n in ns)
    assert any(0 < n < pre for pre, ns in kept for n in ns)
    assert any(n == 0 for pre, ns in kept for n in ns)
    assert kept[1][1] != kept[2][1]


def test_coverage_of_the_results(fixture):
    """the generator's other three conditions, restated from the fixture and the regenerated inputs:
    a detection from a location whose |shape_pred| lies between the two clips, an image that ends
    under max_per_img and one that is cut by it"""
    clip, under, cut = False, False, False
    for k, case in enumerate(ga_ref.GA_CASES):
        maps, metas = ga_ref.ga_head_outputs(k), ga_ref.case_metas(k)
        every = ga_ref.get_bboxes(maps, metas, case[6], case[4], 0.05, 0.5, 10 ** 6)
        for b in range(case[1]):
            ids = fixture['ids_%d_%d' % (k, b)]
            big = np.concatenate([np.abs(sh[b]).reshape(2, -1).max(0) > ga_ref.CLIP_BOX for sh in maps[3]])
            clip |= bool(big[ids].any())
            n = len(every[b][1])
            under |= n < case[5] and len(ids) == n
            cut |= n > case[5] and len(ids) == case[5]
    assert clip and under and cut


def test_state_dict_names_match_the_reference():
    from iouaware.ga_head import IoUawareGARetinaHead
    rec = _ref()
    kw = {k: v for k, v in rec['model']['bbox_head'].items() if k != 'type'}
    head = IoUawareGARetinaHead(**kw)
    want = [[k[len('bbox_head.'):], s] for k, s in rec['state_dict'] if k.startswith('bbox_head.')]
    assert [[k, list(v.shape)] for k, v in head.state_dict().items()] == want
    names = [k for k, _ in want]
    for must in ('cls_convs.0.conv.weight', 'conv_loc.weight', 'conv_shape.bias',
                 'feature_adaption_cls.conv_offset.weight', 'feature_adaption_cls.conv_adaption.weight',
                 'feature_adaption_reg.conv_adaption.weight', 'retina_cls.bias', 'retina_reg.weight',
                 'retina_iou.weight'):
        assert must in names
    assert 'feature_adaption_cls.conv_offset.bias' not in names
    head.init_weights()
    assert float(head.conv_loc.bias.detach()) == pytest.approx(-np.log(99.0))


def test_config_builds_under_retinanet(tmp_path):
    """the GA-RetinaNet settings with the head type swapped build under RetinaNet with the
    reference's parameter names, shapes and order"""
    import iouaware
    from iouaware.config import Config
    from iouaware.detectors import RetinaNet
    from iouaware.ga_head import IoUawareGARetinaHead
    rec = _ref()
    assert rec['model']['bbox_head']['type'] == 'IoUawareGARetinaHead'
    path = tmp_path / 'ga.py'
    path.write_text('model = %r\ntest_cfg = %r\n' % (rec['model'], rec['test_cfg']))
    cfg = Config.fromfile(str(path))
    cfg.model['pretrained'] = None
    m = iouaware.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    assert isinstance(m, RetinaNet) and type(m.bbox_head) is IoUawareGARetinaHead
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == rec['state_dict']
    assert m.bbox_head.num_anchors == 1 and m.bbox_head.loc_filter_thr == 0.01


def test_only_the_iou_aware_ga_head_is_registered():
    from iouaware.registry import HEADS
    names = HEADS.module_dict if hasattr(HEADS, 'module_dict') else HEADS._module_dict
    assert 'IoUawareGARetinaHead' in names
    assert 'GARetinaHead' not in names and 'GARPNHead' not in names and 'GuidedAnchorHead' not in names


def test_reference_signatures():
    from iouaware.ga_head import IoUawareGARetinaHead
    assert list(inspect.signature(IoUawareGARetinaHead.get_bboxes).parameters) == [
        'self', 'cls_scores', 'bbox_preds', 'iou_preds', 'shape_preds', 'loc_preds', 'gt_bboxes', 'gt_labels',
        'img_metas', 'cfg', 'rescale']
    assert list(inspect.signature(IoUawareGARetinaHead.loss).parameters) == [
        'self', 'cls_scores', 'bbox_preds', 'iou_preds', 'shape_preds', 'loc_preds', 'gt_bboxes', 'gt_labels',
        'img_metas', 'cfg', 'gt_bboxes_ignore']


def test_loss_refuses_by_name():
    from iouaware.config import ConfigDict
    from iouaware.ga_head import IoUawareGARetinaHead
    head = IoUawareGARetinaHead(81, 16, feat_channels=16)
    with pytest.raises(NotImplementedError) as e:
        head.loss([], [], [], [], [], [], [], [], ConfigDict())
    for word in ('IoUawareGARetinaHead', 'ga_loc_target', 'ga_shape_target', 'ApproxMaxIoUAssigner',
                 'bounded IoU loss'):
        assert word in str(e.value)


def test_softmax_and_soft_nms_are_refused_by_name():
    from iouaware.config import ConfigDict
    from iouaware.ga_head import IoUawareGARetinaHead
    with pytest.raises(NotImplementedError, match='use_sigmoid_cls=False'):
        IoUawareGARetinaHead(81, 16, feat_channels=16,
                             loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
    head = IoUawareGARetinaHead(81, 16, feat_channels=16, anchor_strides=[8, 16, 32, 64, 128]).eval()
    sizes = synth.level_shapes(64, 96)
    maps = [[torch.zeros(1, ch, h, w) for h, w in sizes] for ch in (80, 4, 1, 2, 1)]
    meta = [dict(img_shape=(64, 96, 3), scale_factor=1.0, pad_shape=(64, 96, 3))]
    cfg = ConfigDict(nms_pre=100, score_thr=0.05, nms=dict(type='soft_nms', iou_thr=0.5), max_per_img=100)
    with pytest.raises(NotImplementedError, match='soft_nms'):
        head.get_bboxes(*maps, None, None, meta, cfg, False)


def test_compat_names_exist():
    import iouaware
    from iouaware import compat, ga_head, masked_conv
    compat.install()
    import mmdet.models.anchor_heads
    import mmdet.ops
    import mmdet.ops.masked_conv
    assert mmdet.ops.MaskedConv2d is masked_conv.MaskedConv2d is iouaware.MaskedConv2d
    assert mmdet.ops.masked_conv2d is masked_conv.masked_conv2d is iouaware.masked_conv2d
    assert mmdet.ops.masked_conv.MaskedConv2d is masked_conv.MaskedConv2d
    assert mmdet.ops.masked_conv.masked_conv2d is masked_conv.masked_conv2d
    assert mmdet.models.anchor_heads.IoUawareGARetinaHead is ga_head.IoUawareGARetinaHead
    assert not hasattr(mmdet.models.anchor_heads, 'GARetinaHead')


def test_cpu_tensors_and_unsupported_arguments_are_refused():
    from iouaware import masked_conv
    from iouaware._lib import IouAwareLibraryError
    from iouaware.config import ConfigDict
    from iouaware.ga_head import IoUawareGARetinaHead
    x, w3 = torch.zeros(1, 8, 5, 7), torch.zeros(3, 8, 3, 3)
    mask = torch.ones(1, 5, 7, dtype=torch.bool)
    with pytest.raises(IouAwareLibraryError, match='input is on cpu'):
        masked_conv.masked_conv2d(x, mask, w3, None, padding=1)
    with pytest.raises(IouAwareLibraryError, match='mask'):
        masked_conv.compact_mask(mask)
    with pytest.raises(TypeError, match='float16'):
        masked_conv.masked_conv2d(x.half(), mask, w3.half(), None, padding=1)
    with pytest.raises(TypeError, match='bfloat16'):
        masked_conv.masked_conv2d(x.bfloat16(), mask, w3.bfloat16(), None, padding=1)
    with pytest.raises(NotImplementedError, match='stride=2'):
        masked_conv.masked_conv2d(x, mask, w3, None, padding=1, stride=2)
    with pytest.raises(NotImplementedError, match='padding=0'):
        masked_conv.masked_conv2d(x, mask, w3, None, padding=0)
    with pytest.raises(NotImplementedError, match='kernel_size'):
        masked_conv.masked_conv2d(x, mask, torch.zeros(3, 8, 5, 5), None, padding=2)
    with pytest.raises(NotImplementedError, match='in_channels=6'):
        masked_conv.masked_conv2d(torch.zeros(1, 6, 5, 7), mask, torch.zeros(3, 6, 1, 1), None)
    with pytest.raises(ValueError, match='mask must have shape'):
        masked_conv.masked_conv2d(torch.zeros(2, 8, 5, 7), mask, w3, None, padding=1)
    # mask=None is the plain convolution, on any device, and trainable
    m = masked_conv.MaskedConv2d(8, 3, 3, padding=1)
    xin = torch.randn(1, 8, 5, 7)
    y = m(xin)
    assert torch.equal(y, torch.nn.functional.conv2d(xin, m.weight, m.bias, padding=1))
    y.sum().backward()
    assert m.weight.grad is not None
    # the head: eval forward and get_bboxes need device tensors
    head = IoUawareGARetinaHead(81, 16, feat_channels=16, anchor_strides=[8, 16, 32, 64, 128]).eval()
    with torch.no_grad(), pytest.raises(IouAwareLibraryError):
        head([torch.zeros(1, 16, 4, 6)])
    sizes = synth.level_shapes(64, 96)
    maps = [[torch.zeros(1, ch, h, w) for h, w in sizes] for ch in (80, 4, 1, 2, 1)]
    meta = [dict(img_shape=(64, 96, 3), scale_factor=1.0, pad_shape=(64, 96, 3))]
    cfg = ConfigDict(nms_pre=100, score_thr=0.05, nms=dict(type='nms', iou_thr=0.5), max_per_img=100)
    with pytest.raises(IouAwareLibraryError, match='cls_score'):
        head.get_bboxes(*maps, None, None, meta, cfg, False)


def test_guided_struct_layout_and_entry_refusals():
    """the new structs extend, not change, the pinned ones; the entries refuse a geometry with more
    than one anchor, a softmax or channels-last geometry and a negative score_thr before anything
    is enqueued (no device needed: the checks come first)"""
    import ctypes
    from iouaware import _lib
    from iouaware.ga_head import IoUawareGARetinaHead
    assert ctypes.sizeof(_lib.GuidedGeom) == ctypes.sizeof(_lib.HeadGeom) + 8 * 4 + 4 + 4
    assert _lib.GuidedGeom.head.offset == 0
    assert ctypes.sizeof(_lib.GuidedLevelPtrs) == 5 * 8 * 8
    head = IoUawareGARetinaHead(81, 16, feat_channels=16, octave_base_scale=4, anchor_strides=[8, 16, 32, 64, 128])
    geom = head.geometry(synth.level_shapes(64, 96), 60)
    assert (geom.N, geom.R) == (129, 60 + 24 + 6 + 2 + 1)
    base = [list(geom.struct.head.base_anchors[l][0]) for l in range(5)]
    assert base == [ga_ref.square_base(s).tolist() for s in synth.STRIDES]
    L = _lib.lib()
    assert L.ia_guided_get_bboxes_workspace_bytes(geom.ref(), 2) > 0
    p = _lib.GuidedLevelPtrs()
    for f in ('cls', 'reg', 'iou', 'shape', 'loc'):
        for l in range(5):
            getattr(p, f)[l] = 256                                # never dereferenced: refused first
    ws = ctypes.c_void_p(256)
    args = (1, ws, ws, 0)
    tail = (0.5, 100, ws, 1 << 30, ws, ws, ws, ws, None)
    assert L.ia_guided_get_bboxes(geom.ref(), ctypes.byref(p), *args, -0.1, *tail) == -1
    assert L.ia_guided_get_bboxes(geom.ref(), ctypes.byref(p), *args, float('nan'), *tail) == -1
    for field, value in (('num_anchors', 2), ('layout', _lib.IA_LAYOUT_NHWC), ('cls_activation', _lib.IA_CLS_SOFTMAX)):
        g = _lib.GuidedGeom.from_buffer_copy(geom.struct)
        setattr(g.head, field, value)
        assert L.ia_guided_rowmax(ctypes.byref(g), ctypes.byref(p), 1, ws, None) == -1
        assert L.ia_guided_get_bboxes(ctypes.byref(g), ctypes.byref(p), *args, 0.05, *tail) == -1
    p.loc[2] = None
    assert L.ia_guided_rowmax(geom.ref(), ctypes.byref(p), 1, ws, None) == -1
