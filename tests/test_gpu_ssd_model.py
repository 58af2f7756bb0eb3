"""-m gpu: SSD300 built from the recorded ssd300_coco config, image -> detections on the HIP route
(L2Norm kernel, ia_ssd_get_bboxes) against tests/ssd_ref.py on the model's own head outputs; the
SSD512 geometry end to end."""
import json
import os

import numpy as np
import pytest
import torch

import ssd_ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _build(name, seed=0, bg_bias=None):
    import iouaware
    from iouaware.config import ConfigDict
    with open(os.path.join(GOLD, 'ssd_ref.json')) as fh:
        cfg = json.load(fh)['configs'][name]
    torch.manual_seed(seed)
    det = iouaware.build_detector(ConfigDict(dict(cfg['model'], pretrained=None)), train_cfg=None,
                                  test_cfg=ConfigDict(cfg['test_cfg']))
    if bg_bias is not None:
        # At random init the class logits have a standard deviation near 1 on the L2-normalised level and
        # more on the deeper ones, so the best of 80 foreground softmax scores lies near 0.08 and ALL 8 732
        # rows pass score_thr = 0.02 (measured on the CPU; a negative background bias only adds to that).
        # A background bias of +8 leaves the rows with the largest foreground logits: about 1 500 per
        # image on the first three levels for the input below.
        with torch.no_grad():
            for conv, a in zip(det.bbox_head.cls_convs, det.bbox_head.num_anchors):
                conv.bias.view(a, -1)[:, 0] = bg_bias
    return det.cuda().eval()


@pytest.fixture(scope='module')
def ssd300():
    det = _build('ssd300_coco', bg_bias=8.0)
    torch.manual_seed(5)
    img = torch.randn(2, 3, 300, 300, device='cuda') * 10
    metas = [dict(ori_shape=(300, 300, 3), img_shape=(300, 300, 3), pad_shape=(300, 300, 3), scale_factor=1.0,
                  flip=False),
             dict(ori_shape=(240, 300, 3), img_shape=(288, 300, 3), pad_shape=(300, 300, 3), scale_factor=1.2,
                  flip=False)]
    with torch.no_grad():
        feats = det.extract_feat(img)
        cls, reg = det.bbox_head(feats)
    return dict(det=det, img=img, metas=metas, feats=feats, cls=cls, reg=reg)


def _ref(s, rescale):
    head = s['det'].bbox_head
    hd = dict(ssd_ref.ANCHOR_SETTINGS['ssd300_coco'], target_means=head.target_means, target_stds=head.target_stds)
    return ssd_ref.get_bboxes([c.cpu() for c in s['cls']], [r.cpu() for r in s['reg']], s['metas'], rescale, head=hd,
                              num_classes=81)


@pytest.mark.parametrize('rescale', [False, True])
def test_simple_test_device_equals_ssd_ref_on_the_models_head_outputs(ssd300, rescale):
    from iouaware import ssd_ops
    det, head = ssd300['det'], ssd300['det'].bbox_head
    assert [tuple(c.shape[-2:]) for c in ssd300['cls']] == ssd_ref.SSD300_SIZES
    geom = head.geometry(ssd_ref.SSD300_SIZES)
    best = ssd_ops.ssd_rowscore(geom, ssd300['cls'], ssd300['reg'])
    kept = (best > det.test_cfg.score_thr).sum(1).tolist()
    print('rows above score_thr per image: %s' % kept)
    assert 10 <= kept[0] <= 8192 and kept[1] <= 8192          # not an empty result, and the fast path
    with torch.no_grad():
        dets, labels, rows, num = det.simple_test_device(ssd300['img'], ssd300['metas'], rescale=rescale)
    assert head.overflow.tolist() == [0, 0]
    want = _ref(ssd300, rescale)
    got = [t.cpu().numpy() for t in (dets, labels, rows, num)]
    assert got[3].tolist() == [len(w[0]) for w in want] and got[3][0] >= 10
    for b, (wd, wl, wi) in enumerate(want):
        n = int(got[3][b])
        d, l, i = ssd_ref.canonical(got[0][b, :n], got[1][b, :n].astype(np.int64), got[2][b, :n].astype(np.int64))
        wd, wl, wi = ssd_ref.canonical(wd, wl, wi)
        assert np.array_equal(i, wi) and np.array_equal(l, wl)
        # this build's detection contract (gpu_util.close): 1e-4, relative for values above 1
        err = float((np.abs(d.astype(np.float64) - wd) / np.maximum(1.0, np.abs(wd))).max())
        print('image %d: %d detections, largest difference %.2e (relative above 1)' % (b, n, err))
        assert err <= 1e-4


def test_l2norm_of_conv4_3_on_the_hip_route(ssd300):
    """the backbone's first output (eval: the kernel) against the expression in fp64 on conv4_3's
    activations, under the L2Norm gate: <= 1e-4 * max|y| and <= 4 x torch's fp32 evaluation"""
    vgg = ssd300['det'].backbone
    with torch.no_grad():
        x = ssd300['img']
        for i, layer in enumerate(vgg.features):
            x = layer(x)
            if i == 22:
                break
        w, eps = vgg.l2_norm.weight.detach(), vgg.l2_norm.eps
        y = vgg.l2_norm(x)
        assert not vgg.l2_norm.training
        vgg.l2_norm.train()
        y_train = vgg.l2_norm(x)
        vgg.l2_norm.eval()
    xc, wc = x.cpu(), w.cpu()
    want = ssd_ref.l2norm(xc.double(), wc.double(), eps)
    err = float((y.cpu().double() - want).abs().max())
    err_torch = float((ssd_ref.l2norm(xc, wc, eps).double() - want).abs().max())
    ymax = float(want.abs().max())
    print('conv4_3 L2Norm: error %.3e, torch fp32 on the CPU %.3e, max|y| %.3e' % (err, err_torch, ymax))
    assert tuple(y.shape) == (2, 512, 38, 38) and ymax > 0
    assert err <= 1e-4 * ymax and err <= 4 * err_torch
    assert float((y_train - y).abs().max()) <= 1e-4 * ymax
    # the detector's own first feature map is this tensor
    assert torch.equal(ssd300['feats'][0], y)


def test_simple_test_returns_bbox2result_lists(ssd300):
    det = ssd300['det']
    with torch.no_grad():
        res = det.simple_test(ssd300['img'][:1], ssd300['metas'][:1], rescale=False)
        both = det.simple_test_batch(ssd300['img'], ssd300['metas'], rescale=False)
    assert isinstance(res, list) and len(res) == 80
    assert all(isinstance(r, np.ndarray) and r.ndim == 2 and r.shape[1] == 5 and r.dtype == np.float32 for r in res)
    assert sum(r.shape[0] for r in res) >= 10
    assert len(both) == 2 and all(len(r) == 80 for r in both)
    want = _ref(ssd300, False)[0]
    assert sum(r.shape[0] for r in both[0]) == len(want[0])
    for c in range(80):
        assert both[0][c].shape[0] == int((want[1] == c).sum())


def test_ssd512_builds_and_runs_seven_levels():
    det = _build('ssd512_coco', seed=1)
    head = det.bbox_head
    torch.manual_seed(2)
    img = torch.randn(1, 3, 512, 512, device='cuda') * 40
    with torch.no_grad():
        cls, reg = det.forward_head(img)
    assert [tuple(c.shape[-2:]) for c in cls] == ssd_ref.SSD512_SIZES
    assert [c.shape[1] for c in cls] == [a * 81 for a in (4, 6, 6, 6, 6, 4, 4)]
    assert [r.shape[1] for r in reg] == [a * 4 for a in (4, 6, 6, 6, 6, 4, 4)]
    geom = head.geometry(ssd_ref.SSD512_SIZES)
    assert geom.L == 7 and geom.R == 24564 and geom.Rk == 8192
    meta = [dict(img_shape=(512, 512, 3), scale_factor=1.0)]
    with torch.no_grad():
        dets, labels, rows, num = head.get_bboxes_batched(cls, reg, meta, det.test_cfg)
    n = int(num[0])
    assert 0 <= n <= 200 and bool((rows[0, :n] >= 0).all()) and bool((rows[0, :n] < 24564).all())
    assert bool((labels[0, :n] >= 0).all()) and bool((labels[0, :n] < 80).all())
