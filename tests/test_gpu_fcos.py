"""GPU: IoU-aware FCOS -- the HIP GroupNorm + ReLU of the towers, the point-head decode
(ia_point_get_bboxes), the fused Winograd head, the detector end to end and one training step,
against fp64 torch, a numpy composition of the oracle's primitives and reference fixtures
(tests/golden/fcos_*.npz, tests/golden/make_golden_fcos.py)."""
import json
import os

import numpy as np
import pytest
import torch

import synth_fcos

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
DEV = torch.device('cuda:0')
TOL = 1e-4
# GroupNorm bars, in units of the output scale (gamma ~ 1): the fp64 statistics leave only the
# rounding of x * s + t (~ |mean|/std * 2^-24 each); a one-pass fp32 E[x^2] - E[x]^2 misses the
# |mean|/std = 200 bar by ~(mean/std)^2 * 2^-24 (asserted below on the same data)
GN_TOL = 2e-5                 # |mean| ~ 0
GN_TOL_SHIFTED = 2e-4         # |mean| / std = 200


def _levels(pad_h, pad_w):
    return synth_fcos.level_shapes(pad_h, pad_w)


def _acts(seed, B, sizes, ch=512, mean_over_std=0.0):
    g = torch.Generator().manual_seed(seed)
    xs = []
    for (h, w) in sizes:
        x = torch.randn((B, ch, h, w), generator=g) * 0.7
        if mean_over_std:        # every group: std 0.007, mean 0.007 * mean_over_std
            x = x * 0.01 + 0.007 * mean_over_std
        xs.append(x)
    return xs


def _gn_ref(xs, gamma, beta, groups):
    gn = torch.nn.GroupNorm(groups, xs[0].shape[1], eps=1e-5).double()
    with torch.no_grad():
        gn.weight.copy_(gamma.double())
        gn.bias.copy_(beta.double())
        return [torch.relu(gn(x.double())) for x in xs]


def _gn_run(xs, gamma, beta, groups):
    from iouaware import fcos_ops
    dev = [x.to(DEV).contiguous(memory_format=torch.channels_last) for x in xs]
    fcos_ops.groupnorm_relu_(dev, gamma.to(DEV), beta.to(DEV), groups)
    torch.cuda.synchronize()
    return [d.cpu() for d in dev]


@pytest.mark.parametrize('mean_over_std', [0.0, 200.0])
def test_groupnorm_against_fp64(mean_over_std):
    sizes = _levels(800, 1344)
    xs = _acts(1, 2, sizes, mean_over_std=mean_over_std)
    g = torch.Generator().manual_seed(2)
    gamma, beta = torch.rand(512, generator=g) + 0.5, torch.randn(512, generator=g) * 0.3
    ref = _gn_ref(xs, gamma, beta, 64)
    out = _gn_run(xs, gamma, beta, 64)
    bar = GN_TOL_SHIFTED if mean_over_std else GN_TOL
    for l, (o, r) in enumerate(zip(out, ref)):
        err = float((o.double() - r).abs().max())
        print('level %d: max error %.2e (bar %.0e)' % (l, err, bar))
        assert err <= bar, (l, err)
    if mean_over_std:
        # the bar separates: a one-pass fp32 variance on the same data misses it
        x = xs[0][0].reshape(64, -1)
        m32 = x.mean(1)
        v32 = (x * x).mean(1) - m32 * m32
        v64 = x.double().var(1, unbiased=False)
        rel = float(((v32.double() - v64) / v64).abs().max())
        print('one-pass fp32 variance: relative error %.2e' % rel)
        assert rel * 0.5 * 3 > GN_TOL_SHIFTED, rel     # |d rstd / rstd| = |d var / var| / 2, outputs ~3 std


def test_groupnorm_bits_repeat_and_do_not_depend_on_the_batch():
    sizes = _levels(800, 1344)
    xs = _acts(3, 8, sizes, mean_over_std=10.0)
    gamma, beta = torch.rand(512) + 0.5, torch.randn(512) * 0.3
    a = _gn_run(xs, gamma, beta, 64)
    b = _gn_run(xs, gamma, beta, 64)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    alone = _gn_run([x[5:6] for x in xs], gamma, beta, 64)
    assert all(torch.equal(u[5:6], v) for u, v in zip(a, alone))


# ------------------------------------------------------------------ point decode
def _np_sig_pow(x, e):
    import oracle
    s = oracle.vec('sigmoidf', x)
    out = oracle.vec('expf', (np.float32(e) * oracle.vec('logf', s)).astype(np.float32))
    return np.where(s == 0, np.float32(0), out).astype(np.float32)


def _oracle_point_get_bboxes(cls, reg, iou, strides, img_shape, sf, rescale, nms_pre, score_thr,
                             iou_thr, max_per_img, alpha=0.3):
    """numpy composition of the oracle's primitives (one image; cls (C,H,W) etc. per level)"""
    import oracle
    rows_box, rows_sc, rows_pt = [], [], []
    for l, (c, r, i) in enumerate(zip(cls, reg, iou)):
        C, H, W = c.shape
        fi = _np_sig_pow(i.reshape(-1), np.float32(1) - np.float32(alpha))
        sc = (_np_sig_pow(c.reshape(C, -1).T, alpha) * fi[:, None]).astype(np.float32)
        idx = np.arange(H * W)
        if 0 < nms_pre < H * W:
            idx = np.lexsort((idx, -sc.max(1)))[:nms_pre]
        ys, xs = idx // W, idx % W
        px = (xs * strides[l] + strides[l] // 2).astype(np.float32)
        py = (ys * strides[l] + strides[l] // 2).astype(np.float32)
        d = r.reshape(4, -1)[:, idx]
        b = np.stack([px - d[0], py - d[1], px + d[2], py + d[3]], 1).astype(np.float32)
        b[:, 0::2] = np.clip(b[:, 0::2], np.float32(0), np.float32(img_shape[1] - 1))
        b[:, 1::2] = np.clip(b[:, 1::2], np.float32(0), np.float32(img_shape[0] - 1))
        if rescale:
            b = (b / np.float32(sf)).astype(np.float32)
        rows_box.append(b)
        rows_sc.append(sc[idx])
        rows_pt.append(idx + sum(h * w for (_, h, w) in [x.shape for x in cls[:l]]))
    boxes, scores, pts = np.concatenate(rows_box), np.concatenate(rows_sc), np.concatenate(rows_pt)
    found = []
    for c in range(scores.shape[1]):
        rows = np.nonzero(scores[:, c] > np.float32(score_thr))[0]
        if rows.size == 0:
            continue
        dets = np.concatenate([boxes[rows], scores[rows, c:c + 1]], 1)
        for k in oracle.nms(dets, iou_thr):
            found.append((-scores[rows[k], c], c, rows[k]))
    found.sort()
    found = found[:max_per_img]
    return dict(boxes=boxes, scores=scores, points=pts,
                dets=np.array([list(boxes[r]) + [-s] for s, _, r in found], np.float32).reshape(-1, 5),
                labels=np.array([c for _, c, _ in found], np.int64),
                rows=np.array([r for _, _, r in found], np.int64))


def _to_dev(xs, nhwc):
    out = [torch.from_numpy(x).to(DEV) for x in xs]
    return [t.contiguous(memory_format=torch.channels_last) for t in out] if nhwc else out


@pytest.mark.parametrize('nhwc', [False, True])
@pytest.mark.parametrize('pad,nms_pre,rescale', [((320, 448), 150, True), ((320, 448), 150, False),
                                                 ((320, 448), 3000, True),
                                                 ((800, 1344), 1000, True)])    # filtered top-k
def test_point_decode_bit_exact_against_oracle(nhwc, pad, nms_pre, rescale):
    from iouaware import fcos_ops
    pad_h, pad_w = pad
    sizes = _levels(pad_h, pad_w)
    cls, reg, ctr, iou = synth_fcos.head_outputs(31, 2, sizes)
    geom = fcos_ops.PointGeometry(sizes, synth_fcos.STRIDES, 80, nms_pre, 0.3)
    shapes = [(pad_h - 20, pad_w - 7, 3), (pad_h, pad_w - 48, 3)]
    factors = [0.75, 1.5]
    dets, labels, rows, num, views = fcos_ops.point_get_bboxes(
        geom, _to_dev(cls, nhwc), _to_dev(reg, nhwc), _to_dev(iou, nhwc), shapes, factors, rescale,
        0.05, 0.5, 100, debug=True)
    torch.cuda.synchronize()
    cand = views['cand_idx'].cpu().numpy()
    lvl_off = np.cumsum([0] + [h * w for (h, w) in sizes])
    cand_off = np.cumsum([0] + geom.level_cands)
    for b in range(2):
        o = _oracle_point_get_bboxes([c[b] for c in cls], [r[b] for r in reg], [i[b] for i in iou],
                                     synth_fcos.STRIDES, shapes[b], factors[b], rescale, nms_pre,
                                     0.05, 0.5, 100)
        pts = np.concatenate([cand[b, cand_off[l]:cand_off[l + 1]] + lvl_off[l]
                              for l in range(len(sizes))])
        assert np.array_equal(pts, o['points'])
        assert np.array_equal(views['boxes'][b].cpu().numpy(), o['boxes'])
        assert np.array_equal(views['scores_t'][b, :, :geom.R].cpu().numpy().T, o['scores'])
        n = int(num[b])
        assert n == len(o['labels']) > 0
        assert np.array_equal(dets[b, :n].cpu().numpy(), o['dets'])
        assert np.array_equal(labels[b, :n].cpu().numpy(), o['labels'])
        assert np.array_equal(rows[b, :n].cpu().numpy(), o['rows'])


def _match_sets(ours_d, ours_l, ref_d, ref_l):
    """detections as sets: every reference detection matched to one of ours of the same class"""
    assert len(ours_d) == len(ref_d)
    used = np.zeros(len(ours_d), bool)
    for d, l in zip(ref_d, ref_l):
        cand = np.nonzero((ours_l == l) & ~used)[0]
        err = np.abs(ours_d[cand] - d).max(1) if cand.size else np.array([np.inf])
        k = int(np.argmin(err))
        assert err[k] <= TOL * max(1.0, float(np.abs(d).max())), (d, l)
        used[cand[k]] = True


def test_point_get_bboxes_against_reference_fixture():
    from iouaware.fcos_head import IoUawareFCOSHead
    from iouaware.config import ConfigDict
    g = np.load(os.path.join(GOLD, 'fcos_get_bboxes.npz'))
    pad_h, pad_w = (int(v) for v in g['pad'])
    sizes = _levels(pad_h, pad_w)
    cls, reg, ctr, iou = synth_fcos.head_outputs(int(g['seed']), 2, sizes)
    head = IoUawareFCOSHead(81, 256, strides=[8, 16, 32, 64, 128]).to(DEV)
    metas = [dict(img_shape=(150, 213, 3), scale_factor=0.75), dict(img_shape=(160, 200, 3),
                                                                     scale_factor=1.25)]
    for tag, nms_pre, rescale in (('pre100_r', 100, True), ('pre100', 100, False),
                                  ('pre1000_r', 1000, True)):
        cfg = ConfigDict(dict(nms_pre=nms_pre, min_bbox_size=0, score_thr=0.05,
                              nms=dict(type='nms', iou_thr=0.5), max_per_img=100))
        for nhwc in (False, True):
            res = head.get_bboxes(_to_dev(cls, nhwc), _to_dev(reg, nhwc), _to_dev(ctr, nhwc),
                                  _to_dev(iou, nhwc), None, None, metas, cfg, rescale)
            for b, (d, l) in enumerate(res):
                rd, rl = g['dets_%s_%d' % (tag, b)], g['labels_%s_%d' % (tag, b)]
                d, l = d.cpu().numpy(), l.cpu().numpy()
                _match_sets(d, l, rd, rl)
                # same order too (the fixture's score gaps are far above the rounding)
                assert np.abs(d - rd).max() <= TOL * max(1.0, float(np.abs(rd).max()))
                assert np.array_equal(l, rl)


# ------------------------------------------------------------------ model level
def _model(seed, winograd=None):
    import iouaware
    from iouaware.config import Config
    import tempfile
    with open(os.path.join(GOLD, 'fcos_ref.json')) as fh:
        cfg = json.load(fh)['config']
    with tempfile.NamedTemporaryFile('w', suffix='.py', delete=False) as fh:
        fh.write('\n'.join('%s = %r' % (k, v) for k, v in sorted(cfg.items())) + '\n')
    try:
        cfg = Config.fromfile(fh.name)
    finally:
        os.unlink(fh.name)
    cfg.model['pretrained'] = None
    m = iouaware.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    state = m.state_dict()
    synth_fcos.fill_state(state, seed)
    m.load_state_dict(state)
    return cfg, m.to(DEV)


def test_fused_head_matches_module_head():
    from iouaware.fuse import fuse_inference
    _, m = _model(5)
    m.eval()
    head = m.bbox_head
    sizes = _levels(256, 320)
    g = torch.Generator().manual_seed(12)
    feats = [torch.randn((2, 256, h, w), generator=g).to(DEV).contiguous(
        memory_format=torch.channels_last) for (h, w) in sizes]
    with torch.no_grad():
        ref = head(feats)
        fuse_inference(m, winograd=True)
        runner = head._ia_wino
        calls = runner.calls
        out = head(feats)
    torch.cuda.synchronize()
    assert runner.calls == calls + 1, 'the Winograd FCOS runner was not used'
    assert not hasattr(head.cls_convs[0], '_ia_fused')
    for kind, a, b in zip(('cls', 'bbox', 'ctr', 'iou'), out, ref):
        for l, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape and x.is_contiguous(memory_format=torch.channels_last)
            scale = max(1.0, float(y.abs().max()))
            err = float((x - y).abs().max())
            assert err <= TOL * scale, (kind, l, err, scale)


@pytest.mark.parametrize('path', ['module', 'fused', 'winograd'])
def test_detector_end_to_end_against_reference(path):
    from iouaware.fuse import fuse_inference
    g = np.load(os.path.join(GOLD, 'fcos_e2e.npz'))
    cfg, m = _model(int(g['weight_seed']))
    m.eval()
    img_h, img_w, pad_h, pad_w = (int(v) for v in g['shape'])
    x = torch.from_numpy(synth_fcos.image(int(g['image_seed']), 1, pad_h, pad_w, img_h, img_w)).to(DEV)
    if path != 'module':
        fuse_inference(m, winograd=(path == 'winograd'))
    if path == 'winograd':
        x = x.contiguous(memory_format=torch.channels_last)
    meta = dict(ori_shape=(96, 120, 3), img_shape=(img_h, img_w, 3), pad_shape=(pad_h, pad_w, 3),
                scale_factor=float(g['scale_factor']), flip=False)
    gb, gl = synth_fcos.gts(int(g['gt_seed']), 1, img_h, img_w)
    with torch.no_grad():
        res = m(img=[x], img_meta=[[meta]], return_loss=False, rescale=True,
                gt_bboxes=[[torch.from_numpy(gb[0]).to(DEV)]],
                gt_labels=[[torch.from_numpy(gl[0]).to(DEV)]])
        outs = m.bbox_head(m.extract_feat(x))
    if path == 'winograd':
        assert m.bbox_head._ia_wino.calls >= 2
    assert len(res) == 80
    dets = np.concatenate(res, 0)
    labels = np.concatenate([np.full(len(r), c) for c, r in enumerate(res)])
    # the head outputs against the reference's (the error the kept-id check is measured against)
    head_err = 0.0
    for kind, ts in zip(('cls', 'bbox', 'ctr', 'iou'), outs):
        for l, t in enumerate(ts):
            ref = g['%s_%d' % (kind, l)]
            head_err = max(head_err, float(np.abs(t.cpu().numpy() - ref).max()) /
                           max(1.0, float(np.abs(ref).max())))
    print('%s: head-output error %.2e (relative), %d detections' % (path, head_err, len(dets)))
    assert head_err <= 1e-4
    _match_sets(dets, labels, g['dets'], g['labels'])


def test_training_step_against_reference():
    from iouaware.config import ConfigDict
    g = np.load(os.path.join(GOLD, 'fcos_train.npz'), allow_pickle=False)
    img_h, img_w, pad_h, pad_w = (int(v) for v in g['shape'])
    for tag in ('pos', 'nopos'):
        cfg, m = _model(int(g['weight_seed']))
        m.train()
        x = torch.from_numpy(synth_fcos.image(int(g['image_seed']), 2, pad_h, pad_w, img_h, img_w)).to(DEV)
        metas = [dict(ori_shape=(img_h, img_w, 3), img_shape=(img_h, img_w, 3),
                      pad_shape=(pad_h, pad_w, 3), scale_factor=1.0, flip=False)] * 2
        if tag == 'pos':
            gb = [g['pos_gt_bboxes_%d' % i] for i in range(2)]
            gl = [g['pos_gt_labels_%d' % i] for i in range(2)]
        else:
            gb = [np.array([[0.5, 0.5, 3.0, 3.0]], np.float32)] * 2
            gl = [np.array([3], np.int64)] * 2
        # the bbox_preds gradient must carry the non-detached IoU-target path: check with a hook
        outs = m.bbox_head(m.extract_feat(x))
        losses = m.bbox_head.loss(*(outs + ([torch.from_numpy(b).to(DEV) for b in gb],
                                            [torch.from_numpy(b).to(DEV) for b in gl], metas,
                                            ConfigDict(cfg.train_cfg))))
        for k, v in losses.items():
            ref = g['%s_%s' % (tag, k)]
            assert abs(float(v.sum()) - float(ref.sum())) <= TOL * max(1.0, abs(float(ref.sum()))), \
                (tag, k, float(v.sum()), float(ref.sum()))
        if tag == 'pos':
            gi = torch.autograd.grad(losses['loss_iou'].sum(), outs[1], allow_unused=True,
                                     retain_graph=True)
            assert any(t is not None and float(t.abs().sum()) > 0 for t in gi), \
                'loss_iou does not reach bbox_preds: IoU target detached'
        sum(v.sum() for v in losses.values()).backward()
        named = dict(m.named_parameters())
        for n, ref in zip(g['%s_grad_names' % tag], g['%s_grad_norms' % tag]):
            p = named[str(n)]
            got = 0.0 if p.grad is None else float(p.grad.norm())
            assert abs(got - ref) <= 2e-4 * max(1.0, ref), (tag, str(n), got, float(ref))


def test_config_to_batched_results_with_no_torch_groupnorm():
    """Config -> build_detector -> fuse_inference(winograd=True) -> simple_test_batch: per-class
    arrays, and no tower GroupNorm module runs in eval mode"""
    from iouaware.fuse import fuse_inference
    _, m = _model(5)
    m.eval()
    fuse_inference(m, winograd=True)
    ran = []
    hooks = [mod.register_forward_hook(lambda *a: ran.append(1))
             for mod in m.modules() if isinstance(mod, torch.nn.GroupNorm)]
    x = torch.from_numpy(synth_fcos.image(6, 2, 128, 160, 120, 150)).to(DEV).contiguous(
        memory_format=torch.channels_last)
    meta = [dict(ori_shape=(120, 150, 3), img_shape=(120, 150, 3), pad_shape=(128, 160, 3),
                 scale_factor=1.0, flip=False)] * 2
    with torch.no_grad():
        res = m.simple_test_batch(x, meta, rescale=True)
    for h in hooks:
        h.remove()
    assert not ran
    assert len(res) == 2 and all(len(r) == 80 for r in res)
    assert sum(len(a) for a in res[0]) > 0
