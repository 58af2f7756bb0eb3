"""GPU: plain FCOS (FCOSHead) -- the centerness-factor point decode (ia_point_ctr_get_bboxes)
bit for bit against a numpy composition of the oracle's primitives, get_bboxes / the detector /
one training step against reference fixtures (tests/golden/fcos_plain_*.npz,
tests/golden/make_golden_fcos_plain.py), the fused head against the module head, and
multiclass_nms(score_factors=)."""
import json
import os
import tempfile

import numpy as np
import pytest
import torch

import synth_fcos
import synth_fcos_plain

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
DEV = torch.device('cuda:0')
TOL = 1e-4
SENTINEL = np.float32(-1.0)          # what the decode writes for a pair whose raw score fails


# ------------------------------------------------------------------ oracle composition
def _oracle_ctr_get_bboxes(cls, reg, ctr, strides, img_shape, sf, rescale, nms_pre, score_thr,
                           iou_thr, max_per_img):
    """one image (cls (C,H,W) etc. per level): sigmoid (oracle), fp32 product, row max, top-k
    (score desc, index asc), distance2bbox, raw threshold, per-class oracle NMS on the product,
    then the reference's output order (concatenation, or the score sort above max_per_img)"""
    import oracle
    thr = np.float32(score_thr)
    rows_box, rows_raw, rows_prod, rows_pt, rowmax = [], [], [], [], []
    base = 0
    for l, (c, r, t) in enumerate(zip(cls, reg, ctr)):
        C, H, W = c.shape
        f = oracle.vec('sigmoidf', t.reshape(-1))
        s = oracle.vec('sigmoidf', np.ascontiguousarray(c.reshape(C, -1).T))
        prod = (s * f[:, None]).astype(np.float32)
        rowmax.append(prod.max(1))
        idx = np.arange(H * W)
        if 0 < nms_pre < H * W:
            idx = np.lexsort((idx, -prod.max(1)))[:nms_pre]
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
        rows_raw.append(s[idx])
        rows_prod.append(prod[idx])
        rows_pt.append(idx + base)
        base += H * W
    boxes, raw, prod = np.concatenate(rows_box), np.concatenate(rows_raw), np.concatenate(rows_prod)
    written = np.where(raw > thr, prod, SENTINEL).astype(np.float32)
    found = []
    for c in range(raw.shape[1]):
        rows = np.nonzero(raw[:, c] > thr)[0]
        if rows.size == 0:
            continue
        dets = np.concatenate([boxes[rows], prod[rows, c:c + 1]], 1)
        for k in np.sort(oracle.nms(dets, iou_thr)):
            found.append((c, rows[k]))
    if len(found) > max_per_img:
        found = sorted(found, key=lambda cr: (-prod[cr[1], cr[0]], cr[0], cr[1]))[:max_per_img]
    return dict(boxes=boxes, scores=written, points=np.concatenate(rows_pt),
                rowmax=np.concatenate(rowmax), best=written.max(1),
                dets=np.array([list(boxes[r]) + [prod[r, c]] for c, r in found],
                              np.float32).reshape(-1, 5),
                labels=np.array([c for c, _ in found], np.int64),
                rows=np.array([r for _, r in found], np.int64))


def _to_dev(xs, nhwc):
    out = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in xs]
    return [t.contiguous(memory_format=torch.channels_last) for t in out] if nhwc else out


def _run_and_check(cls, reg, ctr, sizes, shapes, factors, rescale, nms_pre, nhwc, score_thr=0.05,
                   max_per_img=100):
    from iouaware import fcos_ops
    B = cls[0].shape[0]
    geom = fcos_ops.PointGeometry(sizes, synth_fcos.STRIDES, 80, nms_pre)
    dets, labels, rows, num, views = fcos_ops.point_ctr_get_bboxes(
        geom, _to_dev(cls, nhwc), _to_dev(reg, nhwc), _to_dev(ctr, nhwc), shapes, factors, rescale,
        score_thr, 0.5, max_per_img, debug=True)
    torch.cuda.synchronize()
    cand = views['cand_idx'].cpu().numpy()
    lvl_off = np.cumsum([0] + [h * w for (h, w) in sizes])
    cand_off = np.cumsum([0] + geom.level_cands)
    outs = []
    for b in range(B):
        o = _oracle_ctr_get_bboxes([c[b] for c in cls], [r[b] for r in reg], [t[b] for t in ctr],
                                   synth_fcos.STRIDES, shapes[b], factors[b], rescale, nms_pre,
                                   score_thr, 0.5, max_per_img)
        assert np.array_equal(views['rowmax'][b].cpu().numpy(), o['rowmax'])
        pts = np.concatenate([cand[b, cand_off[l]:cand_off[l + 1]] + lvl_off[l]
                              for l in range(len(sizes))])
        assert np.array_equal(pts, o['points'])
        assert np.array_equal(views['boxes'][b].cpu().numpy(), o['boxes'])
        assert np.array_equal(views['scores_t'][b, :, :geom.R].cpu().numpy().T, o['scores'])
        assert np.array_equal(views['best_score'][b].cpu().numpy(), o['best'])
        n = int(num[b])
        assert n == len(o['labels'])
        d = dets[b, :n].cpu().numpy()
        assert np.array_equal(d, o['dets'])
        assert np.array_equal(labels[b, :n].cpu().numpy(), o['labels'])
        assert np.array_equal(rows[b, :n].cpu().numpy(), o['rows'])
        assert (d[:, 4] >= 0).all()                    # no sentinel reaches an output row
        outs.append((d, labels[b, :n].cpu().numpy()))
    return outs


@pytest.mark.parametrize('nhwc', [False, True])
@pytest.mark.parametrize('pad,nms_pre,rescale', [((320, 448), 150, True), ((320, 448), 150, False),
                                                 ((320, 448), 3000, True),
                                                 ((800, 1344), 1000, True)])
def test_ctr_decode_bit_exact_against_oracle(nhwc, pad, nms_pre, rescale):
    pad_h, pad_w = pad
    sizes = synth_fcos.level_shapes(pad_h, pad_w)
    cls, reg, ctr = synth_fcos_plain.head_outputs(31, 2, sizes)
    shapes = [(pad_h - 20, pad_w - 7, 3), (pad_h, pad_w - 48, 3)]
    outs = _run_and_check(cls, reg, ctr, sizes, shapes, [0.75, 1.5], rescale, nms_pre, nhwc)
    assert all(len(d) > 0 for d, _ in outs)


@pytest.mark.parametrize('nhwc', [False, True])
def test_ctr_decode_hand_made_threshold_cases(nhwc):
    """raw > thr > product is kept; raw <= thr with a large centerness is dropped; a centerness
    logit whose sigmoid underflows to 0 keeps its pair with score 0"""
    sizes = synth_fcos.level_shapes(64, 96)
    cls = [np.full((1, 80, h, w), -20.0, np.float32) for (h, w) in sizes]
    reg = [np.full((1, 4, h, w), 6.0, np.float32) for (h, w) in sizes]
    ctr = [np.zeros((1, 1, h, w), np.float32) for (h, w) in sizes]
    cls[0][0, 3, 1, 1], ctr[0][0, 0, 1, 1] = 0.0, -3.0         # raw 0.5, product 0.0237
    cls[0][0, 5, 4, 6], ctr[0][0, 0, 4, 6] = -3.0, 10.0        # raw 0.0474 <= 0.05, product ~0.047
    cls[1][0, 7, 2, 3], ctr[1][0, 0, 2, 3] = 2.0, -200.0       # raw 0.88, product 0
    (d, l), = _run_and_check(cls, reg, ctr, sizes, [(64, 96, 3)], [1.0], False, 1000, nhwc)
    assert l.tolist() == [3, 7]
    assert 0 < d[0, 4] < 0.05 and d[1, 4] == 0.0
    assert d[0, :4].tolist() == [6.0, 6.0, 18.0, 18.0]          # point (12, 12), distances 6


def _metas(pad_h, pad_w):
    return synth_fcos_plain.get_bboxes_metas(pad_h, pad_w)


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


def test_get_bboxes_against_reference_fixture():
    from iouaware.config import ConfigDict
    from iouaware.fcos_head import FCOSHead
    g = np.load(os.path.join(GOLD, 'fcos_plain_get_bboxes.npz'))
    head = FCOSHead(81, 256, strides=[8, 16, 32, 64, 128]).to(DEV)
    below = 0
    for tag, pad_h, pad_w, nms_pre, rescale, shift in synth_fcos_plain.GET_BBOXES_CASES:
        sizes = synth_fcos.level_shapes(pad_h, pad_w)
        cls, reg, ctr = synth_fcos_plain.head_outputs(int(g['seed']), 2, sizes, shift)
        cfg = ConfigDict(dict(nms_pre=nms_pre, min_bbox_size=0, score_thr=0.05,
                              nms=dict(type='nms', iou_thr=0.5), max_per_img=100))
        for nhwc in (False, True):
            res = head.get_bboxes(_to_dev(cls, nhwc), _to_dev(reg, nhwc), _to_dev(ctr, nhwc),
                                  _metas(pad_h, pad_w), cfg, rescale)
            for b, (d, l) in enumerate(res):
                rd, rl = g['dets_%s_%d' % (tag, b)], g['labels_%s_%d' % (tag, b)]
                d, l = d.cpu().numpy(), l.cpu().numpy()
                assert len(rd) > 0
                _match_sets(d, l, rd, rl)
                if nhwc:
                    below += int((rd[:, 4] < 0.05).sum())
    assert below > 0, 'the fixture has no kept detection with raw > score_thr > product'


# ------------------------------------------------------------------ model level
CONFIG = 'fcos_r50_caffe_fpn_gn_1x_4gpu'


def _model(seed):
    import iouaware
    from iouaware.config import Config
    with open(os.path.join(GOLD, 'fcos_plain_ref.json')) as fh:
        rec = json.load(fh)[CONFIG]
    with tempfile.NamedTemporaryFile('w', suffix='.py', delete=False) as fh:
        fh.write('\n'.join('%s = %r' % (k, rec[k]) for k in ('model', 'train_cfg', 'test_cfg')) + '\n')
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
    sizes = synth_fcos.level_shapes(256, 320)
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
    assert len(out) == len(ref) == 3
    for kind, a, b in zip(('cls', 'bbox', 'ctr'), out, ref):
        for l, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape and x.is_contiguous(memory_format=torch.channels_last)
            scale = max(1.0, float(y.abs().max()))
            err = float((x - y).abs().max())
            assert err <= TOL * scale, (kind, l, err, scale)


@pytest.mark.parametrize('path', ['module', 'fused', 'winograd'])
def test_detector_end_to_end_against_reference(path):
    from iouaware.fuse import fuse_inference
    g = np.load(os.path.join(GOLD, 'fcos_plain_e2e.npz'))
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
    with torch.no_grad():
        res = m(img=[x], img_meta=[[meta]], return_loss=False, rescale=True)
        outs = m.bbox_head(m.extract_feat(x))
        # the per-image route (get_bboxes without gt arguments) gives the same detections
        per_image = m.bbox_head.get_bboxes(*(outs + ([meta], m.test_cfg, True)))[0]
    if path == 'winograd':
        assert m.bbox_head._ia_wino.calls >= 2
    assert len(res) == 80 and len(outs) == 3
    dets = np.concatenate(res, 0)
    labels = np.concatenate([np.full(len(r), c) for c, r in enumerate(res)])
    head_err = 0.0
    for kind, ts in zip(('cls', 'bbox', 'ctr'), outs):
        for l, t in enumerate(ts):
            ref = g['%s_%d' % (kind, l)]
            head_err = max(head_err, float(np.abs(t.cpu().numpy() - ref).max()) /
                           max(1.0, float(np.abs(ref).max())))
    print('%s: head-output error %.2e (relative), %d detections' % (path, head_err, len(dets)))
    assert head_err <= 1e-4
    _match_sets(dets, labels, g['dets'], g['labels'])
    _match_sets(per_image[0].cpu().numpy(), per_image[1].cpu().numpy(), g['dets'], g['labels'])


def test_training_step_against_reference():
    from iouaware.config import ConfigDict
    g = np.load(os.path.join(GOLD, 'fcos_plain_train.npz'), allow_pickle=False)
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
        outs = m.bbox_head(m.extract_feat(x))
        losses = m.bbox_head.loss(*(outs + ([torch.from_numpy(b).to(DEV) for b in gb],
                                            [torch.from_numpy(b).to(DEV) for b in gl], metas,
                                            ConfigDict(cfg.train_cfg))))
        assert sorted(losses) == ['loss_centerness', 'loss_cls', 'loss_reg']
        for k, v in losses.items():
            ref = g['%s_%s' % (tag, k)]
            assert abs(float(v.sum()) - float(ref.sum())) <= TOL * max(1.0, abs(float(ref.sum()))), \
                (tag, k, float(v.sum()), float(ref.sum()))
        sum(v.sum() for v in losses.values()).backward()
        named = dict(m.named_parameters())
        for n, ref in zip(g['%s_grad_names' % tag], g['%s_grad_norms' % tag]):
            p = named[str(n)]
            got = 0.0 if p.grad is None else float(p.grad.norm())
            assert abs(got - ref) <= 2e-4 * max(1.0, ref), (tag, str(n), got, float(ref))


# ------------------------------------------------------------------ multiclass_nms(score_factors=)
def _oracle_multiclass_nms(boxes, scores, factors, score_thr, iou_thr, max_num):
    """bbox_nms.py:33-56 with score_factors, on the oracle's NMS"""
    import oracle
    out, labels = [], []
    for i in range(1, scores.shape[1]):
        rows = np.nonzero(scores[:, i] > np.float32(score_thr))[0]
        if rows.size == 0:
            continue
        s = (scores[rows, i] * factors[rows]).astype(np.float32)
        dets = np.concatenate([boxes[rows], s[:, None]], 1).astype(np.float32)
        keep = np.sort(oracle.nms(dets, iou_thr))
        out.append(dets[keep])
        labels.append(np.full(len(keep), i - 1, np.int64))
    if not out:
        return np.zeros((0, 5), np.float32), np.zeros((0,), np.int64)
    out, labels = np.concatenate(out), np.concatenate(labels)
    if out.shape[0] > max_num:
        order = np.argsort(-out[:, 4], kind='stable')[:max_num]
        out, labels = out[order], labels[order]
    return out, labels


def _nms_inputs(seed, n, ncls):
    rs = np.random.RandomState(seed)
    xy = rs.uniform(0, 400, (n, 2))
    wh = rs.uniform(8, 80, (n, 2))
    boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    scores = (rs.uniform(0, 1, (n, ncls + 1)) ** 3).astype(np.float32)
    factors = rs.uniform(0, 1, n).astype(np.float32)
    factors[::17] = 0.0                                  # exact zeros keep their pairs
    return boxes, scores, factors


@pytest.mark.parametrize('n,ncls,max_num', [(600, 20, 100), (600, 20, 1000), (200, 3, 1000),
                                            (9000, 2, 100)])
def test_multiclass_nms_score_factors_against_oracle(n, ncls, max_num):
    """batched route (n <= IA_MAX_CANDIDATES) and the per-class route beyond it"""
    from iouaware.nms_op import multiclass_nms
    boxes, scores, factors = _nms_inputs(n + ncls, n, ncls)
    ref_d, ref_l = _oracle_multiclass_nms(boxes, scores, factors, 0.05, 0.5, max_num)
    if len(ref_d) < max_num:                             # raw > thr > product pairs are kept
        assert (ref_d[:, 4] < 0.05).any()
    d, l = multiclass_nms(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), 0.05,
                          dict(type='nms', iou_thr=0.5), max_num,
                          score_factors=torch.from_numpy(factors).to(DEV))
    assert np.array_equal(d.cpu().numpy(), ref_d)
    assert np.array_equal(l.cpu().numpy(), ref_l)


def test_multiclass_soft_nms_score_factors_thresholds_the_raw_score():
    from iouaware.nms_op import multiclass_nms
    boxes, scores, factors = _nms_inputs(7, 300, 6)
    cfg = dict(type='soft_nms', iou_thr=0.5, min_score=1e-3)
    d, l = multiclass_nms(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), 0.05,
                          cfg, 1000, score_factors=torch.from_numpy(factors).to(DEV))
    # the same problem with the masked products as scores and a threshold below 0
    masked = np.where(scores > np.float32(0.05), scores * factors[:, None], -1.0).astype(np.float32)
    d2, l2 = multiclass_nms(torch.from_numpy(boxes).to(DEV), torch.from_numpy(masked).to(DEV), -0.5,
                            cfg, 1000)
    assert np.array_equal(d.cpu().numpy(), d2.cpu().numpy())
    assert np.array_equal(l.cpu().numpy(), l2.cpu().numpy())
    assert len(d) > 0 and (d[:, 4] >= 0).all()


# ------------------------------------------------------------------ determinism
def test_bits_repeat_and_do_not_depend_on_the_batch():
    from iouaware import fcos_ops
    sizes = synth_fcos.level_shapes(320, 448)
    cls, reg, ctr = synth_fcos_plain.head_outputs(17, 8, sizes)
    geom = fcos_ops.PointGeometry(sizes, synth_fcos.STRIDES, 80, 150)
    shapes = [(320 - 3 * b, 448 - 5 * b, 3) for b in range(8)]
    factors = [1.0 + 0.1 * b for b in range(8)]

    def run(sl, nhwc):
        out = fcos_ops.point_ctr_get_bboxes(
            geom, _to_dev([c[sl] for c in cls], nhwc), _to_dev([r[sl] for r in reg], nhwc),
            _to_dev([t[sl] for t in ctr], nhwc), shapes[sl], factors[sl], True, 0.05, 0.5, 100)
        torch.cuda.synchronize()
        return [t.cpu() for t in out]

    for nhwc in (False, True):
        a = run(slice(0, 8), nhwc)
        b = run(slice(0, 8), nhwc)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        alone = run(slice(5, 6), nhwc)
        n = int(a[3][5])
        assert n == int(alone[3][0]) > 0
        for u, v in zip(a[:3], alone[:3]):
            assert torch.equal(u[5, :n], v[0, :n])


def test_config_to_batched_results_with_no_torch_groupnorm():
    """config -> build_detector -> fuse_inference(winograd=True) -> simple_test_batch: per-class
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
