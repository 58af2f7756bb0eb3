"""GPU: plain RetinaNet (RetinaHead) -- the IA_CLS_*_NOIOU anchor decode bit for bit against a
numpy composition of the oracle's primitives (sigmoid / exp, delta2bbox, NMS, the reference's
output order), the device sigmoid's monotonicity that the row maximum on logits relies on,
get_bboxes against the reference fixture (tests/golden/retina_plain_get_bboxes.npz, written by
tests/golden/make_golden_retina_plain.py), and one training step on the HIP losses."""
import os

import numpy as np
import pytest
import torch

import synth
import gpu_util as G

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
DEV = torch.device("cuda:0")
IA_E_ARG = -1                        # include/iouaware.h


def _head(softmax=False, num_classes=81):
    from iouaware.head import RetinaHead
    kw = dict(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)) \
        if softmax else {}
    return RetinaHead(num_classes, 256, anchor_strides=list(synth.STRIDES), **kw)


# ------------------------------------------------------------------ oracle composition
def _scores(x, softmax):
    """x (n, Cin) logits of one level in reference row order -> (n, C) scores (fp32, the kernels'
    operation sequence: sigmoid; or m = max of all C + 1 logits, s = sum of exp(x - m) in class
    order, p = exp(x_c - m) / s for the foreground columns)"""
    import oracle
    if not softmax:
        return oracle.vec('sigmoidf', np.ascontiguousarray(x))
    m = x.max(1, keepdims=True)
    e = oracle.vec('expf', np.ascontiguousarray(x - m, np.float32))
    s = np.zeros(x.shape[0], np.float32)
    for c in range(x.shape[1]):
        s = (s + e[:, c]).astype(np.float32)
    return (e[:, 1:] / s[:, None]).astype(np.float32)


def _oracle_get_bboxes(cls, reg, base, img_shape, sf, rescale, nms_pre, score_thr, iou_thr,
                       max_per_img, softmax):
    """one image: cls (A*Cin, H, W), reg (A*4, H, W) per level (fp32 values of the stored maps)"""
    import oracle
    A = base.shape[1]
    rowmax, cand, boxes, scores = [], [], [], []
    for l, (c, r) in enumerate(zip(cls, reg)):
        _, H, W = c.shape
        x = c.reshape(A, -1, H * W).transpose(2, 0, 1).reshape(H * W * A, -1)   # row p*A + a
        s = _scores(x, softmax)
        rm = s.max(1)
        rowmax.append(rm)
        idx = np.arange(rm.size)
        if 0 < nms_pre < rm.size:
            idx = np.lexsort((idx, -rm))[:nms_pre]
        cand.append(idx.astype(np.int32))
        anchors = oracle.grid_anchors(base[l], H, W, synth.STRIDES[l])
        d = r.reshape(A, 4, H * W).transpose(2, 0, 1).reshape(H * W * A, 4)
        b = oracle.delta2bbox(anchors[idx], d[idx], max_shape=img_shape[:2])
        if rescale:
            f = np.asarray(sf, np.float32).reshape(-1)
            b = (b / (np.repeat(f, 4) if f.size == 1 else f)).astype(np.float32)
        boxes.append(b)
        scores.append(s[idx])
    boxes, scores = np.concatenate(boxes), np.concatenate(scores)
    found = []
    for c in range(scores.shape[1]):
        rows = np.nonzero(scores[:, c] > np.float32(score_thr))[0]
        if rows.size:
            dets = np.concatenate([boxes[rows], scores[rows, c:c + 1]], 1)
            found += [(c, rows[k]) for k in np.sort(oracle.nms(dets, iou_thr))]
    if len(found) > max_per_img:
        found = sorted(found, key=lambda cr: (-scores[cr[1], cr[0]], cr[0], cr[1]))[:max_per_img]
    return dict(rowmax=rowmax, cand=np.concatenate(cand), boxes=boxes, scores=scores,
                dets=np.array([list(boxes[r]) + [scores[r, c]] for c, r in found],
                              np.float32).reshape(-1, 5),
                labels=np.array([c for c, _ in found], np.int64),
                rows=np.array([r for _, r in found], np.int64))


def _run_and_check(cls, reg, sizes, shapes, factors, rescale, nms_pre, nhwc, softmax=False,
                   dtype=torch.float32, score_thr=0.05, max_per_img=100, in_place=None):
    from iouaware import ops
    head = _head(softmax, cls[0].shape[1] // 9 + (0 if softmax else 1))
    geom = head.geometry(sizes, nms_pre)
    dc, dr = G.to_dev(cls, dtype), G.to_dev(reg, dtype)
    if nhwc:
        dc, dr = [[t.contiguous(memory_format=torch.channels_last) for t in x] for x in (dc, dr)]
    # the oracle sees the values the kernels read (bf16 storage rounds the logits)
    cls = [t.float().cpu().numpy() for t in dc]
    reg = [t.float().cpu().numpy() for t in dr]
    natural = ops.geometry_for(geom, dc, dr, None).layout == 1
    if in_place is not None:
        assert natural == in_place          # channels-last maps consumed as they are, or transposed
    dets, labels, rows, num, dbg = ops.get_bboxes(geom, dc, dr, None, shapes, factors, rescale,
                                                  score_thr, 0.5, max_per_img, debug=True)
    lz = ops.get_bboxes(geom, dc, dr, None, shapes, factors, rescale, score_thr, 0.5, max_per_img)
    for x, y in zip(lz, (dets, labels, rows, num)):
        assert torch.equal(x, y), 'lazy NMS differs'
    torch.cuda.synchronize()
    dbg = {k: v.cpu().numpy() for k, v in dbg.items()}
    base = np.stack([g.base_anchors.numpy() for g in head.anchor_generators])
    for b in range(cls[0].shape[0]):
        o = _oracle_get_bboxes([c[b] for c in cls], [r[b] for r in reg], base, shapes[b],
                               factors[b], rescale, nms_pre, score_thr, 0.5, max_per_img, softmax)
        off = 0
        for l, (h, w) in enumerate(sizes):
            n_l = h * w * geom.A
            dev = dbg['rowmax'][b][off:off + n_l]
            if not natural:
                dev = dev.reshape(geom.A, h * w).T.reshape(-1)
            assert G.same_bits(dev, o['rowmax'][l]), 'rowmax img %d level %d' % (b, l)
            off += n_l
        assert np.array_equal(dbg['cand_idx'][b], o['cand']), 'top-k img %d' % b
        assert G.same_bits(dbg['boxes'][b], o['boxes']), 'boxes img %d' % b
        assert G.same_bits(dbg['scores_t'][b][:, :geom.R].T, o['scores']), 'scores img %d' % b
        n = int(num[b])
        assert n == len(o['labels'])
        assert G.same_bits(dets[b, :n].cpu().numpy(), o['dets'])
        assert np.array_equal(labels[b, :n].cpu().numpy(), o['labels'])
        assert np.array_equal(rows[b, :n].cpu().numpy(), o['rows'])
    return dets, labels, num


def _outputs(seed, B, sizes, softmax=False, spread=2.0, cin=None):
    rs = np.random.RandomState(seed)
    cin = cin or (81 if softmax else 80)
    cls = [(rs.standard_normal((B, 9 * cin, h, w)) * spread - 3.5).astype(np.float32) for h, w in sizes]
    reg = [(rs.standard_normal((B, 36, h, w)) * 0.3).astype(np.float32) for h, w in sizes]
    return cls, reg


@pytest.mark.parametrize('nhwc', [False, True])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('nms_pre,rescale,factors', [(150, True, [0.75, 1.5]),
                                                     (4000, False, [1.0, 1.0]),
                                                     (300, True, [[0.5, 0.6, 0.7, 0.8], 1.25])])
def test_sigmoid_decode_bit_exact_against_oracle(nhwc, dtype, nms_pre, rescale, factors):
    sizes = synth.level_shapes(128, 192)
    cls, reg = _outputs(71, 2, sizes)
    shapes = [(120, 185, 3), (128, 150, 3)]
    dets, _, num = _run_and_check(cls, reg, sizes, shapes, factors, rescale, nms_pre, nhwc,
                                  dtype=dtype)
    assert (num.cpu() > 0).all()


@pytest.mark.parametrize('nhwc', [False, True])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('cin', [81, 80])
@pytest.mark.parametrize("nms_pre", [100, 4000])
def test_softmax_decode_bit_exact_against_oracle(nhwc, dtype, cin, nms_pre):
    """cin = 81 (80 foreground classes): a channels-last class row is no whole number of 16-byte
    vectors, so the maps are transposed to NCHW; cin = 80 (79 foreground classes): channels-last
    maps are consumed in place by the channels-last branch of the softmax kernels"""
    sizes = synth.level_shapes(64, 96)
    cls, reg = _outputs(72, 2, sizes, softmax=True, spread=3.0, cin=cin)
    in_place = nhwc and (cin * (4 if dtype == torch.float32 else 2)) % 16 == 0
    _run_and_check(cls, reg, sizes, [(64, 90, 3), (60, 96, 3)], [1.0, 2.0], True, nms_pre, nhwc,
                   softmax=True, dtype=dtype, in_place=in_place)


@pytest.mark.parametrize('nhwc', [False, True])
def test_hand_made_ties(nhwc):
    """saturated rows (sigmoid == 1.0f from different logits), equal sigmoids from different
    logits in one row, and a score exactly at score_thr (not kept: '>' like bbox_nms.py:34)"""
    import oracle
    sizes = synth.level_shapes(64, 96)
    cls = [np.full((1, 720, h, w), -12.0, np.float32) for (h, w) in sizes]
    reg = [np.zeros((1, 36, h, w), np.float32) for (h, w) in sizes]
    for k, v in enumerate((30.0, 40.0, 95.0, 17.5)):          # all saturate to 1.0f
        cls[0][0, (k % 9) * 80 + 3, 2 + k, 5] = v
    cls[1][0, 7, 1, 1], cls[1][0, 9, 1, 1] = 20.0, 25.0          # equal sigmoid, two classes
    x = np.float32(np.log(0.05 / 0.95))
    while oracle.vec('sigmoidf', np.array([x], np.float32))[0] < np.float32(0.05):
        x = np.nextafter(x, np.float32(1))
    at = x if oracle.vec('sigmoidf', np.array([x], np.float32))[0] == np.float32(0.05) else None
    cls[2][0, 11, 0, 0] = x
    dets, labels, num = _run_and_check(cls, reg, sizes, [(64, 96, 3)], [1.0], False, 20, nhwc)
    n = int(num[0])
    assert n >= 5 and (dets[0, :n, 4].cpu() > 0.05).all()
    if at is not None:
        assert 11 not in labels[0, :n].cpu().tolist()


def test_soft_nms_case_against_oracle():
    import oracle
    from iouaware import ops
    sizes = synth.level_shapes(64, 96)
    cls, reg = _outputs(73, 1, sizes)
    head = _head()
    geom = head.geometry(sizes, 80)
    dets, labels, _, num = ops.get_bboxes(geom, G.to_dev(cls), G.to_dev(reg), None, [(64, 96, 3)],
                                          [1.0], False, 0.05, 0.5, 100,
                                          soft=dict(method='linear', sigma=0.5, min_score=1e-3))
    base = np.stack([g.base_anchors.numpy() for g in head.anchor_generators])
    o = _oracle_get_bboxes([c[0] for c in cls], [r[0] for r in reg], base, (64, 96, 3), 1.0, False,
                           80, 0.05, 0.5, 100, False)
    ref = oracle.multiclass_soft_nms(o['boxes'], o['scores'], 0.05, 0.5, 'linear', 0.5, 1e-3, 100)
    ref_d, ref_l = ref['det_bboxes'], ref['det_labels']
    n = int(num[0])
    assert n == ref_d.shape[0] and n > 0
    assert G.same_bits(dets[0, :n].cpu().numpy(), ref_d)
    assert np.array_equal(labels[0, :n].cpu().numpy(), np.asarray(ref_l))


def test_noiou_kind_rejects_an_iou_map_and_iou_kind_a_missing_one():
    from iouaware import _lib, ops
    import ctypes as C
    sizes = synth.level_shapes(64, 96)
    cls, reg = _outputs(74, 1, sizes)
    geom = _head().geometry(sizes, 50)
    dc, dr = G.to_dev(cls), G.to_dev(reg)
    p, B, dt, g = ops.level_ptrs(geom, dc, dr, None)
    iou = torch.zeros(9 * sum(h * w for h, w in sizes), device=DEV)
    p.iou[0] = iou.data_ptr()
    out = torch.empty((1, g.N), device=DEV)
    rc = _lib.lib().ia_decode_fuse_rowmax(g.ref(), C.byref(p), 1, dt, out.data_ptr(), None)
    assert rc == IA_E_ARG
    ia = ops.HeadGeometry(sizes, synth.STRIDES, np.stack([x.base_anchors.numpy() for x in
                                                          _head().anchor_generators]), 80, 50)
    p.iou[0] = None
    assert _lib.lib().ia_decode_fuse_rowmax(ia.ref(), C.byref(p), 1, dt, out.data_ptr(), None) == \
        IA_E_ARG


def test_device_sigmoid_never_decreases():
    """the row maximum is taken on the logits: sigmoidf_ must be non-decreasing over every float of
    [-110, 100] (beyond: 0 and 1 exactly), chunk borders included"""
    from iouaware import ops
    def ascending(k0, k1):
        """floats number k0 .. k1 - 1 of [-110, 100] in ascending order, as a device tensor"""
        k = torch.arange(k0, k1, dtype=torch.int64, device=DEV)
        b = torch.where(k < n_neg, neg_top - k, k - n_neg)       # -110 .. -0, then +0 .. 100
        b = torch.where(b >= 2 ** 31, b - 2 ** 32, b)
        return b.to(torch.int32).view(torch.float32)

    neg_top = int(np.float32(-110.0).view(np.uint32))           # bits of the negatives fall towards -0
    n_neg = neg_top - 0x80000000 + 1
    total = n_neg + int(np.float32(100.0).view(np.uint32)) + 1
    prev = None
    chunk = 1 << 26
    for i in range(0, total, chunk):
        x = ascending(i, min(i + chunk, total))
        assert bool((x[1:] >= x[:-1]).all())
        y = ops.test_math(2, x)
        if prev is not None:
            assert bool(y[0] >= prev), 'decreasing step at a chunk border'
        assert bool((y[1:] >= y[:-1]).all()), 'decreasing step in chunk %d' % (i // chunk)
        prev = y[-1]
    assert float(ops.test_math(2, ascending(0, 1))[0]) >= 0.0
    assert float(prev) == 1.0


def test_get_bboxes_against_reference_fixture():
    from iouaware.config import ConfigDict
    f = np.load(os.path.join(GOLD, 'retina_plain_get_bboxes.npz'))
    head = _head()
    k = 0
    while 'case_%d' % k in f:
        seed, B, ph, pw, nms_pre, rescale = [int(v) for v in f['case_%d' % k]]
        sf = [float(v) for v in f['sf_%d' % k]]
        cls, reg, _ = synth.head_outputs(seed, B, ph, pw, 'A')
        metas = [dict(img_shape=(ph - 9 * b, pw - 13 * b, 3), scale_factor=sf[b],
                      pad_shape=(ph, pw, 3)) for b in range(B)]
        cfg = ConfigDict(nms_pre=nms_pre, min_bbox_size=0, score_thr=0.05,
                         nms=dict(type='nms', iou_thr=0.5), max_per_img=100)
        res = head.get_bboxes(G.to_dev(cls), G.to_dev(reg), None, None, metas, cfg, bool(rescale))
        for b, (d, l) in enumerate(res):
            rd, rl = f['dets_%d_%d' % (k, b)], f['labels_%d_%d' % (k, b)]
            assert d.shape[0] == rd.shape[0]
            d = d.cpu().numpy()
            assert np.array_equal(l.cpu().numpy(), rl)               # 0-based, like the reference's
            # boxes: |a - b| <= 1e-4 * max(1, |b|) per coordinate; scores: 1e-4 absolute
            assert (np.abs(d[:, :4] - rd[:, :4]) <= 1e-4 * np.maximum(1.0, np.abs(rd[:, :4]))).all()
            assert (np.abs(d[:, 4] - rd[:, 4]) <= 1e-4).all()
        k += 1
    assert k == 2


def test_one_image_alone_matches_batch_and_repeats():
    from iouaware import ops
    sizes = synth.level_shapes(128, 192)
    cls, reg = _outputs(75, 8, sizes)
    geom = _head().geometry(sizes, 1000)
    dc = [t.contiguous(memory_format=torch.channels_last) for t in G.to_dev(cls)]
    dr = [t.contiguous(memory_format=torch.channels_last) for t in G.to_dev(reg)]
    shapes, sfs = [(128, 192, 3)] * 8, [1.0] * 8
    a = ops.get_bboxes(geom, dc, dr, None, shapes, sfs, True, 0.05, 0.5, 100)
    b = ops.get_bboxes(geom, dc, dr, None, shapes, sfs, True, 0.05, 0.5, 100)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    one = ops.get_bboxes(geom, [c[3:4] for c in dc], [r[3:4] for r in dr], None, shapes[:1],
                         sfs[:1], True, 0.05, 0.5, 100)
    n = int(one[3][0])
    assert n == int(a[3][3]) and torch.equal(one[0][0, :n], a[0][3, :n])
    assert torch.equal(one[1][0, :n], a[1][3, :n])


@pytest.mark.module_path
def test_training_step_on_the_hip_losses():
    """loss() returns exactly loss_cls / loss_bbox per level with finite values, backward reaches
    every parameter with finite gradients, and the HIP assigner's targets give the same losses as
    the torch target path (no comparison against the oracle's loss sums here)"""
    from iouaware.config import ConfigDict
    torch.manual_seed(0)
    losses_kw = dict(loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25,
                                   loss_weight=1.0),
                     loss_bbox=dict(type='SmoothL1Loss', beta=0.11, loss_weight=1.0))
    from iouaware.head import RetinaHead
    head = RetinaHead(81, 256, **losses_kw).to(DEV)
    head.init_weights()
    sizes = synth.level_shapes(128, 192)
    feats = [torch.randn(2, 256, h, w, device=DEV) for h, w in sizes]
    cls, reg = head(feats)
    gts = [torch.tensor([[10., 12., 80., 90.], [50., 40., 150., 120.]], device=DEV),
           torch.tensor([[30., 20., 100., 110.]], device=DEV)]
    labels = [torch.tensor([3, 17], device=DEV), torch.tensor([45], device=DEV)]
    metas = [dict(pad_shape=(128, 192, 3), img_shape=(128, 192, 3))] * 2
    cfg = ConfigDict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.4,
                                   min_pos_iou=0, ignore_iof_thr=-1),
                     allowed_border=-1, pos_weight=-1, debug=False)
    losses = head.loss(cls, reg, gts, labels, metas, cfg)
    assert sorted(losses) == ['loss_bbox', 'loss_cls']
    assert all(len(v) == 5 for v in losses.values())
    total = sum(sum(v) for v in losses.values())
    assert torch.isfinite(total).all() and float(total) > 0
    total.sum().backward()
    for name, p in head.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    # the device assigner and the torch path give the same losses
    head2 = RetinaHead(81, 256, **losses_kw).to(DEV)
    head2.load_state_dict(head.state_dict())
    head2._device_targets_ok = lambda *a: False
    cls2, reg2 = head2(feats)
    l2 = head2.loss(cls2, reg2, gts, labels, metas, cfg)
    for k in losses:
        for x, y in zip(losses[k], l2[k]):
            assert torch.allclose(x, y, rtol=1e-4, atol=1e-6), k
