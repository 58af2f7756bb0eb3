"""GPU: device target assignment (csrc/assign.hip) against the targets the
reference's anchor_target produced (tests/golden/losses_small.npz) and against the torch
implementation in iouaware/targets.py on random batches."""
import os

import numpy as np
import pytest
import torch

import synth
import gpu_util as G

pytestmark = pytest.mark.gpu


def test_device_targets_equal_reference(golden_dir):
    from iouaware import ops
    f = np.load(os.path.join(golden_dir, 'losses_small.npz'))
    ih, iw, ph, pw = [int(v) for v in f['img']]
    B = int(f['batch'])
    geom, base = G.geometry(ph, pw, -1)
    gts = [torch.from_numpy(f['gt_bboxes_%d' % b]).cuda() for b in range(B)]
    gls = [torch.from_numpy(f['gt_labels_%d' % b]).cuda() for b in range(B)]
    labels, lw, bt, bw, counts = ops.anchor_targets(geom, gts, gls, [(ph, pw, 3)] * B, 0.5, 0.4, 0.0,
                                                    -1)
    assert int(counts[:, 0].clamp(min=1).sum()) == int(f['num_total_pos'])
    assert int(counts[:, 1].clamp(min=1).sum()) == int(f['num_total_neg'])
    for l in range(5):
        assert np.array_equal(labels[l].cpu().numpy(), f['labels_%d' % l])
        assert np.array_equal(lw[l].cpu().numpy(), f['label_weights_%d' % l])
        assert np.array_equal(bw[l].cpu().numpy(), f['bbox_weights_%d' % l])
        assert np.allclose(bt[l].cpu().numpy(), f['bbox_targets_%d' % l], rtol=1e-5, atol=1e-6)


def test_device_targets_and_losses_mixed_pad_shapes_equal_reference(golden_dir):
    """T1 pinned on the reference: images of different pad_shape in one batch (partly false
    valid_flags / inside_flags, `unmap`): ia_anchor_targets and the whole head.loss (device
    targets + all-levels loss kernels, both layouts) against tests/golden/losses_mixed_pad.npz"""
    from iouaware import ops
    from iouaware.head import IoUawareRetinaHead
    from test_host_targets import HEAD_KW, TRAIN_CFG
    f = np.load(os.path.join(golden_dir, 'losses_mixed_pad.npz'))
    ph, pw = [int(v) for v in f['tensor']]
    B = int(f['batch'])
    shapes = [[int(v) for v in f['shapes'][b]] for b in range(B)]
    geom, base = G.geometry(ph, pw, -1)
    gts = [torch.from_numpy(f['gt_bboxes_%d' % b]).cuda() for b in range(B)]
    gls = [torch.from_numpy(f['gt_labels_%d' % b]).cuda() for b in range(B)]
    pads = [(s[2], s[3], 3) for s in shapes]
    labels, lw, bt, bw, counts = ops.anchor_targets(geom, gts, gls, pads, 0.5, 0.4, 0.0, -1)
    assert int(counts[:, 0].clamp(min=1).sum()) == int(f['num_total_pos'])
    assert int(counts[:, 1].clamp(min=1).sum()) == int(f['num_total_neg'])
    for l in range(5):
        assert np.array_equal(labels[l].cpu().numpy(), f['labels_%d' % l])
        assert np.array_equal(lw[l].cpu().numpy(), f['label_weights_%d' % l])
        assert np.array_equal(bw[l].cpu().numpy(), f['bbox_weights_%d' % l])
        assert np.allclose(bt[l].cpu().numpy(), f['bbox_targets_%d' % l], rtol=1e-5, atol=1e-6)
        inval = torch.from_numpy(f['valid_1_%d' % l] == 0).cuda()
        assert int(inval.sum()) > 0 and float(lw[l][1][inval].abs().sum()) == 0.0
    # the loss dict and the gradients of the head outputs, as the reference's autograd gives them
    cls, reg, iou = synth.head_outputs(int(f['seed']), B, ph, pw, str(f['kind']))
    assert synth.checksum(cls + reg + iou) == int(f['checksum'])
    head = IoUawareRetinaHead(**HEAD_KW).cuda()
    metas = [synth.img_meta(*s) for s in shapes]
    for channels_last in (False, True):
        c, r, i = [[t.contiguous(memory_format=torch.channels_last) if channels_last else t
                    for t in G.to_dev(x)] for x in (cls, reg, iou)]
        for t in c + r + i:
            t.requires_grad_(True)
        losses = head.loss(c, r, i, gts, gls, metas, TRAIN_CFG)
        for k in ('loss_cls', 'loss_bbox', 'losses_iou'):
            got = np.array([float(x) for x in losses[k]])
            assert np.all(np.abs(got - f[k]) <= 1e-4 * np.maximum(np.abs(f[k]), 1e-6)), (k, got, f[k])
        sum(sum(v) for v in losses.values()).backward()
        for l in range(5):
            for key, g in (('g_cls_%d' % l, c[l].grad), ('g_reg_%d' % l, r[l].grad),
                           ('g_iou_%d' % l, i[l].grad)):
                want = f[key].astype(np.float64)
                got = g.contiguous().cpu().numpy().reshape(-1)[f[key + '_idx']].astype(np.float64)
                assert np.abs(got - want).max() <= 2e-4 * max(np.abs(want).max(), 1e-30), key
                tot = float(g.double().sum())
                assert abs(tot - float(f[key + '_sum'])) <= 2e-4 * max(float(f[key + '_abs']), 1e-30)


@pytest.mark.parametrize('seed,pad', [(1, (800, 1344)), (2, (320, 416)), (3, (608, 1024))])
def test_device_targets_equal_torch_path(seed, pad):
    """full-size and odd-size batches, padded images (valid flags), many gts"""
    from iouaware import ops
    from iouaware.head import IoUawareRetinaHead
    from iouaware.targets import anchor_target
    from test_host_targets import HEAD_KW, TRAIN_CFG
    ph, pw = pad
    B = 3
    head = IoUawareRetinaHead(**HEAD_KW)
    sizes = synth.level_shapes(ph, pw)
    geom = head.geometry(sizes, -1)
    gts, gls = synth.train_targets(seed, B, ph - 40, pw - 70, max_gt=30)
    # image 0 narrower than the pad: part of the feature map is invalid
    metas = [synth.img_meta(ph - 40, pw - 70, ph - (32 if b == 0 else 0), pw - (64 if b == 0 else 0))
             for b in range(B)]
    gtb = [torch.from_numpy(x).cuda() for x in gts]
    gtl = [torch.from_numpy(x).cuda() for x in gls]
    anchors, flags = head.get_anchors(sizes, metas, device='cuda')
    ref = anchor_target(anchors, flags, gtb, metas, head.target_means, head.target_stds, TRAIN_CFG,
                        gt_labels_list=gtl, label_channels=80, sampling=False)
    labels, lw, bt, bw, counts = ops.anchor_targets(geom, gtb, gtl, [m['pad_shape'] for m in metas],
                                                    0.5, 0.4, 0.0, -1)
    assert int(counts[:, 0].clamp(min=1).sum()) == ref[4]
    assert int(counts[:, 1].clamp(min=1).sum()) == ref[5]
    for l in range(5):
        assert torch.equal(labels[l], ref[0][l].reshape(labels[l].shape))
        assert torch.equal(lw[l], ref[1][l].reshape(lw[l].shape))
        assert torch.equal(bw[l], ref[3][l].reshape(bw[l].shape))
        assert torch.allclose(bt[l], ref[2][l].reshape(bt[l].shape), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------ the assigner's edges
# The adversarial inputs of synth_targets.py (ties, IoUs exactly on a threshold, duplicate / tiny /
# outside gts, partly invalid maps, 1 / 257 / 512 gts, no labels, real means and stds) through
# ops.anchor_targets, against the plain numpy evaluation (assign_ref.py) and the reference's own
# results (tests/golden/targets_edge.npz, made on the CPU: first index on ties).  The torch route
# on the device is no yardstick here: `max` there may pick another index on ties.
import synth_targets  # noqa: E402

LEVEL_KEYS = ('labels', 'label_weights', 'bbox_targets', 'bbox_weights')


def _edge_geometry(c):
    from iouaware.head import IoUawareRetinaHead
    from test_host_targets import HEAD_KW
    head = IoUawareRetinaHead(**synth_targets.head_kw(c, HEAD_KW))
    geom = head.geometry(c['featmap_sizes'], -1)
    assert geom.N == c['anchors'].shape[0] and list(geom.level_anchors) == c['level_anchors']
    return geom


def _edge_device(c, geom, images):
    """ops.anchor_targets on the images `images` (indices into the case's batch) -> numpy"""
    from iouaware import ops
    gts = [torch.from_numpy(c['gts'][i]).cuda() for i in images]
    gls = None if c['labels'] is None else [torch.from_numpy(c['labels'][i]).cuda() for i in images]
    pads = [tuple(c['pads'][i]) + (3,) for i in images]
    out = ops.anchor_targets(geom, gts, gls, pads, c['pos_iou_thr'], c['neg_iou_thr'],
                             c['min_pos_iou'], c['pos_weight'])
    torch.cuda.synchronize()
    res = {k: [t.cpu().numpy() for t in out[i]] for i, k in enumerate(LEVEL_KEYS)}
    res['counts'] = out[4].cpu().numpy()
    return res


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('name', synth_targets.CASES)
def test_edge_cases_equal_assign_ref_and_reference(golden_dir, name):
    """labels, weights and counts exactly, the deltas to rtol 1e-5 / atol 1e-6 (another `logf`),
    exact zeros where the gt is the anchor; the by-value entry (B <= IA_MAX_TARGET_BATCH) and
    the padded entry (the images repeated to IA_MAX_TARGET_BATCH + 1) give the same bits, and so
    does a second call"""
    from iouaware import _lib
    c = synth_targets.case(name)
    geom = _edge_geometry(c)
    B, L = len(c['gts']), len(c['level_anchors'])
    ref = synth_targets.reference(c)
    f = np.load(os.path.join(golden_dir, 'targets_edge.npz'))
    p = name + '/'
    assert int(f[p + 'checksum']) == c['checksum']
    got = _edge_device(c, geom, list(range(B)))
    assert got['counts'].dtype == np.int32 and np.array_equal(got['counts'], ref['counts'])
    assert int(np.maximum(got['counts'][:, 0], 1).sum()) == int(f[p + 'num_total_pos'])
    assert int(np.maximum(got['counts'][:, 1], 1).sum()) == int(f[p + 'num_total_neg'])
    for l in range(L):
        for k in LEVEL_KEYS:
            for want in (ref[k][l], f[p + '%s_%d' % (k, l)]):
                if k == 'bbox_targets':
                    assert np.allclose(got[k][l], want, rtol=1e-5, atol=1e-6), (k, l)
                else:
                    assert got[k][l].dtype == want.dtype and np.array_equal(got[k][l], want), (k, l)
    if name == 'gt_is_anchor':
        row = int(np.nonzero((c['anchors'] == c['gts'][0][0]).all(1))[0][0])
        full = np.concatenate([got['bbox_targets'][l][0] for l in range(L)])
        lab = np.concatenate([got['labels'][l][0] for l in range(L)])
        assert lab[row] == c['labels'][0][0] and (full[row] == 0).all()
    again = _edge_device(c, geom, list(range(B)))
    n_big = _lib.IA_MAX_TARGET_BATCH + 1
    assert B <= _lib.IA_MAX_TARGET_BATCH
    images = [i % B for i in range(n_big)]
    big = _edge_device(c, geom, images)
    assert _same_bits(again['counts'], got['counts'])
    assert _same_bits(big['counts'], got['counts'][images])
    for l in range(L):
        for k in LEVEL_KEYS:
            assert _same_bits(again[k][l], got[k][l]), ('second call', k, l)
            assert _same_bits(big[k][l], got[k][l][images]), ('padded entry', k, l)


def _routing_inputs():
    """513 gts = one 1 x 1 box in front of 512 whose last is a copy of it: the copy claims every
    anchor the first one would (step 4, later wins) and no IoU reaches 0.5, so the first box
    claims nothing and the 512 without it give the same targets"""
    import assign_ref
    boxes, labels = synth_targets.lattice(511)
    t = np.array([[77., 33., 77., 33.]], np.float32)
    g512, l512 = np.concatenate([boxes, t]), np.concatenate([labels, [9]]).astype(np.int64)
    g513, l513 = np.concatenate([t, g512]), np.concatenate([[70], l512]).astype(np.int64)
    anchors, level_anchors, sizes, A = assign_ref.pyramid(synth_targets.TENSOR)
    valid = assign_ref.pyramid_valid(sizes, synth_targets.STRIDES, A, synth_targets.TENSOR)
    r512 = assign_ref.assign_image(anchors, valid, g512, l512)
    r513 = assign_ref.assign_image(anchors, valid, g513, l513)
    assert g512.shape[0] == 512 and g513.shape[0] == 513 and (r513['gt_inds'] == 1).sum() == 0
    assert r513['overlaps'].max() < 0.5 and (r513['gt_inds'] == 513).sum() >= 2
    for k in LEVEL_KEYS:
        assert np.array_equal(r512[k], r513[k])
    return (g512, l512), (g513, l513)


def test_head_loss_routes_by_gt_count(monkeypatch):
    """_device_targets_ok: up to 512 gts per image the device assigner runs, with 513 the torch
    route (targets.py) does and the call goes through; the 513th box claims nothing, so both
    calls give the same loss_cls / loss_bbox (1e-4 relative, the bound of the mixed-pad test).
    An image without gts sends the batch to the torch route, whose assigner raises 'No gt or
    bboxes' as the reference's does -- pinned as it is."""
    from iouaware import ops
    from iouaware.head import IoUawareRetinaHead
    from test_host_targets import HEAD_KW, TRAIN_CFG
    (g512, l512), (g513, l513) = _routing_inputs()
    ph, pw = synth_targets.TENSOR
    B = 2
    cls, reg, iou = synth.head_outputs(7, B, ph, pw, 'A')
    c, r, i = G.to_dev(cls), G.to_dev(reg), G.to_dev(iou)
    head = IoUawareRetinaHead(**HEAD_KW).cuda()
    metas = [synth.img_meta(ph, pw, ph, pw) for _ in range(B)]
    small_g, small_l = synth_targets.NORMAL, synth_targets.NORMAL_L
    calls = []
    real = ops.anchor_targets

    def spy(*a, **k):
        calls.append(max(int(g.shape[0]) for g in a[1]))
        return real(*a, **k)

    monkeypatch.setattr(ops, 'anchor_targets', spy)
    losses = {}
    for key, (g, l) in (('512', (g512, l512)), ('513', (g513, l513))):
        gts = [torch.from_numpy(small_g).cuda(), torch.from_numpy(g).cuda()]
        gls = [torch.from_numpy(small_l).cuda(), torch.from_numpy(l).cuda()]
        n = len(calls)
        out = head.loss(c, r, i, gts, gls, metas, TRAIN_CFG)
        assert len(calls) - n == (1 if key == '512' else 0), key
        losses[key] = {k: np.array([float(x) for x in out[k]]) for k in ('loss_cls', 'loss_bbox')}
    assert calls == [512]
    for k in ('loss_cls', 'loss_bbox'):
        a, b = losses['512'][k], losses['513'][k]
        assert np.all(np.isfinite(a)) and a.sum() > 0
        assert np.all(np.abs(a - b) <= 1e-4 * np.maximum(np.abs(b), 1e-6)), (k, a, b)
    gts = [torch.from_numpy(small_g).cuda(), torch.zeros((0, 4), device='cuda')]
    gls = [torch.from_numpy(small_l).cuda(), torch.zeros((0,), dtype=torch.int64, device='cuda')]
    assert not head._device_targets_ok(TRAIN_CFG, gts, None, torch.device('cuda'))
    with pytest.raises(ValueError, match='No gt or bboxes'):
        head.loss(c, r, i, gts, gls, metas, TRAIN_CFG)
    assert calls == [512]
