"""-m gpu: the SSD decode (csrc/ssddecode.hip) -- stages 1 and 3 against the existing softmax path
bit for bit, the whole entry against tests/ssd_ref.py on the recorded cases, the compaction at its
edges, the capacity of the batched NMS (exactly IA_MAX_CANDIDATES kept rows, one more), guards and
run-to-run bits."""
import numpy as np
import pytest
import torch

import ssd_ref

pytestmark = pytest.mark.gpu

CAP = 8192
# compaction edges: 560 rows in three 256-row workgroups, 4 / 6 / 6 / 6 / 4 / 4 anchors
EDGE_SIZES = [(9, 9), (5, 5), (3, 3), (2, 2), (1, 1), (1, 1)]
EDGE_NC = 6                                   # 5 foreground classes


def _head(nc):
    from iouaware.ssd_head import SSDHead
    return SSDHead(num_classes=nc, **ssd_ref.CASE_HEAD)


def _dev(arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _metas(case):
    return [m['img_shape'] for m in case['metas']], [m['scale_factor'] for m in case['metas']]


@pytest.fixture(scope='module')
def recorded():
    """the recorded cases once: head outputs, ssd_ref's detections per rescale setting"""
    out = {}
    for name, case in ssd_ref.CASES.items():
        cls, reg = ssd_ref.head_outputs(name)
        tc, tr = [torch.from_numpy(c) for c in cls], [torch.from_numpy(r) for r in reg]
        ref = {rs: ssd_ref.get_bboxes(tc, tr, case['metas'], rs, num_classes=case['num_classes'])
               for rs in case['rescale']}
        out[name] = dict(cls=cls, reg=reg, ref=ref)
    return out


def _same_detections(got, want, tol=1e-4):
    """got: (dets, labels, rows, num) device tensors; want: ssd_ref's per-image list"""
    dets, labels, rows, num = [t.cpu().numpy() for t in got]
    assert num.tolist() == [len(w[0]) for w in want]
    for b, (wd, wl, wi) in enumerate(want):
        n = int(num[b])
        d, l, i = ssd_ref.canonical(dets[b, :n], labels[b, :n].astype(np.int64), rows[b, :n].astype(np.int64))
        wd, wl, wi = ssd_ref.canonical(wd, wl, wi)
        assert np.array_equal(i, wi) and np.array_equal(l, wl), b
        # this build's detection contract (gpu_util.close): tol, relative for values above 1
        err = float((np.abs(d.astype(np.float64) - wd) / np.maximum(1.0, np.abs(wd))).max()) if n else 0.0
        print('image %d: %d detections, largest difference %.2e (relative above 1)' % (b, n, err))
        assert err <= tol


# ------------------------------------------------------------------ stages 1 and 3 against the existing path
@pytest.mark.parametrize('name', ['ssd300', 'small'])
def test_stages_equal_the_softmax_path_bit_for_bit(recorded, name):
    from iouaware import ops, ssd_ops
    case = ssd_ref.CASES[name]
    nc = case['num_classes']
    head = _head(nc)
    geom = head.geometry(case['sizes'])
    cls, reg = _dev(recorded[name]['cls']), _dev(recorded[name]['reg'])
    shapes, factors = _metas(case)
    B = cls[0].shape[0]
    best = ssd_ops.ssd_rowscore(geom, cls, reg)
    all_rows = torch.arange(geom.R, dtype=torch.int32, device='cuda').repeat(B, 1).contiguous()
    count = torch.full((B,), geom.R, dtype=torch.int32, device='cuda')
    for rescale in (False, True):
        boxes, scores_t, bs = ssd_ops.ssd_gather_decode(geom, cls, reg, all_rows, count, geom.R, shapes, factors,
                                                        rescale)
        assert torch.equal(bs.view(torch.int32), best.view(torch.int32))
        for l in range(geom.L):
            A, (h, w) = geom.A[l], geom.featmap_sizes[l]
            n, off = h * w * A, geom.level_off[l]
            one = ops.HeadGeometry([(h, w)], [geom.strides[l]], head.anchor_generators[l].base_anchors.numpy()[None],
                                   nc - 1, nms_pre=-1, means=head.target_means, stds=head.target_stds, softmax=True,
                                   iou_branch=False)
            rm = ops.decode_fuse_rowmax(one, [cls[l]], [reg[l]], None)          # (B, A, HW) anchor-major
            rm = rm.view(B, A, h * w).permute(0, 2, 1).reshape(B, n)
            assert torch.equal(rm.view(torch.int32), best[:, off:off + n].view(torch.int32)), l
            cand = torch.arange(n, dtype=torch.int32, device='cuda').repeat(B, 1).contiguous()
            bx, st, be = ops.gather_decode(one, [cls[l]], [reg[l]], None, cand, shapes, factors, rescale)
            assert torch.equal(bx.view(torch.int32), boxes[:, off:off + n].view(torch.int32)), l
            assert torch.equal(st[:, :, :n].view(torch.int32), scores_t[:, :, off:off + n].view(torch.int32)), l
            assert torch.equal(be.view(torch.int32), bs[:, off:off + n].view(torch.int32)), l


# ------------------------------------------------------------------ whole entry on the recorded cases
@pytest.mark.parametrize('name,rescale', [('ssd300', False), ('small', False), ('small', True)])
def test_whole_entry_equals_ssd_ref_on_the_recorded_cases(recorded, name, rescale):
    from iouaware import ssd_ops
    case = ssd_ref.CASES[name]
    head = _head(case['num_classes'])
    geom = head.geometry(case['sizes'])
    cls, reg = _dev(recorded[name]['cls']), _dev(recorded[name]['reg'])
    shapes, factors = _metas(case)
    out = ssd_ops.ssd_get_bboxes(geom, cls, reg, shapes, factors, rescale, ssd_ref.SCORE_THR, ssd_ref.IOU_THR,
                                 ssd_ref.MAX_PER_IMG, debug=True)
    assert out[4].tolist() == [0] * len(shapes)
    kept = out[5]['kept_count'].tolist()
    assert all(10 <= k <= CAP for k in kept), kept
    _same_detections(out[:4], recorded[name]['ref'][rescale])
    # the head's own entry points give the same
    from iouaware.config import ConfigDict
    cfg = ConfigDict(dict(nms=dict(type='nms', iou_thr=ssd_ref.IOU_THR), min_bbox_size=0,
                          score_thr=ssd_ref.SCORE_THR, max_per_img=ssd_ref.MAX_PER_IMG))
    res = head.get_bboxes(cls, reg, None, None, case['metas'], cfg, rescale)
    for b, (d, l) in enumerate(res):
        n = int(out[3][b])
        assert l.dtype == torch.int64 and torch.equal(d, out[0][b, :n]) and torch.equal(l, out[1][b, :n].long())


# ------------------------------------------------------------------ compaction edges
def _edge_logits(masks):
    """masks (B, R) bool -> cls[l] (B, A_l * nc, H, W): background logit +12 (best foreground score
    about 6e-6), lowered to -2 on the chosen rows, whose class 1 + row % 5 is lifted (best score above 0.3)"""
    B, R = masks.shape
    logits = np.zeros((B, R, EDGE_NC), np.float32)
    logits[:, :, 0] = np.where(masks, -2.0, 12.0)
    # no two chosen rows with the same score in a class (the NMS order is then a property of the inputs)
    r = np.arange(R)
    lift = np.zeros((R, EDGE_NC), np.float32)
    lift[r, 1 + r % (EDGE_NC - 1)] = 1.0 + 1e-3 * r
    logits += np.where(masks[:, :, None], lift[None], np.float32(0))
    A = ssd_ref.num_anchors(ssd_ref.CASE_HEAD['anchor_ratios'])
    cls, reg, off = [], [], 0
    for (h, w), a in zip(EDGE_SIZES, A):
        n = h * w * a
        cls.append(np.ascontiguousarray(logits[:, off:off + n].reshape(B, h, w, a * EDGE_NC).transpose(0, 3, 1, 2)))
        reg.append(np.zeros((B, a * 4, h, w), np.float32))
        off += n
    assert off == R
    return cls, reg


def _edge_masks():
    R = 560
    rng = np.random.RandomState(77)
    cases = {}
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        m = np.zeros((2, R), bool)
        m[0, :n] = True                                         # the first n rows: runs across wave / workgroup ends
        m[1, rng.choice(R, n, replace=False)] = True            # n rows anywhere
        cases['count_%d' % n] = m
    m = np.zeros((1, R), bool)
    m[0, [323, 324]] = True                                     # last row of the 4-anchor level, first of the 6-anchor one
    cases['level_boundary'] = m
    m = np.zeros((1, R), bool)
    m[0, 556:] = True                                           # only the last 1 x 1 level
    cases['last_level_only'] = m
    m = np.zeros((3, R), bool)
    m[0, rng.choice(R, 7, replace=False)] = True
    m[2, rng.choice(R, 130, replace=False)] = True              # image 1 keeps nothing
    cases['batch_3'] = m
    m = np.ones((1, R), bool)
    cases['all_rows'] = m
    return cases


@pytest.mark.parametrize('which', sorted(_edge_masks()))
def test_compaction_edges(which):
    from iouaware import ssd_ops
    masks = _edge_masks()[which]
    B, R = masks.shape
    head = _head(EDGE_NC)
    geom = head.geometry(EDGE_SIZES)
    assert geom.R == R and geom.level_off[1] == 324 and geom.level_off[5] == 556
    cls, reg = _edge_logits(masks)
    best = ssd_ops.ssd_rowscore(geom, _dev(cls), _dev(reg))
    assert torch.equal(best.cpu() > ssd_ref.SCORE_THR, torch.from_numpy(masks))
    # outputs pre-filled with a sentinel that the kernels never write (their own fill behind the count is
    # -1), with guards
    G, SENTINEL = 1024, 0x5A5A5A5A
    bufs = [torch.full((n + 2 * G,), SENTINEL, dtype=torch.int32, device='cuda') for n in (B * CAP, B, B)]
    outs = (bufs[0][G:G + B * CAP].view(B, CAP), bufs[1][G:G + B], bufs[2][G:G + B])
    kept_rows, kept_count, overflow = ssd_ops.ssd_compact(best, ssd_ref.SCORE_THR, out=outs)
    torch.cuda.synchronize()
    for buf in bufs:
        assert bool((buf[:G] == SENTINEL).all()) and bool((buf[-G:] == SENTINEL).all())
    assert kept_count.tolist() == masks.sum(1).tolist() and overflow.tolist() == [0] * B
    for b in range(B):
        want = torch.nonzero(torch.from_numpy(masks[b])).flatten().to(torch.int32)
        n = want.numel()
        assert torch.equal(kept_rows[b, :n].cpu(), want)
        assert bool((kept_rows[b, n:] == -1).all())
    again = ssd_ops.ssd_compact(best, ssd_ref.SCORE_THR)
    assert all(torch.equal(a, b) for a, b in zip(again, (kept_rows, kept_count, overflow)))
    # the whole entry on the same maps
    shapes, factors = [(300, 300, 3)] * B, [1.0] * B
    out = ssd_ops.ssd_get_bboxes(geom, _dev(cls), _dev(reg), shapes, factors, False, ssd_ref.SCORE_THR,
                                 ssd_ref.IOU_THR, ssd_ref.MAX_PER_IMG)
    ref = ssd_ref.get_bboxes([torch.from_numpy(c) for c in cls], [torch.from_numpy(r) for r in reg],
                             [dict(img_shape=s, scale_factor=1.0) for s in shapes], False, num_classes=EDGE_NC)
    assert out[4].tolist() == [0] * B
    _same_detections(out[:4], ref)
    for b in range(B):
        assert (len(ref[b][0]) == 0) == (not masks[b].any())


# ------------------------------------------------------------------ capacity
def _capacity_inputs(n_keep):
    """SSD300 geometry, 5 classes, one image: n_keep rows (drawn over all levels) with the background
    lowered, random foreground logits and small random deltas"""
    rng = np.random.RandomState(4000 + n_keep)
    R = 8732
    logits = rng.randn(1, R, EDGE_NC).astype(np.float32)
    mask = np.zeros(R, bool)
    mask[rng.choice(R, n_keep, replace=False)] = True
    logits[0, :, 0] = np.where(mask, -2.0, 14.0)
    deltas = (rng.randn(1, R, 4) * 0.5).astype(np.float32)
    A = ssd_ref.num_anchors(ssd_ref.CASE_HEAD['anchor_ratios'])
    cls, reg, off = [], [], 0
    for (h, w), a in zip(ssd_ref.SSD300_SIZES, A):
        n = h * w * a
        cls.append(np.ascontiguousarray(logits[:, off:off + n].reshape(1, h, w, a * EDGE_NC).transpose(0, 3, 1, 2)))
        reg.append(np.ascontiguousarray(deltas[:, off:off + n].reshape(1, h, w, a * 4).transpose(0, 3, 1, 2)))
        off += n
    return cls, reg, mask


@pytest.mark.parametrize('n_keep', [CAP, CAP + 1])
def test_capacity(n_keep):
    from iouaware import ssd_ops
    from iouaware.config import ConfigDict
    head = _head(EDGE_NC)
    geom = head.geometry(ssd_ref.SSD300_SIZES)
    assert geom.R == 8732 and geom.Rk == CAP
    cls, reg, mask = _capacity_inputs(n_keep)
    metas = [dict(img_shape=(300, 300, 3), scale_factor=1.0)]
    ref = ssd_ref.get_bboxes([torch.from_numpy(c) for c in cls], [torch.from_numpy(r) for r in reg], metas, False,
                             num_classes=EDGE_NC)
    assert len(ref[0][0]) == ssd_ref.MAX_PER_IMG
    dc, dr = _dev(cls), _dev(reg)
    out = ssd_ops.ssd_get_bboxes(geom, dc, dr, [(300, 300, 3)], [1.0], False, ssd_ref.SCORE_THR, ssd_ref.IOU_THR,
                                 ssd_ref.MAX_PER_IMG, debug=True)
    assert out[5]['kept_count'].tolist() == [n_keep]
    cfg = ConfigDict(dict(nms=dict(type='nms', iou_thr=ssd_ref.IOU_THR), min_bbox_size=0,
                          score_thr=ssd_ref.SCORE_THR, max_per_img=ssd_ref.MAX_PER_IMG))
    if n_keep <= CAP:
        assert out[4].tolist() == [0]
        assert torch.equal(out[5]['kept_rows'][0].cpu(), torch.from_numpy(np.nonzero(mask)[0].astype(np.int32)))
        _same_detections(out[:4], ref)
        got = head.get_bboxes_batched(dc, dr, metas, cfg)
        assert head.overflow.tolist() == [0] and torch.equal(got[3], out[3])
    else:
        assert out[4].tolist() == [1] and out[3].tolist() == [0]         # flagged, never truncated
        got = head.get_bboxes_batched(dc, dr, metas, cfg, check_overflow=True)
        assert head.overflow.tolist() == [1]
        _same_detections(got, ref)
        left = head.get_bboxes_batched(dc, dr, metas, cfg, check_overflow=False)
        assert head.overflow.tolist() == [1] and left[3].tolist() == [0]


# ------------------------------------------------------------------ guards, run-to-run bits
def _guarded(nbytes, G=4096):
    buf = torch.full((nbytes + 2 * G,), 0xFF, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 256 == 0
    return buf, buf[G:G + nbytes]


def _guard_case(which, recorded):
    """-> (geometry, cls, reg on the device, img shapes, scale factors, rescale, ssd_ref's detections)"""
    if which == 'small':                          # the recorded case: R = 192 = Rs
        case = ssd_ref.CASES['small']
        geom = _head(case['num_classes']).geometry(case['sizes'])
        shapes, factors = _metas(case)
        return (geom, _dev(recorded['small']['cls']), _dev(recorded['small']['reg']), shapes, factors, True,
                recorded['small']['ref'][True])
    # the 560-row edge geometry: R % 64 = 48, so scores_t and keep_rows carry 16 padding columns per
    # class that no stage writes -- they hold the 0xFF pre-fill (NaN as floats) during the NMS
    masks = _edge_masks()['batch_3']
    cls, reg = _edge_logits(masks)
    shapes, factors = [(300, 300, 3)] * 3, [1.0] * 3
    ref = ssd_ref.get_bboxes([torch.from_numpy(c) for c in cls], [torch.from_numpy(r) for r in reg],
                             [dict(img_shape=s, scale_factor=1.0) for s in shapes], False, num_classes=EDGE_NC)
    geom = _head(EDGE_NC).geometry(EDGE_SIZES)
    assert geom.Rk == 560 and geom.Rs == 576
    return geom, _dev(cls), _dev(reg), shapes, factors, False, ref


@pytest.mark.parametrize('which', ['small', 'edge560'])
def test_guards_and_same_bits_in_two_runs(recorded, which):
    from iouaware import _lib, ssd_ops
    geom, cls, reg, shapes, factors, rescale, ref = _guard_case(which, recorded)
    B, M = len(shapes), ssd_ref.MAX_PER_IMG
    nbytes = _lib.lib().ia_ssd_get_bboxes_workspace_bytes(geom.ref(), B)
    runs = []
    for _ in range(2):
        wbuf, ws = _guarded(nbytes)
        sizes = (B * M * 5 * 4, B * M * 4, B * M * 4, B * 4, B * 4)
        pairs = [_guarded(n) for n in sizes]
        views = (pairs[0][1].view(torch.float32).view(B, M, 5), pairs[1][1].view(torch.int32).view(B, M),
                 pairs[2][1].view(torch.int32).view(B, M), pairs[3][1].view(torch.int32),
                 pairs[4][1].view(torch.int32))
        out = ssd_ops.ssd_get_bboxes(geom, cls, reg, shapes, factors, rescale, ssd_ref.SCORE_THR, ssd_ref.IOU_THR, M,
                                     debug=True, workspace=ws, outputs=views)
        torch.cuda.synchronize()
        for buf, view in [(wbuf, ws)] + pairs:
            G = (buf.numel() - view.numel()) // 2
            assert bool((buf[:G] == 0xFF).all()) and bool((buf[-G:] == 0xFF).all())
        num = out[3].tolist()
        rec = [out[3].cpu(), out[4].cpu()]
        for b, n in enumerate(num):
            rec += [out[0][b, :n].cpu().view(torch.int32), out[1][b, :n].cpu(), out[2][b, :n].cpu()]
        v = out[5]
        kc = v['kept_count'].tolist()
        rec += [v['rowscore'].cpu().view(torch.int32), v['kept_rows'].cpu(), v['kept_count'].cpu()]
        for b, n in enumerate(kc):
            rec += [v['boxes'][b, :n].cpu().view(torch.int32), v['scores_t'][b, :, :n].cpu().view(torch.int32),
                    v['best_score'][b, :n].cpu().view(torch.int32)]
        runs.append(rec)
    _same_detections(out[:4], ref)
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs))


def test_bad_arguments_are_refused():
    from iouaware import _lib, ssd_ops
    geom = _head(EDGE_NC).geometry(EDGE_SIZES)
    cls, reg = _edge_logits(np.zeros((1, 560), bool))
    with pytest.raises(ValueError, match='threshold'):
        ssd_ops.ssd_get_bboxes(geom, _dev(cls), _dev(reg), [(300, 300, 3)], [1.0], False, -0.1, 0.45, 200)
    with pytest.raises(_lib.IouAwareLibraryError, match='max_per_img'):
        ssd_ops.ssd_get_bboxes(geom, _dev(cls), _dev(reg), [(300, 300, 3)], [1.0], False, 0.02, 0.45, 5000)
