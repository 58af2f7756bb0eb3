"""GPU: the guided-anchor decode (csrc/guideddecode.hip) and IoUawareGARetinaHead on the HIP
masked convolution, against the reference's recorded results (tests/golden/ga_get_bboxes.npz,
ga_forward.npz) and the plain-torch definition tests/ga_ref.py.  TOL as in
tests/test_gpu_fcos_plain.py: identical kept-location ids and labels, boxes and scores within 1e-4
of max(1, |value|) (the device's exp / sigmoid are the library's own restatements, not torch's)."""
import json
import os

import numpy as np
import pytest
import torch

import ga_ref
import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
DEV = torch.device('cuda:0')
TOL = 1e-4


def _head(**kw):
    from iouaware.ga_head import IoUawareGARetinaHead
    args = dict(ga_ref.FWD_HEAD, in_channels=256, feat_channels=256, anchor_strides=[8, 16, 32, 64, 128])
    args.update(kw)
    return IoUawareGARetinaHead(**args).eval()


def _dev(maps):
    return [[torch.from_numpy(np.ascontiguousarray(m)).to(DEV) for m in kind] for kind in maps]


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool((np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b))).all())


def _ids(geom, views, rows, b, k):
    """candidate rows of image b's k detections -> location ids (level offset + position)"""
    cand = views['cand_idx'][b].cpu().numpy().astype(np.int64)
    off = np.concatenate([[0], np.cumsum(geom.level_points)])
    coff = np.concatenate([[0], np.cumsum(geom.level_cands)])
    r = rows[b, :k].cpu().numpy().astype(np.int64)
    lvl = np.searchsorted(coff, r, side='right') - 1
    return off[lvl] + cand[r]


def _run_case(k, use_loc_filter=True, maps=None):
    from iouaware import ga_ops
    case = ga_ref.GA_CASES[k]
    B, ph, pw, nms_pre, max_per_img, rescale = case[1], case[2], case[3], case[4], case[5], case[6]
    maps = ga_ref.ga_head_outputs(k) if maps is None else maps
    metas = ga_ref.case_metas(k)
    head = _head()
    geom = head.geometry(synth.level_shapes(ph, pw), nms_pre, use_loc_filter)
    dets, labels, rows, num, views = ga_ops.guided_get_bboxes(
        geom, *_dev(maps), [m['img_shape'] for m in metas], [m['scale_factor'] for m in metas], rescale, 0.05, 0.5,
        max_per_img, debug=True)
    torch.cuda.synchronize()
    out = []
    for b, n in enumerate(num.tolist()):
        out.append((dets[b, :n].cpu().numpy(), labels[b, :n].cpu().numpy().astype(np.int64), _ids(geom, views, rows, b, n)))
    return out, maps, metas, case


def _same_detections(got, want):
    d, l, i = ga_ref.canonical(*got)
    rd, rl, ri = ga_ref.canonical(*want)
    assert len(l) == len(rl), (len(l), len(rl))
    assert np.array_equal(l, rl) and np.array_equal(i, ri)
    assert _close(d, rd), float(np.abs(d - rd).max())


@pytest.mark.parametrize('k', range(len(ga_ref.GA_CASES)))
def test_guided_get_bboxes_against_the_reference(k):
    g = np.load(os.path.join(GOLD, 'ga_get_bboxes.npz'))
    out = _run_case(k)[0]
    for b, got in enumerate(out):
        _same_detections(got, (g['dets_%d_%d' % (k, b)], g['labels_%d_%d' % (k, b)], g['ids_%d_%d' % (k, b)]))


def test_head_get_bboxes_is_that_path():
    """the head's get_bboxes (reference signature, per-image lists) on case 1"""
    from iouaware.config import ConfigDict
    g = np.load(os.path.join(GOLD, 'ga_get_bboxes.npz'))
    case = ga_ref.GA_CASES[1]
    cfg = ConfigDict(nms_pre=case[4], min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_thr=0.5),
                     max_per_img=case[5])
    res = _head().get_bboxes(*_dev(ga_ref.ga_head_outputs(1)), None, None, ga_ref.case_metas(1), cfg, case[6])
    for b, (d, l) in enumerate(res):
        assert l.dtype == torch.long and d.shape == (len(g['labels_1_%d' % b]), 5)
        assert sorted(l.tolist()) == sorted(g['labels_1_%d' % b].tolist())
        assert _close(np.sort(d[:, 4].cpu().numpy()), np.sort(g['dets_1_%d' % b][:, 4]))


def test_without_the_location_filter():
    """use_loc_filter = 0 (the reference in training mode): every location is a candidate"""
    k = 1
    out, maps, metas, case = _run_case(k, use_loc_filter=False)
    want = ga_ref.get_bboxes(maps, metas, case[6], case[4], 0.05, 0.5, case[5], use_loc_filter=False)
    filtered = ga_ref.get_bboxes(maps, metas, case[6], case[4], 0.05, 0.5, case[5])
    for b in range(case[1]):
        _same_detections(out[b], want[b])
    assert any(not np.array_equal(np.sort(want[b][2]), np.sort(filtered[b][2])) for b in range(case[1]))


def test_image_without_a_kept_location():
    """image 1 keeps nothing on any level: zero detections; image 0 is what it is alone"""
    maps = ga_ref.ga_head_outputs(1)
    for lo in maps[4]:
        lo[1] = np.float32(-20.0)
    out, _, metas, case = _run_case(1, maps=maps)
    assert len(out[1][1]) == 0
    g = np.load(os.path.join(GOLD, 'ga_get_bboxes.npz'))
    _same_detections(out[0], (g['dets_1_0'], g['labels_1_0'], g['ids_1_0']))


def _big_level():
    """one level of 104 x 128 = 13312 locations (above the top-k's dense limit: the filtered
    selection), nms_pre 1000, about 1 % kept: a row-max array of mostly zeros"""
    rs = np.random.RandomState(31)
    h, w = 104, 128
    maps = [(rs.standard_normal((1, 80, h, w)) * 2 - 5).astype(np.float32),
            (rs.standard_normal((1, 4, h, w)) * 0.5).astype(np.float32),
            (rs.standard_normal((1, 1, h, w)) * 1.5).astype(np.float32),
            (rs.standard_normal((1, 2, h, w)) * 2.5).astype(np.float32),
            (rs.standard_normal((1, 1, h, w)) * 1.0 - 6.9).astype(np.float32)]
    return [[m] for m in maps], (h, w)


@pytest.mark.parametrize('which', ['case0', 'case1', 'big'])
def test_stage_entries_against_ga_ref(which):
    """ia_guided_rowmax: the kept locations' row maxima, +0.0f to the bit elsewhere; ia_select_topk on
    it: the kept locations by (score descending, index ascending), then -- where fewer are kept than
    the level's quota -- the lowest filtered-out indices; ia_guided_gather_decode: boxes and scores of
    the kept candidates, zeros for the filtered-out ones"""
    from iouaware import ga_ops, ops
    if which == 'big':
        maps, (h, w) = _big_level()
        sizes, strides, nms_pre, B = [(h, w)], [8], 1000, 1
        metas = [dict(img_shape=(h * 8 - 5, w * 8 - 3, 3), scale_factor=1.0)]
        head = _head(anchor_strides=[8])
    else:
        k = int(which[-1])
        case = ga_ref.GA_CASES[k]
        maps, metas = ga_ref.ga_head_outputs(k), ga_ref.case_metas(k)
        sizes, strides, nms_pre, B = synth.level_shapes(case[2], case[3]), list(synth.STRIDES), case[4], case[1]
        head = _head()
    geom = head.geometry(sizes, nms_pre)
    dm = _dev(maps)
    rowmax = ga_ops.guided_rowmax(geom, *dm)
    cand = ops.select_topk(geom.head, rowmax)
    boxes, scores_t, best = ga_ops.guided_gather_decode(geom, *dm, cand, [m['img_shape'] for m in metas],
                                                        [m['scale_factor'] for m in metas], False)
    torch.cuda.synchronize()
    rowmax, cand = rowmax.cpu().numpy(), cand.cpu().numpy()
    boxes, scores_t, best = boxes.cpu().numpy(), scores_t.cpu().numpy(), best.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(geom.level_points)])
    coff = np.concatenate([[0], np.cumsum(geom.level_cands)])
    for b in range(B):
        per = [[torch.from_numpy(m[b]) for m in kind] for kind in maps]
        rb, rs_, ri, _ = ga_ref.candidates_single(*per, metas[b]['img_shape'], nms_pre, strides=strides)
        rb, rs_, ri = rb.numpy(), rs_.numpy(), ri.numpy()
        for l in range(len(sizes)):
            keep = ga_ref.keep_mask(per[4][l]).numpy()
            n = len(keep)
            rm = rowmax[b, off[l]:off[l + 1]]
            sc = (per[0][l].reshape(80, -1).sigmoid() * per[2][l].reshape(1, -1).sigmoid()).max(0)[0].numpy()
            assert bool((rm[~keep].view(np.uint32) == 0).all())                  # +0.0f
            assert _close(rm[keep], sc[keep])
            c = cand[b, coff[l]:coff[l + 1]].astype(np.int64)
            assert len(np.unique(c)) == len(c) and c.min() >= 0 and c.max() < n
            ck = c[keep[c]]
            want = ri[(ri >= off[l]) & (ri < off[l + 1])] - off[l]               # the reference's candidates
            assert np.array_equal(np.sort(ck), np.sort(want))
            if 0 < nms_pre < n:
                assert bool(np.all(np.diff(rm[c]) <= 0))                         # descending score
                rest = c[~keep[c]]
                if len(rest):                                                    # the quota is filled with the
                    assert len(ck) == keep.sum()                                 # lowest filtered-out indices
                    assert np.array_equal(rest, np.nonzero(~keep)[0][:len(rest)])
                    assert np.array_equal(c[len(ck):], rest)
            else:
                assert np.array_equal(c, np.arange(n))                           # natural order, no top-k
            rows = np.arange(coff[l], coff[l + 1])
            dead = rows[~keep[c]]
            assert bool((boxes[b, dead].view(np.uint32) == 0).all()) and bool((best[b, dead].view(np.uint32) == 0).all())
            assert bool((scores_t[b][:, dead].view(np.uint32) == 0).all())
            live = rows[keep[c]]
            pos = {int(i): j for j, i in enumerate(ri)}
            j = np.array([pos[int(off[l] + p)] for p in c[keep[c]]], np.int64)
            if len(j):
                assert _close(boxes[b, live], rb[j]), float(np.abs(boxes[b, live] - rb[j]).max())
                assert _close(scores_t[b][:, live].T, rs_[j])
                assert _close(best[b, live], rs_[j].max(1))


def test_head_forward_against_the_reference():
    """the eval forward of the small head of ga_forward.npz (name-seeded weights, batch 1) under the
    map gates of tests/test_gpu_masked_conv.py, per map and level as max|got - ref| / max|ref| against
    the fp64 forward of the reference head (the same tensors converted, recorded by the generator):
        gate A  <= 1e-4, and
        gate B  <= 4 x the same figure of the reference head's own fp32 forward on the CPU (the
                recorded fp32 maps: one evaluation; after five to six layers its error is a sum of
                many roundings, 3e-07 .. 1.3e-06 here, not the luck of one short sum)
    and exactly +0.0f where the mask is false.  At batch 2 -- this build's per-image masks -- each
    image's maps are what the image gives alone: gate A between the two (the towers are library
    convolutions, whose bits may depend on the batch) and the same zero pattern."""
    import dcn_ref as R
    from iouaware.ga_head import IoUawareGARetinaHead
    g = np.load(os.path.join(GOLD, 'ga_forward.npz'))
    head = IoUawareGARetinaHead(**ga_ref.FWD_HEAD).eval()
    head.load_state_dict(ga_ref.fill_head_state(head.state_dict(), ga_ref.FWD['seed']))
    head = head.to(DEV)
    feats = [torch.from_numpy(f).to(DEV) for f in ga_ref.forward_features()]
    with torch.no_grad():
        outs = head(feats)
        other = [torch.flip(f, dims=(2, 3)).contiguous() for f in feats]
        both = head([torch.cat((f, o)) for f, o in zip(feats, other)])
        alone = head(other)
    torch.cuda.synchronize()
    assert len(outs) == 5
    for l in range(len(feats)):
        mask = torch.from_numpy(g['loc_pred_%d' % l]).sigmoid()[:, 0] >= 0.01
        assert 0 < int(mask.sum()) < mask.numel()
        for name, o in zip(ga_ref.FWD_MAPS, outs):
            x = o[l].cpu()
            y32, y64 = torch.from_numpy(g['%s_%d' % (name, l)]), torch.from_numpy(g['%s_%d_f64' % (name, l)])
            assert x.shape == y64.shape, name
            e, h = R.rel_err(x, y64), R.rel_err(y32, y64)
            print('  level %d %-10s %.2e (%.2f x the fp32 figure %.2e)' % (l, name, e, e / h, h))
            assert h > 0
            assert e <= R.GATE_A, 'gate A: %s level %d %.3e' % (name, l, e)
            assert e <= R.GATE_B * h, 'gate B: %s level %d HIP %.3e vs fp32 %.3e = %.2f x' % (name, l, e, h, e / h)
            if name in ('cls_score', 'bbox_pred', 'iou_pred'):
                zero = x.permute(0, 2, 3, 1)[~mask]
                assert bool((zero.contiguous().view(torch.int32) == 0).all()), name
        for o2, o1, oa in zip(both, outs, alone):
            for part, one in ((o2[l][:1], o1[l]), (o2[l][1:], oa[l])):
                assert R.rel_err(part, one) <= R.GATE_A
                assert torch.equal(part == 0, one == 0)


def test_simple_test_of_a_random_r50():
    """the GA-RetinaNet config with the head swapped, random initialisation, one 64 x 96 image"""
    import iouaware
    from iouaware.config import ConfigDict
    with open(os.path.join(GOLD, 'ga_ref.json')) as fh:
        rec = json.load(fh)
    model = dict(rec['model'], pretrained=None)
    torch.manual_seed(3)
    m = iouaware.build_detector(ConfigDict(model), train_cfg=None, test_cfg=ConfigDict(rec['test_cfg']))
    m.init_weights()
    m = m.to(DEV).eval()
    img = torch.randn(1, 3, 64, 96, device=DEV)
    meta = [dict(ori_shape=(60, 90, 3), img_shape=(64, 96, 3), pad_shape=(64, 96, 3), scale_factor=1.0, flip=False)]
    with torch.no_grad():
        res = m.simple_test(img, meta, rescale=True)
        outs = m.forward_head(img)
    assert len(res) == 80 and all(r.shape[1] == 5 and r.dtype == np.float32 for r in res)
    assert len(outs) == 5 and [tuple(o.shape[1:]) for o in (outs[0][0], outs[1][0], outs[2][0], outs[3][0], outs[4][0])] \
        == [(80, 8, 12), (4, 8, 12), (1, 8, 12), (2, 8, 12), (1, 8, 12)]
    assert all(bool(torch.isfinite(t).all()) for o in outs for t in o)
