"""Adversarial inputs for the anchor target assigner (csrc/assign.hip, iouaware/targets.py):
ties, IoUs exactly on a threshold, duplicate and degenerate boxes, gts outside the valid region,
the gt-count limits.  Deterministic (no random numbers at all), numpy only; shared by the
fixture generator (tests/golden/make_golden.py targets_edge), the CPU tests and the GPU tests.

Small pyramids: a 96 x 160 batch tensor gives levels 12x20, 6x10, 3x5, 2x3, 1x2, i.e.
N = 9 * 323 = 2907 anchors (no multiple of 256: the last workgroup is partial); one case at
64 x 64 (ends in two 1x1 maps) and one with scales_per_octave = 1 (A = 3).

Most gts have integer or half-integer coordinates and the anchors are integers (the generator
rounds the base anchors), so the intended ties and threshold hits are exact in float32.  Wherever
a case aims at an event, `case()` asserts with assign_ref that the event occurs: an input that
drifts fails here instead of testing nothing.  CHECKSUMS pins the inputs themselves.
"""
import functools

import numpy as np

import assign_ref as R
from synth import checksum

F = np.float32
STRIDES = (8, 16, 32, 64, 128)
RATIOS = (0.5, 1.0, 2.0)
TENSOR = (96, 160)
MAX_GT = 512                       # kMaxGt of csrc/assign.hip
A0 = (52., 28., 83., 59.)          # level 0, cell (y 5, x 8), ratio 1, scale 4: a 32 x 32 anchor

CASES = ('dup', 'sym', 'gt_is_anchor', 'thr_exact', 'thr_exact_q', 'many_claims', 'tiny', 'outside',
         'outside_minpos', 'valid_edge', 'G1', 'G257', 'G512', 'G1_G512', 'rpn_style', 'stds',
         'c64', 'a3')

# crc32 over every gt box and label array of the case, in image order
CHECKSUMS = {
    'dup': 148822041, 'sym': 1865409571, 'gt_is_anchor': 2185278053, 'thr_exact': 2780163844,
    'thr_exact_q': 2780163844, 'many_claims': 434995125, 'tiny': 3061138921, 'outside': 3053028044,
    'outside_minpos': 3053028044, 'valid_edge': 2098761528, 'G1': 3099788103, 'G257': 604206609,
    'G512': 1145378594, 'G1_G512': 239798842, 'rpn_style': 1760113898, 'stds': 776574102,
    'c64': 3713847166, 'a3': 1029385621,
}


def lattice(g):
    """g small distinct boxes on a 24-column lattice inside 160 x 96, labels 1..80"""
    i = np.arange(g)
    x1 = 0.5 + 6.5 * (i % 24)
    y1 = 1.0 + 4.0 * (i // 24)
    w = 5 + (i % 5)
    h = 3 + (i % 3)
    boxes = np.stack([x1, y1, x1 + w, y1 + h], 1).astype(F)
    assert np.unique(boxes, axis=0).shape[0] == g and boxes[:, 3].max() < TENSOR[0]
    return boxes, (1 + (i * 7) % 80).astype(np.int64)


NORMAL = np.array([[20.5, 10., 70., 50.5], [90., 30.5, 140.5, 80.], [4., 60., 40., 90.]], F)
NORMAL_L = np.array([5, 17, 80], np.int64)


def _spec(name):
    """-> dict(tensor, pads, gts, labels, and the non-default settings)"""
    x1, y1, x2, y2 = A0
    s = dict(tensor=TENSOR, pads=None, labels=None, pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0.0,
             pos_weight=-1.0, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), scales_per_octave=3)
    if name == 'dup':
        box = [50.5, 27., 85.5, 60.]
        s.update(gts=[np.array([box, box, [100., 50., 130., 80.]], F)],
                 labels=[np.array([3, 7, 11], np.int64)])
    elif name == 'sym':
        # mirrored about A0's centre x = 67.5: every anchor centred there sees both alike
        s.update(gts=[np.array([[x1 - 4, y1, x2 - 4, y2], [x1 + 4, y1, x2 + 4, y2]], F)],
                 labels=[np.array([21, 42], np.int64)])
    elif name == 'gt_is_anchor':
        # level 0, cell (y 6, x 10), ratio 0.5, scale 4: base (-19, -7, 26, 14) + (80, 48)
        s.update(gts=[np.array([[61., 41., 106., 62.], [10., 60.5, 50.5, 90.]], F)],
                 labels=[np.array([9, 33], np.int64)])
    elif name in ('thr_exact', 'thr_exact_q'):
        # IoU with a 32 x 32 anchor (area 1024), gt of the anchor's height:
        #   22 wide, 18 inside:  576 / (1024 + 704 - 576) = 1/2
        #   24 wide, 16 inside:  512 / (1024 + 768 - 512) = 2/5
        #   18 wide, 10 inside:  320 / (1024 + 576 - 320) = 1/4
        # each gt lies wholly inside the anchor one cell to the left, which is its maximum, so
        # step 4 leaves the threshold anchors alone
        s.update(gts=[np.array([[x1 - 4, y1, x1 + 17, y2],
                                [108. - 8, 28., 108. + 15, 59.],
                                [52. - 8, 60., 52. + 9, 91.]], F)],
                 labels=[np.array([2, 4, 6], np.int64)])
        if name == 'thr_exact_q':
            s.update(neg_iou_thr=0.25)
    elif name == 'many_claims':
        # a flat band: twenty level-1 anchors (46 high, 90 wide) hold it alike and tie for its
        # maximum; P overlaps A0 by 0.88, Q lies inside A0 and A0 is Q's only maximum
        s.update(gts=[np.array([[-100., 40., 260., 47.], [x1 + 1, y1 + 1, x2 + 1, y2 + 1],
                                [x1 + 4, y1 + 4, x2 - 4, y2 - 4]], F)],
                 labels=[np.array([1, 50, 60], np.int64)])
    elif name == 'tiny':
        s.update(gts=[np.array([[60., 44., 60., 44.], [62., 44., 62., 44.],
                                [100.5, 20.5, 100.5, 20.5], [0., 0., 0., 0.]], F)],
                 labels=[np.array([8, 16, 24, 32], np.int64)])
    elif name in ('outside', 'outside_minpos'):
        s.update(gts=[np.array([NORMAL[0], [5000., 5000., 5040., 5040.], NORMAL[1]], F)],
                 labels=[np.array([5, 77, 17], np.int64)])
        if name == 'outside_minpos':
            s.update(min_pos_iou=0.3)
    elif name == 'valid_edge':
        # image 1 is 80 x 104 inside the 96 x 160 tensor: one gt across x = 104, one beyond it
        s.update(pads=[TENSOR, (80, 104)],
                 gts=[NORMAL[:2].copy(),
                      np.array([[20., 20., 60., 60.], [90., 30., 130., 70.], [120.5, 10., 150., 40.5]], F)],
                 labels=[NORMAL_L[:2].copy(), np.array([12, 13, 14], np.int64)])
    elif name == 'G1':
        s.update(gts=[np.array([[30.5, 20., 90., 70.5]], F)], labels=[np.array([44], np.int64)])
    elif name in ('G257', 'G512'):
        b, l = lattice(int(name[1:]))
        s.update(gts=[b], labels=[l])
    elif name == 'G1_G512':
        b, l = lattice(MAX_GT)
        s.update(gts=[np.array([[30.5, 20., 90., 70.5]], F), b], labels=[np.array([44], np.int64), l])
    elif name == 'rpn_style':
        s.update(gts=[NORMAL.copy()], labels=None, pos_weight=2.0)
    elif name == 'stds':
        s.update(gts=[NORMAL.copy()], labels=[NORMAL_L.copy()], means=(0.1, -0.1, 0.05, 0.),
                 stds=(0.1, 0.1, 0.2, 0.2))
    elif name == 'c64':
        s.update(tensor=(64, 64), gts=[np.array([[10., 8.5, 40.5, 50.], [30., 30., 63., 63.]], F)],
                 labels=[np.array([3, 4], np.int64)])
    elif name == 'a3':
        box = [50.5, 27., 85.5, 60.]
        s.update(scales_per_octave=1, gts=[np.array([box, box, NORMAL[2]], F)],
                 labels=[np.array([3, 7, 80], np.int64)])
    else:
        raise KeyError(name)
    if s['pads'] is None:
        s['pads'] = [s['tensor']] * len(s['gts'])
    return s


def assign_kw(c):
    return dict(pos_iou_thr=c['pos_iou_thr'], neg_iou_thr=c['neg_iou_thr'], min_pos_iou=c['min_pos_iou'],
                pos_weight=c['pos_weight'], means=c['means'], stds=c['stds'])


def reference(c, **switches):
    """assign_ref on a case (the switches for the sensitivity test)"""
    kw = assign_kw(c)
    kw.update(switches)
    return R.assign_batch(c['anchors'], c['level_anchors'], c['valids'], c['gts'], c['labels'], **kw)


def _row(c, box):
    """index among the valid anchors of image 0 of the anchor with these coordinates"""
    a = c['anchors'][c['valids'][0]]
    hit = np.nonzero((a == np.asarray(box, F)).all(1))[0]
    assert hit.size == 1, (box, hit)
    return int(hit[0])


def _check_events(name, c):
    """the event each case aims at really occurs; -> the events as a dict (for the summary)"""
    ref = reference(c)
    im = ref['images'][0]
    ov, gi = im['overlaps'], im['gt_inds'][im['keep']]
    ev = dict(G=[int(g.shape[0]) for g in c['gts']], N=int(c['anchors'].shape[0]))
    if name in ('dup', 'a3'):
        assert np.array_equal(ov[0], ov[1])
        at_max = ov[0] == ov[0].max()
        over = (ov.max(0) >= F(0.5)) & (ov.argmax(0) == 0) & ~at_max
        assert over.sum() >= 1 and at_max.sum() >= 1
        assert (gi[over] == 1).all() and (gi[at_max] == 2).all()     # argmax: first; step 4: later
        ev.update(tie_first_copy=int(over.sum()), claimed_by_second_copy=int(at_max.sum()))
    if name == 'sym':
        tie = ov[0] == ov[1]
        hi, lo = tie & (ov[0] >= F(0.5)), tie & (ov[0] > 0) & (ov[0] < F(0.5))
        assert hi.sum() >= 2 and lo.sum() >= 2
        a0 = _row(c, A0)
        assert ov[0, a0] == ov[0].max() and ov[1, a0] == ov[1].max() and gi[a0] == 2
        ev.update(ties_above_half=int(hi.sum()), ties_below_half=int(lo.sum()))
    if name == 'gt_is_anchor':
        r = _row(c, c['gts'][0][0])
        assert ov[0, r] == F(1.0) and gi[r] == 1
        assert (im['bbox_targets'][im['keep']][r] == 0).all()
        ev.update(iou_one=1)
    if name in ('thr_exact', 'thr_exact_q'):
        mx = ov.max(0)
        r_half, r_neg = _row(c, A0), _row(c, (108., 28., 139., 59.))
        r_q = _row(c, (52., 60., 83., 91.))
        assert mx[r_half] == F(0.5) and ov[0, r_half] == F(0.5) and gi[r_half] == 1     # meets >= 0.5
        assert mx[r_neg] == F(0.4) and mx[r_neg] == F(2.0) / F(5.0) and mx[r_q] == F(0.25)
        if name == 'thr_exact':
            assert gi[r_neg] == -1 and gi[r_q] == 0          # 0.4f < 0.4f fails: ignored
        else:
            assert gi[r_neg] == -1 and gi[r_q] == -1         # 0.25 < 0.25 fails: ignored
        ev.update(iou_half=int((mx == F(0.5)).sum()), iou_two_fifths=int((mx == F(0.4)).sum()),
                  iou_quarter=int((mx == F(0.25)).sum()))
    if name == 'many_claims':
        band = ov[0] == ov[0].max()
        assert band.sum() >= 16 and ov[0].max() < F(0.4) and (gi[band] == 1).all()
        a0 = _row(c, A0)
        assert ov[:, a0].argmax() == 1 and ov[1, a0] >= F(0.5) and ov[2, a0] == ov[2].max()
        assert (ov[2] == ov[2].max()).sum() == 1 and gi[a0] == 3              # step 4 over step 3
        ev.update(band_ties=int(band.sum()), step4_over_step3=1)
    if name == 'tiny':
        assert (c['gts'][0][:, 0] == c['gts'][0][:, 2]).all() and ov.max() < F(0.4)
        for g in range(4):
            assert (ov[g] == ov[g].max()).sum() >= 2
        shared = (ov[0] == ov[0].max()) & (ov[1] == ov[1].max())
        assert shared.sum() >= 1 and (gi[shared] == 2).all()
        assert im['bbox_targets'][im['keep']][gi > 0][:, 2:].max() < -3.0       # log(1 / 22) and below
        ev.update(best_iou=float(ov.max()), shared_claims=int(shared.sum()))
    if name in ('outside', 'outside_minpos'):
        assert (ov[1] == 0).all()
        if name == 'outside':
            assert (gi == 2).sum() == gi.size - (ov[2] == ov[2].max()).sum() and (gi == 2).sum() > 1000
        else:
            assert (gi == 2).sum() == 0 and (gi == 0).sum() > 1000
        ev.update(anchors_of_the_outside_gt=int((gi == 2).sum()))
    if name == 'valid_edge':
        im1 = ref['images'][1]
        inval = ~im1['keep']
        assert inval.sum() > 500 and ref['images'][0]['keep'].all()
        assert (im1['label_weights'][inval] == 0).all() and (im1['labels'][inval] == 0).all()
        g1 = im1['gt_inds'][im1['keep']]
        assert (g1 == 2).sum() >= 1 and (g1 == 3).sum() >= 1      # both still claim valid anchors
        ev.update(invalid_anchors=int(inval.sum()))
    if name in ('G257', 'G512', 'G1_G512'):
        last = ref['images'][-1]
        g = last['gt_inds'][last['keep']]
        assert c['gts'][-1].shape[0] == (257 if name == 'G257' else MAX_GT)
        assert (g > 256).sum() >= 1 and (g == c['gts'][-1].shape[0]).sum() >= 1
        ev.update(anchors_of_gts_past_256=int((g > 256).sum()))
    if name == 'G1':
        assert c['gts'][0].shape[0] == 1
    if name == 'rpn_style':
        assert c['labels'] is None and set(np.unique(im['label_weights'])) == {0.0, 1.0, 2.0}
        assert set(np.unique(im['labels'])) == {0, 1}
    if name == 'c64':
        assert c['featmap_sizes'][-2:] == [(1, 1), (1, 1)] and c['anchors'].shape[0] == 774
    if name == 'a3':
        assert c['A'] == 3 and c['anchors'].shape[0] == 969
    elif name != 'c64':
        assert c['A'] == 9 and c['anchors'].shape[0] == 2907 and c['featmap_sizes'][-1] == (1, 2)
    return ev


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: tensor (H, W), pads [(h, w)] per image, gts [(G, 4) float32], labels [(G,) int64]
    or None, pos_iou_thr, neg_iou_thr, min_pos_iou, pos_weight, means, stds, scales_per_octave;
    the numpy anchors (N, 4), level_anchors [N_l], featmap_sizes, A, valids [(N,) bool] per image;
    checksum; events (what was asserted to occur)"""
    c = _spec(name)
    c['name'] = name
    c['anchors'], c['level_anchors'], c['featmap_sizes'], c['A'] = R.pyramid(
        c['tensor'], STRIDES, 4, c['scales_per_octave'], RATIOS)
    c['valids'] = [R.pyramid_valid(c['featmap_sizes'], STRIDES, c['A'], p) for p in c['pads']]
    c['checksum'] = checksum(list(c['gts']) + (list(c['labels']) if c['labels'] is not None else []))
    if name in CHECKSUMS:
        assert c['checksum'] == CHECKSUMS[name], (name, c['checksum'])
    c['events'] = _check_events(name, c)
    return c


def head_kw(c, base_kw):
    """constructor arguments of the head for a case, from the standard ones"""
    kw = dict(base_kw)
    kw.update(scales_per_octave=c['scales_per_octave'], target_means=list(c['means']),
              target_stds=list(c['stds']))
    return kw


def metas(c):
    from synth import img_meta
    return [img_meta(p[0], p[1], p[0], p[1]) for p in c['pads']]


def train_cfg(c):
    """the train_cfg dict of a case (plain dicts: wrap in the config class of whoever uses it)"""
    return dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=c['pos_iou_thr'],
                              neg_iou_thr=c['neg_iou_thr'], min_pos_iou=c['min_pos_iou'],
                              ignore_iof_thr=-1),
                allowed_border=-1, pos_weight=c['pos_weight'], debug=False)


if __name__ == '__main__':
    for n in CASES:
        cc = case(n)
        print("    %r: %d,   # %s" % (n, cc['checksum'], cc['events']))
