"""Plain-torch CPU definition of what the guided-anchor head's HIP code computes: the masked
convolution and the guided get_bboxes (reference iou_aware_ga_retina_head.py / guided_anchor_head.py
/ masked_conv.py, restated), plus the seeded synthetic head outputs of the GA fixtures.

`get_bboxes_single(..., variant=...)` also evaluates four WRONG variants, so that a test can show
that the fixture tells them apart:
    'sqrt'        the sqrt * sqrt score fusion of IoUawareRetinaHead
    'clip'        the guided anchor formed with the 16 / 1000 clip of the box decode
    'mask0'       image 0's location mask used for every image (get_bboxes, batch level)
    'topk_all'    the per-level top-k taken over all locations, the filter behind it
"""
import numpy as np
import torch
import torch.nn.functional as F

import synth

C = 80
STRIDES = synth.STRIDES
OCTAVE_BASE_SCALE = 4
LOC_FILTER_THR = 0.01
CLIP_BOX = float(np.abs(np.log(16 / 1000)))
CLIP_ANCHOR = float(np.abs(np.log(1e-6)))


# ------------------------------------------------------------------ masked convolution
def masked_conv2d(x, mask, weight, bias, padding, dtype=None):
    """x (B, C, H, W), mask (B, H, W) bool -> the convolution where the mask is set, exactly 0
    elsewhere; dtype: evaluate in that precision (fp64 yardstick / plain fp32)"""
    dtype = dtype or x.dtype
    y = F.conv2d(x.to(dtype), weight.to(dtype), None if bias is None else bias.to(dtype), padding=padding)
    return torch.where(mask[:, None], y, torch.zeros((), dtype=dtype))      # +0.0 where the mask is false


# ------------------------------------------------------------------ synthetic head outputs
# per case: per image, per level the mean of the location logits (std 2; the keep threshold
# sigmoid(loc) >= 0.01 is loc >= -4.595): 0 keeps nearly everything, -4.6 about half, -14 nothing
GA_CASES = [
    # (seed, batch, pad h, pad w, nms_pre, max_per_img, rescale, scale factors, cls mean, loc means)
    (2101, 1, 64, 96, 40, 150, False, [1.0], -7.0, [[-3.0, -4.6, 0.0, -14.0, 0.0]]),
    (2102, 2, 128, 192, 150, 100, True, [0.75, 1.5], -4.5,
     [[0.0, -4.6, -14.0, 0.0, 0.0], [-4.6, 0.0, -3.0, -14.0, -14.0]]),
]
SHAPE_PLANTS = 6          # per (image, level 0 / 1): locations given a |shape_pred| of 5.5 and a strong class


def ga_head_outputs(case):
    """-> cls[L] (B, 80, H, W), reg[L] (B, 4, ..), iou[L] (B, 1, ..), shape[L] (B, 2, ..), loc[L]
    (B, 1, ..) float32 arrays of GA_CASES[case], from numpy's frozen legacy stream"""
    seed, B, ph, pw = GA_CASES[case][:4]
    cmu, lmu = GA_CASES[case][8], GA_CASES[case][9]
    rs = np.random.RandomState(seed)
    cls, reg, iou, shape, loc = [], [], [], [], []
    for l, (h, w) in enumerate(synth.level_shapes(ph, pw)):
        cls.append((rs.standard_normal((B, C, h, w)) * 2.0 + cmu).astype(np.float32))
        reg.append((rs.standard_normal((B, 4, h, w)) * 0.5).astype(np.float32))
        iou.append((rs.standard_normal((B, 1, h, w)) * 1.5).astype(np.float32))
        shape.append((rs.standard_normal((B, 2, h, w)) * 1.0).astype(np.float32))
        lo = rs.standard_normal((B, 1, h, w)) * 2.0
        for b in range(B):
            lo[b] += lmu[b][l]
        loc.append(lo.astype(np.float32))
    # planted: kept locations with a very small guided anchor (shape -5.5: between the two clips)
    # and one strong class, so that detections depend on the anchor clip
    for b in range(B):
        for l in (0, 1):
            h, w = cls[l].shape[2:]
            for _ in range(SHAPE_PLANTS):
                y, x, c = rs.randint(0, h), rs.randint(0, w), rs.randint(0, C)
                shape[l][b, :, y, x] = np.float32(-5.5)
                loc[l][b, 0, y, x] = np.float32(3.0)
                cls[l][b, c, y, x] = np.float32(rs.uniform(2.0, 4.0))
                iou[l][b, 0, y, x] = np.float32(rs.uniform(1.0, 3.0))
    return cls, reg, iou, shape, loc


def square_base(stride, octave_base_scale=OCTAVE_BASE_SCALE):
    """base anchor of AnchorGenerator(stride, [octave_base_scale], [1.0])"""
    s = float(stride) * octave_base_scale
    c = 0.5 * (stride - 1)
    return np.round(np.array([c - 0.5 * (s - 1), c - 0.5 * (s - 1), c + 0.5 * (s - 1), c + 0.5 * (s - 1)],
                             np.float32))


def squares(h, w, stride):
    """(h * w, 4) fp32 square anchors, x fastest"""
    base = torch.from_numpy(square_base(stride))
    sx = (torch.arange(0, w) * stride).to(torch.float32)
    sy = (torch.arange(0, h) * stride).to(torch.float32)
    xx = sx.repeat(h)
    yy = sy.view(-1, 1).expand(h, w).reshape(-1)
    return base[None] + torch.stack([xx, yy, xx, yy], dim=-1)


def delta2bbox(rois, deltas, means, stds, max_shape=None, clip=CLIP_BOX):
    means = deltas.new_tensor(means)[None]
    stds = deltas.new_tensor(stds)[None]
    d = deltas * stds + means
    dx, dy = d[:, 0], d[:, 1]
    dw = d[:, 2].clamp(min=-clip, max=clip)
    dh = d[:, 3].clamp(min=-clip, max=clip)
    px = (rois[:, 0] + rois[:, 2]) * 0.5
    py = (rois[:, 1] + rois[:, 3]) * 0.5
    pw = rois[:, 2] - rois[:, 0] + 1.0
    ph = rois[:, 3] - rois[:, 1] + 1.0
    gw = pw * dw.exp()
    gh = ph * dh.exp()
    gx = torch.addcmul(px, pw, dx)
    gy = torch.addcmul(py, ph, dy)
    x1 = gx - gw * 0.5 + 0.5
    y1 = gy - gh * 0.5 + 0.5
    x2 = gx + gw * 0.5 - 0.5
    y2 = gy + gh * 0.5 - 0.5
    if max_shape is not None:
        x1 = x1.clamp(min=0, max=max_shape[1] - 1)
        y1 = y1.clamp(min=0, max=max_shape[0] - 1)
        x2 = x2.clamp(min=0, max=max_shape[1] - 1)
        y2 = y2.clamp(min=0, max=max_shape[0] - 1)
    return torch.stack([x1, y1, x2, y2], dim=-1)


def nms(dets, iou_thr):
    """greedy NMS on (n, 5) fp32 rows -> kept indices in ascending order, as the reference's CPU
    kernel returns them (a box is suppressed at IoU >= iou_thr, +1 pixel convention, fp32 arithmetic)"""
    d = dets.numpy()
    x1, y1, x2, y2, sc = d[:, 0], d[:, 1], d[:, 2], d[:, 3], d[:, 4]
    areas = (x2 - x1 + np.float32(1)) * (y2 - y1 + np.float32(1))
    order = np.argsort(-sc, kind='stable')
    dead = np.zeros(len(d), bool)
    keep = []
    for _i, i in enumerate(order):
        if dead[i]:
            continue
        keep.append(i)
        rest = order[_i + 1:]
        ww = np.maximum(np.float32(0), np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + np.float32(1))
        hh = np.maximum(np.float32(0), np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + np.float32(1))
        inter = ww * hh
        ovr = inter / (areas[i] + areas[rest] - inter)
        dead[rest[ovr >= np.float32(iou_thr)]] = True
    return np.sort(np.asarray(keep, np.int64))


def multiclass_nms(boxes, scores, ids, score_thr, iou_thr, max_num):
    """boxes (n, 4), scores (n, C), ids (n,) -> dets (k, 5), labels (k,), ids (k,): per class the rows
    with score > score_thr through NMS, classes concatenated in order; more than max_num survivors:
    the max_num best by score (descending)"""
    out_d, out_l, out_i = [], [], []
    for c in range(scores.shape[1]):
        sel = scores[:, c] > score_thr
        if not sel.any():
            continue
        d = torch.cat([boxes[sel], scores[sel, c][:, None]], dim=1)
        k = nms(d, iou_thr)
        out_d.append(d[k])
        out_l.append(torch.full((len(k),), c, dtype=torch.long))
        out_i.append(ids[sel][k])
    if not out_d:
        return torch.zeros((0, 5)), torch.zeros((0,), dtype=torch.long), torch.zeros((0,), dtype=torch.long)
    d, l, i = torch.cat(out_d), torch.cat(out_l), torch.cat(out_i)
    if d.shape[0] > max_num:
        order = d[:, 4].sort(descending=True)[1][:max_num]
        d, l, i = d[order], l[order], i[order]
    return d, l, i


def keep_mask(loc, use_loc_filter=True, thr=LOC_FILTER_THR):
    """loc (1, H, W) logits -> (H * W,) bool"""
    s = loc.sigmoid()
    return (s >= thr if use_loc_filter else s >= 0.0).reshape(-1)


def candidates_single(cls, reg, iou, shape, loc, img_shape, nms_pre, use_loc_filter=True, variant=None,
                      masks=None, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), strides=STRIDES):
    """one image: per-level lists of torch tensors (ch, H, W) -> the candidates handed to the NMS:
    boxes (n, 4) (clamped, not rescaled), scores (n, C), ids (n,) (location id: level offset +
    y * W + x), and per level the row maxima of the kept locations (for margins)"""
    mlvl_b, mlvl_s, mlvl_i, rowmax = [], [], [], []
    off = 0
    for l in range(len(cls)):
        h, w = cls[l].shape[-2:]
        n = h * w
        mask = keep_mask(loc[l], use_loc_filter) if masks is None else masks[l]
        ids = torch.arange(n) + off
        off += n
        sc = cls[l].permute(1, 2, 0).reshape(-1, C)
        io = iou[l].permute(1, 2, 0).reshape(-1)
        if variant == 'sqrt':
            scores = sc.sigmoid().sqrt() * io.sigmoid().sqrt()[:, None]
        else:
            scores = sc.sigmoid() * io.sigmoid()[:, None]
        deltas = torch.zeros(n, 4)
        deltas[:, 2:] = shape[l].permute(1, 2, 0).reshape(-1, 2)
        anchors = delta2bbox(squares(h, w, strides[l]), deltas, means, stds,
                             clip=CLIP_BOX if variant == 'clip' else CLIP_ANCHOR)
        bp = reg[l].permute(1, 2, 0).reshape(-1, 4)
        if variant == 'topk_all':
            if 0 < nms_pre < n:
                top = scores.max(1)[0].topk(nms_pre)[1]
                scores, anchors, bp, ids, mask = scores[top], anchors[top], bp[top], ids[top], mask[top]
            scores, anchors, bp, ids = scores[mask], anchors[mask], bp[mask], ids[mask]
            rowmax.append(scores.max(1)[0] if len(ids) else scores.new_zeros(0))
            if not len(ids):
                continue
        else:
            if mask.sum() == 0:
                rowmax.append(scores.new_zeros(0))
                continue
            scores, anchors, bp, ids = scores[mask], anchors[mask], bp[mask], ids[mask]
            rowmax.append(scores.max(1)[0])
            if 0 < nms_pre < scores.shape[0]:
                top = scores.max(1)[0].topk(nms_pre)[1]
                scores, anchors, bp, ids = scores[top], anchors[top], bp[top], ids[top]
        mlvl_b.append(delta2bbox(anchors, bp, means, stds, img_shape))
        mlvl_s.append(scores)
        mlvl_i.append(ids)
    if not mlvl_b:
        return torch.zeros((0, 4)), torch.zeros((0, C)), torch.zeros((0,), dtype=torch.long), rowmax
    return torch.cat(mlvl_b), torch.cat(mlvl_s), torch.cat(mlvl_i), rowmax


def get_bboxes_single(cls, reg, iou, shape, loc, img_shape, scale_factor, rescale, nms_pre, score_thr,
                      iou_thr, max_per_img, use_loc_filter=True, variant=None, masks=None):
    """-> dets (k, 5) fp32, labels (k,) int64, ids (k,) int64 (the location each detection came from).
    An image without a kept location: zero detections."""
    boxes, scores, ids, _ = candidates_single(cls, reg, iou, shape, loc, img_shape, nms_pre, use_loc_filter,
                                              variant, masks)
    if rescale:
        boxes = boxes / boxes.new_tensor(scale_factor)
    return multiclass_nms(boxes, scores, ids, score_thr, iou_thr, max_per_img)


def get_bboxes(maps, metas, rescale, nms_pre, score_thr, iou_thr, max_per_img, use_loc_filter=True, variant=None):
    """maps: (cls[L], reg[L], iou[L], shape[L], loc[L]) of (B, ch, H, W) numpy arrays -> per image
    (dets, labels, ids) numpy"""
    t = [[torch.from_numpy(np.ascontiguousarray(m)) for m in kind] for kind in maps]
    B = t[0][0].shape[0]
    out = []
    for b in range(B):
        masks = None
        if variant == 'mask0':
            masks = [keep_mask(lo[0], use_loc_filter) for lo in t[4]]
        per = [[m[b] for m in kind] for kind in t]
        d, l, i = get_bboxes_single(*per, metas[b]['img_shape'], metas[b]['scale_factor'], rescale, nms_pre,
                                    score_thr, iou_thr, max_per_img, use_loc_filter,
                                    None if variant == 'mask0' else variant, masks)
        out.append((d.numpy(), l.numpy(), i.numpy()))
    return out


def case_metas(case):
    seed, B, ph, pw, nms_pre, max_per_img, rescale, sf = GA_CASES[case][:8]
    return [dict(img_shape=(ph - 9 * b, pw - 13 * b, 3), scale_factor=sf[b], pad_shape=(ph, pw, 3))
            for b in range(B)]


def canonical(dets, labels, ids):
    """rows ordered by (label, score descending, id): the order-free form two results are compared in"""
    order = np.lexsort((ids, -dets[:, 4].astype(np.float64), labels))
    return dets[order], labels[order], ids[order]


# ------------------------------------------------------------------ the head-forward fixture
# a small head (16 channels: 4 per deformable group) on two levels, weights filled by name from a seed
FWD = dict(seed=2201, feat_seed=2202, channels=16, sizes=[(8, 12), (5, 7)], strides=[8, 16])
FWD_HEAD = dict(num_classes=81, in_channels=16, stacked_convs=4, feat_channels=16, octave_base_scale=4,
                scales_per_octave=3, octave_ratios=[0.5, 1.0, 2.0], anchor_strides=[8, 16],
                anchor_base_sizes=None, anchoring_means=[.0, .0, .0, .0], anchoring_stds=[1.0, 1.0, 1.0, 1.0],
                target_means=(.0, .0, .0, .0), target_stds=[1.0, 1.0, 1.0, 1.0], loc_filter_thr=0.01,
                loss_loc=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                loss_shape=dict(type='IoULoss', style='bounded', beta=0.2, loss_weight=1.0),
                loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                loss_bbox=dict(type='SmoothL1Loss', beta=0.04, loss_weight=1.0))
FWD_MAPS = ('cls_score', 'bbox_pred', 'iou_pred', 'shape_pred', 'loc_pred')


def fill_head_state(state, seed):
    """fill a GA head's state dict (name -> tensor, in place) from `seed`; depends on names and
    shapes only.  He-scaled tower weights; conv_loc around the keep threshold (bias -log(99), as
    init_weights sets it, weights scaled up so that the logits spread by about +-2 around it)"""
    rs = np.random.RandomState(seed)
    for key in sorted(state.keys()):
        t = state[key]
        shape = tuple(t.shape)
        if t.dim() == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            gain = np.sqrt(2.0 / fan_in)
            if key.startswith('conv_loc.'):
                gain *= 3.0
            if 'conv_offset' in key:
                gain = 0.5
            v = rs.standard_normal(shape) * gain
        elif key == 'conv_loc.bias':
            v = np.full(shape, -np.log(99.0))
        else:
            v = rs.standard_normal(shape) * 0.1
        state[key] = torch.from_numpy(np.asarray(v, np.float32))
    return state


def forward_features():
    rs = np.random.RandomState(FWD['feat_seed'])
    return [rs.standard_normal((1, FWD['channels'], h, w)).astype(np.float32) for (h, w) in FWD['sizes']]
