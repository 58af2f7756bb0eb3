"""Plain numpy evaluation of the anchor target assignment (reference mmdet/core/anchor/
anchor_target.py:129-242, assigners/max_iou_assigner.py:98-201, bbox/geometry.py:48-64,
bbox/transforms.py:6-41, anchor/anchor_generator.py) -- the yardstick of the device assigner
(csrc/assign.hip) and of iouaware/targets.py.  numpy only: no torch, nothing from iouaware.

One image at a time, the way the reference works: the full (G, N_valid) IoU matrix in float32
with the reference's operation order, the four assigner steps in the reference's order (a Python
loop over the gts for step 4), bbox2delta, `unmap` to the invalid anchors, the counts.

Four switches turn single rules into the nearest wrong variant (defaults = the reference); they
exist so that test_host_targets.py can show that the adversarial inputs (synth_targets.py) tell
the variants apart:
    argmax_tie           'first' | 'last'            which gt an anchor with equal IoUs goes to
    claim_order          'later_wins' | 'earlier_wins'   step 4: whose claim stands
    pos_cmp / neg_cmp    'ge' | 'gt',  'lt' | 'le'   the threshold comparisons
    zero_overlap_claims  True | False                a gt without overlap claims every
                                                     zero-overlap anchor (min_pos_iou = 0)
"""
import numpy as np

F = np.float32


# ------------------------------------------------------------------ anchors (base + shift, fp32)
def retina_scales(octave_base_scale=4, scales_per_octave=3):
    return (np.array([2 ** (i / scales_per_octave) for i in range(scales_per_octave)])
            * octave_base_scale).astype(F)


def base_anchors(base_size, scales, ratios):
    """gen_base_anchors (scale_major, ctr=None): (len(ratios) * len(scales), 4) float32"""
    scales, ratios = np.asarray(scales, F), np.asarray(ratios, F)
    w = h = F(base_size)
    x_ctr, y_ctr = F(0.5 * (base_size - 1)), F(0.5 * (base_size - 1))
    h_ratios = np.sqrt(ratios)
    w_ratios = F(1) / h_ratios
    ws = (w * w_ratios[:, None] * scales[None, :]).reshape(-1)
    hs = (h * h_ratios[:, None] * scales[None, :]).reshape(-1)
    half = F(0.5)
    out = np.stack([x_ctr - half * (ws - F(1)), y_ctr - half * (hs - F(1)),
                    x_ctr + half * (ws - F(1)), y_ctr + half * (hs - F(1))], -1)
    return np.round(out).astype(F)                  # half-to-even, like torch.round


def grid_anchors(base, featmap_size, stride):
    fh, fw = featmap_size
    sx = np.tile(np.arange(fw) * stride, fh)
    sy = np.repeat(np.arange(fh) * stride, fw)
    shifts = np.stack([sx, sy, sx, sy], -1).astype(F)
    return (base[None, :, :] + shifts[:, None, :]).reshape(-1, 4)


def valid_flags(featmap_size, valid_size, num_base):
    fh, fw = featmap_size
    vh, vw = valid_size
    assert vh <= fh and vw <= fw
    vx = (np.arange(fw) < vw)
    vy = (np.arange(fh) < vh)
    v = np.tile(vx, fh) & np.repeat(vy, fw)
    return np.repeat(v, num_base)


def level_shapes(pad_h, pad_w, strides):
    """feature-map sizes of a stride-2 pyramid (ceil division at every halving)"""
    out, h, w, cur = [], pad_h, pad_w, 1
    for s in strides:
        while cur < s:
            h, w, cur = (h + 1) // 2, (w + 1) // 2, cur * 2
        out.append((h, w))
    return out


def pyramid(tensor_hw, strides=(8, 16, 32, 64, 128), octave_base_scale=4, scales_per_octave=3,
            ratios=(0.5, 1.0, 2.0)):
    """-> (anchors (N, 4) float32 of all levels, [N_l], featmap sizes, A) for a batch tensor of
    tensor_hw = (H, W)"""
    sizes = level_shapes(tensor_hw[0], tensor_hw[1], strides)
    scales = retina_scales(octave_base_scale, scales_per_octave)
    levels = [grid_anchors(base_anchors(s, scales, ratios), fs, s) for s, fs in zip(strides, sizes)]
    return np.concatenate(levels), [a.shape[0] for a in levels], sizes, len(ratios) * len(scales)


def pyramid_valid(sizes, strides, num_base, pad_shape):
    """AnchorHead.get_anchors: valid flags of one image from its pad_shape (anchor_head.py:135-146)"""
    out = []
    for (fh, fw), s in zip(sizes, strides):
        vh = min(int(np.ceil(pad_shape[0] / s)), fh)
        vw = min(int(np.ceil(pad_shape[1] / s)), fw)
        out.append(valid_flags((fh, fw), (vh, vw), num_base))
    return np.concatenate(out)


# ------------------------------------------------------------------ the assigner
def bbox_overlaps(gt, boxes):
    """(G, 4), (N, 4) float32 -> (G, N) float32: `+1` widths, ov / ((area_gt + area_box) - ov)"""
    gt, boxes = np.asarray(gt, F), np.asarray(boxes, F)
    one = F(1)
    lt = np.maximum(gt[:, None, :2], boxes[None, :, :2])
    rb = np.minimum(gt[:, None, 2:], boxes[None, :, 2:])
    wh = np.maximum(rb - lt + one, F(0))
    ov = wh[:, :, 0] * wh[:, :, 1]
    area1 = (gt[:, 2] - gt[:, 0] + one) * (gt[:, 3] - gt[:, 1] + one)
    area2 = (boxes[:, 2] - boxes[:, 0] + one) * (boxes[:, 3] - boxes[:, 1] + one)
    out = ov / (area1[:, None] + area2[None, :] - ov)
    assert out.dtype == F
    return out


def bbox2delta(proposals, gt, means, stds):
    p, g = np.asarray(proposals, F), np.asarray(gt, F)
    half, one = F(0.5), F(1)
    px, py = (p[:, 0] + p[:, 2]) * half, (p[:, 1] + p[:, 3]) * half
    pw, ph = p[:, 2] - p[:, 0] + one, p[:, 3] - p[:, 1] + one
    gx, gy = (g[:, 0] + g[:, 2]) * half, (g[:, 1] + g[:, 3]) * half
    gw, gh = g[:, 2] - g[:, 0] + one, g[:, 3] - g[:, 1] + one
    d = np.stack([(gx - px) / pw, (gy - py) / ph, np.log(gw / pw), np.log(gh / ph)], -1)
    d = (d - np.asarray(means, F)[None]) / np.asarray(stds, F)[None]
    assert d.dtype == F
    return d


def assign_wrt_overlaps(ov, pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0.0, argmax_tie='first',
                        claim_order='later_wins', pos_cmp='ge', neg_cmp='lt',
                        zero_overlap_claims=True):
    """(G, N) float32 overlaps -> (N,) int64: -1 ignored, 0 negative, k > 0 assigned to gt k - 1.
    A float32 tensor compared with a Python float compares in float32: the thresholds are
    rounded to float32 first."""
    G, N = ov.shape
    assert G >= 1 and N >= 1 and ov.dtype == F
    pos_thr, neg_thr, min_pos = F(pos_iou_thr), F(neg_iou_thr), F(min_pos_iou)
    assigned = np.full(N, -1, np.int64)                                    # step 1
    max_ov = ov.max(0)
    if argmax_tie == 'first':
        argmax_ov = ov.argmax(0)
    else:
        assert argmax_tie == 'last'
        argmax_ov = G - 1 - ov[::-1].argmax(0)
    gt_max = ov.max(1)
    neg = (max_ov < neg_thr) if neg_cmp == 'lt' else (max_ov <= neg_thr)
    assert neg_cmp in ('lt', 'le') and pos_cmp in ('ge', 'gt')
    assigned[(max_ov >= 0) & neg] = 0                                      # step 2
    pos = (max_ov >= pos_thr) if pos_cmp == 'ge' else (max_ov > pos_thr)
    assigned[pos] = argmax_ov[pos] + 1                                     # step 3
    assert claim_order in ('later_wins', 'earlier_wins')
    order = range(G) if claim_order == 'later_wins' else range(G - 1, -1, -1)
    for i in order:                                                        # step 4
        if gt_max[i] >= min_pos and (zero_overlap_claims or gt_max[i] > 0):
            assigned[ov[i] == gt_max[i]] = i + 1
    return assigned


def assign_image(anchors, valid, gt_boxes, gt_labels=None, pos_iou_thr=0.5, neg_iou_thr=0.4,
                 min_pos_iou=0.0, pos_weight=-1.0, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.),
                 **switches):
    """anchor_target_single with allowed_border = -1, PseudoSampler, unmap_outputs.
    -> dict: labels (N) int64, label_weights (N), bbox_targets (N, 4), bbox_weights (N, 4),
    gt_inds (N) int64 (the assigner's result; -2 on invalid anchors), overlaps (G, N_valid),
    keep (N) bool, num_pos, num_neg"""
    anchors = np.asarray(anchors, F)
    keep = np.asarray(valid).astype(bool)
    gt = np.asarray(gt_boxes, F).reshape(-1, 4)
    if not keep.any() or gt.shape[0] == 0:
        raise ValueError('No gt or bboxes')
    a = anchors[keep]
    ov = bbox_overlaps(gt, a)
    assigned = assign_wrt_overlaps(ov, pos_iou_thr, neg_iou_thr, min_pos_iou, **switches)
    pos = np.nonzero(assigned > 0)[0]
    neg = np.nonzero(assigned == 0)[0]
    nv = a.shape[0]
    bt, bw = np.zeros((nv, 4), F), np.zeros((nv, 4), F)
    labels, lw = np.zeros(nv, np.int64), np.zeros(nv, F)
    if pos.size:
        bt[pos] = bbox2delta(a[pos], gt[assigned[pos] - 1], means, stds)
        bw[pos] = 1.0
        labels[pos] = 1 if gt_labels is None else np.asarray(gt_labels, np.int64)[assigned[pos] - 1]
        lw[pos] = 1.0 if pos_weight <= 0 else pos_weight
    if neg.size:
        lw[neg] = 1.0
    N = anchors.shape[0]

    def unmap(x, fill=0):
        out = np.full((N,) + x.shape[1:], fill, x.dtype)
        out[keep] = x
        return out

    return dict(labels=unmap(labels), label_weights=unmap(lw), bbox_targets=unmap(bt),
                bbox_weights=unmap(bw), gt_inds=unmap(assigned, -2), overlaps=ov, keep=keep,
                num_pos=int(pos.size), num_neg=int(neg.size))


def assign_batch(anchors, level_anchors, valids, gt_boxes, gt_labels=None, **kw):
    """anchor_target for a batch: per-level (B, N_l[, 4]) arrays (images_to_levels), counts (B, 2)
    int32 = (positives, negatives) per image, num_total_pos / num_total_neg = sum_i max(n_i, 1)
    (anchor_target.py:94-95), and the per-image results under 'images'."""
    B = len(gt_boxes)
    imgs = [assign_image(anchors, valids[b], gt_boxes[b],
                         None if gt_labels is None else gt_labels[b], **kw) for b in range(B)]
    out = dict(images=imgs)
    for key in ('labels', 'label_weights', 'bbox_targets', 'bbox_weights'):
        full = np.stack([r[key] for r in imgs])
        lv, off = [], 0
        for n in level_anchors:
            lv.append(full[:, off:off + n])
            off += n
        out[key] = lv
    out['counts'] = np.array([[r['num_pos'], r['num_neg']] for r in imgs], np.int32)
    out['num_total_pos'] = int(sum(max(r['num_pos'], 1) for r in imgs))
    out['num_total_neg'] = int(sum(max(r['num_neg'], 1) for r in imgs))
    return out
