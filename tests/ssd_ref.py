"""Plain-torch restatement of the SSD model (any dtype, CPU): the anchors of SSDHead, SSDVGG.forward,
L2Norm, SSDHead.forward and get_bboxes (softmax over the C + 1 logits of every anchor row, delta2bbox,
multiclass_nms on a plain greedy NMS) -- the yardstick of tests/test_host_ssd.py and the GPU tests,
and the regenerator of the seeded inputs whose reference results tests/golden/make_golden_ssd.py
records.  Written from the model's published definition; it shares no code with the package.
"""
import numpy as np
import torch
import torch.nn.functional as F

CLIP = float(abs(np.log(16 / 1000)))
SCORE_THR, IOU_THR, MAX_PER_IMG = 0.02, 0.45, 200

SSD300_SIZES = [(38, 38), (19, 19), (10, 10), (5, 5), (3, 3), (1, 1)]
SSD512_SIZES = [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
SMALL_SIZES = [(5, 5), (3, 3), (2, 2), (1, 1), (1, 1), (1, 1)]
RATIOS6 = ([2], [2, 3], [2, 3], [2, 3], [2], [2])
RATIOS7 = ([2], [2, 3], [2, 3], [2, 3], [2, 3], [2], [2])
STRIDES300 = (8, 16, 32, 64, 100, 300)
STRIDES512 = (8, 16, 32, 64, 128, 256, 512)

# the four (input_size, basesize_ratio_range) settings of the reference's configs
ANCHOR_SETTINGS = {
    'ssd300_coco': dict(input_size=300, basesize_ratio_range=(0.15, 0.9), anchor_strides=STRIDES300,
                        anchor_ratios=RATIOS6, in_channels=(512, 1024, 512, 256, 256, 256)),
    'ssd300_voc': dict(input_size=300, basesize_ratio_range=(0.2, 0.9), anchor_strides=STRIDES300,
                       anchor_ratios=RATIOS6, in_channels=(512, 1024, 512, 256, 256, 256)),
    'ssd512_coco': dict(input_size=512, basesize_ratio_range=(0.1, 0.9), anchor_strides=STRIDES512,
                        anchor_ratios=RATIOS7, in_channels=(512, 1024, 512, 256, 256, 256, 256)),
    'ssd512_voc': dict(input_size=512, basesize_ratio_range=(0.15, 0.9), anchor_strides=STRIDES512,
                       anchor_ratios=RATIOS7, in_channels=(512, 1024, 512, 256, 256, 256, 256)),
}

# the recorded get_bboxes cases: SSD300 COCO anchors on both; `hot` rows per image get one class lifted
# above the background, every other row stays far below score_thr
CASES = {
    'ssd300': dict(seed=3101, sizes=SSD300_SIZES, num_classes=81, hot=320,
                   metas=[dict(img_shape=(300, 300, 3), scale_factor=1.0)], rescale=(False,)),
    'small': dict(seed=3102, sizes=SMALL_SIZES, num_classes=6, hot=70,
                  metas=[dict(img_shape=(300, 300, 3), scale_factor=1.25),
                         dict(img_shape=(270, 300, 3), scale_factor=np.array([0.9, 0.8, 0.9, 0.8], np.float32)),
                         dict(img_shape=(300, 241, 3), scale_factor=2.0)], rescale=(False, True)),
}
CASE_HEAD = dict(ANCHOR_SETTINGS['ssd300_coco'], target_means=(.0, .0, .0, .0), target_stds=(0.1, 0.1, 0.2, 0.2))


# ------------------------------------------------------------------ anchors
def anchor_sizes(input_size, basesize_ratio_range, num_levels):
    lo, hi = int(basesize_ratio_range[0] * 100), int(basesize_ratio_range[1] * 100)
    step = int(np.floor(hi - lo) / (num_levels - 2))
    mins = [int(input_size * r / 100) for r in range(lo, hi + 1, step)]
    maxs = [int(input_size * (r + step) / 100) for r in range(lo, hi + 1, step)]
    first = {(300, 0.15): (7, 15), (300, 0.2): (10, 20), (512, 0.1): (4, 10), (512, 0.15): (7, 15)}
    a, b = first[(input_size, basesize_ratio_range[0])]
    return [int(input_size * a / 100)] + mins, [int(input_size * b / 100)] + maxs


def base_anchors(input_size, basesize_ratio_range, anchor_strides, anchor_ratios, **unused):
    """one (A_l, 4) fp32 tensor per level: [small square, large square, small x (1/r, r) ...]"""
    mins, maxs = anchor_sizes(input_size, basesize_ratio_range, len(anchor_strides))
    out = []
    for k, stride in enumerate(anchor_strides):
        scales = torch.tensor([1., np.sqrt(maxs[k] / mins[k])], dtype=torch.float32)
        ratios = [1.]
        for r in anchor_ratios[k]:
            ratios += [1 / r, r]
        ratios = torch.tensor(ratios, dtype=torch.float32)
        c = (stride - 1) / 2.
        hr = torch.sqrt(ratios)
        wr = 1 / hr
        ws = (float(mins[k]) * scales[:, None] * wr[None, :]).reshape(-1)
        hs = (float(mins[k]) * scales[:, None] * hr[None, :]).reshape(-1)
        all_ = torch.stack([c - 0.5 * (ws - 1), c - 0.5 * (hs - 1), c + 0.5 * (ws - 1), c + 0.5 * (hs - 1)],
                           dim=-1).round()
        n = len(ratios)
        out.append(all_[[0, n] + list(range(1, n))])
    return out


def grid_anchors(base, size, stride):
    """(H * W * A, 4): row (y * W + x) * A + a"""
    h, w = size
    sx = (torch.arange(0, w) * stride).to(base.dtype)
    sy = (torch.arange(0, h) * stride).to(base.dtype)
    xx = sx.repeat(h)
    yy = sy.view(-1, 1).expand(h, w).reshape(-1)
    shifts = torch.stack([xx, yy, xx, yy], dim=-1)
    return (base[None] + shifts[:, None]).reshape(-1, 4)


# ------------------------------------------------------------------ network
def l2norm(x, weight, eps=1e-10):
    norm = x.pow(2).sum(1, keepdim=True).sqrt() + eps
    return weight[None, :, None, None].expand_as(x) * x / norm


def vgg_forward(state, x, input_size, eps=1e-10):
    """SSDVGG.forward from a reference-named state dict: the 2-2-3-3-3 VGG-16 body with ceil-mode
    pools and no last pool, pool3x3 / dilated fc6 / fc7, the extra layers, L2Norm on conv4_3"""
    outs, idx = [], 0

    def conv(x, name, **kw):
        return F.conv2d(x, state[name + '.weight'], state[name + '.bias'], **kw)
    for stage, n in enumerate((2, 2, 3, 3, 3)):
        for _ in range(n):
            x = F.relu(conv(x, 'features.%d' % idx, padding=1))
            idx += 2
            if idx - 1 == 22:
                outs.append(x)
        if stage < 4:
            x = F.max_pool2d(x, 2, 2, ceil_mode=True)
            idx += 1
    assert idx == 30
    x = F.max_pool2d(x, 3, 1, 1)
    x = F.relu(conv(x, 'features.31', padding=6, dilation=6))
    x = F.relu(conv(x, 'features.33'))
    outs.append(x)
    extra = {300: ((1, 1, 0), (3, 2, 1), (1, 1, 0), (3, 2, 1), (1, 1, 0), (3, 1, 0), (1, 1, 0), (3, 1, 0)),
             512: ((1, 1, 0), (3, 2, 1)) * 4 + ((1, 1, 0), (4, 1, 1))}[input_size]
    for i, (k, s, p) in enumerate(extra):
        x = F.relu(conv(x, 'extra.%d' % i, stride=s, padding=p))
        if i % 2 == 1:
            outs.append(x)
    outs[0] = l2norm(outs[0], state['l2_norm.weight'], eps)
    return outs


def head_forward(state, feats, prefix=''):
    cls = [F.conv2d(f, state['%scls_convs.%d.weight' % (prefix, i)], state['%scls_convs.%d.bias' % (prefix, i)],
                    padding=1) for i, f in enumerate(feats)]
    reg = [F.conv2d(f, state['%sreg_convs.%d.weight' % (prefix, i)], state['%sreg_convs.%d.bias' % (prefix, i)],
                    padding=1) for i, f in enumerate(feats)]
    return cls, reg


# ------------------------------------------------------------------ get_bboxes
def delta2bbox(rois, deltas, means, stds, max_shape=None, clip=CLIP):
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
    """greedy NMS on (n, 5) rows in their own dtype -> kept indices ascending (suppression at
    IoU >= iou_thr, +1 pixel convention; equal scores: the lower row first)"""
    d = dets.numpy()
    one, zero, thr = d.dtype.type(1), d.dtype.type(0), d.dtype.type(iou_thr)
    x1, y1, x2, y2, sc = d[:, 0], d[:, 1], d[:, 2], d[:, 3], d[:, 4]
    areas = (x2 - x1 + one) * (y2 - y1 + one)
    order = np.argsort(-sc, kind='stable')
    dead = np.zeros(len(d), bool)
    keep = []
    for _i, i in enumerate(order):
        if dead[i]:
            continue
        keep.append(i)
        rest = order[_i + 1:]
        ww = np.maximum(zero, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + one)
        hh = np.maximum(zero, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + one)
        inter = ww * hh
        ovr = inter / (areas[i] + areas[rest] - inter)
        dead[rest[ovr >= thr]] = True
    return np.sort(np.asarray(keep, np.int64))


def multiclass_nms(boxes, scores, score_thr, iou_thr, max_num):
    """boxes (n, 4), scores (n, C + 1) with column 0 = background -> dets (k, 5), labels (k,) 0-based
    foreground class, ids (k,) row ids: per class the rows with score > score_thr through NMS, classes
    concatenated in order; more than max_num survivors: the max_num best by score (stable)"""
    out_d, out_l, out_i = [], [], []
    for c in range(1, scores.shape[1]):
        sel = (scores[:, c] > score_thr).nonzero().flatten()
        if sel.numel() == 0:
            continue
        d = torch.cat([boxes[sel], scores[sel, c][:, None]], dim=1)
        k = nms(d, iou_thr)
        out_d.append(d[k])
        out_l.append(torch.full((len(k),), c - 1, dtype=torch.long))
        out_i.append(sel[k])
    if not out_d:
        return boxes.new_zeros((0, 5)), torch.zeros((0,), dtype=torch.long), torch.zeros((0,), dtype=torch.long)
    d, l, i = torch.cat(out_d), torch.cat(out_l), torch.cat(out_i)
    if d.shape[0] > max_num:
        order = d[:, 4].sort(descending=True, stable=True)[1][:max_num]
        d, l, i = d[order], l[order], i[order]
    return d, l, i


def candidates_single(cls, reg, base, strides, num_classes, means, stds, img_shape):
    """cls[l] (A_l * num_classes, H, W), reg[l] (A_l * 4, H, W) of one image -> boxes (R, 4), scores
    (R, num_classes) over ALL rows in the order level, (y, x), anchor"""
    boxes, scores = [], []
    for c, r, b, s in zip(cls, reg, base, strides):
        sc = c.permute(1, 2, 0).reshape(-1, num_classes).softmax(-1)
        deltas = r.permute(1, 2, 0).reshape(-1, 4)
        anchors = grid_anchors(b.to(c.dtype), c.shape[-2:], s)
        boxes.append(delta2bbox(anchors, deltas, means, stds, img_shape))
        scores.append(sc)
    return torch.cat(boxes), torch.cat(scores)


def get_bboxes(cls, reg, metas, rescale, head=CASE_HEAD, num_classes=81, score_thr=SCORE_THR, iou_thr=IOU_THR,
               max_per_img=MAX_PER_IMG):
    """cls[l] (B, A_l * num_classes, H, W), reg[l] (B, A_l * 4, H, W) tensors -> per image
    (dets (k, 5), labels (k,), ids (k,)) numpy arrays"""
    base = base_anchors(**head)
    out = []
    for b, meta in enumerate(metas):
        boxes, scores = candidates_single([c[b] for c in cls], [r[b] for r in reg], base, head['anchor_strides'],
                                          num_classes, head['target_means'], head['target_stds'],
                                          meta['img_shape'])
        if rescale:
            sf = meta['scale_factor']
            boxes = boxes / boxes.new_tensor(np.asarray(sf, np.float64).reshape(-1))
        d, l, i = multiclass_nms(boxes, scores, score_thr, iou_thr, max_per_img)
        out.append((d.numpy(), l.numpy(), i.numpy()))
    return out


def canonical(dets, labels, ids):
    """rows ordered by (label, score descending, id): the order-free form two results are compared in"""
    order = np.lexsort((ids, -dets[:, 4].astype(np.float64), labels))
    return dets[order], labels[order], ids[order]


# ------------------------------------------------------------------ seeded inputs
def num_anchors(anchor_ratios):
    return [2 * len(r) + 2 for r in anchor_ratios]


def head_outputs(name):
    """the recorded case's head outputs from its seed: (cls[l] (B, A_l * nc, H, W), reg[l]) fp32 numpy.
    Background logit +9 on every row (the best foreground score then lies near 1e-3); `hot` rows per
    image, drawn over all rows, have one class lifted to a score between about 0.05 and 0.95."""
    case = CASES[name]
    rng = np.random.RandomState(case['seed'])
    nc, B = case['num_classes'], len(case['metas'])
    A = num_anchors(CASE_HEAD['anchor_ratios'])
    rows = [h * w * a for (h, w), a in zip(case['sizes'], A)]
    R = sum(rows)
    logits = rng.randn(B, R, nc).astype(np.float32)
    logits[:, :, 0] += 9.0
    for b in range(B):
        hot = rng.choice(R, case['hot'], replace=False)
        cls_id = rng.randint(1, nc, size=case['hot'])
        logits[b, hot, cls_id] = (9.0 + rng.uniform(-3.0, 3.0, size=case['hot'])).astype(np.float32)
    deltas = rng.randn(B, R, 4).astype(np.float32)
    cls, reg, off = [], [], 0
    for (h, w), a, n in zip(case['sizes'], A, rows):
        cls.append(np.ascontiguousarray(
            logits[:, off:off + n].reshape(B, h, w, a * nc).transpose(0, 3, 1, 2)))
        reg.append(np.ascontiguousarray(deltas[:, off:off + n].reshape(B, h, w, a * 4).transpose(0, 3, 1, 2)))
        off += n
    return cls, reg


def fill_state(state, seed):
    """fill a state dict (name -> tensor, in place) from `seed` by names and shapes only: He-scaled
    convolution weights, small biases, the L2Norm weight around its scale"""
    for k in sorted(state):
        v = state[k]
        rng = np.random.RandomState((seed + sum(ord(ch) * (i + 1) for i, ch in enumerate(k))) % (2 ** 31))
        if k.endswith('l2_norm.weight'):
            a = 20.0 + rng.uniform(-2, 2, size=tuple(v.shape))
        elif v.dim() == 4:
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]
            a = rng.randn(*v.shape) * np.sqrt(2.0 / fan_in)
        else:
            a = rng.uniform(-0.1, 0.1, size=tuple(v.shape))
        state[k] = torch.from_numpy(np.asarray(a)).to(v.dtype)
    return state
