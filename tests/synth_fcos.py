"""Seeded synthetic inputs of the IoU-aware FCOS fixtures (tests/golden/fcos_*.npz,
tests/golden/make_golden_fcos.py): head outputs, gt boxes and "trained-like" name-seeded weights.
Both sides (the reference in the build container, this build on the GPU box) regenerate the
inputs from the seeds stored in the fixtures."""
import numpy as np

STRIDES = (8, 16, 32, 64, 128)
C = 80
FCOS_CLS_BIAS = -4.0


def level_shapes(pad_h, pad_w, strides=STRIDES):
    return [((pad_h + s - 1) // s, (pad_w + s - 1) // s) for s in strides]


def head_outputs(seed, batch, sizes, num_classes=C):
    """(cls, bbox, centerness, iou) per level, NCHW fp32: logits with a wide spread (few ties),
    positive distances (already exponentiated, as the head's forward returns them)"""
    rs = np.random.RandomState(seed)
    cls, reg, ctr, iou = [], [], [], []
    for l, (h, w) in enumerate(sizes):
        cls.append((rs.standard_normal((batch, num_classes, h, w)) * 2.0 - 3.0).astype(np.float32))
        reg.append(np.exp(rs.standard_normal((batch, 4, h, w)) * 0.6 + np.log(4.0 * STRIDES[l]))
                   .astype(np.float32))
        ctr.append(rs.standard_normal((batch, 1, h, w)).astype(np.float32))
        iou.append((rs.standard_normal((batch, 1, h, w)) * 1.5).astype(np.float32))
    return cls, reg, ctr, iou


def min_score_gap(cls, iou, alpha=0.3):
    """smallest distance between two distinct fused scores of one image (row maxima and every
    class column): the margin a reordering by rounding would have to cross"""
    gaps = []
    for b in range(cls[0].shape[0]):
        sc = np.concatenate([
            ((1 / (1 + np.exp(-c[b].astype(np.float64)))) ** alpha *
             (1 / (1 + np.exp(-i[b].astype(np.float64)))) ** (1 - alpha)).reshape(c.shape[1], -1)
            for c, i in zip(cls, iou)], axis=1)
        for v in list(sc) + [sc.max(0)]:
            s = np.sort(v[v > 0.04])
            if s.size > 1:
                gaps.append(np.diff(s).min())
    return float(min(gaps))


def gts(seed, batch, img_h, img_w, max_gt=6):
    """gt boxes (x1, y1, x2, y2) and labels 1..C per image; some boxes nested / overlapping so
    points lie in several gts"""
    rs = np.random.RandomState(seed)
    boxes, labels = [], []
    for _ in range(batch):
        g = rs.randint(2, max_gt + 1)
        x1 = rs.uniform(0, img_w * 0.6, g)
        y1 = rs.uniform(0, img_h * 0.6, g)
        bw = rs.uniform(8, img_w * 0.8, g)
        bh = rs.uniform(8, img_h * 0.8, g)
        b = np.stack([x1, y1, np.minimum(x1 + bw, img_w - 1), np.minimum(y1 + bh, img_h - 1)], 1)
        b[-1] = [b[0, 0] + 2, b[0, 1] + 2, b[0, 2] - 2, b[0, 3] - 2]     # nested in box 0
        boxes.append(np.round(b).astype(np.float32))
        labels.append(rs.randint(1, C + 1, g).astype(np.int64))
    return boxes, labels


def fill_state(state, seed):
    """fill an FCOS detector state dict (name -> tensor, in place) from `seed`; depends on names
    and shapes only (identical in the reference and in this build)."""
    import torch
    rs = np.random.RandomState(seed)
    for key in sorted(state.keys()):
        t = state[key]
        if key.endswith('num_batches_tracked'):
            continue
        shape = tuple(t.shape)
        leaf = key.split('.')[-1]
        if key.endswith('running_mean'):
            v = rs.standard_normal(shape) * 0.05
        elif key.endswith('running_var'):
            v = rs.uniform(0.8, 1.2, shape)
        elif t.dim() == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            gain = np.sqrt(2.0 / fan_in)
            if key.startswith('neck.'):
                gain = np.sqrt(1.0 / fan_in)
                if '.lateral_convs.' in key:
                    gain *= 0.125
            if '.fcos_cls.' in key or '.fcos_iou.' in key:
                gain = 1.5 * np.sqrt(1.0 / fan_in)
            if '.fcos_reg.' in key or '.fcos_centerness.' in key:
                gain = 0.3 * np.sqrt(1.0 / fan_in)
            v = rs.standard_normal(shape) * gain
        elif leaf == 'scale':
            v = rs.uniform(0.8, 1.2, shape)
        elif leaf == 'weight':                                   # BatchNorm / GroupNorm scale
            v = rs.uniform(0.8, 1.2, shape)
            if '.bn3.' in key:
                v = v * 0.25
        elif leaf == 'bias':
            v = rs.standard_normal(shape) * (0.05 if key.startswith('backbone.') else 0.02)
            if '.fcos_cls.' in key:
                v = FCOS_CLS_BIAS + rs.standard_normal(shape) * 0.5
            if '.fcos_reg.' in key:
                v = v + 2.5                                      # distances of ~12 * stride^0
        else:
            raise KeyError('fill_state: no rule for %s %s' % (key, shape))
        t.copy_(torch.from_numpy(np.asarray(v, np.float32)).reshape(t.shape))


def image(seed, batch, pad_h, pad_w, img_h, img_w):
    rs = np.random.RandomState(seed)
    img = rs.standard_normal((batch, 3, pad_h, pad_w)).astype(np.float32)
    img[:, :, img_h:, :] = 0
    img[:, :, :, img_w:] = 0
    return img
