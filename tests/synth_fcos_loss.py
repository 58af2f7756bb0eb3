"""Seeded inputs and yardsticks of the FCOS training kernels (tests/test_*_fcos_loss.py,
tests/golden/make_golden_fcos_loss.py): fractional gt boxes that put positives on every pyramid
level, a numpy evaluation of the point targets (any dtype, lowest index on equal areas), the
conditions the comparisons rest on, and the torch `_loss` body as the fp64 yardstick."""
import contextlib

import numpy as np

import synth_fcos

STRIDES = synth_fcos.STRIDES
RANGES = ((-1, 64), (64, 128), (128, 256), (256, 512), (512, 1e8))
INF = 1e8
C = synth_fcos.C

# (name, pad h, pad w, img h, img w, batch, gt seed, gts per image from..to, head-output seed)
MAIN = ('main', 800, 1344, 800, 1333, 4, 31, 8, 40, 41)
SMALL = ('small', 128, 160, 120, 150, 2, 33, 3, 8, 43)
# the first image of MAIN alone (what fits the fixture's size cap with every target row)
MAIN1 = ('main1', 800, 1344, 800, 1333, 1, 31, 8, 40, 41)


def gts(seed, batch, img_h, img_w, gmin, gmax, num_classes=C):
    """fractional gt boxes: side log-uniform in [8, 0.9 min(h, w)], aspect log-uniform in
    [e^-0.7, e^0.7], anywhere inside the image; labels 1..C"""
    rs = np.random.RandomState(seed)
    boxes, labels = [], []
    for _ in range(batch):
        g = rs.randint(gmin, gmax + 1)
        side = np.exp(rs.uniform(np.log(8.0), np.log(0.9 * min(img_h, img_w)), g))
        asp = np.exp(rs.uniform(-0.7, 0.7, g))
        bw = np.minimum(side * np.sqrt(asp), img_w - 2.0)
        bh = np.minimum(side / np.sqrt(asp), img_h - 2.0)
        x1 = rs.uniform(0, 1, g) * (img_w - 1 - bw)
        y1 = rs.uniform(0, 1, g) * (img_h - 1 - bh)
        boxes.append(np.stack([x1, y1, x1 + bw, y1 + bh], 1).astype(np.float32))
        labels.append(rs.randint(1, num_classes + 1, g).astype(np.int64))
    return boxes, labels


def case_inputs(case):
    """-> sizes, gt boxes, gt labels, (cls, reg, ctr, iou) numpy head outputs"""
    _, ph, pw, ih, iw, B, gseed, gmin, gmax, hseed = case
    sizes = synth_fcos.level_shapes(ph, pw)
    gb, gl = gts(gseed, B, ih, iw, gmin, gmax)
    return sizes, gb, gl, synth_fcos.head_outputs(hseed, B, sizes)


def points(sizes, dtype, strides=STRIDES):
    out = []
    for (h, w), s in zip(sizes, strides):
        y, x = np.meshgrid(np.arange(h) * s, np.arange(w) * s, indexing='ij')
        out.append((np.stack([x.reshape(-1), y.reshape(-1)], -1) + s // 2).astype(dtype))
    return out


def np_targets(sizes, gb, gl, dtype=np.float32, ranges=RANGES, strides=STRIDES):
    """fcos_target in numpy, every operation in `dtype`: -> labels[L] (B, N_l) int64,
    bbox_targets[L] (B, N_l, 4).  np.argmin takes the first (lowest-index) minimum."""
    pts = points(sizes, dtype, strides)
    labels = [[] for _ in sizes]
    targets = [[] for _ in sizes]
    for b, lab in zip(gb, gl):
        b = b.astype(dtype)
        one = dtype(1)
        area = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
        for l, p in enumerate(pts):
            lo, hi = dtype(ranges[l][0]), dtype(ranges[l][1])
            d = np.stack([p[:, 0, None] - b[None, :, 0], p[:, 1, None] - b[None, :, 1],
                          b[None, :, 2] - p[:, 0, None], b[None, :, 3] - p[:, 1, None]], -1)
            mx = d.max(-1)
            cand = (d.min(-1) > 0) & (mx >= lo) & (mx <= hi)
            a = np.where(cand, area[None], dtype(INF))
            arg = a.argmin(1)
            amin = a[np.arange(len(p)), arg]
            labels[l].append(np.where(amin == dtype(INF), 0, lab[arg]).astype(np.int64))
            targets[l].append(d[np.arange(len(p)), arg])
    return [np.stack(x) for x in labels], [np.stack(x) for x in targets]


def check_conditions(sizes, gb, gl, min_pos_per_level=0):
    """what the comparisons rest on: pairwise different fp32 areas per image, and no label that
    differs between the fp32 and the fp64 evaluation.  -> positives per level"""
    for b in gb:
        area = (b[:, 2] - b[:, 0] + np.float32(1)) * (b[:, 3] - b[:, 1] + np.float32(1))
        assert len(np.unique(area)) == len(area), 'two gts of equal area'
    l32, _ = np_targets(sizes, gb, gl, np.float32)
    l64, _ = np_targets(sizes, gb, gl, np.float64)
    for a, b in zip(l32, l64):
        assert np.array_equal(a, b), 'a label sits on a rounding edge'
    pos = [int((a > 0).sum()) for a in l32]
    assert min(pos) >= min_pos_per_level, pos
    return pos


def edge_ties(sizes, labels, targets, reg, strides=STRIDES):
    """number of positive points whose predicted box has an edge exactly on the target box's edge
    (where max / min have no unique sub-gradient), fp32"""
    ties = 0
    for l, p in enumerate(points(sizes, np.float32, strides)):
        B = labels[l].shape[0]
        d = reg[l].reshape(B, 4, -1).transpose(0, 2, 1)
        t = targets[l].astype(np.float32)
        pos = labels[l] > 0
        sgn = (-1, -1, 1, 1)
        for k in range(4):
            c = p[None, :, k % 2]
            ties += int(((c + sgn[k] * d[..., k]) == (c + sgn[k] * t[..., k]))[pos].sum())
    return ties


# ------------------------------------------------------------------ the torch route as yardstick
def onehot_focal(pred, target, gamma, alpha, reduction='none'):
    """the quantity the focal op defines: the sigmoid focal loss on the one-hot of the integer
    targets, any dtype, in torch ops"""
    import torch
    import torch.nn.functional as F
    onehot = torch.zeros_like(pred)
    pos = torch.nonzero(target >= 1).squeeze(1)
    onehot[pos, target[pos] - 1] = 1
    p = pred.sigmoid()
    pt = (1 - p) * onehot + p * (1 - onehot)
    w = (alpha * onehot + (1 - alpha) * (1 - onehot)) * pt.pow(gamma)
    loss = F.binary_cross_entropy_with_logits(pred, onehot, reduction='none') * w
    assert reduction == 'none'
    return loss


@contextlib.contextmanager
def torch_route(cpu_focal=False, detach_iou_target=False):
    """inside: the heads' `_loss` torch body runs with the one-hot focal formula instead of the HIP
    op (cpu_focal) and / or with the IoU target detached"""
    from iouaware import fcos_head
    saved = fcos_head.sigmoid_focal_loss, fcos_head.bbox_overlaps
    if cpu_focal:
        fcos_head.sigmoid_focal_loss = onehot_focal
    if detach_iou_target:
        fcos_head.bbox_overlaps = lambda *a, **k: saved[1](*a, **k).detach()
    try:
        yield
    finally:
        fcos_head.sigmoid_focal_loss, fcos_head.bbox_overlaps = saved


def make_head(iou_branch, fuse, **kw):
    from iouaware.fcos_head import FCOSHead, IoUawareFCOSHead
    args = dict(num_classes=C + 1, in_channels=32, feat_channels=32, stacked_convs=1,
                strides=STRIDES, regress_ranges=RANGES)
    args.update(kw)
    head = (IoUawareFCOSHead if iou_branch else FCOSHead)(**args)
    head.fuse_loss = fuse
    return head


def head_loss(head, outs, gb, gl, gamma=2.0, alpha=0.25):
    """head.loss on per-level output lists (cls, reg, ctr[, iou]) -> the loss dict"""
    from iouaware.config import ConfigDict
    cfg = ConfigDict(dict(gamma=gamma, alpha=alpha))
    return head.loss(*(list(outs) + [gb, gl, None, cfg]))


def yardstick(iou_branch, outs_np, gb, gl, gamma=2.0, alpha=0.25, detach_iou_target=False,
              grad_of=None):
    """the torch `_loss` body in fp64 on the CPU.  -> (losses {key: float}, grads {key: [L arrays]} of
    `grad_of` (a loss key, or 'sum') with respect to every head output)"""
    import torch
    outs = [[torch.from_numpy(x).double().requires_grad_(True) for x in m]
            for m in outs_np[:4 if iou_branch else 3]]
    head = make_head(iou_branch, False)
    with torch_route(cpu_focal=True, detach_iou_target=detach_iou_target):
        losses = head_loss(head, outs, [torch.from_numpy(b).double() for b in gb],
                           [torch.from_numpy(x) for x in gl], gamma, alpha)
    vals = {k: float(v.detach().sum()) for k, v in losses.items()}
    grads = None
    if grad_of is not None:
        tgt = sum(v.sum() for v in losses.values()) if grad_of == 'sum' else losses[grad_of].sum()
        flat = [t for m in outs for t in m]
        gs = torch.autograd.grad(tgt, flat, allow_unused=True)
        L = len(outs[0])
        gs = [np.zeros(t.shape) if g is None else g.numpy() for g, t in zip(gs, flat)]
        grads = {k: gs[i * L:(i + 1) * L] for i, k in enumerate(('cls', 'reg', 'ctr', 'iou')[:len(outs)])}
    return vals, grads
