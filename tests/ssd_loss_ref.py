"""Plain-torch restatement of SSD's training loss (any dtype, CPU): the targets of the SSD configs
(MaxIoUAssigner with pos_iou_thr = neg_iou_thr = 0.5, min_pos_iou = 0, gt_max_assign_all = False, no
sampling, bbox2delta), and per image the softmax cross-entropy with hard-negative mining and
smooth-L1 -- the yardstick of tests/test_host_ssd_loss.py and the GPU tests, and the regenerator of the
seeded inputs whose reference results tests/golden/make_golden_ssd_loss.py records.  Written from the
published definition; it shares no code with the package.

TIE RULE of the mining: with t the k-th largest loss among the negatives, a negative is selected when
its loss is above t, or equal to t and among the first k - #(loss > t) such rows in ascending row
order.  Here that is an explicit sort by (loss descending, row id ascending).  The loss value does not
depend on the rule.
"""
import numpy as np
import torch

import ssd_ref

MID_SIZES = [(19, 19), (10, 10), (5, 5), (3, 3), (2, 2), (1, 1)]
# a geometry whose 24 564 keys do not fit the mining kernel's LDS budget (12 288 rows), at 3 logits per row
BIG_SIZES = ssd_ref.SSD512_SIZES
NEG_POS_RATIO, BETA = 3, 1.0
POS_IOU = 0.5
HEAD = ssd_ref.CASE_HEAD
HEAD512 = dict(ssd_ref.ANCHOR_SETTINGS['ssd512_coco'], target_means=(.0, .0, .0, .0), target_stds=(0.1, 0.1, 0.2, 0.2))

# kinds of image: 'few' ground-truth boxes near anchors (k < num_neg); 'many' boxes laid on anchors, so many
# positives that 3 * num_pos > num_neg (k == num_neg); 'tie' as 'few', with the rows around the mining
# threshold given bit-identical logits (TIE_BELOW of them above the cut, TIE_ABOVE behind it)
CASES = {
    'small': dict(seed=4101, sizes=ssd_ref.SMALL_SIZES, num_classes=6, head=HEAD, kinds=('few', 'many', 'tie'),
                  pad=(300, 300)),
    'mid': dict(seed=4102, sizes=MID_SIZES, num_classes=81, head=HEAD, kinds=('few', 'few'), pad=(300, 300)),
    'ssd300': dict(seed=4103, sizes=ssd_ref.SSD300_SIZES, num_classes=81, head=HEAD, kinds=('few', 'tie'),
                   pad=(300, 300)),
    'big': dict(seed=4105, sizes=BIG_SIZES, num_classes=3, head=HEAD512, kinds=('few', 'tie'), pad=(512, 512)),
}
TIE_BELOW, TIE_ABOVE = 3, 4


# ------------------------------------------------------------------ targets
def all_anchors(head, sizes):
    base = ssd_ref.base_anchors(**head)
    return torch.cat([ssd_ref.grid_anchors(b, s, st) for b, s, st in zip(base, sizes, head['anchor_strides'])])


def overlaps(gt, anchors):
    """(G, R) IoU with the +1 pixel convention"""
    a1 = (gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1)
    a2 = (anchors[:, 2] - anchors[:, 0] + 1) * (anchors[:, 3] - anchors[:, 1] + 1)
    lt = torch.max(gt[:, None, :2], anchors[None, :, :2])
    rb = torch.min(gt[:, None, 2:], anchors[None, :, 2:])
    wh = (rb - lt + 1).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (a1[:, None] + a2[None] - inter)


def assign(ov):
    """(G, R) IoU -> (R,) 0 = negative, g + 1 = positive for gt g: the anchor's best gt where that IoU
    >= 0.5; then every gt takes its single best anchor, later gts over earlier ones"""
    best, arg = ov.max(0)
    out = torch.zeros(ov.shape[1], dtype=torch.long)
    pos = best >= POS_IOU
    out[pos] = arg[pos] + 1
    for g in range(ov.shape[0]):
        out[ov[g].argmax()] = g + 1
    return out


def targets_single(anchors, gt, gt_labels, means, stds):
    a = assign(overlaps(gt, anchors))
    pos = a > 0
    labels = torch.zeros(len(a), dtype=torch.long)
    labels[pos] = gt_labels[a[pos] - 1]
    bt = torch.zeros_like(anchors)
    bw = torch.zeros_like(anchors)
    p, g = anchors[pos], gt[a[pos] - 1]
    pw, ph = p[:, 2] - p[:, 0] + 1.0, p[:, 3] - p[:, 1] + 1.0
    gw, gh = g[:, 2] - g[:, 0] + 1.0, g[:, 3] - g[:, 1] + 1.0
    d = torch.stack([((g[:, 0] + g[:, 2]) * 0.5 - (p[:, 0] + p[:, 2]) * 0.5) / pw,
                     ((g[:, 1] + g[:, 3]) * 0.5 - (p[:, 1] + p[:, 3]) * 0.5) / ph,
                     torch.log(gw / pw), torch.log(gh / ph)], dim=-1)
    bt[pos] = (d - d.new_tensor(means)[None]) / d.new_tensor(stds)[None]
    bw[pos] = 1.0
    return labels, torch.ones(len(a), dtype=anchors.dtype), bt, bw


def targets(anchors, gts, gt_labels, means, stds):
    """-> labels (B, R) int64, label_weights (B, R), bbox_targets (B, R, 4), bbox_weights (B, R, 4),
    num_total_pos = sum over the images of max(num_pos, 1)"""
    per = [targets_single(anchors, g, l, means, stds) for g, l in zip(gts, gt_labels)]
    out = [torch.stack(t) for t in zip(*per)]
    return out + [int(sum(max(int((l > 0).sum()), 1) for l in out[0]))]


# ------------------------------------------------------------------ loss
def rows(maps, ch):
    """per-level (B, A_l * ch, H, W) -> (B, R, ch), rows in the order level, (y, x), anchor"""
    B = maps[0].shape[0]
    return torch.cat([m.permute(0, 2, 3, 1).reshape(B, -1, ch) for m in maps], 1)


def cross_entropy(x, labels):
    m = x.max(-1, keepdim=True)[0]
    lse = m[:, 0] + (x - m).exp().sum(-1).log()
    return lse - x.gather(1, labels[:, None])[:, 0]


def mine(ce, labels, ratio=NEG_POS_RATIO):
    """ce (R,), labels (R,) -> (selected bool (R,) with the positives set, num_pos, k)"""
    ce = ce.detach()
    neg = (labels == 0).nonzero().flatten()
    npos = int((labels > 0).sum())
    k = min(ratio * npos, len(neg))
    v = ce[neg].double().numpy() + 0.0
    neg = neg.numpy()
    order = np.lexsort((neg, -v))                # loss descending, then row id ascending
    sel = labels > 0
    sel[torch.from_numpy(neg[order[:k]])] = True
    return sel, npos, k


def loss_single(x, reg, labels, lw, bt, bw, avg, ratio=NEG_POS_RATIO, beta=BETA):
    ce = cross_entropy(x, labels) * lw
    sel, npos, k = mine(ce, labels, ratio)
    loss_cls = ce[sel].sum() / avg
    diff = (reg - bt).abs()
    l1 = torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta)
    return loss_cls, (l1 * bw).sum() / avg, sel, npos, k


def loss(cls, reg, labels, lw, bt, bw, avg, ratio=NEG_POS_RATIO, beta=BETA, grad_out=None):
    """per-level maps (leaf tensors are differentiated) + image-major targets -> dict: loss_cls (B,),
    loss_bbox (B,), sel (B, R) bool, counts (B, 2), and with grad_out ((B, 2) weights of the losses)
    grad_cls (B, R, C + 1), grad_reg (B, R, 4) in row order.  Everything in the dtype of the maps."""
    dt = cls[0].dtype
    cls = [c.detach().clone().requires_grad_(True) for c in cls]
    reg = [r.detach().clone().requires_grad_(True) for r in reg]
    B = cls[0].shape[0]
    nc = sum(c[0].numel() for c in cls) // labels.shape[1]
    xr, rr = rows(cls, nc), rows(reg, 4)
    out = dict(loss_cls=[], loss_bbox=[], sel=[], counts=[])
    for b in range(B):
        lc, lb, sel, npos, k = loss_single(xr[b], rr[b], labels[b], lw[b].to(dt), bt[b].to(dt), bw[b].to(dt), avg,
                                           ratio, beta)
        out['loss_cls'].append(lc); out['loss_bbox'].append(lb); out['sel'].append(sel); out['counts'].append((npos, k))
    res = dict(loss_cls=torch.stack(out['loss_cls']), loss_bbox=torch.stack(out['loss_bbox']),
               sel=torch.stack(out['sel']), counts=np.asarray(out['counts'], np.int64))
    if grad_out is not None:
        go = torch.as_tensor(grad_out, dtype=dt)
        total = (res['loss_cls'] * go[:, 0]).sum() + (res['loss_bbox'] * go[:, 1]).sum()
        total.backward()
        res['grad_cls'] = rows([c.grad for c in cls], nc)
        res['grad_reg'] = rows([r.grad for r in reg], 4)
    res['loss_cls'], res['loss_bbox'] = res['loss_cls'].detach(), res['loss_bbox'].detach()
    return res


# ------------------------------------------------------------------ seeded inputs
def to_maps(x, sizes, A):
    """(B, R, ch) numpy -> per-level (B, A_l * ch, H, W) contiguous numpy"""
    B, _, ch = x.shape
    out, off = [], 0
    for (h, w), a in zip(sizes, A):
        n = h * w * a
        out.append(np.ascontiguousarray(x[:, off:off + n].reshape(B, h, w, a * ch).transpose(0, 3, 1, 2)))
        off += n
    return out


def _gts(rng, kind, anchors, pad, nc):
    if kind == 'many':
        n = max(60, len(anchors) // 12)
        idx = rng.choice(len(anchors), n, replace=False)
        gt = anchors[idx].astype(np.float64) + rng.uniform(-0.9, 0.9, size=(n, 4))
    else:
        # a few anchors, every edge moved by up to a fifth of the anchor's size
        n = int(rng.randint(3, 8))
        a = anchors[rng.choice(len(anchors), n, replace=False)].astype(np.float64)
        size = np.tile(a[:, 2:] - a[:, :2] + 1, 2)
        gt = a + rng.uniform(-0.2, 0.2, size=(n, 4)) * size
    return gt.astype(np.float32), rng.randint(1, nc, size=n).astype(np.int64)


def inputs(name):
    """the case's inputs from its seed -> dict: anchors (R, 4), gt_bboxes / gt_labels (lists of tensors),
    metas, the targets (labels, label_weights, bbox_targets, bbox_weights, num_total_pos) and the head
    outputs cls[l] / reg[l] (fp32 tensors), `tie_rows` per image (row ids with bit-identical logits)"""
    case = CASES[name]
    rng = np.random.RandomState(case['seed'])
    head, sizes, nc = case['head'], case['sizes'], case['num_classes']
    A = ssd_ref.num_anchors(head['anchor_ratios'])
    anchors = all_anchors(head, sizes)
    R, B = anchors.shape[0], len(case['kinds'])
    gts, gls = zip(*[_gts(rng, k, anchors.numpy(), case['pad'], nc) for k in case['kinds']])
    gts, gls = [torch.from_numpy(g) for g in gts], [torch.from_numpy(l) for l in gls]
    tg = targets(anchors, gts, gls, head['target_means'], head['target_stds'])
    logits = (rng.randn(B, R, nc) * 2.0).astype(np.float32)
    logits[:, :, 0] += 2.0
    deltas = (rng.randn(B, R, 4) * 0.7).astype(np.float32)
    tie_rows = []
    for b, kind in enumerate(case['kinds']):
        tie = np.zeros(0, np.int64)
        if kind == 'tie':
            lab = tg[0][b].numpy()
            neg = np.nonzero(lab == 0)[0]
            k = NEG_POS_RATIO * int((lab > 0).sum())
            x = logits[b, neg].astype(np.float64)
            ce = np.log(np.exp(x - x.max(1, keepdims=True)).sum(1)) + x.max(1) - x[:, 0]
            order = np.argsort(-ce, kind='stable')
            tie = np.sort(neg[order[k - TIE_BELOW:k + TIE_ABOVE]])
            logits[b, tie] = logits[b, neg[order[k]]]
        tie_rows.append(tie)
    metas = [dict(img_shape=case['pad'] + (3,), pad_shape=case['pad'] + (3,), scale_factor=1.0, flip=False)] * B
    return dict(anchors=anchors, gt_bboxes=gts, gt_labels=gls, metas=metas, targets=tg, tie_rows=tie_rows,
                cls=[torch.from_numpy(c) for c in to_maps(logits, sizes, A)],
                reg=[torch.from_numpy(r) for r in to_maps(deltas, sizes, A)], A=A, R=R, B=B, num_classes=nc)


def margins(inp, b):
    """fp64 facts of image b the fixtures rest on -> dict: iou (smallest distance of an IoU from 0.5),
    best (smallest lead of a gt's best anchor over its second best), gap (k-th minus (k+1)-th largest
    negative loss; None when k == num_neg or k == 0), k, num_pos, num_neg"""
    ov = overlaps(inp['gt_bboxes'][b].double(), inp['anchors'].double())
    top2 = ov.topk(2, dim=1)[0]
    lab = inp['targets'][0][b]
    x = rows([c.double() for c in inp['cls']], inp['num_classes'])[b]
    ce = cross_entropy(x, lab)
    neg = ce[lab == 0].sort(descending=True)[0]
    npos = int((lab > 0).sum())
    k = min(NEG_POS_RATIO * npos, len(neg))
    gap = float(neg[k - 1] - neg[k]) if 0 < k < len(neg) else None
    return dict(iou=float((ov - POS_IOU).abs().min()), best=float((top2[:, 0] - top2[:, 1]).min()), gap=gap, k=k,
                num_pos=npos, num_neg=len(neg))
