"""float64 torch-autograd yardstick of the FCOS heads' loss (csrc/pointloss.hip), stated per positive
point and not per head: the centerness target c, the aligned (+1) IoU u of distance2bbox(point, pred)
and distance2bbox(point, target), the terms -log(u) c, BCE(ctr, c), BCE(iou, u), and the four
normalised losses of DESIGN.md "Loss formulas"

    loss_cls = focal sum / (n + B)      loss_reg = sum -log(u) c / sum c
    loss_centerness = sum BCE(ctr, c) / n      loss_iou = sum BCE(iou, u) / n     (u attached or not)

with the gradient of each with respect to every input (and scale_l, where the regression input is
raw: d = exp(scale_l x)).  Written with torch.max / torch.min / clamp(min=0) as
iouaware/bbox.py::bbox_overlaps is, so that autograd's conventions at a tie (half and half) and at a
clamp are the torch route's; u is not clamped.  n = 0: the positive-only losses and gradients are 0.
The focal term is synth_fcos_loss.onehot_focal."""
import numpy as np
import torch
import torch.nn.functional as F

import synth_fcos_loss as S

KEYS = ('loss_cls', 'loss_reg', 'loss_centerness', 'loss_iou')


def point_terms(pts, d, t, xc, xi=None, attach=True):
    """tensors of one dtype: pts (P, 2), distances d and targets t (P, 4), logits xc, xi (P,)
    -> c, u, (-log(u) c, BCE(xc, c), BCE(xi, u) or None), each (P,)"""
    lr, tb = t[:, [0, 2]], t[:, [1, 3]]
    c = torch.sqrt((lr.min(-1)[0] / lr.max(-1)[0]) * (tb.min(-1)[0] / tb.max(-1)[0]))

    def box(q):
        return torch.stack([pts[:, 0] - q[:, 0], pts[:, 1] - q[:, 1], pts[:, 0] + q[:, 2], pts[:, 1] + q[:, 3]], -1)
    p, g = box(d), box(t)
    wh = (torch.min(p[:, 2:], g[:, 2:]) - torch.max(p[:, :2], g[:, :2]) + 1).clamp(min=0)
    ov = wh[:, 0] * wh[:, 1]
    ap = (p[:, 2] - p[:, 0] + 1) * (p[:, 3] - p[:, 1] + 1)
    at = (g[:, 2] - g[:, 0] + 1) * (g[:, 3] - g[:, 1] + 1)
    u = ov / (ap + at - ov)
    reg = -u.log() * c
    ctr = F.binary_cross_entropy_with_logits(xc, c, reduction='none')
    iou = None
    if xi is not None:
        iou = F.binary_cross_entropy_with_logits(xi, u if attach else u.detach(), reduction='none')
    return c, u, (reg, ctr, iou)


def evaluate(pos, cls, labels, batch, scales=None, attach=True, with_iou=True, gamma=2.0, alpha=0.25,
             grads=True, dtype=torch.float64):
    """pos: numpy arrays of the P positive points -- 'pts' (P, 2), 'reg' (P, 4) (distances; with
    `scales` (L,) the raw x of d = exp(scales[level] x)), 'level' (P,), 'tgt' (P, 4), 'ctr' (P,),
    'iou' (P,); cls (N, C) logits and labels (N,) of EVERY point.
    -> dict(c, u, terms {key: (P,)}, losses {key: float}, grads {key: {kind: array}}): kinds 'cls' (N, C),
    'reg' (P, 4), 'ctr' (P,), 'iou' (P,), 'scale' (L,); the gradient of each normalised loss on its own."""
    T = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)   # noqa: E731
    leaves = dict(cls=T(cls), reg=T(pos['reg']).reshape(-1, 4), ctr=T(pos['ctr']).reshape(-1))
    if with_iou:
        leaves['iou'] = T(pos['iou']).reshape(-1)
    if scales is not None:
        leaves['scale'] = T(scales)
    for v in leaves.values():
        v.requires_grad_(True)
    P = leaves['reg'].shape[0]
    d = leaves['reg']
    if scales is not None:
        lvl = torch.from_numpy(np.asarray(pos['level'], np.int64))
        d = (leaves['scale'][lvl][:, None] * d).exp()
    c, u, (reg, ctr, iou) = point_terms(T(pos['pts']).reshape(-1, 2), d, T(pos['tgt']).reshape(-1, 4),
                                        leaves['ctr'], leaves.get('iou'), attach)
    focal = S.onehot_focal(leaves['cls'], torch.from_numpy(np.asarray(labels, np.int64)), gamma, alpha)
    zero = leaves['reg'].sum() * 0
    losses = dict(loss_cls=focal.sum() / (P + batch),
                  loss_reg=reg.sum() / c.sum() if P else zero,
                  loss_centerness=ctr.sum() / P if P else zero)
    terms = dict(loss_reg=reg, loss_centerness=ctr)
    if with_iou:
        losses['loss_iou'] = iou.sum() / P if P else zero
        terms['loss_iou'] = iou
    out = dict(c=c.detach().numpy(), u=u.detach().numpy(),
               terms={k: v.detach().numpy() for k, v in terms.items()},
               losses={k: float(v.detach()) for k, v in losses.items()}, grads=None)
    if grads:
        out['grads'] = {}
        names = list(leaves)
        for k, v in losses.items():
            gs = torch.autograd.grad(v, [leaves[n] for n in names], allow_unused=True, retain_graph=True)
            out['grads'][k] = {n: (np.zeros(tuple(leaves[n].shape)) if g is None else g.double().numpy())
                               for n, g in zip(names, gs)}
    return out


# ------------------------------------------------------------------ per-level maps <-> positive points
def gather(sizes, labels, targets, outs, strides=S.STRIDES):
    """labels[L] (B, N_l), targets[L] (B, N_l, 4) (synth_fcos_loss.np_targets), outs = (cls, reg, ctr
    [, iou]) per-level NCHW arrays -> (pos dict of `evaluate` plus 'b', 'p' (P,), level-major and
    image-major inside a level; flat cls (N, C); flat labels (N,))"""
    pts = S.points(sizes, np.float64, strides)
    keys = ('pts', 'reg', 'level', 'tgt', 'ctr', 'iou', 'b', 'p')
    acc = {k: [] for k in keys}
    fc, fl = [], []
    for l in range(len(sizes)):
        B = labels[l].shape[0]
        b, p = np.nonzero(labels[l] > 0)
        flat = lambda m: np.asarray(m[l], np.float64).reshape(B, m[l].shape[1], -1)   # noqa: E731
        acc['pts'].append(pts[l][p])
        acc['reg'].append(flat(outs[1])[b, :, p])
        acc['level'].append(np.full(len(b), l, np.int64))
        acc['tgt'].append(np.asarray(targets[l], np.float64)[b, p])
        acc['ctr'].append(flat(outs[2])[b, 0, p])
        acc['iou'].append(flat(outs[3])[b, 0, p] if len(outs) > 3 else np.zeros(len(b)))
        acc['b'].append(b)
        acc['p'].append(p)
        fc.append(flat(outs[0]).transpose(0, 2, 1).reshape(-1, outs[0][l].shape[1]))
        fl.append(labels[l].reshape(-1))
    return {k: np.concatenate(v) for k, v in acc.items()}, np.concatenate(fc), np.concatenate(fl)


def scatter(pos, g, sizes, batch):
    """the gradients {kind: array} of `evaluate` -> {kind: [L] NCHW float64 maps} ('scale' as it is)"""
    out = {}
    off = 0
    for kind, ch in (('cls', None), ('reg', 4), ('ctr', 1), ('iou', 1)):
        if kind not in g:
            continue
        maps = []
        for l, (h, w) in enumerate(sizes):
            if kind == 'cls':
                n = batch * h * w
                maps.append(g['cls'][off:off + n].reshape(batch, h, w, -1).transpose(0, 3, 1, 2).copy())
                off += n
                continue
            m = np.zeros((batch, ch, h * w))
            sel = pos['level'] == l
            m[pos['b'][sel], :, pos['p'][sel]] = g[kind][sel].reshape(-1, ch)
            maps.append(m.reshape(batch, ch, h, w))
        out[kind] = maps
    if 'scale' in g:
        out['scale'] = g['scale']
    return out


def yardstick_maps(sizes, labels, targets, outs, scales=None, attach=True, with_iou=True, gamma=2.0,
                   alpha=0.25, strides=S.STRIDES):
    """`evaluate` on per-level maps -> (losses {key: float}, grads {key: {kind: [L] maps}}, pos, raw result)"""
    outs = outs[:4 if with_iou else 3]
    pos, fc, fl = gather(sizes, labels, targets, outs, strides)
    B = labels[0].shape[0]
    r = evaluate(pos, fc, fl, B, scales, attach, with_iou, gamma, alpha)
    return r['losses'], {k: scatter(pos, g, sizes, B) for k, g in r['grads'].items()}, pos, r


def combine(grads, weights, keys=KEYS):
    """sum_k weights[k] * (gradient maps of loss k): what the node returns for upstream `weights`"""
    out = {}
    for w, k in zip(weights, keys):
        if k not in grads:
            continue
        for kind, v in grads[k].items():
            add = [w * m for m in v] if isinstance(v, list) else w * v
            if kind not in out:
                out[kind] = add
            elif isinstance(v, list):
                out[kind] = [a + b for a, b in zip(out[kind], add)]
            else:
                out[kind] = out[kind] + add
    return out
