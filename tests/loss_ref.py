"""The yardstick of the anchor-head losses: float64, torch autograd, no project code.

The functions take the layouts of the HIP kernels in csrc/loss.hip / csrc/headloss.hip -- NCHW head
outputs (B, A*K, H, W), targets (B, H*W*A[, 4]) in the reference's row order n = p*A + a, the
base anchors of one level, its stride, target means / stds -- and restate what the reference
computes on the rows `map.permute(0, 2, 3, 1).reshape(-1, K)`:

    iou_bce     delta2bbox (core/bbox/transforms.py:44-78) of prediction and target with the same
                anchor, aligned bbox_overlaps (core/bbox/geometry.py:34-47), BCE-with-logits
                against the IoU, attached or detached (iou_aware_retina_head.py:256-259,276-281)
    smooth_l1   weighted_smoothl1 / weighted_iou_balanced_smoothl1 (core/loss/losses.py:385-458)
    focal       py_sigmoid_focal_loss / iou_balanced_sigmoid_focal_loss (losses.py:226-374)

Inputs are float32 (or bf16-rounded float32) arrays; every one is widened to float64 first, and
so are the fp32 scalars the kernels receive (beta, alpha, 1 - alpha, max_ratio, means, stds), so
that a knee or a clamp sits at the same number on both sides.  Each function returns the SUM of
the elementwise loss and the gradients of gscale * sum.

Nothing at a non-differentiable point is written out: torch.max / torch.min split a tie 0.5 / 0.5,
clamp passes the gradient at its bound, torch.where(d < beta, ...) takes the linear branch at
d == beta -- the conventions csrc/ia_loss.hpp documents are autograd's own.

focal forms 1 - sigmoid(x) as sigmoid(-x) and the cross entropy as softplus (logaddexp): both stay
normal float64 numbers without cancellation for |x| <= 110 (sigmoid(-110) = 1.7e-48), so pt ** gamma
and its derivative are finite for every gamma > 0.  (1 - sigmoid(x) by subtraction is exactly 0
above x = 37, and 0 ** (gamma - 1) * 0 is NaN for gamma < 1.)
"""
import numpy as np
import torch

MAX_RATIO = float(np.float32(4.135166556742356))      # |log(16 / 1000)| as the kernels hold it


def f64(a):
    if torch.is_tensor(a):
        return a.detach().cpu().to(torch.float64)
    return torch.from_numpy(np.array(a, copy=True)).to(torch.float64)


def _f32s(v):
    """a python scalar / sequence as the fp32 numbers a kernel receives, widened"""
    return torch.from_numpy(np.asarray(v, np.float32).astype(np.float64))


def rows(m, A):
    """(B, A*K, H, W) -> (B, H*W, A, K): the reference's permute(0, 2, 3, 1).reshape"""
    B, ch, H, W = m.shape
    return m.permute(0, 2, 3, 1).reshape(B, H * W, A, ch // A)


def grid_anchors(base, H, W, stride):
    """base (A, 4) -> (H*W, A, 4), position-major like AnchorGenerator.grid_anchors"""
    base = f64(base)
    p = torch.arange(H * W)
    sx = ((p % W) * stride).to(torch.float64)
    sy = ((p // W) * stride).to(torch.float64)
    return base[None, :, :] + torch.stack([sx, sy, sx, sy], 1)[:, None, :]


def delta2bbox(anc, d, means, stds):
    d = d * stds + means
    dx, dy = d[..., 0], d[..., 1]
    dw = d[..., 2].clamp(min=-MAX_RATIO, max=MAX_RATIO)
    dh = d[..., 3].clamp(min=-MAX_RATIO, max=MAX_RATIO)
    px = (anc[..., 0] + anc[..., 2]) * 0.5
    py = (anc[..., 1] + anc[..., 3]) * 0.5
    pw = anc[..., 2] - anc[..., 0] + 1.0
    ph = anc[..., 3] - anc[..., 1] + 1.0
    gw = pw * dw.exp()
    gh = ph * dh.exp()
    gx = px + pw * dx
    gy = py + ph * dy
    return torch.stack([gx - gw * 0.5 + 0.5, gy - gh * 0.5 + 0.5,
                        gx + gw * 0.5 - 0.5, gy + gh * 0.5 - 0.5], -1)


def aligned_iou(b1, b2):
    lt = torch.max(b1[..., :2], b2[..., :2])
    rb = torch.min(b1[..., 2:], b2[..., 2:])
    wh = (rb - lt + 1).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    area1 = (b1[..., 2] - b1[..., 0] + 1) * (b1[..., 3] - b1[..., 1] + 1)
    area2 = (b2[..., 2] - b2[..., 0] + 1) * (b2[..., 3] - b2[..., 1] + 1)
    return overlap / (area1 + area2 - overlap)


def _softplus(z):
    return torch.logaddexp(z, torch.zeros_like(z))


def iou_bce(bbox_pred, iou_pred, bbox_targets, bbox_weights, base, stride, means=(0, 0, 0, 0),
            stds=(1, 1, 1, 1), gscale=1.0, attach=True):
    """-> dict(sum, iou (B, HW*A), g_iou (B, A, H, W), g_box (B, A*4, H, W) or None)"""
    reg = f64(bbox_pred).requires_grad_(True)
    xl_map = f64(iou_pred).requires_grad_(True)
    B, A, H, W = xl_map.shape
    bt = f64(bbox_targets).reshape(B, H * W, A, 4)
    w = f64(bbox_weights).reshape(B, H * W, A, 4)[..., 0]
    means, stds = _f32s(means), _f32s(stds)
    anc = grid_anchors(base, H, W, stride)[None]
    pred_box = delta2bbox(anc, rows(reg, A), means, stds)
    target_box = delta2bbox(anc, bt, means, stds)
    iou = aligned_iou(target_box, pred_box)
    t = iou if attach else iou.detach()
    xl = rows(xl_map, A)[..., 0]
    # binary_cross_entropy_with_logits for a soft target: (1 - t) x + softplus(-x)
    loss = ((1 - t) * xl + _softplus(-xl)) * w
    s = loss.sum()
    g_iou, g_box = torch.autograd.grad(s * gscale, [xl_map, reg], allow_unused=True)
    return dict(sum=float(s.detach()), iou=iou.detach().reshape(B, -1), g_iou=g_iou,
                g_box=g_box if attach else None)


def smooth_l1(pred, target, weight, A, beta, gscale=1.0, iou=None, delta=None):
    """iou / delta: the IoU-balanced form, weight * iou ** delta (detached).  -> dict(sum, grad)"""
    reg = f64(pred).requires_grad_(True)
    B, ch, H, W = reg.shape
    tg = f64(target).reshape(B, H * W, A, 4)
    w = f64(weight).reshape(B, H * W, A, 4)
    if iou is not None:
        w = w * f64(iou).reshape(B, H * W, A, 1).pow(float(np.float32(delta)))
    beta = float(np.float32(beta))
    d = (rows(reg, A) - tg).abs()
    loss = torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta)
    s = (loss * w).sum()
    g, = torch.autograd.grad(s * gscale, [reg])
    return dict(sum=float(s.detach()), grad=g)


def focal(cls, labels, label_weights, A, gamma=2.0, alpha=0.25, gscale=1.0, iou=None, eta=None):
    """labels (B, HW*A) in 0..C (0 = background), label_weights (B, HW*A).
    iou / eta: iou_balanced_sigmoid_focal_loss (the IoU_balanced_Cls branch).
    -> dict(sum, grad (B, A*C, H, W), sums3 = [S0, S1, S2] of the balanced form or None)"""
    x_map = f64(cls).requires_grad_(True)
    B, ch, H, W = x_map.shape
    Cn = ch // A
    x = rows(x_map, A)
    lab = torch.from_numpy(np.array(labels, copy=True)).reshape(B, H * W, A, 1).to(torch.int64)
    t = (lab == torch.arange(1, Cn + 1).reshape(1, 1, 1, Cn)).to(torch.float64)
    lw = f64(label_weights).reshape(B, H * W, A, 1)
    a_pos = float(np.float32(alpha))
    a_neg = float(np.float32(1.0 - alpha))
    gamma = float(np.float32(gamma))
    p, q = torch.sigmoid(x), torch.sigmoid(-x)
    pt = q * t + p * (1 - t)
    weight = (a_pos * t + a_neg * (1 - t)) * lw
    bce = _softplus(-x) * t + _softplus(x) * (1 - t)
    loss1 = bce * (weight * pt.pow(gamma))
    sums3 = None
    if iou is None:
        s = loss1.sum()
    else:
        iw = (t * f64(iou).reshape(B, H * W, A, 1)).pow(float(np.float32(eta)))
        loss2 = loss1 * ((1 - t) + iw)
        normalizer = (loss1 * t).sum() / ((loss2 * t).sum() + 1e-6)
        s = (loss1 * ((1 - t) + iw * normalizer).detach()).sum()
        sums3 = [float(v.detach().sum()) for v in (loss1 * (1 - t), loss1 * t, loss2 * t)]
    g, = torch.autograd.grad(s * gscale, [x_map])
    return dict(sum=float(s.detach()), grad=g, sums3=sums3)
