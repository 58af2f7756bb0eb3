"""The yardstick of BalancedL1Loss: float64, torch autograd, no project code, in the layouts of
tests/loss_ref.py (NCHW deltas (B, A*4, H, W), targets / weights (B, H*W*A, 4) in the reference's row
order).  It restates weighted_balanced_l1_loss (reference core/loss/losses.py:482-520): with
d = |pred - target| and b = e^(gamma / alpha) - 1,

    d < beta:   alpha / b * (b d + 1) * log(b d / beta + 1) - alpha d
    otherwise:  gamma d + gamma / b - alpha beta

times the weight.  Inputs are float32 (or bf16-rounded float32) arrays widened to float64; beta, alpha
and gamma widen from the fp32 numbers the kernels receive, so that the knee sits at the same number on
both sides.  torch.where(d < beta, ...) takes the linear branch at d == beta and abs() has gradient 0
at 0: autograd's conventions are the reference's.  Returns the SUM and the gradient of gscale * sum.

`evaluate(dtype=torch.float32)` is the same expression in plain float32 torch -- the reference's own
arithmetic -- whose distance from the float64 result is the error table E_ref the GPU bars rest on.
"""
import math

import numpy as np
import torch

from loss_ref import f64, rows


def evaluate(pred, target, weight, A, beta, alpha, gamma, gscale=1.0, dtype=torch.float64):
    """-> dict(sum (python float), grad (B, A*4, H, W) of gscale * sum, in `dtype`)"""
    reg = f64(pred).to(dtype).requires_grad_(True)
    B, ch, H, W = reg.shape
    tg = f64(target).to(dtype).reshape(B, H * W, A, 4)
    w = f64(weight).to(dtype).reshape(B, H * W, A, 4)
    beta, alpha, gamma = (float(np.float32(v)) for v in (beta, alpha, gamma))
    b = math.e ** (gamma / alpha) - 1
    d = (rows(reg, A) - tg).abs()
    loss = torch.where(d < beta, alpha / b * (b * d + 1) * torch.log(b * d / beta + 1) - alpha * d,
                       gamma * d + gamma / b - alpha * beta)
    s = (loss * w).sum()
    g, = torch.autograd.grad(s * gscale, [reg])
    return dict(sum=float(s.detach()), grad=g)


def balanced_l1(pred, target, weight, A, beta, alpha=0.5, gamma=1.5, gscale=1.0):
    return evaluate(pred, target, weight, A, beta, alpha, gamma, gscale, torch.float64)
