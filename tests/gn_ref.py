"""A plain GroupNorm + ReLU over a list of pyramid levels, forward and backward, in any dtype: the
yardstick (fp64) and the precision reference (fp32) of the HIP training node
(csrc/groupnorm.hip, fcos_ops.groupnorm_relu; tests/test_gpu_groupnorm_train.py).

Per level x (B, C, H, W), statistics per (image, group) over C / groups x H x W values with a
two-pass variance (mean first, then the mean of the squared deviations: no E[x^2] - E[x]^2), torch
nn.GroupNorm semantics (biased variance, eps inside the root).  With xh = (x - mean) * rstd,
pre = xh * gamma + beta, g = dy * [pre > 0] and n = C / groups * H * W:

    dbeta_c = sum g,  dgamma_c = sum g * xh          over all pixels, images and levels
    dx = rstd * (gamma * g - mean_grp(gamma * g) - xh * mean_grp(gamma * g * xh))

`fault` evaluates the backward with one structural fault of the kind the gates must catch
(tests/test_host_gn_ref.py): 'lost_chunk' leaves the last CHUNK pixels of every level's image out of
the two group sums; 'level_dgamma' returns the parameter gradients of the last level alone."""
import torch

CHUNK = 256             # IA_GN_CHUNK: pixels per workgroup of the kernels
GATE_A = 1e-4           # the project's contract: every tensor within 1e-4 of its maximum
GATE_B = 4.0            # at most this multiple of the fp32 helper's error on the same tensors ...
FLOOR = 2.0 ** -22      # ... or this, for what the helper gets (almost) exactly
# (factor and floor of wino_ref.GATE_B / tests/test_gpu_fcos_loss.py)


def rel_err(got, ref):
    """max|got - ref| / max|ref| in fp64"""
    ref = ref.double()
    return float((got.to(ref.device).double() - ref).abs().max() / ref.abs().max())


def gate_b(helper_err):
    return max(GATE_B * helper_err, FLOOR)


def _stats(x, groups, eps):
    B, C, H, W = x.shape
    xg = x.reshape(B, groups, -1)
    mean = xg.mean(2, keepdim=True)
    var = ((xg - mean) ** 2).mean(2, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + eps)


def forward(xs, gamma, beta, groups, eps=1e-5, relu=True, dtype=torch.float64, pre=False):
    """-> ys (the pre-activations xh * gamma + beta with pre=True)"""
    gm, bt = gamma.to(dtype).view(1, -1, 1, 1), beta.to(dtype).view(1, -1, 1, 1)
    out = []
    for x in xs:
        x = x.to(dtype)
        mean, rstd = _stats(x, groups, eps)
        xh = ((x.reshape(x.shape[0], groups, -1) - mean) * rstd).reshape(x.shape)
        y = xh * gm + bt
        out.append(y if pre or not relu else y.clamp(min=0))
    return out


def backward(xs, dys, gamma, beta, groups, eps=1e-5, relu=True, dtype=torch.float64, fault=None):
    """-> (dxs, dgamma, dbeta)"""
    gm, bt = gamma.to(dtype).view(1, -1, 1, 1), beta.to(dtype).view(1, -1, 1, 1)
    dxs = []
    dgamma = torch.zeros(gamma.numel(), dtype=dtype)
    dbeta = torch.zeros(gamma.numel(), dtype=dtype)
    for x, dy in zip(xs, dys):
        x, dy = x.to(dtype), dy.to(dtype)
        B, C, H, W = x.shape
        mean, rstd = _stats(x, groups, eps)
        xh = ((x.reshape(B, groups, -1) - mean) * rstd).reshape(x.shape)
        g = dy * ((xh * gm + bt) > 0).to(dtype) if relu else dy
        lvl_dbeta, lvl_dgamma = g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))
        if fault == 'level_dgamma':
            dbeta, dgamma = lvl_dbeta, lvl_dgamma
        else:
            dbeta, dgamma = dbeta + lvl_dbeta, dgamma + lvl_dgamma
        n = C // groups * H * W
        a, b = gm * g, gm * g * xh
        if fault == 'lost_chunk' and H * W > 1:
            keep = torch.ones(H * W, dtype=dtype)
            keep[-min(CHUNK, H * W - 1):] = 0
            a, b = a * keep.view(1, 1, H, W), b * keep.view(1, 1, H, W)
        m1 = a.reshape(B, groups, -1).sum(2, keepdim=True) / n
        m2 = b.reshape(B, groups, -1).sum(2, keepdim=True) / n
        dx = rstd * ((gm * g).reshape(B, groups, -1) - m1 - xh.reshape(B, groups, -1) * m2)
        dxs.append(dx.reshape(x.shape))
    return dxs, dgamma, dbeta


def safe_upstream(xs, ups, gamma, beta, groups, eps=1e-5, margin=1e-4):
    """the upstream gradients with zeros where the fp64 pre-activation is within `margin` of its
    level's max-abs of zero: no mask that rounding could flip carries a gradient.
    -> (ups, the share of elements zeroed)"""
    pres = forward(xs, gamma, beta, groups, eps, dtype=torch.float64, pre=True)
    out, dropped, total = [], 0, 0
    for p, u in zip(pres, ups):
        near = p.abs() <= margin * p.abs().max()
        out.append(torch.where(near, torch.zeros_like(u), u))
        dropped += int(near.sum())
        total += near.numel()
    return out, dropped / total
