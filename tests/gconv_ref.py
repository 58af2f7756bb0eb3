"""The yardstick of the grouped 3x3 training node (iouaware/train_fuse.py: grouped_conv3x3_train;
csrc/gconv.hip, csrc/gconv_bwd.hip): torch autograd of F.conv2d(x, w, b, stride, 1, groups=g) on the
CPU, in fp64 as the definition and in fp32 as "what a plain fp32 evaluation of the same sums loses".
Test-only, nothing imported from the project.  The gates are the project's own (tests/wino_ref.py:
gates, GATE_A, GATE_B, the helper's error floored at one fp32 unit roundoff).

With the ReLU the yardstick takes the mask from the NODE's output (y > 0): a sign flip of a value
within rounding of zero is not a gradient error; y itself is checked separately against relu(conv).

`input_grad` restates the input gradient as the gather the stride-2 kernel performs, with switches
for the nearest wrong variants (taps not flipped, group block not transposed, terms of a missing
output row / column clamped instead of masked), so that a host test can show that the test inputs
tell them apart."""
import torch
import torch.nn.functional as F


def _cpu(t, dtype):
    return None if t is None else t.detach().to('cpu', dtype).contiguous()


def out_size(n, stride):
    return (n - 1) // stride + 1


def conv(x, w, b, stride, groups, dtype=torch.float64):
    """conv(x, w, stride, pad 1, groups) + b before the ReLU -> CPU tensor of `dtype`"""
    return F.conv2d(_cpu(x, dtype), _cpu(w, dtype), _cpu(b, dtype), stride, 1, groups=groups)


def conv_per_group(x, w, b, stride, groups, dtype=torch.float64):
    """the same map as `groups` ungrouped convolutions, one per slice of the channels"""
    x, w, b = _cpu(x, dtype), _cpu(w, dtype), _cpu(b, dtype)
    cg = w.shape[1]
    co = w.shape[0] // groups
    ys = [F.conv2d(x[:, g * cg:(g + 1) * cg], w[g * co:(g + 1) * co],
                   None if b is None else b[g * co:(g + 1) * co], stride, 1) for g in range(groups)]
    return torch.cat(ys, 1)


def conv_train(x, w, b, dy, stride, groups, relu, dtype=torch.float64, mask=None):
    """y = relu?(conv + b) and the gradients of <y, dy> w.r.t. x, w and b -> dict(y=, dx=, dW=,
    db= [None without b]) of CPU tensors of `dtype`.  mask (with relu): the positions where the
    gradient passes (the node's y > 0); default: the yardstick's own y > 0."""
    x = _cpu(x, dtype).requires_grad_(True)
    w = _cpu(w, dtype).requires_grad_(True)
    b = None if b is None else _cpu(b, dtype).requires_grad_(True)
    z = F.conv2d(x, w, b, stride, 1, groups=groups)
    dz = _cpu(dy, dtype)
    y = z.detach()
    if relu:
        y = y.clamp(min=0)
        m = (z.detach() > 0) if mask is None else mask.detach().to('cpu')
        dz = dz * m.to(dtype)
    leaves = [x, w] + ([b] if b is not None else [])
    grads = torch.autograd.grad((z * dz).sum(), leaves)
    return dict(y=y, dx=grads[0], dW=grads[1], db=grads[2] if b is not None else None)


def adjoint_weight(w, groups):
    """(C, Cg, 3, 3) -> the weight of the input-gradient convolution, same shape: taps flipped in
    both directions, input and output channel swapped inside each group (square groups)"""
    C, cg = w.shape[:2]
    assert C == groups * cg
    return w.reshape(groups, cg, cg, 3, 3).transpose(1, 2).flip(3, 4).reshape(C, cg, 3, 3).contiguous()


def input_grad(dz, w, stride, groups, H, W, flip=True, transpose=True, clamp=False):
    """dx (B, C, H, W) from dz (B, C, Ho, Wo) in gather form: input pixel (y, x) sums, over the taps
    (ky, kx) with (y + 1 - ky) and (x + 1 - kx) divisible by the stride, dz at the output pixel
    ((y + 1 - ky) / s, (x + 1 - kx) / s) times W[o][i][ky][kx].  The right evaluation has
    flip = transpose = True, clamp = False.  flip=False reads tap (2 - ky, 2 - kx); transpose=False
    swaps o and i inside the group; clamp=True reads output row Ho - 1 / column Wo - 1 where row Ho /
    column Wo is asked for (even H / W under stride 2)."""
    dz, w = dz.double().cpu(), w.double().cpu()
    B, C, Ho, Wo = dz.shape
    cg = C // groups
    wg = w.reshape(groups, cg, cg, 3, 3)                 # [g][o][i][ky][kx]
    if not transpose:
        wg = wg.transpose(1, 2)
    dzg = dz.reshape(B, groups, cg, Ho, Wo)
    dx = torch.zeros(B, groups, cg, H, W, dtype=torch.float64)

    def taps(n, no, k):
        src, dst = [], []
        for p in range(n):
            num = p + 1 - k
            if num < 0 or num % stride:
                continue
            o = num // stride
            if o >= no:
                if not clamp:
                    continue
                o = no - 1
            dst.append(p)
            src.append(o)
        return torch.tensor(src, dtype=torch.long), torch.tensor(dst, dtype=torch.long)
    for ky in range(3):
        sy, dy_ = taps(H, Ho, ky)
        for kx in range(3):
            sx, dx_ = taps(W, Wo, kx)
            if not len(sy) or not len(sx):
                continue
            wt = wg[:, :, :, ky, kx] if flip else wg[:, :, :, 2 - ky, 2 - kx]
            part = torch.einsum('bgoyx,goi->bgiyx', dzg[:, :, :, sy][:, :, :, :, sx], wt)
            dx[:, :, :, dy_.view(-1, 1), dx_.view(1, -1)] += part
    return dx.reshape(B, C, H, W)


def pack_fp32(w, scale=None):
    """numpy transcription of the fp32 operand layout of csrc/ia_gconv.hpp (gconv_pack_elem, plain
    pack): (C, Cg, 3, 3) fp32 weight -> (SG, 9, NB, 4, NB, 64), element [sg][t][ci][c][co][lane] =
    W[o][in % Cg][t] * scale[o] (one fp32 product) with o = sg*16*NB + 16*co + (lane & 15),
    in = sg*16*NB + 16*ci + 4*(lane >> 4) + c, zero across groups"""
    import numpy as np
    w = np.asarray(w, np.float32)
    C, cg = w.shape[0], w.shape[1]
    nb = 2 if cg == 32 else 1
    sgc = 16 * nb
    sg, t, ci, c, co, lane = np.ix_(*(np.arange(n) for n in (C // sgc, 9, nb, 4, nb, 64)))
    o = sg * sgc + 16 * co + (lane & 15) + 0 * (t + ci + c)
    i = sg * sgc + 16 * ci + 4 * (lane >> 4) + c + 0 * (t + co)
    v = w.reshape(C, cg, 9)[o, i % cg, t + 0 * o]
    if scale is not None:
        v = v * np.asarray(scale, np.float32)[o]
    return np.where(o // cg == i // cg, v, np.float32(0)).astype(np.float32)
