"""The yardstick of the bf16 training convolution (csrc/conv3x3_bf16_bwd.hip,
iouaware/conv3x3_bf16_train.py): torch autograd of F.conv2d on the CPU, in fp64 as the definition and
in fp32 as "what a plain fp32 evaluation of the same sums loses" -- both on the operands as the
kernels see them, i.e. x, w and dy already rounded to bf16.  Test-only, nothing imported from the
project.  The gates are the project's own (tests/wino_ref.py: gates, GATE_A, GATE_B)."""
import torch
import torch.nn.functional as F

BF16_RNE = 2.0 ** -8       # one round-to-nearest-even rounding to bf16: at most 2^-8 of the value


def _cpu(t, dtype):
    return t.detach().to('cpu', dtype).contiguous()


def conv_grads(xs, w, dys, dtype=torch.float64, want=('dx', 'dw', 'db')):
    """3x3 / stride 1 / pad 1 convolution with ONE weight over a list of levels: the gradients of
    sum_l <conv(x_l, w) + b, dy_l> w.r.t. the inputs, the weight and the bias.
    xs: per-level (B, cin, H, W); w (cout, cin, 3, 3); dys: per-level (B, cout, H, W); any dtype /
    device / strides -> dict(dx=[per level], dw=, db=) of CPU tensors of `dtype`"""
    xs = [_cpu(x, dtype).requires_grad_('dx' in want) for x in xs]
    w = _cpu(w, dtype).requires_grad_('dw' in want)
    b = torch.zeros(w.shape[0], dtype=dtype).requires_grad_('db' in want)
    total = sum((F.conv2d(x, w, b, 1, 1) * _cpu(dy, dtype)).sum() for x, dy in zip(xs, dys))
    leaves = ([*xs] if 'dx' in want else []) + ([w] if 'dw' in want else []) + ([b] if 'db' in want else [])
    grads = list(torch.autograd.grad(total, leaves))
    out = {}
    if 'dx' in want:
        out['dx'] = grads[:len(xs)]
        grads = grads[len(xs):]
    if 'dw' in want:
        out['dw'] = grads.pop(0)
    if 'db' in want:
        out['db'] = grads.pop(0)
    return out


def conv_grads_groups(xs_groups, w, dys_groups, dtype=torch.float64, want=('dx', 'dw', 'db')):
    """the same for `groups` independent convolutions whose weights are stacked along dim 0 ->
    dict(dx=[per group [per level]], dw=(groups * cout, cin, 3, 3), db=(groups * cout,))"""
    n = len(xs_groups)
    cout = w.shape[0] // n
    parts = [conv_grads(xs_groups[g], w[g * cout:(g + 1) * cout], dys_groups[g], dtype, want) for g in range(n)]
    out = {}
    if 'dx' in want:
        out['dx'] = [p['dx'] for p in parts]
    if 'dw' in want:
        out['dw'] = torch.cat([p['dw'] for p in parts])
    if 'db' in want:
        out['db'] = torch.cat([p['db'] for p in parts])
    return out


def bf16_bound(want, floor=2e-3):
    """elementwise bound of a bf16 result against its fp64 definition: one rounding, plus `floor`
    roundings of the largest value for what the fp32 accumulation leaves (the forward kernel's
    bound, tests/test_gpu_conv3x3_bf16.py)"""
    return BF16_RNE * want.abs() + floor * BF16_RNE * float(want.abs().max())
