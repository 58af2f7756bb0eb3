"""The yardstick of the strided 3x3 training node (iouaware/train_fuse.py: conv3x3_strided; csrc/im2col.hip:
k_im2col3x3, k_col2im3x3): torch autograd of F.conv2d with a stride on the CPU, in fp64 as the
definition and in fp32 as "what a plain fp32 evaluation of the same sums loses".  Test-only, nothing
imported from the project.  The gates are the project's own (tests/wino_ref.py: gates, GATE_A,
GATE_B).  `col2im` restates the kernel's contract term by term: the same fp32 adds in the same order,
so its result is the kernel's bit for bit."""
import torch
import torch.nn.functional as F


def _cpu(t, dtype):
    return None if t is None else t.detach().to('cpu', dtype).contiguous()


def preactivation(x, w, b, stride, dtype=torch.float64):
    """conv(x, w, stride, pad 1) + b before the ReLU -> CPU tensor of `dtype`"""
    return F.conv2d(_cpu(x, dtype), _cpu(w, dtype), _cpu(b, dtype), stride, 1)


def conv_train(x, w, b, dy, stride, relu, dtype=torch.float64):
    """y = relu?(conv(x, w, stride, pad 1) + b) and the gradients of <y, dy> w.r.t. x, w and b.
    x (B, cin, H, W); w (cout, cin, 3, 3); b (cout,) or None; dy (B, cout, Ho, Wo); any dtype /
    device / strides -> dict(y=, dx=, dW=, db= [None without b]) of CPU tensors of `dtype`"""
    x = _cpu(x, dtype).requires_grad_(True)
    w = _cpu(w, dtype).requires_grad_(True)
    b = None if b is None else _cpu(b, dtype).requires_grad_(True)
    y = F.conv2d(x, w, b, stride, 1)
    if relu:
        y = y.clamp(min=0)
    leaves = [x, w] + ([b] if b is not None else [])
    grads = torch.autograd.grad((y * _cpu(dy, dtype)).sum(), leaves)
    return dict(y=y.detach(), dx=grads[0], dW=grads[1], db=grads[2] if b is not None else None)


def out_size(n, stride):
    return (n - 1) // stride + 1


def col2im(dcol, B, H, W, C, stride):
    """dcol (B * Ho * Wo, 9 * C) fp32 -> dx (B, H, W, C) fp32 on the CPU:
    dx[b][yi][xi][c] = sum over the taps (dy, dx), tap = dy * 3 + dx, with yi = yo * stride + dy - 1,
    xi = xo * stride + dx - 1 for an output pixel (yo, xo), of dcol[(b, yo, xo)][tap * C + c] -- the
    taps added one after the other in ascending order, each in one fp32 add onto a sum that starts
    at 0.0f; pixels that no tap reads stay 0.0f"""
    assert dcol.dtype == torch.float32
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    d = dcol.detach().cpu().reshape(B, Ho, Wo, 9, C)
    dx = torch.zeros(B, H, W, C, dtype=torch.float32)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        yo = [o for o in range(Ho) if 0 <= o * stride + ky - 1 < H]
        xo = [o for o in range(Wo) if 0 <= o * stride + kx - 1 < W]
        if not yo or not xo:
            continue
        yi = torch.tensor([o * stride + ky - 1 for o in yo]).view(-1, 1)
        xi = torch.tensor([o * stride + kx - 1 for o in xo]).view(1, -1)
        # within one tap every (yi, xi) occurs once: one add per element and tap
        dx[:, yi, xi] = dx[:, yi, xi] + d[:, torch.tensor(yo).view(-1, 1), torch.tensor(xo).view(1, -1), tap]
    return dx
