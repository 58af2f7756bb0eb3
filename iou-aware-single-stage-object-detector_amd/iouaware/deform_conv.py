"""Deformable convolution, DCN v1 (`deform_conv`, `DeformConv`, `DeformConvPack`) and v2
(`modulated_deform_conv`, `ModulatedDeformConv`, `ModulatedDeformConvPack`): the operator API of
the reference's mmdet/ops/dcn on this build's HIP kernels (csrc/deform.hip) -- the deformable
im2col, the library GEMM with bias in its epilogue, and in backward the `dcol` product, the
adjoint gather and the weight-gradient product on the recomputed column matrix.

fp32 on a ROCm device only; 3x3 kernels, groups = 1, any stride / dilation >= 1 and padding >= 0,
in_channels a multiple of 4 * deformable_groups.  Anything else is refused with an error that
names the argument; there is no CPU path.  Inputs may be NCHW-contiguous or channels-last (the
kernels work channels-last; other layouts are converted) and the output has the input's memory
format.

Reproducibility: y, d_offset, d_mask, dW and db have the same bits in every run.  **dx does not**:
it is scattered with fp32 atomicAdd (four corners per column element) and the order in which the
adds of different output pixels arrive is not fixed -- the one place on the training routes of
this build where that holds.
"""
import math

import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from . import _lib, ops


def _one(v, name):
    """an int or a pair of two equal ints -> the int"""
    a, b = _pair(v)
    if int(a) != int(b):
        raise NotImplementedError('%s=%s: the HIP deformable convolution takes one %s for both '
                                  'directions' % (name, (a, b), name))
    return int(a)


def _check(x, offset, mask, weight, bias, stride, padding, dilation, groups, dg):
    """the refusals of both ops, each naming what is not supported -> (stride, padding, dilation)"""
    if x.dim() != 4 or offset.dim() != 4 or weight.dim() != 4:
        raise ValueError('input, offset and weight must be 4-D, got %d-D, %d-D and %d-D'
                         % (x.dim(), offset.dim(), weight.dim()))
    if int(groups) != 1:
        raise NotImplementedError('groups=%d: the HIP deformable convolution supports groups=1 only'
                                  % int(groups))
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise NotImplementedError('kernel_size=%s: the HIP deformable convolution supports 3x3 kernels only'
                                  % (tuple(weight.shape[2:]),))
    if weight.shape[1] != x.shape[1]:
        raise ValueError('weight has %d input channels, the input %d' % (weight.shape[1], x.shape[1]))
    dg = int(dg)
    if dg < 1 or x.shape[1] % (4 * dg):
        raise NotImplementedError('deformable_groups=%d: in_channels=%d must be a multiple of '
                                  '4 * deformable_groups' % (dg, x.shape[1]))
    s, p, d = _one(stride, 'stride'), _one(padding, 'padding'), _one(dilation, 'dilation')
    if s < 1 or d < 1 or p < 0:
        raise ValueError('stride=%d / dilation=%d must be >= 1 and padding=%d >= 0' % (s, d, p))
    Ho, Wo = ops.deform_out_hw(int(x.shape[2]), int(x.shape[3]), s, p, d)
    if Ho < 1 or Wo < 1:
        raise ValueError('convolution input is too small (output would be %dx%d)' % (Ho, Wo))
    B = int(x.shape[0])
    if tuple(offset.shape) != (B, dg * 18, Ho, Wo):
        raise ValueError('offset must have shape %s, got %s' % ((B, dg * 18, Ho, Wo), tuple(offset.shape)))
    if mask is not None and tuple(mask.shape) != (B, dg * 9, Ho, Wo):
        raise ValueError('mask must have shape %s, got %s' % ((B, dg * 9, Ho, Wo), tuple(mask.shape)))
    # (the argument refusals above come first, then the dtype, the device last)
    for name, t in (('input', x), ('offset', offset), ('mask', mask), ('weight', weight), ('bias', bias)):
        if t is not None and t.dtype != torch.float32:
            raise TypeError('%s has dtype %s: the deformable convolution kernels are float32 only'
                            % (name, t.dtype))
    for name, t in (('input', x), ('offset', offset), ('mask', mask), ('weight', weight), ('bias', bias)):
        if t is not None and not t.is_cuda:
            raise _lib.IouAwareLibraryError(
                '%s is on %s: the deformable convolution runs on gfx950 HIP kernels and has no CPU '
                'fallback' % (name, t.device))
    return s, p, d


def _cl(t):
    cl = torch.channels_last
    return t if t.is_contiguous(memory_format=cl) else t.contiguous(memory_format=cl)


class _DeformConv3x3(Function):
    """both ops (mask None: v1).  col_cap: see ops.deform_conv3x3"""

    @staticmethod
    def forward(ctx, x, offset, mask, weight, bias, stride, padding, dilation, dg, col_cap):
        nchw = x.is_contiguous() and not x.is_contiguous(memory_format=torch.channels_last)
        xc, oc = _cl(x.detach()), _cl(offset.detach())
        mc = None if mask is None else _cl(mask.detach())
        w_kn = ops.conv3x3_weight_kn(weight)                    # (9 Cin, Cout), row tap * Cin + c
        y = ops.deform_conv3x3(xc, oc, mc, w_kn, None if bias is None else bias.detach().contiguous(),
                               stride, padding, dilation, dg, col_cap=col_cap)
        ctx.geom = (stride, padding, dilation, dg, col_cap)
        ctx.nchw = nchw
        ctx.save_for_backward(xc, oc, mc, w_kn)
        return y.contiguous() if nchw else y

    @staticmethod
    @once_differentiable             # raw kernels on detached tensors: a double backward is an error
    def backward(ctx, dy):
        from .winograd_train import relu_bwd_bias_grad
        xc, oc, mc, w_kn = ctx.saved_tensors
        stride, padding, dilation, dg, col_cap = ctx.geom
        nx, no, nm, nw, nb = ctx.needs_input_grad[:5]
        g, db = relu_bwd_bias_grad(dy, None, bias_grad=nb)      # channels-last g, the column sum
        dx, do, dm, dw = ops.deform_conv3x3_backward(g, xc, oc, mc, w_kn, stride, padding, dilation, dg,
                                                     need=(nx, no, nm, nw), col_cap=col_cap)
        if dw is not None:                                      # (Cout, 9 Cin) = (Cout, 3, 3, Cin) order
            dw = dw.view(dw.shape[0], 3, 3, xc.shape[1]).permute(0, 3, 1, 2)
        if ctx.nchw:
            dx, do, dm = (None if t is None else t.contiguous() for t in (dx, do, dm))
        return dx, do, dm, dw, db, None, None, None, None, None


def deform_conv(input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1,
                im2col_step=64, col_cap=None):
    """DCN v1 (reference mmdet/ops/dcn/functions/deform_conv.py): input (B, C, H, W), offset
    (B, dg * 18, Ho, Wo), weight (Cout, C, 3, 3) -> (B, Cout, Ho, Wo) in the input's memory format.
    im2col_step is accepted and ignored (the batch is cut by the column buffer's byte cap,
    `col_cap`, default ops.DEFORM_COL_CAP).  dx is not bit-reproducible (module docstring)."""
    s, p, d = _check(input, offset, None, weight, None, stride, padding, dilation, groups, deformable_groups)
    return _DeformConv3x3.apply(input, offset, None, weight, None, s, p, d, int(deformable_groups), col_cap)


def modulated_deform_conv(input, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1,
                          deformable_groups=1, col_cap=None):
    """DCN v2: as deform_conv with every sample multiplied by mask (B, dg * 9, Ho, Wo), plus bias"""
    if mask is None:
        raise ValueError('modulated_deform_conv needs a mask')
    s, p, d = _check(input, offset, mask, weight, bias, stride, padding, dilation, groups, deformable_groups)
    return _DeformConv3x3.apply(input, offset, mask, weight, bias, s, p, d, int(deformable_groups), col_cap)


class _DeformBase(nn.Module):
    """what the four modules share: the reference's attribute and parameter names (`weight`
    (Cout, Cin / groups, kh, kw), `bias` or None) and its initialisation, uniform in
    +-1 / sqrt(Cin * kh * kw) with a zero bias.  The reference keeps stride / padding / dilation as
    pairs in the v1 modules and as given in the modulated ones; so do these."""

    def _setup(self, in_channels, out_channels, kernel_size, stride, padding, dilation, groups,
               deformable_groups, bias, pairs):
        for what, n in (('in_channels', in_channels), ('out_channels', out_channels)):
            assert n % groups == 0, '%s=%d is not a multiple of groups=%d' % (what, n, groups)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size = _pair(kernel_size)
        conv = _pair if pairs else (lambda v: v)
        self.stride, self.padding, self.dilation = conv(stride), conv(padding), conv(dilation)
        self.groups, self.deformable_groups = groups, deformable_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.in_channels * self.kernel_size[0] * self.kernel_size[1])
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            if self.bias is not None:
                self.bias.zero_()

    def _offset_conv(self, per_tap):
        """the zero-initialised convolution that predicts per_tap values per tap and deformable group,
        with the geometry of the deformable convolution itself (as the reference builds it: kernel,
        stride and padding; not the dilation)"""
        k = self.kernel_size
        conv = nn.Conv2d(self.in_channels, self.deformable_groups * per_tap * k[0] * k[1], kernel_size=k,
                         stride=_pair(self.stride), padding=_pair(self.padding), bias=True)
        nn.init.zeros_(conv.weight)
        nn.init.zeros_(conv.bias)
        return conv


class DeformConv(_DeformBase):
    """DCN v1 layer without bias (`bias=True` is an AssertionError, as in the reference); forward(x, offset)"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 deformable_groups=1, bias=False):
        super(DeformConv, self).__init__()
        assert not bias, 'DeformConv has no bias'
        self._setup(in_channels, out_channels, kernel_size, stride, padding, dilation, groups,
                    deformable_groups, False, pairs=True)

    def forward(self, x, offset):
        return deform_conv(x, offset, self.weight, self.stride, self.padding, self.dilation, self.groups,
                           self.deformable_groups)


class DeformConvPack(DeformConv):
    """DeformConv that predicts its own offsets: `conv_offset`, zero at construction"""

    def __init__(self, *args, **kwargs):
        super(DeformConvPack, self).__init__(*args, **kwargs)
        self.conv_offset = self._offset_conv(2)

    def init_offset(self):
        nn.init.zeros_(self.conv_offset.weight)
        nn.init.zeros_(self.conv_offset.bias)

    def forward(self, x):
        return DeformConv.forward(self, x, self.conv_offset(x))


class ModulatedDeformConv(_DeformBase):
    """DCN v2 layer; forward(x, offset, mask)"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 deformable_groups=1, bias=True):
        super(ModulatedDeformConv, self).__init__()
        self.with_bias = bias
        self._setup(in_channels, out_channels, kernel_size, stride, padding, dilation, groups,
                    deformable_groups, bias, pairs=False)

    def forward(self, x, offset, mask):
        return modulated_deform_conv(x, offset, mask, self.weight, self.bias, self.stride, self.padding,
                                     self.dilation, self.groups, self.deformable_groups)


class ModulatedDeformConvPack(ModulatedDeformConv):
    """ModulatedDeformConv that predicts offsets and mask: `conv_offset_mask`, zero at construction.
    Its output is cut in three along the channels: offset = cat(first, second), mask = sigmoid(third)"""

    def __init__(self, *args, **kwargs):
        super(ModulatedDeformConvPack, self).__init__(*args, **kwargs)
        self.conv_offset_mask = self._offset_conv(3)

    def init_offset(self):
        nn.init.zeros_(self.conv_offset_mask.weight)
        nn.init.zeros_(self.conv_offset_mask.bias)

    def forward(self, x):
        a, b, logits = self.conv_offset_mask(x).chunk(3, dim=1)
        return ModulatedDeformConv.forward(self, x, torch.cat((a, b), dim=1), torch.sigmoid(logits))
