"""Masked convolution (`masked_conv2d`, `MaskedConv2d`): the operator API of the reference's
mmdet/ops/masked_conv on this build's HIP kernels (csrc/masked_conv.hip) -- the convolution is
evaluated only where a mask is set and is exactly 0 elsewhere; the inference layers of the
guided-anchor heads.

    compact_mask      mask -> kept pixel list, rank map, count (wave ballots + prefix scan)
    masked im2col     the kept pixels' im2col rows, 16 bytes per lane
    library GEMM      ia_linear_bias_act, k = taps * C, the bias in its epilogue
    masked scatter    every element of the dense result written once, +0.0 where the mask is false

fp32 on a ROCm device only; stride 1 with kernel 1x1 / padding 0 or kernel 3x3 / padding 1,
in_channels a multiple of 4.  Anything else is refused with an error that names the argument; there
is no CPU path and, as in the reference, no gradient.  Inputs may be NCHW-contiguous or
channels-last (the kernels work channels-last); the output is NCHW-contiguous for an NCHW-contiguous
input and channels-last otherwise.

The mask is (1, H, W) with a batch of 1 -- the reference's contract -- or (B, H, W), one mask per
image (this build's extension).

Host synchronisation: the library GEMM takes its row count from the host, so the number of kept
pixels is copied back once per compaction (4 bytes; `MaskCompaction.n`).  The reference
synchronises at the same place (`torch.nonzero`).  A caller with several masks can compact them all
into one count vector first and read it back in one copy (`compact_mask(count_out=...)` or
`compact_logits`, which thresholds sigmoid(logit) inside the compaction,
`MaskCompaction.set_n`): IoUawareGARetinaHead does, one copy per forward.

GEMM shapes: the row count is rounded up to ROW_GRANULE (1024) rows -- the gather writes the rows
behind the count as zeros -- so that a level of H x W pixels meets at most ceil(H * W / 1024)
different GEMM shapes per layer (17 for the largest level of an 800 x 1344 input) whatever its
masks are; the GEMM runs in the frozen tuning mode (table entry, else the library heuristic's first
kernel).  The output width is padded to a multiple of 16 columns (zero weights), so the 4- and
1-channel layers take the same library path as the wide ones.  The column matrix of one GEMM stays
under COL_CAP bytes: longer row lists are processed in chunks.

Reproducibility: the same bits in every run (no atomics; the row order is the ascending pixel order).
"""
import ctypes as C

import torch
import torch.nn as nn
from torch.nn.modules.utils import _pair

from . import _lib, ops
from .ops import _ptr, _stream

ROW_GRANULE = 1024
COL_CAP = 256 << 20
_N_ALIGN = 16


class MaskCompaction(object):
    """the kept pixels of a (B, H, W) mask: `idx` (B * H * W,) int32 whose first `n` entries are
    the kept flat pixel indices in ascending order, `rank` (B, H, W) int32 (row, or -1), `count`
    a (1,) int32 device view; `n` the host copy of the count (one D2H copy, made on first use)"""

    def __init__(self, shape, idx, rank, count):
        self.shape, self.idx, self.rank, self.count = shape, idx, rank, count
        self._n = None

    @property
    def n(self):
        if self._n is None:
            self._n = int(self.count.item())            # the host synchronisation of the operator
        return self._n

    def set_n(self, n):
        """the count as the caller read it back (one copy for several compactions)"""
        self._n = int(n)
        return self


def _mask_u8(mask):
    if mask.dtype == torch.bool:
        mask = mask.contiguous().view(torch.uint8)
    elif mask.dtype != torch.uint8:
        raise TypeError('mask has dtype %s: a bool or uint8 mask is needed' % mask.dtype)
    return mask.contiguous()


def _compact(entry, src, extra, shape, count_out):
    total = src.numel()
    L = _lib.lib()
    nbytes = L.ia_mask_compact_workspace_bytes(total)
    if nbytes == 0:
        raise _lib.IouAwareLibraryError('mask of %d pixels: 1 .. 2^31 - 1 are supported' % total)
    dev = src.device
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    idx = torch.empty(total, dtype=torch.int32, device=dev)
    rank = torch.empty(shape, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev) if count_out is None else count_out
    if count.dtype != torch.int32 or count.numel() != 1 or not count.is_cuda:
        raise ValueError('count_out must be a (1,) int32 device tensor')
    _lib.check(getattr(L, entry)(_ptr(src), *extra, total, _ptr(idx), _ptr(rank), _ptr(count), _ptr(ws), nbytes,
                                 _stream()), entry)
    return MaskCompaction(shape, idx, rank, count)


def compact_mask(mask, count_out=None):
    """(B, H, W) bool / uint8 device mask -> MaskCompaction (three launches, no atomics, no host
    synchronisation).  count_out: a (1,) int32 device tensor to receive the count (a slice of a
    caller's vector)."""
    if mask.dim() != 3:
        raise ValueError('mask must be (B, H, W), got %d-D' % mask.dim())
    ops._require_gpu(mask, 'mask')
    m = _mask_u8(mask)
    return _compact('ia_mask_compact', m, (), tuple(m.shape), count_out)


def compact_logits(logits, thr, count_out=None):
    """compact_mask of `sigmoid(logits) >= thr` for (B, H, W) fp32 device logits, the threshold
    taken inside the compaction kernels with the expression the guided decode applies to its
    location maps (ia_logit_compact): no mask tensor, and the two can never disagree on a location"""
    if logits.dim() != 3:
        raise ValueError('logits must be (B, H, W), got %d-D' % logits.dim())
    ops._require_gpu(logits, 'logits')
    if logits.dtype != torch.float32:
        raise TypeError('logits have dtype %s: float32 is needed' % logits.dtype)
    if not 0.0 <= float(thr) <= 1.0:
        raise ValueError('thr=%r: a probability is needed' % (thr,))
    x = logits.detach().contiguous()
    return _compact('ia_logit_compact', x, (float(thr),), tuple(x.shape), count_out)


def _one(v, name):
    a, b = _pair(v)
    if int(a) != int(b):
        raise NotImplementedError('%s=%s: the HIP masked convolution takes one %s for both directions'
                                  % (name, (a, b), name))
    return int(a)


def _check(x, mask, weight, bias, padding, stride):
    """the refusals, each naming what is not supported -> kernel size"""
    if x.dim() != 4 or weight.dim() != 4:
        raise ValueError('input and weight must be 4-D, got %d-D and %d-D' % (x.dim(), weight.dim()))
    s, p = _one(stride, 'stride'), _one(padding, 'padding')
    if s != 1:
        raise NotImplementedError('stride=%d: the HIP masked convolution supports stride=1 only' % s)
    k = tuple(int(v) for v in weight.shape[2:])
    if k not in ((1, 1), (3, 3)):
        raise NotImplementedError('kernel_size=%s: the HIP masked convolution supports 1x1 and 3x3 '
                                  'kernels only' % (k,))
    if p != (k[0] - 1) // 2:
        raise NotImplementedError('padding=%d: the HIP masked convolution supports padding=%d with a '
                                  '%dx%d kernel only' % (p, (k[0] - 1) // 2, k[0], k[1]))
    if weight.shape[1] != x.shape[1]:
        raise ValueError('weight has %d input channels, the input %d (groups=1 only)'
                         % (weight.shape[1], x.shape[1]))
    if x.shape[1] % 4:
        raise NotImplementedError('in_channels=%d: the HIP masked convolution needs a multiple of 4'
                                  % x.shape[1])
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError('bias must have shape (%d,)' % weight.shape[0])
    B, _, H, W = x.shape
    if mask is not None:
        if mask.dim() != 3 or tuple(mask.shape[1:]) != (H, W) or mask.shape[0] not in (1, B) \
                or (mask.shape[0] == 1 and B != 1):
            raise ValueError('mask must have shape (1, %d, %d) with a batch of 1 or (%d, %d, %d), got %s'
                             % (H, W, B, H, W, tuple(mask.shape)))
    for name, t in (('input', x), ('weight', weight), ('bias', bias)):
        if t is not None and t.dtype != torch.float32:
            raise TypeError('%s has dtype %s: the masked convolution kernels are float32 only'
                            % (name, t.dtype))
    for name, t in (('input', x), ('mask', mask), ('weight', weight), ('bias', bias)):
        if t is not None and not t.is_cuda:
            raise _lib.IouAwareLibraryError(
                '%s is on %s: the masked convolution runs on gfx950 HIP kernels and has no CPU '
                'fallback' % (name, t.device))
    return k[0]


def pack_weight(weight, bias):
    """(n, C, k, k) weight and (n,) bias or None -> the GEMM operands: (k * k * C, n16) fp32, row
    (dy * k + dx) * C + c, and (n16,) fp32, n16 = n rounded up to 16 (zero columns)"""
    w = weight.detach().float()
    n, c, kh, kw = w.shape
    npad = (n + _N_ALIGN - 1) // _N_ALIGN * _N_ALIGN
    w_kn = w.new_zeros((kh * kw * c, npad))
    w_kn[:, :n] = w.permute(2, 3, 1, 0).reshape(kh * kw * c, n)
    b = w.new_zeros(npad)
    if bias is not None:
        b[:n] = bias.detach().float()
    return w_kn, b, n


def masked_conv_packed(x, comp, packed, ksize, col_cap=None, y_out=None, out=None):
    """the operator on prepared operands: x channels-last fp32 (B, C, H, W), comp a MaskCompaction of
    its (B, H, W) mask, packed = pack_weight(...) -> channels-last (B, n, H, W).
    y_out / out (tests): a (rows_pad, n16) fp32 buffer for the GEMM result and a channels-last
    (B, n, H, W) result tensor to write into instead of fresh ones."""
    w_kn, b, n = packed
    B, Cc, H, W = (int(v) for v in x.shape)
    if tuple(comp.shape) != (B, H, W):
        raise ValueError('the compaction is of a %s mask, the input is %s' % (comp.shape, (B, H, W)))
    k, npad = int(w_kn.shape[0]), int(w_kn.shape[1])
    total = B * H * W
    L = _lib.lib()
    if out is None:
        out = torch.empty((B, n, H, W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    elif tuple(out.shape) != (B, n, H, W) or out.dtype != torch.float32 \
            or not out.is_contiguous(memory_format=torch.channels_last):
        raise ValueError('out must be a channels-last fp32 (B, n, H, W) tensor')
    kept = comp.n
    y = None
    if kept > 0:
        rows_pad = (kept + ROW_GRANULE - 1) // ROW_GRANULE * ROW_GRANULE
        if y_out is not None:
            if y_out.dtype != torch.float32 or not y_out.is_contiguous() or y_out.numel() < rows_pad * npad:
                raise ValueError('y_out must be a contiguous fp32 buffer of %d x %d' % (rows_pad, npad))
            y = y_out
        else:
            y = torch.empty((rows_pad, npad), dtype=torch.float32, device=x.device)
        cap = COL_CAP if col_cap is None else int(col_cap)
        step = max(ROW_GRANULE, cap // (k * 4) // ROW_GRANULE * ROW_GRANULE)
        ops._ensure_gemm_table()
        ws = ops._workspace(x.device, ops._LT_WS_BYTES)
        for r0 in range(0, rows_pad, step):
            rows = min(step, rows_pad - r0)
            col = ops._col_buffer(x.device, rows * k * 4)
            _lib.check(L.ia_masked_im2col(_ptr(x), _ptr(comp.idx), kept, r0, rows, _ptr(col), B, H, W, Cc,
                                          ksize, _stream()), 'ia_masked_im2col')
            _lib.check(L.ia_linear_bias_act(_ptr(col), _ptr(w_kn), _ptr(b), None,
                                            C.c_void_p(y.data_ptr() + r0 * npad * 4), rows, k, npad, 0,
                                            _ptr(ws), ops._LT_WS_BYTES, _stream()),
                       'ia_linear_bias_act (masked)')
    _lib.check(L.ia_masked_scatter(_ptr(y), npad, _ptr(comp.rank), _ptr(out), total, n, _stream()),
               'ia_masked_scatter')
    return out


def masked_conv2d(features, mask, weight, bias, padding=0, stride=1, col_cap=None, packed=None):
    """reference mmdet/ops/masked_conv/functions/masked_conv.py: features (B, C, H, W), mask
    (1, H, W) [B = 1] or (B, H, W), nonzero = evaluate; weight (n, C, k, k), bias (n,) or None ->
    (B, n, H, W), exactly 0 where the mask is false: NCHW-contiguous for an NCHW-contiguous input,
    channels-last for every other input (a channels-last one is consumed as it is, any other layout
    is converted first).  No gradient.  packed: the operands of pack_weight(weight, bias), for a
    caller that keeps them (MaskedConv2d does)."""
    if mask is None:
        raise ValueError('masked_conv2d needs a mask')
    ksize = _check(features, mask, weight, bias, padding, stride)
    x = features.detach()
    nchw = x.is_contiguous() and not x.is_contiguous(memory_format=torch.channels_last)
    xc = x if x.is_contiguous(memory_format=torch.channels_last) else x.contiguous(memory_format=torch.channels_last)
    out = masked_conv_packed(xc, compact_mask(mask), packed or pack_weight(weight, bias), ksize, col_cap)
    return out.contiguous() if nchw else out


class MaskedConv2d(nn.Conv2d):
    """reference mmdet/ops/masked_conv/modules/masked_conv.py: a Conv2d whose forward takes an
    optional mask.  mask=None: the plain (trainable) convolution; with a mask: masked_conv2d, for
    inference only."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 bias=True):
        super(MaskedConv2d, self).__init__(in_channels, out_channels, kernel_size, stride, padding,
                                           dilation, groups, bias)

    def forward(self, input, mask=None):
        if mask is None:
            return super(MaskedConv2d, self).forward(input)
        if _pair(self.dilation) != (1, 1) or self.groups != 1:
            raise NotImplementedError('dilation=%s / groups=%d: the HIP masked convolution supports '
                                      'dilation=1 and groups=1 only' % (self.dilation, self.groups))
        # the GEMM operands are repacked only when a parameter changed
        params = (self.weight,) if self.bias is None else (self.weight, self.bias)
        key = tuple((p.data_ptr(), p._version, str(p.device)) for p in params)
        if getattr(self, '_packed_key', None) != key:
            self._packed_key, self._packed = key, pack_weight(self.weight, self.bias)
        return masked_conv2d(input, mask, self.weight, self.bias, self.padding, self.stride, packed=self._packed)
