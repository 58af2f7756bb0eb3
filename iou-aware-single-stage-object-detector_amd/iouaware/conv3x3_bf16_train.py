"""Mixed-precision training of the RetinaNet and FCOS heads: bf16 activations and gradients on this
library's MFMA convolution kernels (and, in the FCOS towers, its bf16 GroupNorm + ReLU node), fp32
master weights and fp32 weight / bias / GroupNorm parameter gradients (opt-in:
`head.train_bf16 = True`).

Reference: mmdet/models/anchor_heads/retina_head.py:79-90 / iou_aware_retina_head.py:171-219 (4 + 4
tower ConvModules with ReLU, retina_cls, retina_reg [, retina_iou], weights shared by the pyramid
levels); the reference has no mixed-precision route.  One shared-weight convolution over ALL levels
and BOTH towers is one autograd node:

    forward     pack the fp32 weight (one launch: round to bf16 + fragment order), then
                csrc/conv3x3_bf16.hip: y_l = conv(x_l, w) + b [ReLU], bf16 channels-last
    backward    g = dy where y > 0, db = column sums of g       ia_relu_bwd_bias_grad_bf16
                dx = conv(g, w^T rotated by 180 degrees)          the SAME forward kernel on the
                                                                  adjoint weight (one pack launch)
                dW = sum over pixels of g (x) x, fp32             csrc/conv3x3_bf16_bwd.hip

Channel padding: the input-gradient convolution reads g as its input and the kernel takes inputs of
a multiple of 32 channels, so the outputs (720, 36 / 46 channels) live in tensors whose channel
width is the next multiple of 32 (736, 64).  Two things keep the padding harmless: the forward
output tensors are allocated zero-filled (their padding is never written), and in backward g is
written into a ONCE-ZEROED buffer of the padded width that is kept per shape (the mask kernel writes
the real channels only) while the adjoint weight carries ZERO ROWS for the padded channels.
Without ReLU, bias gradient and padding (the FCOS tower convolutions) g is dy itself: no copy.

The FCOS heads (fcos_head_forward; reference fcos_head.py / iou_aware_fcos_head.py: 4 + 4
ConvModules of 3x3 convolution without bias + GroupNorm + ReLU): per tower layer one convolution
node for both towers and ONE fcos_ops.groupnorm_relu_bf16 node on the 2F-channel activation; the
output convolutions write fp32 NCHW maps for the fused loss node.
"""
import collections
import ctypes as C

import torch

from . import ops

_CL = torch.channels_last
_BF = torch.bfloat16


def _pad32(n):
    return (n + 31) // 32 * 32


def _alloc_levels(like, width, zero=False):
    """one flat (pixels of all levels, width) bf16 buffer -> its per-level channels-last
    (B, width, H, W) views: the levels follow each other in memory, so row-wise kernels take all of
    them in one launch"""
    rows = [x.shape[0] * x.shape[2] * x.shape[3] for x in like]
    make = torch.zeros if zero else torch.empty
    flat = make((sum(rows), width), dtype=_BF, device=like[0].device)
    out, o = [], 0
    for x, r in zip(like, rows):
        out.append(flat[o:o + r].view(x.shape[0], x.shape[2], x.shape[3], width).permute(0, 3, 1, 2))
        o += r
    return out


_ZEROED = collections.OrderedDict()     # once-zeroed padded gradient buffers, least recently used first
_ZEROED_ENTRIES = 8


def _zeroed_levels(like, width, real):
    """per-level (B, width, H, W) views of a buffer whose channels [real, width) are zero and stay
    zero: callers write channels [0, real) only"""
    key = (tuple(tuple(x.shape) for x in like), width, real, like[0].device, ops.stream_id())
    buf = _ZEROED.get(key)
    if buf is None:
        while len(_ZEROED) >= _ZEROED_ENTRIES:
            _ZEROED.popitem(last=False)
        buf = _ZEROED[key] = _alloc_levels(like, width, zero=True)
    else:
        _ZEROED.move_to_end(key)
    return buf


def _cl_bf16(t):
    """a bf16 tensor the kernels can address: channels-last or a channel slice of one"""
    if t.dtype != _BF:
        t = t.to(_BF)                     # (an incoming gradient; the inputs are checked in conv_levels)
    try:
        ops._cl_pix_stride(t, 'conv3x3_bf16_train')
        return t
    except TypeError:
        return t.contiguous(memory_format=_CL)


def _addressable(groups):
    """whether the convolution kernels can read these per-group level lists as an input: 16-byte
    pixels and one pixel stride for all of them"""
    ts = [t for g in groups for t in g]
    strides = set(ops._cl_pix_stride(t, 'conv3x3_bf16_train') for t in ts)
    return len(strides) == 1 and strides.pop() % 8 == 0 and all(t.data_ptr() % 16 == 0 for t in ts)


def _storage(t):
    return t.untyped_storage().data_ptr()


def _same_view(a, b):
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


def _mask_and_bias_grad(dys, ys, gs, n, want_db):
    """per level: g = dy masked by y > 0 (ys None: a copy of dy), db = the column sums of g summed
    over the levels (None unless want_db).  dys / ys / gs: per-level (B, n, H, W) tensors; levels
    that follow each other in memory in all three operands share one launch."""
    what = 'conv3x3_bf16_train'
    operands = (dys, ys, gs)
    runs = []                             # [[(address, row stride, storage) or None per operand], rows]
    for l, d in enumerate(dys):
        ent = [None if o is None else (o[l].data_ptr(), ops._cl_pix_stride(o[l], what), _storage(o[l]))
               for o in operands]
        rows = d.shape[0] * d.shape[2] * d.shape[3]
        # (views of ONE storage only: two separate allocations that happen to be neighbours must not
        # share a launch, or the order of the bias-gradient sums would depend on where the allocator
        # put them and the bits would change from run to run)
        if runs and all(e is None or (p[1] == e[1] and p[2] == e[2] and p[0] + 2 * runs[-1][1] * e[1] == e[0])
                        for p, e in zip(runs[-1][0], ent)):
            runs[-1][1] += rows
        else:
            runs.append([ent, rows])
    db = None
    for (pd, py, pg), rows in runs:
        b = ops.relu_bwd_bias_grad_bf16_rows(dys[0].device, pd[0], pd[1], py and py[0], py[1] if py else 0,
                                             rows, n, pg[0], pg[1], want_db)
        if want_db:
            db = b if db is None else db + b
    return db


def _wide(ts, n):
    """the (B, n, H, W) tensors that start where the channel slices `ts` start"""
    return [t.as_strided((t.shape[0], n, t.shape[2], t.shape[3]), t.stride()) for t in ts]


class _Bf16ConvLevels(torch.autograd.Function):
    """conv3x3 (stride 1, pad 1) + bias (+ ReLU) with ONE fp32 weight (groups * cout, cin, 3, 3) over
    `groups` lists of bf16 level tensors; outputs: groups x levels bf16 tensors, the channel slices
    [g * P, g * P + cout) of one (B, groups * P, H, W) tensor per level, P = cout rounded up to 32.
    `padded` (the subclass _Bf16ConvLevelsPadded, one group): the outputs are the (B, P, H, W) tensors
    themselves (zeros behind cout), and backward takes gradients of that width as they are (the padding's
    gradient is not read)"""

    @staticmethod
    def forward(ctx, weight, bias, relu, groups, *xs):
        return _Bf16ConvLevels._forward(ctx, False, weight, bias, relu, groups, xs)

    @staticmethod
    def _forward(ctx, padded, weight, bias, relu, groups, xs):
        L = len(xs) // groups
        xg = [[_cl_bf16(x) for x in xs[g * L:(g + 1) * L]] for g in range(groups)]
        cout, cin = weight.shape[0] // groups, weight.shape[1]
        # both towers on ONE input (the first tower layer): one convolution with 2 * cout outputs
        shared = groups == 2 and cout % 32 == 0 and all(_same_view(a, b) for a, b in zip(*xg))
        ge, ce = (1, 2 * cout) if shared else (groups, cout)      # what the kernels see
        P = _pad32(ce)
        with torch.no_grad():
            wp = ops.conv3x3_bf16_pack(weight, groups=ge)
            b = None if bias is None else bias.detach().float().contiguous()
            # (zero-filled when padded: the padding channels are never written)
            bufs = _alloc_levels(xg[0], ge * P, zero=P != ce)
            yk = [[t[:, g * P:g * P + ce] for t in bufs] for g in range(ge)]
            ops.conv3x3_bf16_levels(xg[:ge], wp, b, ce, yk, relu=relu, cin=cin)
            ys = [[t[:, g * cout:(g + 1) * cout] for t in bufs] for g in range(groups)] if shared else yk
        ctx.relu, ctx.has_bias, ctx.groups, ctx.L, ctx.shared = bool(relu), bias is not None, groups, L, shared
        ctx.padded = bool(padded)
        flat_x = [x for g in range(ge) for x in xg[g]]
        ctx.save_for_backward(weight, *flat_x, *(bufs if relu else []))
        if padded:
            return tuple(bufs)
        return tuple(y for g in range(groups) for y in ys[g])

    @staticmethod
    def backward(ctx, *dys):
        saved = ctx.saved_tensors
        groups, L, shared = ctx.groups, ctx.L, ctx.shared
        weight = saved[0]
        cout, cin = weight.shape[0] // groups, weight.shape[1]
        ge, ce = (1, 2 * cout) if shared else (groups, cout)
        P = _pad32(ce)
        xg = [list(saved[1 + g * L:1 + (g + 1) * L]) for g in range(ge)]
        ybufs = list(saved[1 + ge * L:1 + ge * L + L]) if ctx.relu else None
        with torch.no_grad():
            dyg = [[_cl_bf16(d) for d in dys[g * L:(g + 1) * L]] for g in range(groups)]
            if ctx.padded:                # (B, P, H, W) gradients: the real channels, where they lie
                dyg = [[d[:, :cout] for d in dyg[0]]]
            want_b = ctx.has_bias and ctx.needs_input_grad[1]
            need_x = any(ctx.needs_input_grad[4:])
            # the incoming gradients of two groups as ONE (B, 2 * cout, H, W) tensor per level when they
            # are neighbouring channel slices of one storage (the next layer's input gradients are): one
            # pass.  Never for separate allocations that merely lie side by side: see _mask_and_bias_grad
            whole = groups == 2 and P == ce and all(
                b.data_ptr() == a.data_ptr() + 2 * cout and a.stride() == b.stride() and _storage(a) == _storage(b)
                and ops._cl_pix_stride(a, 'conv3x3_bf16_train') >= 2 * cout for a, b in zip(dyg[0], dyg[1]))
            # ---- g = dy masked by the ReLU, db.  Nothing to mask, no bias gradient and no padding (every
            # GroupNorm tower convolution): g IS dy, read where it lies -- when the kernels can address
            # it (16-byte pixels, one pixel stride; one convolution with 2 * cout outputs needs the two
            # towers' gradients as one tensor).  Otherwise g lives in tensors of the padded width: a buffer
            # that was zeroed once when there is padding (only the real channels are ever written)
            direct = not ctx.relu and not want_b and P == ce and (whole or not shared) and _addressable(dyg)
            db = None
            if direct:
                gk = [_wide(dyg[0], 2 * cout)] if shared else dyg
            else:
                gb = _zeroed_levels(xg[0], ge * P, ce) if P != ce else _alloc_levels(xg[0], ge * P)
                gk = [[t[:, g * P:g * P + ce] for t in gb] for g in range(ge)]
            if direct:
                pass
            elif whole:
                db = _mask_and_bias_grad(_wide(dyg[0], 2 * cout), ybufs, gb, 2 * cout, want_b)
            else:
                parts = []
                for g in range(groups):
                    sl = slice(g * cout, (g + 1) * cout) if shared else slice(g * P, g * P + cout)
                    parts.append(_mask_and_bias_grad(
                        dyg[g], None if ybufs is None else [t[:, sl] for t in ybufs],
                        [t[:, sl] for t in gb], cout, want_b))
                db = torch.cat(parts) if want_b else None
            # ---- dx = conv(g, adjoint weight): inputs of P channels (zero weight rows for the padding)
            dxs = [None] * (groups * L)
            if need_x:
                wt = ops.conv3x3_bf16_pack(weight, groups=ge, adjoint=True)
                dxb = _alloc_levels(xg[0], ge * cin)
                dxk = [[t[:, g * cin:(g + 1) * cin] for t in dxb] for g in range(ge)]
                gin = [[t[:, g * P:(g + 1) * P] for t in gb] for g in range(ge)] if P != ce else gk
                ops.conv3x3_bf16_levels(gin, wt, None, cin, dxk, relu=False, cin=P)
                for g in range(ge):       # (shared: the one result is the sum of both towers' gradients)
                    for l in range(L):
                        if ctx.needs_input_grad[4 + g * L + l]:
                            dxs[g * L + l] = dxk[g][l]
            # ---- dW, fp32
            dw = None
            if ctx.needs_input_grad[0]:
                dw = ops.conv3x3_bf16_wgrad_levels(xg, gk, cin, ce)
        return (dw, db, None, None) + tuple(dxs)


class _Bf16ConvLevelsPadded(_Bf16ConvLevels):
    """_Bf16ConvLevels (one group) whose outputs are the tensors of the padded width"""

    @staticmethod
    def forward(ctx, weight, bias, relu, groups, *xs):
        return _Bf16ConvLevels._forward(ctx, True, weight, bias, relu, groups, xs)


def conv_levels(xs_groups, weight, bias=None, relu=False, padded=False):
    """xs_groups: one or two lists (the cls / reg tower) of per-level (B, cin, H, W) bf16 CUDA tensors
    (channels-last or channel slices of channels-last tensors); weight fp32 (groups * cout, cin, 3,
    3), bias fp32 (groups * cout) or None -> per group the list of per-level (B, cout, H, W) bf16
    tensors (channel slices of one channels-last tensor per level).  cin % 32 == 0, cout even.
    Two groups given the SAME input tensors run as one convolution with 2 * cout outputs, and the
    input's gradient is the sum over both.
    padded (one group only): -> [the list of per-level (B, P, H, W) tensors], P = cout rounded up to 32,
    zeros in the channels behind cout; their gradients are taken at that width."""
    groups = len(xs_groups)
    L = len(xs_groups[0])
    if not 1 <= groups <= 2 or any(len(g) != L for g in xs_groups):
        raise ValueError('conv_levels takes one or two groups of the same levels')
    if padded and groups != 1:
        raise ValueError('conv_levels: padded outputs for one group only')
    if any(not x.is_cuda or x.dtype != _BF for g in xs_groups for x in g) or weight.dtype != torch.float32:
        raise TypeError('conv_levels takes bf16 CUDA activations and an fp32 weight')
    node = _Bf16ConvLevelsPadded if padded else _Bf16ConvLevels
    out = node.apply(weight, bias, bool(relu), groups, *[x for g in xs_groups for x in g])
    return [list(out[g * L:(g + 1) * L]) for g in range(groups)]


def _plain(conv):
    from .winograd_train import _plain_3x3
    return _plain_3x3(conv) and conv.weight.dtype == torch.float32


def head_supported(head, sizes, batch):
    """the module side of `usable`: what head_forward computes for this head on per-level (H, W)
    feature sizes.  No device needed (the library's size query runs on the host)."""
    towers = list(head.cls_convs) + list(head.reg_convs)
    outs = [head.retina_cls, head.retina_reg] + ([head.retina_iou] if head.iou_branch else [])
    if head.in_channels % 32 or head.feat_channels % 32 or not towers or \
            len(head.cls_convs) != len(head.reg_convs) or not 1 <= len(sizes) <= 8:
        return False
    if not (all(not m.with_norm and m.with_activatation and _plain(m.conv) for m in towers)
            and all(_plain(c) for c in outs)):
        return False
    from . import _lib
    from .winograd_train import _library_loads
    if not _library_loads():
        return False
    d = _lib.Conv3x3Desc()
    d.num_levels, d.batch, d.groups = len(sizes), int(batch), 2
    d.cin = d.cout = d.x_stride = d.y_stride = int(head.feat_channels)
    for l, (h, w) in enumerate(sizes):
        d.H[l], d.W[l] = int(h), int(w)
    return int(_lib.lib().ia_conv3x3_bf16_wgrad_workspace_bytes(C.byref(d))) > 0


def usable(feats, head):
    """what head_forward covers: CUDA fp32 / bf16 features with autograd on, channel counts the MFMA
    kernels take, towers of plain 3x3 convolution + bias + ReLU, and a library whose weight-gradient
    kernel accepts the level sizes"""
    feats = list(feats)
    return (torch.is_grad_enabled() and len(feats) > 0
            and all(x.is_cuda and x.dtype in (torch.float32, _BF) and x.dim() == 4
                    and x.shape[1] == head.in_channels for x in feats)
            and head_supported(head, [tuple(x.shape[-2:]) for x in feats], feats[0].shape[0]))


def head_forward(head, feats):
    """_RetinaHeadBase.forward (multi_apply(forward_single)) with every convolution one bf16 node over
    all levels: the first tower layer as one convolution with 2F outputs on the shared input, the
    other tower layers as two groups on the channel halves, retina_cls on the cls half and
    retina_reg [| retina_iou] as one convolution on the reg half.  Returns (cls[L], reg[L][, iou[L]])
    as bf16 tensors of the reference's shapes (channel slices of the padded outputs)."""
    xs = [x.to(dtype=_BF, memory_format=_CL) for x in feats]
    cur = [xs, xs]
    for mc, mr in zip(head.cls_convs, head.reg_convs):
        cur = conv_levels(cur, torch.cat([mc.conv.weight, mr.conv.weight]),
                          torch.cat([mc.conv.bias, mr.conv.bias]), relu=True)
    cls_feat, reg_feat = cur
    cls = conv_levels([cls_feat], head.retina_cls.weight, head.retina_cls.bias)[0]
    convs = [head.retina_reg] + ([head.retina_iou] if head.iou_branch else [])
    n = [c.out_channels for c in convs]
    pad = sum(n) % 2                      # the forward kernel stores channel pairs
    if len(convs) == 1 and not pad:
        return cls, conv_levels([reg_feat], head.retina_reg.weight, head.retina_reg.bias)[0]
    w0, b0 = convs[0].weight, convs[0].bias
    w_ri = torch.cat([c.weight for c in convs] + ([w0.new_zeros((pad,) + tuple(w0.shape[1:]))] if pad else []))
    b_ri = torch.cat([c.bias for c in convs] + ([b0.new_zeros(pad)] if pad else []))
    ri = conv_levels([reg_feat], w_ri, b_ri)[0]
    reg = [t[:, :n[0]] for t in ri]
    if not head.iou_branch:
        return cls, reg
    return cls, reg, [t[:, n[0]:n[0] + n[1]] for t in ri]


# ------------------------------------------------------------------ FCOS heads
def fcos_head_supported(head, sizes, batch):
    """the module side of fcos_usable: what fcos_head_forward computes for this head on per-level
    (H, W) feature sizes.  No device needed (the library's size queries run on the host)."""
    from . import _lib, fcos_ops
    from .winograd_train import _fcos_tower_layer, _library_loads
    towers = list(head.cls_convs) + list(head.reg_convs)
    outs = [head.fcos_cls, head.fcos_centerness, head.fcos_reg] + ([head.fcos_iou] if head.iou_branch else [])
    F_ = head.feat_channels
    if head.in_channels % 32 or F_ % 32 or not towers or len(head.cls_convs) != len(head.reg_convs) \
            or not 1 <= len(sizes) <= min(len(head.scales), 8):
        return False
    if not all(_fcos_tower_layer(m, F_) for m in towers):
        return False
    if any(mc.norm.num_groups != mr.norm.num_groups or mc.norm.eps != mr.norm.eps
           for mc, mr in zip(head.cls_convs, head.reg_convs)):
        return False                      # one GroupNorm node for both towers of a layer
    if not all(_plain(c) and c.in_channels == F_ for c in outs):
        return False
    if not _library_loads():
        return False
    if not all(fcos_ops.groupnorm_bf16_supported(sizes, batch, 2 * F_, 2 * n)
               and fcos_ops.groupnorm_bf16_supported(sizes, batch, F_, n)       # (the per-tower fallback)
               for n in set(m.norm.num_groups for m in towers)):
        return False
    d = _lib.Conv3x3Desc()
    d.num_levels, d.batch, d.groups = len(sizes), int(batch), 2
    d.cin = d.cout = d.x_stride = d.y_stride = int(F_)
    for l, (h, w) in enumerate(sizes):
        d.H[l], d.W[l] = int(h), int(w)
    return int(_lib.lib().ia_conv3x3_bf16_wgrad_workspace_bytes(C.byref(d))) > 0


def fcos_usable(feats, head):
    """what fcos_head_forward covers: CUDA fp32 / bf16 features with autograd on, channel counts the
    MFMA kernels take, towers of 3x3 convolution without bias + GroupNorm + ReLU with whole 16-byte
    columns per group, and a library whose weight-gradient and GroupNorm kernels accept the sizes"""
    feats = list(feats)
    return (torch.is_grad_enabled() and len(feats) > 0
            and all(x.is_cuda and x.dtype in (torch.float32, _BF) and x.dim() == 4
                    and x.shape[1] == head.in_channels for x in feats)
            and fcos_head_supported(head, [tuple(x.shape[-2:]) for x in feats], feats[0].shape[0]))


def _packed_weights(convs):
    """several output convolutions of one tower as one: weight and bias, columns padded with zeros to an
    even count (the forward kernel stores channel pairs)"""
    n = [c.out_channels for c in convs]
    pad = sum(n) % 2
    w0, b0 = convs[0].weight, convs[0].bias
    if len(convs) == 1 and not pad:
        return w0, b0
    w = torch.cat([c.weight for c in convs] + ([w0.new_zeros((pad,) + tuple(w0.shape[1:]))] if pad else []))
    b = torch.cat([c.bias for c in convs] + ([b0.new_zeros(pad)] if pad else []))
    return w, b


def _packed_outputs(convs, feat):
    """several output convolutions of one tower as one bf16 node -> per convolution the list of
    per-level fp32 NCHW-contiguous maps"""
    w, b = _packed_weights(convs)
    ys = conv_levels([feat], w, b)[0]
    res, off = [], 0
    for k in [c.out_channels for c in convs]:
        res.append([t[:, off:off + k].to(torch.float32, memory_format=torch.contiguous_format) for t in ys])
        off += k
    return res


def _fcos_towers(head, feats):
    """both GN towers in bf16 -> (cls_feat[L], reg_feat[L]): the features cast once to bf16
    channels-last; per tower layer one convolution node for both towers and ONE GroupNorm + ReLU node
    on the 2F-channel activation"""
    from .fcos_ops import groupnorm_relu_bf16_towers
    xs = [x.to(dtype=_BF, memory_format=_CL) for x in feats]
    cur = [xs, xs]
    for mc, mr in zip(head.cls_convs, head.reg_convs):
        cur = conv_levels(cur, torch.cat([mc.conv.weight, mr.conv.weight]), None, relu=False)
        gc, gr = mc.norm, mr.norm
        cur = list(groupnorm_relu_bf16_towers(cur[0], cur[1], torch.cat([gc.weight, gr.weight]),
                                              torch.cat([gc.bias, gr.bias]), 2 * gc.num_groups, gc.eps))
    return cur


def fcos_head_forward_packed(head, feats):
    """the towers and the two output convolutions of fcos_head_forward, and nothing behind them:
    -> (cls_ctr[L], reg_iou[L]), the bf16 channels-last outputs of the padded width (82 -> 96, 6 -> 32),
    rows [cls | centerness | zeros] and [raw fcos_reg 4 | iou? | zeros], unsliced and unconverted -- what
    fcos_ops.point_head_loss_packed takes.  The convolution node's backward takes a gradient of the
    padded width as it is."""
    cls_feat, reg_feat = _fcos_towers(head, feats)
    wc, bc = _packed_weights([head.fcos_cls, head.fcos_centerness])
    wr, br = _packed_weights([head.fcos_reg] + ([head.fcos_iou] if head.iou_branch else []))
    return (conv_levels([cls_feat], wc, bc, padded=True)[0], conv_levels([reg_feat], wr, br, padded=True)[0])


def fcos_head_forward(head, feats):
    """_FCOSHeadBase.forward (multi_apply(forward_single)) in bf16: the features cast once to bf16
    channels-last; per tower layer one convolution node for both towers (the first as one convolution
    with 2F outputs on the shared input, the others as two groups on the channel halves), no bias, no
    ReLU, and ONE GroupNorm + ReLU node on the 2F-channel activation (2 x num_groups groups, the
    towers' gamma / beta concatenated); fcos_cls | fcos_centerness as one output convolution on the
    cls half (81 -> 82 columns), fcos_reg [| fcos_iou] as one on the reg half (5 -> 6; 4 in the plain
    head).  The outputs become fp32 NCHW maps and bbox_pred = exp(scale_l * reg) runs in torch in
    fp32: the reference's tuple (cls[L], bbox[L], centerness[L][, iou[L]]), which the fused loss node
    takes."""
    cls_feat, reg_feat = _fcos_towers(head, feats)
    cls, ctr = _packed_outputs([head.fcos_cls, head.fcos_centerness], cls_feat)
    ri = _packed_outputs([head.fcos_reg] + ([head.fcos_iou] if head.iou_branch else []), reg_feat)
    bbox = [scale(t).exp() for t, scale in zip(ri[0], head.scales)]
    if not head.iou_branch:
        return cls, bbox, ctr
    return cls, bbox, ctr, ri[1]
